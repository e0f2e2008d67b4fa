"""sel_hfg_conv_step (csrc/hfg_step.hip) against an fp64 statement of its
contract (include/sel.h): F.conv1d(groups=G) / F.conv_transpose1d on
cat(carry, LeakyReLU(new rows)), then bias, residual, tanh, scale, accumulate in
that order.  fp32: <= 1e-5 norm-wise.  bf16: inputs and weights are pre-rounded
to bf16 and compared against fp64 at 5e-2 norm-wise, the bound
tests/test_gpu_stream_step.py uses for the bf16 step.

Beyond the values every launch checks: carry_out is bitwise
[old carry rows T.. | act(new rows)] (LeakyReLU is one multiply, so torch's
result is the kernel's, bit for bit); carry is unchanged; 64-element NaN
canaries on both sides of out and carry_out are intact; a second launch gives
the same bits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 5e-2}
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _rel(a, ref):
    a = a.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def _canaried(shape, dtype, gpu):
    n = int(np.prod(shape))
    flat = torch.full((n + 128,), float("nan"), dtype=dtype, device=gpu)
    return flat, flat[64:64 + n].view(shape)


def _intact(flat):
    return bool(torch.isnan(flat[:64]).all()) and bool(torch.isnan(flat[-64:]).all())


def _rnd(shape, g, dtype, scale=1.0):
    """random values representable in `dtype` (pre-rounded), fp32 on the CPU"""
    return (scale * torch.randn(shape, generator=g)).to(dtype).float()


def _act(x, slope):
    """act() of the contract in x's dtype: fp32 arithmetic, rounded once"""
    xf = x.float()
    return torch.where(xf >= 0, xf, slope * xf).to(x.dtype) if slope != 1.0 else x


class _Layer:
    """One grouped causal layer under test (SEL_PACK_FWD)."""

    def __init__(self, gpu, dtype, g, B, T, C, N, K, dil, G=1, slope=1.0, shared_in=False, shared_res=False,
                 bias=False, tanh=False, scale=1.0, out_dtype=None, w=None):
        from sel import convops as CO
        self.gpu, self.dtype, self.odt = gpu, dtype, out_dtype or dtype
        self.B, self.T, self.C, self.N, self.K, self.dil, self.G = B, T, C, N, K, dil, G
        self.P = (K - 1) * dil
        self.slope, self.shared_in, self.shared_res, self.tanh, self.scale = slope, shared_in, shared_res, tanh, scale
        self.w = _rnd((N, C // G, K), g, dtype, (C // G * K) ** -0.5) if w is None else w
        self.b = torch.randn(N, generator=g) if bias else None
        self.wp = CO.pack(CO.PACK_FWD, self.w.to(gpu), 1, dtype)
        assert tuple(self.wp.shape) == (N, K, C // G)
        self.bias = self.b.to(gpu) if bias else None

    def desc(self, B=None, accumulate=False):
        from sel import hfgops as HF
        B = B or self.B
        return HF.make_desc(B * self.T, self.T, self.C, self.N, self.K, self.dil, self.P, groups=self.G,
                            shared_in=self.shared_in, shared_res=self.shared_res,
                            bias_period=self.N if self.b is not None else 0, tanh=self.tanh, accumulate=accumulate,
                            slope=self.slope, scale=self.scale)

    def ref(self, carry, x, res=None, prev=None):
        """fp64: carry (B, P, C), x (B, T, C or C/G), res (B, T, N or N/G), prev (B, T, N) -> (out (B, T, N), carry_out)"""
        x = x.double()
        a = torch.where(x >= 0, x, self.slope * x)
        if self.shared_in:
            a = a.repeat(1, 1, self.G)
        v = torch.cat((carry.double(), a), 1) if self.P else a
        y = F.conv1d(v.transpose(1, 2), self.w.double(), self.b.double() if self.b is not None else None,
                     dilation=self.dil, groups=self.G).transpose(1, 2)
        if res is not None:
            y = y + (res.double().repeat(1, 1, self.G) if self.shared_res else res.double())
        if self.tanh:
            y = torch.tanh(y)
        y = y * self.scale
        if prev is not None:
            y = y + prev.double()
        return y, v[:, v.shape[1] - self.P:]

    def step(self, carry, x, res=None, prev=None):
        """One launch into canaried buffers (twice); carry / x / res / prev are CPU
        fp32 tensors holding dtype-representable values.  Returns (out, carry_out)
        on the GPU after the structural checks."""
        from sel import streamops as SO
        gpu, dt = self.gpu, self.dtype
        B, T = x.shape[0], x.shape[1]
        d = self.desc(B, prev is not None)
        cg = carry.to(dt).to(gpu).contiguous() if self.P else None
        xg = x.to(dt).to(gpu).contiguous()
        rg = res.to(self.odt).to(gpu).contiguous().view(B * T, -1) if res is not None else None
        keep = cg.clone() if cg is not None else None
        got = []
        for _ in range(2):
            fo, out = _canaried((B * T, self.N), self.odt, gpu)
            if prev is not None:
                out.copy_(prev.to(self.odt).view(B * T, self.N))
            fc, cout = _canaried((B, self.P, self.C), dt, gpu) if self.P else (None, None)
            SO.hfg_conv_step(d, cg, xg.view(B * T, -1), self.wp, self.bias, rg, out, cout)
            got.append((fo, out, fc, cout))
        torch.cuda.synchronize()
        (fo, out, fc, cout), (fo2, out2, fc2, cout2) = got
        assert _intact(fo) and _intact(fo2), "out canary"
        assert not bool(torch.isnan(out.float()).any())
        assert torch.equal(out, out2), "two launches differ"
        if self.P:
            assert _intact(fc) and _intact(fc2), "carry_out canary"
            assert torch.equal(cg, keep), "carry was written"
            assert torch.equal(cout, cout2)
            xa = _act(xg, self.slope)
            if self.shared_in:
                xa = xa.repeat(1, 1, self.G)       # pitch C: the activated new rows once per group
            want = torch.cat((cg, xa), 1)[:, T:].contiguous()
            assert want.shape == cout.shape
            assert torch.equal(cout.view(torch.uint8), want.view(torch.uint8)), "carry_out bits"
        return out, cout

    def check(self, carry, x, res=None, prev=None):
        out, cout = self.step(carry, x, res, prev)
        y, c = self.ref(carry, x, res, prev)
        e = _rel(out.view(y.shape), y)
        assert e <= TOL[self.dtype], e
        if self.P:
            assert _rel(cout, c) <= TOL[self.dtype]
        return out, cout


def _inputs(lay, g, B=None, res=False, negative_carry=False):
    B = B or lay.B
    dt = lay.dtype
    carry = _rnd((B, lay.P, lay.C), g, dt)
    if negative_carry:
        carry = (-carry.abs() - 0.25).to(dt).float()
    x = _rnd((B, lay.T, lay.C // lay.G if lay.shared_in else lay.C), g, dt)
    r = _rnd((B, lay.T, lay.N // lay.G if lay.shared_res else lay.N), g, lay.odt) if res else None
    return carry, x, r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tile_aligned_groups_vector_path(gpu, dtype):
    """G = 3, C = N = 96 (32 per group: two full column tiles per group, 16-byte
    loads), K = 11, dil = 5, T = 5 < P = 50: carry_out keeps 45 old rows.  Three
    hops with carry_out fed back."""
    g = torch.Generator().manual_seed(1)
    lay = _Layer(gpu, dtype, g, 1, 5, 96, 96, 11, 5, G=3, slope=0.1, bias=True)
    carry, x, r = _inputs(lay, g, res=True)
    for hop in range(3):
        _, cout = lay.check(carry, x, r)
        carry = cout.float().cpu()
        _, x, r = _inputs(lay, g, res=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [12, 24])
def test_masked_tiles(gpu, C, dtype):
    """G = 3 at 4 (element-wise operand path) and 8 (16-byte loads) channels per
    group: one masked column tile per group; T = 17 is two row tiles, one partial."""
    g = torch.Generator().manual_seed(2 + C)
    lay = _Layer(gpu, dtype, g, 1, 17, C, C, 11, 3, G=3, slope=0.1, bias=True)
    lay.check(*_inputs(lay, g, res=True))
    lay2 = _Layer(gpu, dtype, g, 2, 17, C, C, 11, 3, G=3, slope=0.1)
    lay2.check(*_inputs(lay2, g))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slope", [0.1, 1.0])
def test_carry_is_not_reactivated(gpu, slope, dtype):
    """The carry holds negative values (<= -0.25): they enter the conv and
    carry_out as they are.  Against the reference that activates the new rows
    only -- and, to show the comparison can tell, the reference that would
    activate the carry too is far outside the bound when slope != 1."""
    g = torch.Generator().manual_seed(5)
    lay = _Layer(gpu, dtype, g, 2, 5, 48, 48, 7, 3, G=3, slope=slope)
    carry, x, _ = _inputs(lay, g, negative_carry=True)
    out, cout = lay.check(carry, x)
    assert torch.equal(cout[:, :lay.P - lay.T].float().cpu(), carry[:, lay.T:])
    if slope != 1.0:
        wrong, _ = lay.ref(torch.where(carry >= 0, carry, slope * carry), x)
        assert _rel(out.view(wrong.shape), wrong) > 10 * TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [96, 12])
def test_shared_input_and_shared_residual(gpu, C, dtype):
    """in_group_stride 0: new rows of pitch C/G read by every group, the carry
    at pitch C (three different per-group histories); carry_out replicated per
    group.  res_group_stride 0: the residual of pitch N/G.  Each alone and both."""
    g = torch.Generator().manual_seed(7 + C)
    for sh_in, sh_res in ((True, False), (False, True), (True, True)):
        lay = _Layer(gpu, dtype, g, 2, 5, C, C, 11, 1, G=3, slope=0.1, shared_in=sh_in, shared_res=sh_res, bias=True)
        carry, x, r = _inputs(lay, g, res=True)
        assert x.shape[-1] == (C // 3 if sh_in else C) and r.shape[-1] == (C // 3 if sh_res else C)
        _, cout = lay.check(carry, x, r)
        if sh_in:
            new = cout[:, lay.P - lay.T:].view(2, lay.T, 3, C // 3)
            assert torch.equal(new[:, :, 0], new[:, :, 1]) and torch.equal(new[:, :, 0], new[:, :, 2])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mrf_mean_by_scaled_accumulation(gpu, dtype):
    """Three launches (K = 3, 7, 11) with out_scale = 1/3 into ONE buffer, the
    second and third with accumulate: the result is the mean of the three
    residual outputs.  The first launch overwrites a buffer full of NaN."""
    from sel import streamops as SO
    g = torch.Generator().manual_seed(11)
    B, T, C = 2, 5, 32
    x = _rnd((B, T, C), g, dtype)
    r = _rnd((B, T, C), g, dtype)
    flat, out = _canaried((B * T, C), dtype, gpu)
    out.fill_(float("nan"))
    mean = 0
    for j, K in enumerate((3, 7, 11)):
        lay = _Layer(gpu, dtype, g, B, T, C, C, K, 1, slope=0.1, bias=True, scale=1.0 / 3)
        carry = _rnd((B, lay.P, C), g, dtype)
        SO.hfg_conv_step(lay.desc(B, accumulate=j > 0), carry.to(dtype).to(gpu), x.to(dtype).to(gpu).view(B * T, C),
                         lay.wp, lay.bias, r.to(dtype).to(gpu).view(B * T, C), out)
        lay.scale = 1.0
        mean = mean + lay.ref(carry, x, r)[0] / 3
    torch.cuda.synchronize()
    assert _intact(flat) and not bool(torch.isnan(out.float()).any())
    e = _rel(out.view(B, T, C), mean)
    assert e <= TOL[dtype], e
    # one accumulating launch alone, through the per-launch checks (prev rounded to the output type)
    lay = _Layer(gpu, dtype, g, B, T, C, C, 7, 1, slope=0.1, bias=True, scale=1.0 / 3)
    lay.check(_rnd((B, lay.P, C), g, dtype), x, r, prev=_rnd((B, T, C), g, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16_in_fp32_out"])
def test_output_conv_tanh(gpu, dtype):
    """N = 1, C = 32, K = 7, LeakyReLU(0.01), tanh; the output is fp32 for both input types."""
    g = torch.Generator().manual_seed(13)
    lay = _Layer(gpu, dtype, g, 2, 60, 32, 1, 7, 1, slope=0.01, bias=True, tanh=True, out_dtype=torch.float32)
    carry, x, _ = _inputs(lay, g)
    out, _ = lay.check(carry, (3.0 * x).to(dtype).float())
    assert out.dtype == torch.float32 and float(out.abs().max()) <= 1.0 and float(out.abs().max()) > 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [1, 5])
def test_upsample_convt_pack(gpu, T, dtype):
    """ConvTranspose1d weight (16, 8, 10), s = 5, through SEL_PACK_CONVT with
    slope 0.1 and a bias of period Cout, B = 2, three hops, against
    conv_transpose1d(cat(buf, act(x)))[s:-s]."""
    from sel import convops as CO
    from sel import hfgops as HF
    from sel import streamops as SO
    B, s, cin, cout = 2, 5, 16, 8
    g = torch.Generator().manual_seed(17)
    w = _rnd((cin, cout, 2 * s), g, dtype, (2 * cin) ** -0.5)
    b = torch.randn(cout, generator=g)
    wp = CO.pack(CO.PACK_CONVT, w.to(gpu), s, dtype)
    assert tuple(wp.shape) == (s * cout, 2, cin)
    d = HF.make_desc(B * T, T, cin, s * cout, 2, 1, 1, bias_period=cout, slope=0.1)
    buf = _rnd((B, cin, 1), g, dtype)
    carry = buf.transpose(1, 2).contiguous().to(dtype).to(gpu)
    for hop in range(3):
        x = _rnd((B, cin, T), g, dtype)
        xd = x.double()
        xb = torch.cat((buf.double(), torch.where(xd >= 0, xd, 0.1 * xd)), -1)
        y = F.conv_transpose1d(xb, w.double(), b.double(), stride=s)[:, :, s:-s]
        buf = xb[:, :, -1:]
        xc = x.transpose(1, 2).contiguous().to(dtype).to(gpu)
        fo, out = _canaried((B * T, s * cout), dtype, gpu)
        fc, cnew = _canaried((B, 1, cin), dtype, gpu)
        SO.hfg_conv_step(d, carry, xc.view(B * T, cin), wp, b.to(gpu), None, out, cnew)
        torch.cuda.synchronize()
        assert _intact(fo) and _intact(fc)
        e = _rel(out.view(B, T * s, cout).transpose(1, 2), y)
        assert e <= TOL[dtype], (hop, e)
        assert torch.equal(cnew, _act(xc, 0.1)[:, -1:])
        carry = cnew.clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_invariance_dilated_groups(gpu, dtype):
    """The tile-aligned layer (T 5, G 3, C = N = 96, K 11, dil 5) at B = 3 equals three B = 1 launches bitwise."""
    from sel import streamops as SO
    g = torch.Generator().manual_seed(21)
    lay = _Layer(gpu, dtype, g, 3, 5, 96, 96, 11, 5, G=3, slope=0.1, bias=True)
    carry, x, r = (v.to(dtype).to(gpu) for v in _inputs(lay, g, res=True))
    out3, c3 = SO.hfg_conv_step(lay.desc(3), carry, x.view(15, 96), lay.wp, lay.bias, r.view(15, 96))
    for b in range(3):
        o, c = SO.hfg_conv_step(lay.desc(1), carry[b:b + 1].contiguous(), x[b].contiguous(), lay.wp, lay.bias,
                                r[b].contiguous())
        assert torch.equal(o, out3.view(3, 5, 96)[b]) and torch.equal(c[0], c3[b]), b


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_invariance_across_the_row_tile_switch(gpu, dtype):
    """A 12-channel G = 3 layer at B = 4 x T = 300: 1200 rows = 75 row tiles take
    four row tiles per block (from 64 tiles on), each B = 1 launch (19 tiles) one
    per block.  Outputs and carry_out are bitwise equal."""
    from sel import streamops as SO
    g = torch.Generator().manual_seed(23)
    lay = _Layer(gpu, dtype, g, 4, 300, 12, 12, 7, 3, G=3, slope=0.1, bias=True)
    carry, x, _ = (v.to(dtype).to(gpu) if v is not None else None for v in _inputs(lay, g))
    out4, c4 = SO.hfg_conv_step(lay.desc(4), carry, x.view(1200, 12), lay.wp, lay.bias)
    y, _ = lay.ref(carry.float().cpu(), x.float().cpu())
    assert _rel(out4.view(4, 300, 12), y) <= TOL[dtype]
    for b in range(4):
        o, c = SO.hfg_conv_step(lay.desc(1), carry[b:b + 1].contiguous(), x[b].contiguous(), lay.wp, lay.bias)
        assert torch.equal(o, out4.view(4, 300, 12)[b]) and torch.equal(c[0], c4[b]), b
