"""sel_conv_step (csrc/stream.hip) against F.conv1d / F.conv_transpose1d in
fp64 on cat(buffer, chunk), three consecutive hops with carry_out fed back as
carry, in fp32 (<= 1e-5 norm-wise) and bf16 (<= 5e-2 norm-wise against the fp32
inputs): the tolerances DESIGN §3 fixes for the conv stack.

Beyond the values, every hop checks: carry_out is bitwise the last P rows of
the activated virtual input; carry is unchanged; 64-element NaN canaries on both
sides of out and carry_out are intact; a second launch gives the same bits.
Where the layer has an ELU, "the activated input" is taken from the kernel
itself -- a 1x1 step with an identity weight returns act(x) exactly (one
product by 1.0, the rest by 0.0) -- and compared with F.elu separately, so the
bitwise check does not hinge on two exp implementations agreeing to the ulp.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 5e-2}
DTYPES = [torch.float32, torch.bfloat16]


def _rel(a, ref):
    a = a.detach().double().cpu()
    return float((a - ref).norm() / (ref.norm() + 1e-300))


def _canaried(shape, dtype, gpu):
    n = int(np.prod(shape))
    flat = torch.full((n + 128,), float("nan"), dtype=dtype, device=gpu)
    return flat, flat[64:64 + n].view(shape)


def _intact(flat):
    return bool(torch.isnan(flat[:64]).all()) and bool(torch.isnan(flat[-64:]).all())


def _activated(x, dtype, gpu):
    """act(x) as the kernel computes it, exactly: a K = 1 step with the identity weight."""
    from sel import convops as CO
    from sel import streamops as SO
    rows, C = x.shape[0] * x.shape[1], x.shape[2]
    eye = torch.eye(C, dtype=dtype, device=gpu).view(C, 1, C).contiguous()
    d = CO.ConvDesc(rows, x.shape[1], C, C, 1, 1, 0, CO.PAD_ZERO, 1, 0)
    out, _ = SO.conv_step(d, None, x.contiguous(), eye)
    a = out.view(x.shape)
    ref = F.elu(x.float())
    # the activation itself: fp32 to a few ulp, bf16 to one rounding of the result
    tol = 1e-6 if dtype == torch.float32 else 2.0 ** -7
    assert float(((a.float() - ref).abs() / (ref.abs() + 1e-3)).max()) <= tol
    assert torch.equal(a[x > 0], x[x > 0])
    return a


class _Layer:
    """One layer under test: the descriptor, the packed weight and the fp64 reference."""

    def __init__(self, gpu, dtype, B, T, C, N, K, dil, w, pack_kind, stride, ref, elu=False, bias=None,
                 bias_period=0):
        from sel import convops as CO
        self.gpu, self.dtype, self.B, self.T, self.C, self.N = gpu, dtype, B, T, C, N
        self.P = (K - 1) * dil
        self.elu, self.ref = elu, ref
        self.desc = CO.ConvDesc(B * T, T, C, N, K, dil, self.P, CO.PAD_ZERO, int(elu), bias_period)
        self.wp = CO.pack(pack_kind, w.to(gpu), stride, dtype)
        assert tuple(self.wp.shape) == (N, K, C)
        self.bias = bias.to(gpu) if bias is not None else None

    def step(self, carry, x, res=None):
        """One launch into canaried buffers; returns (out, carry_out) after the
        structural checks of this hop."""
        from sel import streamops as SO
        odt = self.dtype
        fo, out = _canaried((self.B * self.T, self.N), odt, self.gpu)
        fc, cout = _canaried((self.B, self.P, self.C), self.dtype, self.gpu) if self.P else (None, None)
        keep = carry.clone() if carry is not None else None
        SO.conv_step(self.desc, carry, x, self.wp, self.bias, res, out, cout)
        fo2, out2 = _canaried((self.B * self.T, self.N), odt, self.gpu)
        fc2, cout2 = _canaried((self.B, self.P, self.C), self.dtype, self.gpu) if self.P else (None, None)
        SO.conv_step(self.desc, carry, x, self.wp, self.bias, res, out2, cout2)
        torch.cuda.synchronize()
        assert _intact(fo) and _intact(fo2), "out canary"
        assert not bool(torch.isnan(out.float()).any())
        assert torch.equal(out, out2), "two launches differ"
        if self.P:
            assert _intact(fc) and _intact(fc2), "carry_out canary"
            assert torch.equal(carry, keep), "carry was written"
            assert torch.equal(cout, cout2)
            xa = _activated(x, self.dtype, self.gpu) if self.elu else x
            want = torch.cat((carry, xa.view(self.B, self.T, self.C)), 1)[:, -self.P:]
            assert torch.equal(cout.view(torch.uint8), want.contiguous().view(torch.uint8)), "carry_out bits"
        return out, cout


def _run_plain(gpu, dtype, B, T, C, N, K, dil, elu=False, res=False, bias=False, seed=0):
    """A stride-1 causal layer over three hops; returns the per-hop outputs."""
    from sel import convops as CO
    g = torch.Generator().manual_seed(1000 + seed)
    w = torch.randn(N, C, K, generator=g) / (C * K) ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    P = (K - 1) * dil
    lay = _Layer(gpu, dtype, B, T, C, N, K, dil, w, CO.PACK_FWD, 1, None, elu, b, N if bias else 0)
    buf = torch.randn(B, C, P, generator=g)                       # what pad_buffer holds (already activated)
    carry = buf.transpose(1, 2).contiguous().to(dtype).to(gpu) if P else None
    outs = []
    for hop in range(3):
        x = torch.randn(B, C, T, generator=g)
        r = torch.randn(B, N, T, generator=g) if res else None
        xa = F.elu(x.double()) if elu else x.double()
        xb = torch.cat((buf.double(), xa), -1)
        y = F.conv1d(xb, w.double(), b.double() if bias else None, dilation=dil)
        if res:
            y = y + r.double()
        buf = xb[:, :, xb.shape[-1] - P:]
        xc = x.transpose(1, 2).contiguous().to(dtype).to(gpu)
        rc = r.transpose(1, 2).contiguous().view(B * T, N).to(dtype).to(gpu) if res else None
        out, carry = lay.step(carry, xc, rc)
        e = _rel(out.view(B, T, N).transpose(1, 2), y)
        assert e <= TOL[dtype], (hop, e)
        if P:
            assert _rel(carry.transpose(1, 2), buf) <= TOL[dtype]
        outs.append((xc, rc, out))
    return lay, outs


PLAIN = {
    "one_row_T_lt_P": dict(B=1, T=1, C=512, N=64, K=3, dil=1),
    "carry_keeps_49_rows_elu": dict(B=1, T=5, C=256, N=256, K=7, dil=9, elu=True),
    "pointwise_elu_res": dict(B=3, T=25, C=128, N=128, K=1, dil=1, elu=True, res=True),
    "C1": dict(B=1, T=300, C=1, N=32, K=7, dil=1),
    "N1": dict(B=2, T=300, C=32, N=1, K=7, dil=1),
    "C4_odd_rows_bias": dict(B=2, T=17, C=4, N=8, K=7, dil=3, bias=True),
    "several_row_tiles": dict(B=2, T=600, C=32, N=32, K=7, dil=9),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(PLAIN))
def test_step_plain_layers(gpu, case, dtype):
    _run_plain(gpu, dtype, seed=list(PLAIN).index(case), **PLAIN[case])


def _strided_setup(gpu, dtype, B, seed=7):
    from sel import convops as CO
    g = torch.Generator().manual_seed(seed)
    s, cin, cout = 5, 256, 512
    w = torch.randn(cout, cin, 2 * s, generator=g) / (cin * 2 * s) ** 0.5
    b = torch.randn(cout, generator=g)
    lay = _Layer(gpu, dtype, B, 5, s * cin, cout, 3, 1, w, CO.PACK_FWD_STRIDED, s, None, False, b, cout)
    return g, s, cin, cout, w, b, lay


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
def test_step_strided_downsampling(gpu, B, dtype):
    """(512, 256, 10), s = 5 through SEL_PACK_FWD_STRIDED, 25 new samples per hop,
    against F.conv1d(stride=5) on cat(last 9 samples, x).  The carry is 10 samples;
    the oldest meets a structurally zero weight, so it starts as noise here."""
    g, s, cin, cout, w, b, lay = _strided_setup(gpu, dtype, B)
    buf10 = torch.randn(B, cin, 2 * s, generator=g)
    carry = buf10.transpose(1, 2).contiguous().view(B, 2, s * cin).to(dtype).to(gpu)
    buf = buf10[:, :, 1:]
    for hop in range(3):
        x = torch.randn(B, cin, 25, generator=g)
        xb = torch.cat((buf.double(), x.double()), -1)
        y = F.conv1d(xb, w.double(), b.double(), stride=s)
        buf = xb[:, :, -(2 * s - 1):]
        xc = x.transpose(1, 2).contiguous().view(B * 5, s * cin).to(dtype).to(gpu)
        out, carry = lay.step(carry, xc)
        e = _rel(out.view(B, 5, cout).transpose(1, 2), y)
        assert e <= TOL[dtype], (hop, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 5])
def test_step_transposed_upsampling(gpu, T, dtype):
    """ConvTranspose1d weight (512, 256, 10), s = 5 through SEL_PACK_CONVT, B = 2,
    against conv_transpose1d(cat(buf, x))[s:-s]."""
    from sel import convops as CO
    B, s, cin, cout = 2, 5, 512, 256
    g = torch.Generator().manual_seed(9)
    w = torch.randn(cin, cout, 2 * s, generator=g) / (2 * cin) ** 0.5
    b = torch.randn(cout, generator=g)
    lay = _Layer(gpu, dtype, B, T, cin, s * cout, 2, 1, w, CO.PACK_CONVT, s, None, False, b, cout)
    buf = torch.randn(B, cin, 1, generator=g)
    carry = buf.transpose(1, 2).contiguous().to(dtype).to(gpu)
    for hop in range(3):
        x = torch.randn(B, cin, T, generator=g)
        xb = torch.cat((buf.double(), x.double()), -1)
        y = F.conv_transpose1d(xb, w.double(), b.double(), stride=s)[:, :, s:-s]
        buf = xb[:, :, -1:]
        xc = x.transpose(1, 2).contiguous().view(B * T, cin).to(dtype).to(gpu)
        out, carry = lay.step(carry, xc)
        e = _rel(out.view(B, T * s, cout).transpose(1, 2), y)
        assert e <= TOL[dtype], (hop, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_step_batch_invariance_dilated_elu(gpu, dtype):
    """(T 5, C 256, N 256, K 7, dil 9, ELU): a B = 3 launch equals three B = 1 launches bitwise."""
    from sel import convops as CO
    from sel import streamops as SO
    g = torch.Generator().manual_seed(21)
    T, C, N, K, dil = 5, 256, 256, 7, 9
    P = (K - 1) * dil
    wp = CO.pack(CO.PACK_FWD, (torch.randn(N, C, K, generator=g) / (C * K) ** 0.5).to(gpu), 1, dtype)
    carry = torch.randn(3, P, C, generator=g).to(dtype).to(gpu)
    x = torch.randn(3, T, C, generator=g).to(dtype).to(gpu)
    d3 = CO.ConvDesc(3 * T, T, C, N, K, dil, P, CO.PAD_ZERO, 1, 0)
    d1 = d3.with_(rows=T)
    out3, c3 = SO.conv_step(d3, carry, x.view(3 * T, C), wp)
    for b in range(3):
        o, c = SO.conv_step(d1, carry[b:b + 1].contiguous(), x[b].contiguous(), wp)
        assert torch.equal(o, out3.view(3, T, N)[b]) and torch.equal(c[0], c3[b]), b


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_step_batch_invariance_strided(gpu, dtype):
    from sel import streamops as SO
    g, s, cin, cout, w, b, lay = _strided_setup(gpu, dtype, 3, seed=23)
    carry = torch.randn(3, 2, s * cin, generator=g).to(dtype).to(gpu)
    x = torch.randn(3, 5, s * cin, generator=g).to(dtype).to(gpu)
    out3, c3 = SO.conv_step(lay.desc, carry, x.view(15, s * cin), lay.wp, lay.bias)
    d1 = lay.desc.with_(rows=5)
    for i in range(3):
        o, c = SO.conv_step(d1, carry[i:i + 1].contiguous(), x[i].contiguous(), lay.wp, lay.bias)
        assert torch.equal(o, out3.view(3, 5, cout)[i]) and torch.equal(c[0], c3[i]), i


def test_stream_commit_copies_every_job(gpu):
    """sel_stream_commit: 50 jobs (two launches of at most 48), sizes that are and
    are not multiples of 16 bytes, destinations between canaries."""
    from sel import streamops as SO
    g = torch.Generator().manual_seed(2)
    pairs, flats = [], []
    for j in range(50):
        n = [6, 54 * 512, 1, 1280 * 2, 37][j % 5]
        dt = [torch.float32, torch.bfloat16][j % 2]
        src = torch.randn(n, generator=g).to(dt).to(gpu)
        flat, dst = _canaried((n,), dt, gpu)
        pairs.append((src, dst))
        flats.append(flat)
    SO.commit(pairs)
    torch.cuda.synchronize()
    for (src, dst), flat in zip(pairs, flats):
        assert torch.equal(src, dst) and _intact(flat)
