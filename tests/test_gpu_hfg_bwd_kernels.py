"""Backward of the grouped LeakyReLU-fused conv primitive (csrc/hifigan_bwd.hip,
sel_hfg_conv_bwd_data / sel_hfg_conv_wgrad) against fp64 torch autograd of the
host restatement of tests/test_gpu_hfg_kernels.py (F.conv1d / conv_transpose1d),
computed from the SAME operands: in bf16 the prologue result LeakyReLU(x) is
rounded to bf16 once, as the contract in include/sel.h says (the restatement
takes the rounded VALUE and the exact derivative act'(x), slope at x == 0).

Bounds (the project's): fp32 <= 1e-5 norm-wise; a bf16 gin is one rounded output,
<= 4e-3 norm-wise and |a - b| <= 8e-3 |b| + 2e-3 max|b|; gW and gbias are fp32
sums of exact products of the same operands, <= 1e-5 in both instances.

Shapes: those of the forward file -- B = 2 (no gradient across the sample
boundary), T = 7 (below the 50-row reach of K = 11, d = 5) and T = 130 (crosses
the 64-row tile, ragged tail, 6 row tiles for the split), per-group widths 6,
32, 64, 128, 256, the transposed forms at T = 9, the 32 -> 1 tanh conv.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 2
# (G, C/G, K, dil)
CASES = [(3, 32, 11, 5), (3, 64, 3, 3), (1, 128, 7, 1), (3, 256, 11, 1), (1, 32, 3, 5), (1, 6, 7, 3)]
DTYPES = [torch.bfloat16, torch.float32]
TUNE_SPLIT = 72


def _ids(c):
    return "G%d_C%d_K%d_d%d" % c


def _rel(out, ref):
    out, ref = out.double().cpu(), ref.double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    return float((out - ref).norm() / ref.norm())


def _check_gin(out, ref, dtype, what):
    rel = _rel(out, ref)
    print(f"{what} gin: rel {rel:.2e}")
    if dtype == torch.float32:
        assert rel <= 1e-5, (what, rel)
        return
    assert rel <= 4e-3, (what, rel)
    out, ref = out.double().cpu(), ref.double().cpu()
    tol = 8e-3 * ref.abs() + 2e-3 * ref.abs().max()
    bad = ((out - ref).abs() > tol).sum().item()
    assert bad == 0, (what, bad, float((out - ref).abs().max()))


def _check_sum(out, ref, what):
    rel = _rel(out, ref)
    print(f"{what}: rel {rel:.2e}")
    assert rel <= 1e-5, (what, rel)


def _rand(gen, shape, dtype, dev, scale=1.0):
    return (scale * torch.randn(shape, generator=gen)).to(dtype).to(dev)


def _zeros_in(x):
    """a few exact zeros: act'(0) = slope"""
    x[0, 0, :3] = 0
    x[-1, -1, 1] = 0
    x[0, x.shape[1] // 2, -1] = 0
    return x


def _act64(x, slope):
    """(value, leaf): fp64 activation whose VALUE is the kernel's prologue result
    (fp32 LeakyReLU rounded once to the operand type) and whose derivative wrt the
    fp64 leaf is act'(x) = 1 for x > 0, else slope"""
    xd = x.cpu().double().requires_grad_(True)
    xf = x.cpu().float()
    rounded = torch.where(xf >= 0, xf, xf * slope).to(x.dtype).double()
    a = torch.where(xd > 0, xd, xd * slope)
    return a + (rounded - a).detach(), xd


def _scale64(scale):
    return float(torch.tensor(scale, dtype=torch.float32))


def _grouped(gpu, dtype, G, Cg, K, dil, T, mode, seed):
    from sel import convops as CO
    from sel import hfgops as HF
    gen = torch.Generator().manual_seed(seed)
    C = N = G * Cg
    shared = mode == "shared"
    epi = mode == "epi"
    skip = mode != "plain"
    x = _zeros_in(_rand(gen, (B, T, Cg if shared else C), dtype, gpu))
    w = _rand(gen, (N, Cg, K), dtype, gpu, (Cg * K) ** -0.5)
    gout = _rand(gen, (B, T, N), dtype, gpu)
    prev = _rand(gen, x.shape, dtype, gpu) if epi else None
    scale = 1.0 / 3.0 if epi else 1.0
    d = HF.make_desc(B * T, T, C, N, K, dil, (K - 1) * dil, CO.PAD_ZERO, G, shared, shared, N, slope=0.1, scale=scale,
                     accumulate=epi)
    code = CO._code(dtype)
    lib = CO.L.lib()
    kd, kw = lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), code, code, 0), lib.sel_hfg_conv_bwd_kernel(
        ctypes.byref(d), code, code, 1)
    if dtype == torch.bfloat16 and Cg > 4:
        assert kd in (1, 2, 4) and kw == 1, (kd, kw)      # the matrix-core instances
    else:
        assert kd == 0 and kw == 0, (kd, kw)
    wp = CO.pack(CO.PACK_FWD, w.float(), 1, dtype)
    gin = HF.bwd_data(d, gout, HF.dgrad_pack(wp, G), x, None, gout if skip else None, scale,
                      prev.clone() if epi else None)
    gwp, gb = HF.wgrad(d, gout, x)
    gw = CO.unpack(CO.PACK_FWD, gwp, (N, Cg, K), 1)

    # fp64 autograd of out = scale * (conv(act(x)) + bias + x) from the same operands
    a, xd = _act64(x, 0.1)
    w64 = w.cpu().double().requires_grad_(True)
    b64 = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    ain = a.repeat(1, 1, G) if shared else a
    y = F.conv1d(F.pad(ain.transpose(1, 2), ((K - 1) * dil, 0)), w64, b64, dilation=dil, groups=G).transpose(1, 2)
    if skip:
        y = y + (xd.repeat(1, 1, G) if shared else xd)
    (y * _scale64(scale) * gout.cpu().double()).sum().backward()
    gx = xd.grad + (prev.cpu().double() if epi else 0.0)
    what = f"{mode} G{G} C{Cg} K{K} d{dil} T{T} {dtype}"
    _check_gin(gin, gx, dtype, what)
    _check_sum(gw, w64.grad, what + " gW")
    _check_sum(gb, b64.grad, what + " gbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_grouped_conv_backward(gpu, case, T, dtype):
    """plain: each group reads its own channels, zero pad adjoint, LeakyReLU' mask"""
    _grouped(gpu, dtype, *case, T, "plain", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 3], ids=_ids)
def test_shared_input_and_skip_backward(gpu, case, T, dtype):
    """in_group_stride 0: gin has C/G channels and sums the groups, the skip too"""
    _grouped(gpu, dtype, *case, T, "shared", 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_skip_scale_accumulate_backward(gpu, case, T, dtype):
    """the skip after the mask, out_scale = 1/3, gin added to what is already there"""
    _grouped(gpu, dtype, *case, T, "epi", 3)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("cin,cout,s", [(64, 32, 5), (16, 8, 3)])
def test_transposed_form_backward(gpu, cin, cout, s, dtype):
    """the 2-tap replicate-pad form of CausalConvTranspose1d: row 0 of each sample
    also receives W[k=0]^T gpre[0]; the bias gradient (period cout) sums the s phases"""
    from sel import convops as CO
    from sel import hfgops as HF
    T = 9
    gen = torch.Generator().manual_seed(4)
    x = _zeros_in(_rand(gen, (B, T, cin), dtype, gpu))
    w = _rand(gen, (cin, cout, 2 * s), dtype, gpu, (2 * cin) ** -0.5)
    gout = _rand(gen, (B, T, s * cout), dtype, gpu)
    d = HF.make_desc(B * T, T, cin, s * cout, 2, 1, 1, CO.PAD_REPLICATE, bias_period=cout, slope=0.1)
    wp = CO.pack(CO.PACK_CONVT, w.float(), s, dtype)
    gin = HF.bwd_data(d, gout, HF.dgrad_pack(wp, 1), x)
    gwp, gb = HF.wgrad(d, gout, x)
    gw = CO.unpack(CO.PACK_CONVT, gwp, (cin, cout, 2 * s), s)

    a, xd = _act64(x, 0.1)
    at = a.transpose(1, 2)
    w64 = w.cpu().double().requires_grad_(True)
    b64 = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose1d(torch.cat((at[:, :, :1], at), -1), w64, b64, stride=s)[:, :, s:-s].transpose(1, 2)
    (y * gout.cpu().double().view(B, T * s, cout)).sum().backward()
    what = f"convT {cin}->{cout} s{s} {dtype}"
    _check_gin(gin, xd.grad, dtype, what)
    _check_sum(gw, w64.grad, what + " gW")
    _check_sum(gb, b64.grad, what + " gbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_output_form_backward(gpu, dtype):
    """32 -> 1, K = 7, LeakyReLU(0.01), tanh, fp32 out: tanh' from the saved fp32 out"""
    from sel import convops as CO
    from sel import hfgops as HF
    T, C, K = 301, 32, 7
    gen = torch.Generator().manual_seed(5)
    x = _zeros_in(_rand(gen, (B, T, C), dtype, gpu))
    w = _rand(gen, (1, C, K), dtype, gpu, (C * K) ** -0.5)
    bias = _rand(gen, (1,), torch.float32, gpu, 0.1)
    gout = _rand(gen, (B, T, 1), torch.float32, gpu)
    d = HF.make_desc(B * T, T, C, 1, K, 1, K - 1, bias_period=1, slope=0.01, tanh=True)
    lib = CO.L.lib()
    assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), CO._code(dtype), CO.F32, 0) == 0
    assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), CO._code(dtype), CO.F32, 1) == 0
    wp = CO.pack(CO.PACK_FWD, w.float(), 1, dtype)
    out = HF.prim(d, x, wp, bias, out_dtype=torch.float32)
    gin = HF.bwd_data(d, gout, HF.dgrad_pack(wp, 1), x, out)
    gwp, gb = HF.wgrad(d, gout, x, out)
    gw = CO.unpack(CO.PACK_FWD, gwp, (1, C, K), 1)

    a, xd = _act64(x, 0.01)
    w64 = w.cpu().double().requires_grad_(True)
    b64 = bias.cpu().double().requires_grad_(True)
    y = torch.tanh(F.conv1d(F.pad(a.transpose(1, 2), (K - 1, 0)), w64, b64).transpose(1, 2))
    (y * gout.cpu().double()).sum().backward()
    what = f"output conv {dtype}"
    _check_gin(gin, xd.grad, dtype, what)
    _check_sum(gw, w64.grad, what + " gW")
    _check_sum(gb, b64.grad, what + " gbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_wgrad_is_deterministic_and_split_invariant(gpu, dtype):
    """two runs are bit-identical (fixed-order partials, no atomics); the forced
    split counts 1 and 3 (sel_tune key 72; T = 130, B = 2: 6 row tiles) agree to
    1e-6 and each is bit-identical to itself"""
    from sel import convops as CO
    from sel import hfgops as HF
    G, Cg, K, dil, T = 3, 32, 11, 5, 130
    C = N = G * Cg
    gen = torch.Generator().manual_seed(7)
    x = _rand(gen, (B, T, C), dtype, gpu)
    gout = _rand(gen, (B, T, N), dtype, gpu)
    d = HF.make_desc(B * T, T, C, N, K, dil, (K - 1) * dil, CO.PAD_ZERO, G, bias_period=N, slope=0.1)
    lib = CO.L.lib()
    a, b = HF.wgrad(d, gout, x), HF.wgrad(d, gout, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    forced = {}
    prev = lib.sel_tune(TUNE_SPLIT, 0)
    try:
        for n in (1, 3):
            lib.sel_tune(TUNE_SPLIT, n)
            code = CO._code(dtype)
            per = (N * K * Cg + N) * 4
            assert lib.sel_hfg_conv_wgrad_workspace(ctypes.byref(d), code, code) == n * per
            u, v = HF.wgrad(d, gout, x), HF.wgrad(d, gout, x)
            assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])
            forced[n] = u
    finally:
        lib.sel_tune(TUNE_SPLIT, prev)
    assert _rel(forced[3][0], forced[1][0]) <= 1e-6 and _rel(forced[3][1], forced[1][1]) <= 1e-6
    assert _rel(a[0], forced[1][0]) <= 1e-6


def test_streaming_forms_are_unsupported(gpu):
    from sel import convops as CO
    from sel import hfgops as HF
    lib = CO.L.lib()
    for kw in (dict(T_out=5), dict(act_skip=2)):
        d = HF.make_desc(10, 7 if "T_out" in kw else 5, 32, 32, 3, **kw)
        assert lib.sel_hfg_conv_bwd_kernel(ctypes.byref(d), CO.BF16, CO.BF16, 0) == -3
