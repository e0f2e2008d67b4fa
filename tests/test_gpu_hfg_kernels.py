"""The grouped LeakyReLU-fused conv primitive of the HiFi-GAN generator
(csrc/hifigan.hip, sel_hfg_conv_fwd) against an fp64 restatement kept here:
torch.nn.functional.conv1d / conv_transpose1d on the host, the ops the reference
layers call (conv_layer.py:139-142, :180-183).

bf16: the fp64 reference is computed from the SAME bf16 operands, with the
prologue result LeakyReLU(x) rounded to bf16 once (the contract in include/sel.h).
Kernel and reference then both sum exact bf16 products (fp32 vs fp64), and the
kernel rounds its output once, so the bound is the project's for one
bf16-rounded output (tests/test_gpu_c3.py): <= 4e-3 norm-wise and
|a - b| <= 8e-3 |b| + 2e-3 max|b|.  fp32: <= 1e-5 norm-wise, the project's fp32
conv bound (tests/test_gpu_stream.py).

Shapes: B = 2 (leakage across the sample boundary), T = 7 (below the 50-row
reach of K = 11, d = 5) and T = 130 (crosses the 64-row tile and leaves a ragged
tail); per-group widths 6 (zero-padded to the MFMA K step), 32, 64, 128, 256.
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


def _ids(c):
    return "G%d_C%d_K%d_d%d" % c


def _check(out, ref, dtype, what):
    out, ref = out.double().cpu(), ref.cpu()
    rel = float((out - ref).norm() / ref.norm())
    print(f"{what}: rel {rel:.2e}")
    if dtype == torch.float32:
        assert rel <= 1e-5, (what, rel)
        return
    assert rel <= 4e-3, (what, rel)
    tol = 8e-3 * ref.abs() + 2e-3 * ref.abs().max()
    bad = ((out - ref).abs() > tol).sum().item()
    assert bad == 0, (what, bad, float((out - ref).abs().max()))


def _act(x, slope, skip=0):
    """the kernel's prologue: fp32 LeakyReLU of rows >= skip, rounded once to the operand type"""
    xf = x.float()
    a = torch.where(xf >= 0, xf, xf * slope)
    a[:, :skip] = xf[:, :skip]
    return a.to(x.dtype).double()


def _rand(gen, shape, dtype, dev, scale=1.0):
    return (scale * torch.randn(shape, generator=gen)).to(dtype).to(dev)


def _conv_ref(x, w, bias, G, K, dil, slope, shared, res=None, shared_res=False, tanh=False, scale=1.0, prev=None,
              pad=None, skip=0):
    """fp64 restatement on the host; x (B, T, C or C/G) channels-last, w (N, C/G, K)"""
    a = _act(x.cpu(), slope, skip)
    if shared:
        a = a.repeat(1, 1, G)
    pad = (K - 1) * dil if pad is None else pad
    y = F.conv1d(F.pad(a.transpose(1, 2), (pad, 0)), w.cpu().double(), bias.cpu().double(), dilation=dil, groups=G)
    y = y.transpose(1, 2)
    if res is not None:
        r = res.cpu().double()
        y = y + (r.repeat(1, 1, G) if shared_res else r)
    if tanh:
        y = torch.tanh(y)
    y = y * float(torch.tensor(scale, dtype=torch.float32))
    if prev is not None:
        y = y + prev.cpu().double()
    return y


def _run(gpu, dtype, G, Cg, K, dil, T, mode, seed):
    from sel import convops as CO
    from sel import hfgops as HF
    gen = torch.Generator().manual_seed(seed)
    C = N = G * Cg
    shared = mode == "shared"
    epi = mode == "epi"
    x = _rand(gen, (B, T, Cg if shared else C), dtype, gpu)
    w = _rand(gen, (N, Cg, K), dtype, gpu, (Cg * K) ** -0.5)
    bias = _rand(gen, (N,), torch.float32, gpu, 0.1)
    res = _rand(gen, (B, T, Cg if shared else N), dtype, gpu) if mode != "plain" else None
    prev = _rand(gen, (B, T, N), dtype, gpu) if epi else None
    scale = 1.0 / 3.0 if epi else 1.0
    d = HF.make_desc(B * T, T, C, N, K, dil, (K - 1) * dil, CO.PAD_ZERO, G, shared, shared, N, slope=0.1, scale=scale,
                     accumulate=epi)
    if dtype == torch.bfloat16 and Cg > 4:
        assert CO.L.lib().sel_hfg_conv_kernel(ctypes.byref(d), CO.BF16, CO.BF16) in (1, 2, 4)   # the MFMA tile
    wp = CO.pack(CO.PACK_FWD, w.float(), 1, dtype)
    out = HF.prim(d, x, wp, bias, res, prev.clone() if epi else None).view(B, T, N)
    ref = _conv_ref(x, w, bias, G, K, dil, 0.1, shared, res, shared, False, scale, prev)
    _check(out, ref, dtype, f"{mode} G{G} C{Cg} K{K} d{dil} T{T} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_grouped_conv(gpu, case, T, dtype):
    """in_group_stride = C/G: each group reads its own channels."""
    _run(gpu, dtype, *case, T, "plain", 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 3], ids=_ids)
def test_grouped_conv_shared_input(gpu, case, T, dtype):
    """in_group_stride = 0 (and the residual's): MultiGroupConv1d's repeat without the copy."""
    _run(gpu, dtype, *case, T, "shared", 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_grouped_conv_res_and_accumulate(gpu, case, T, dtype):
    """res and the out = out_prev + v * scale epilogue (the MultiReceptiveField average)."""
    _run(gpu, dtype, *case, T, "epi", 3)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("cin,cout,s", [(64, 32, 5), (16, 8, 3)])
def test_transposed_form(gpu, cin, cout, s, dtype):
    """CausalConvTranspose1d (k = 2s) of LeakyReLU(0.1)(x) as the 2-tap
    replicate-pad form; the replicate pad is per sample (B = 2, T = 9)."""
    from sel import convops as CO
    from sel import hfgops as HF
    T = 9
    gen = torch.Generator().manual_seed(4)
    x = _rand(gen, (B, T, cin), dtype, gpu)
    w = _rand(gen, (cin, cout, 2 * s), dtype, gpu, (2 * cin) ** -0.5)
    bias = _rand(gen, (cout,), torch.float32, gpu, 0.1)
    d = HF.make_desc(B * T, T, cin, s * cout, 2, 1, 1, CO.PAD_REPLICATE, bias_period=cout, slope=0.1)
    out = HF.prim(d, x, CO.pack(CO.PACK_CONVT, w.float(), s, dtype), bias).view(B, T * s, cout)
    a = _act(x.cpu(), 0.1).transpose(1, 2)
    ref = F.conv_transpose1d(torch.cat((a[:, :, :1], a), -1), w.cpu().double(), bias.cpu().double(), stride=s)
    _check(out, ref[:, :, s:-s].transpose(1, 2), dtype, f"convT {cin}->{cout} s{s} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_output_form(gpu, dtype):
    """32 -> 1, K = 7, LeakyReLU(0.01) prologue, tanh epilogue, fp32 out: the thin instance."""
    from sel import convops as CO
    from sel import hfgops as HF
    T, C, K = 301, 32, 7
    gen = torch.Generator().manual_seed(5)
    x = _rand(gen, (B, T, C), dtype, gpu)
    w = _rand(gen, (1, C, K), dtype, gpu, (C * K) ** -0.5)
    bias = _rand(gen, (1,), torch.float32, gpu, 0.1)
    d = HF.make_desc(B * T, T, C, 1, K, 1, K - 1, bias_period=1, slope=0.01, tanh=True)
    assert CO.L.lib().sel_hfg_conv_kernel(ctypes.byref(d), CO._code(dtype), CO.F32) == 0
    out = HF.prim(d, x, CO.pack(CO.PACK_FWD, w.float(), 1, dtype), bias, out_dtype=torch.float32).view(B, T, 1)
    assert out.dtype == torch.float32
    ref = _conv_ref(x, w, bias, 1, K, 1, 0.01, False, tanh=True)
    _check(out, ref, dtype, f"output conv {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_streaming_form(gpu, dtype):
    """T_out < T with pad 0 and act_skip: the valid conv of cat(activated
    buffer, new rows) of a streaming step (conv_layer.py:144-147), 5 new rows
    behind a 50-row buffer, per sample."""
    from sel import convops as CO
    from sel import hfgops as HF
    G, Cg, K, dil, Tn = 3, 32, 11, 5, 5
    P = (K - 1) * dil
    C = N = G * Cg
    gen = torch.Generator().manual_seed(6)
    x = _rand(gen, (B, P + Tn, C), dtype, gpu)
    w = _rand(gen, (N, Cg, K), dtype, gpu, (Cg * K) ** -0.5)
    bias = _rand(gen, (N,), torch.float32, gpu, 0.1)
    res = _rand(gen, (B, Tn, N), dtype, gpu)
    d = HF.make_desc(B * Tn, P + Tn, C, N, K, dil, 0, CO.PAD_ZERO, G, bias_period=N, act_skip=P, slope=0.1, T_out=Tn)
    out = HF.prim(d, x, CO.pack(CO.PACK_FWD, w.float(), 1, dtype), bias, res).view(B, Tn, N)
    ref = _conv_ref(x, w, bias, G, K, dil, 0.1, False, res, pad=0, skip=P)
    _check(out, ref, dtype, f"streaming form {dtype}")


# ---- fused residual layer (sel_hfg_reslayer_fwd) -----------------------------------------------
class _tune:
    """sel_tune key 71 for the duration of a block: 1 = two launches, 2 = fused wherever it applies"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from sel import _lib
        self.prev = _lib.lib().sel_tune(71, self.value)

    def __exit__(self, *exc):
        from sel import _lib
        _lib.lib().sel_tune(71, self.prev)


def _layers(gpu, C, K, dil, G, seed):
    from layers.conv_layer import CausalConv1d
    torch.manual_seed(seed)
    l1 = CausalConv1d(C, C, K, dilation=dil, groups=G)
    l2 = CausalConv1d(C, C, K, dilation=1, groups=G)
    with torch.no_grad():
        for l in (l1, l2):
            l.conv.bias.normal_(0.0, 0.1)
    return l1.to(gpu), l2.to(gpu)


@pytest.mark.parametrize("T", [7, 130])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("dil", [1, 5])
@pytest.mark.parametrize("K", [3, 7, 11])
@pytest.mark.parametrize("Cg", [32, 64])
def test_fused_reslayer(gpu, Cg, K, dil, G, T):
    """out = x + conv2_{K,1}(lrelu(conv1_{K,d}(lrelu(x)) + b1)) + b2 in one launch,
    held to the fp64 bound (h rounded to bf16 where the first of two launches
    stores it: part of the contract) and compared with the two-launch path.

    The two are BIT-IDENTICAL, not merely both inside the bound: per output the
    fused kernel issues the same MFMA sequence as k_hfg_mfma (taps outer,
    32-channel steps inner, one LDS pass since C/G <= 64), rounds h to bf16 and
    its LeakyReLU to bf16 exactly where the two launches do, and shares their
    epilogue code.  G = 3 with dil = 5 runs the shared-input form
    (in_group_stride 0), K = 7 the scale-accumulate epilogue."""
    from sel import hfgops as HF
    C = G * Cg
    shared = G == 3 and dil == 5
    accum = K == 7
    l1, l2 = _layers(gpu, C, K, dil, G, 100 + K)
    gen = torch.Generator().manual_seed(8)
    x = _rand(gen, (B, T, Cg if shared else C), torch.bfloat16, gpu)
    prev = _rand(gen, (B, T, C), torch.bfloat16, gpu) if accum else None
    kw = dict(scale=1.0 / 3.0, out=None) if accum else {}
    with torch.no_grad():
        with _tune(2):
            if accum:
                kw["out"] = prev.clone()
            fused = HF.reslayer(x, l1, l2, 0.1, shared, **kw)
        assert fused is not None
        with _tune(1):
            if accum:
                kw["out"] = prev.clone()
            assert HF.reslayer(x, l1, l2, 0.1, shared, **kw) is None
            h = HF.causal(x, l1, 0.1, shared_in=shared)
            two = HF.causal(h, l2, 0.1, res=x, shared_res=shared, **kw)
    assert torch.equal(fused, two)
    w1, w2 = (l.conv.weight.detach().bfloat16() for l in (l1, l2))
    href = _conv_ref(x, w1, l1.conv.bias.detach(), G, K, dil, 0.1, shared).to(torch.bfloat16)
    ref = _conv_ref(href, w2, l2.conv.bias.detach(), G, K, 1, 0.1, False, x, shared, False,
                    1.0 / 3.0 if accum else 1.0, prev)
    _check(fused, ref, torch.bfloat16, f"fused C{Cg} K{K} d{dil} G{G} T{T}")


def test_fused_reslayer_dispatcher(gpu):
    """SEL_ERR_UNSUPPORTED for C/G = 128 (the wide stages stay on two launches), for fp32,
    and for everything under tune key 71 = 1."""
    from sel import convops as CO
    from sel import hfgops as HF
    l1, l2 = _layers(gpu, 128, 7, 1, 1, 9)
    x = _rand(torch.Generator().manual_seed(9), (B, 7, 128), torch.bfloat16, gpu)
    out = torch.empty_like(x)
    d = HF.make_desc(B * 7, 7, 128, 128, 7, 1, 6, bias_period=128, slope=0.1)
    w1, w2 = HF.packed(l1.conv, CO.PACK_FWD, 1, x.dtype), HF.packed(l2.conv, CO.PACK_FWD, 1, x.dtype)
    lib = CO.L.lib()
    args = (CO.L.ptr(x), CO.L.ptr(w1), CO.L.ptr(l1.conv.bias), CO.L.ptr(w2), CO.L.ptr(l2.conv.bias), CO.L.ptr(out),
            CO.L.stream())
    with _tune(2):
        assert lib.sel_hfg_reslayer_fwd(ctypes.byref(d), CO.BF16, *args) == -3
        assert HF.reslayer(x, l1, l2, 0.1) is None
        l1, l2 = _layers(gpu, 64, 7, 1, 1, 9)
        assert HF.reslayer(x[..., :64].contiguous().float(), l1, l2, 0.1) is None   # fp32: two launches
        assert HF.reslayer(x[..., :64].contiguous(), l1, l2, 0.1) is not None
    with _tune(1):
        assert HF.reslayer(x[..., :64].contiguous(), l1, l2, 0.1) is None
