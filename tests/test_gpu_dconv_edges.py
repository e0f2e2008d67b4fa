"""The discriminator conv kernels (csrc/dconv.hip, csrc/dconv_wgrad.hip, and
conv.hip's warp-specialised kernels behind dconv_ws_fwd) against fp64 torch at their dispatch edges: every
case of tests/dconv_cases.py x {bf16, fp32} through the forward (bias +
LeakyReLU), the adjoint (plain, and with (+ res) * LeakyReLU'(aux)) and the
weight / bias gradient, each held to the bounds derived in that module's
docstring, element by element.  Each test first asserts the kernel names its
case is there for (the library's own reporters), so a dispatch change cannot
move a case onto another kernel unnoticed.  The layout variants check the
contract of include/sel.h: input rows [Tv, Tvs) are not read (they hold 1e3),
output rows [Tvalid, Tvo) come back as exact zeros, and the columns between
the used width and the row pitch are not read (input) and not written (output).

The GAN loss terms (k_gan_reduce* / k_gan_grad*, all five kinds) are checked on
(B, C, T) views of channels-last maps, the 16-B vector and the per-element
kernels both, at a size inside one grid sweep and one just past it."""
import pytest
import torch

import dconv_cases as C

pytestmark = pytest.mark.gpu

_SLOT = {}  # the operands and references of ONE (case, dtype), shared by its tests


def _setup(gpu, name, dtype):
    key = (name, dtype)
    if _SLOT.get("key") != key:
        _SLOT.clear()
        case = C.BY_NAME[name]
        op = C.Operands(case, C.BF16 if dtype == "bf16" else C.F32, gpu)
        _SLOT.update(key=key, op=op, ref=C.reference(op))
    return _SLOT["op"], _SLOT["ref"]


def _check(op, got, ref, S, n, what):
    if op.dt == C.BF16:
        return C.check_bf16(got, ref, what)
    return C.check_f32(got, ref, S, n, what)


def _forward(op, ref, tag):
    from sel import dconvops as DC
    case, df = op.case, op.df
    y = op.out_fwd()
    DC.prim(df, op.x, DC.pack(op.sp, op.w, None, op.dt, 0), y, bias=op.b)
    torch.cuda.synchronize()
    _check(op, y[:, :op.T_out, :case.cout], ref["y"], ref["S_y"], df.K * df.S * df.Cg, f"{tag} forward")
    assert torch.count_nonzero(y[:, op.T_out:, :case.cout]).item() == 0, "rows [Tvalid, Tvo) must be zeros"
    assert bool((y[:, :, case.cout:] == C.OUT_FILL).all()), "columns past the used width were written"


def _adjoint(op, ref, tag):
    from sel import dconvops as DC
    case, da = op.case, op.da
    cols = case.stride * case.cin
    n = da.K * da.S * da.Cg
    wd = DC.pack(op.sp, op.w, None, op.dt, 1)
    for epi in (False, True):
        gin = op.out_adj()
        DC.prim(da, op.g_adj, wd, gin, aux=op.aux if epi else None, res=op.res if epi else None)
        torch.cuda.synchronize()
        k = "gin_epi" if epi else "gin"
        _check(op, gin[:, :da.Tvalid, :cols], ref[k], ref["S_" + k], n, f"{tag} adjoint{' + epilogue' if epi else ''}")
        assert torch.count_nonzero(gin[:, da.Tvalid:, :cols]).item() == 0, "rows [Tvalid, Tvo) must be zeros"
        assert bool((gin[:, :, cols:] == C.OUT_FILL).all()), "columns past the used width were written"


def _wgrad_limits(op, ref):
    """Norm-wise limits (weight, bias) of the case: 1e-5 up to 4096 rows, else
    4 x the error of a plain fp32 torch evaluation of the same sums, capped at 1e-4."""
    rows = op.case.Bs * op.T_out
    if rows <= C.WG_NORM_ROWS:
        return 1e-5, 1e-5
    r32 = C.reference(op, dtype=torch.float32, with_abs=False)
    ew, eb = C._rel(r32["gw"], ref["gw"]), C._rel(r32["gb"], ref["gb"])
    print(f"plain fp32 torch weight gradient over {rows} rows: norm-wise {ew:.3e} (bias {eb:.3e})")
    return C.wgrad_norm_limit(rows, ew), C.wgrad_norm_limit(rows, eb)


def _check_wgrad(op, ref, gw, gb, tag):
    from sel import dconvops as DC
    rows = op.case.Bs * op.T_out
    name, (nsplit, _per, bsplit, _flat) = DC.wgrad_kernel(op.df, op.dt)
    lw, lb = _wgrad_limits(op, ref)
    C.check_wgrad(gw, ref["gw"], ref["S_gw"], rows, nsplit, f"{tag} weight gradient ({name})", lw)
    C.check_wgrad(gb, ref["gb"], ref["S_gb"], rows, bsplit, f"{tag} bias gradient", lb)


def _wgrad(op, ref, tag):
    """(k65: k_dwgrad_mfma takes K = 65 as nine tap groups of <= WG_TAPS = 8 taps,
    one per blockIdx.z % ntg; a block stages span = WG_BM + kn - 1 <= 71 input
    rows for ITS kn <= 8 taps into the xs tile of (WG_BM + WG_TAPS - 1) * 48
    elements the launcher sizes, and indexes it by rr < span and k < kn only;
    K enters through k0 = 8 * group in global addresses (masked by 0 <= t < Tv)
    and the partials' [o][K][nred] index.  No LDS span depends on K, so K > 64,
    which only mfma_ok of the forward excludes, stays inside them.)"""
    from sel import dconvops as DC
    gw, _, gb = DC.wgrad(op.sp, op.df, op.g_wg, op.x, op.w, None, True, True)
    torch.cuda.synchronize()
    _check_wgrad(op, ref, gw, gb, tag)


@pytest.mark.parametrize("what", ["forward", "adjoint", "wgrad"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_dconv_edge_case(gpu, name, dtype, what):
    case = C.BY_NAME[name]
    assert C.names_of(case) == case.names
    op, ref = _setup(gpu, name, dtype)
    {"forward": _forward, "adjoint": _adjoint, "wgrad": _wgrad}[what](op, ref, f"{name} {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_wgrad_pending_two_layers(gpu, dtype):
    """Two layers' partials queued, their final reductions in one launch."""
    from sel import dconvops as DC
    pending, outs = [], []
    for name in ("w3_strided", "shortx6"):
        case = C.BY_NAME[name]
        op = C.Operands(case, C.BF16 if dtype == "bf16" else C.F32, gpu, seed=1)
        gw, _, gb = DC.wgrad(op.sp, op.df, op.g_wg, op.x, op.w, None, True, True, pending)
        outs.append((op, gw, gb))
    assert len(pending) == 2
    DC.finish_pending(pending)
    torch.cuda.synchronize()
    for op, gw, gb in outs:
        _check_wgrad(op, C.reference(op), gw, gb, f"{op.case.name} {dtype} pending")


# ---------------------------------------------------------------- GAN terms
SWEEP = 8192 * 256     # threads of one grid sweep of launch_blocks


def _off_kinks(a):
    """Keep |a - 1| and |a + 1| above 2^-6: the hinge terms' kinks."""
    return torch.where((a.abs() - 1).abs() <= 2.0 ** -6, torch.full_like(a, 0.5), a)


GAN_KINDS = ("hinge_real", "hinge_fake", "neg_mean", "mse_to", "l1_mean")


def _gan_call(DC, kind, a, b):
    if kind == "hinge_real":
        return DC.hinge(a, True)
    if kind == "hinge_fake":
        return DC.hinge(a, False)
    if kind == "neg_mean":
        return DC.neg_mean(a)
    if kind == "mse_to":
        return DC.mse_to(a, 1.0)
    return DC.l1_mean(a, b, 0.5)


def _gan_ref(kind, a, b):
    """(value, |term| per element) in the dtype of a (fp64)."""
    if kind == "hinge_real":       # -mean min(a - 1, 0)
        t = torch.relu(1 - a)
    elif kind == "hinge_fake":     # -mean min(-a - 1, 0)
        t = torch.relu(1 + a)
    elif kind == "neg_mean":
        return -a.mean(), a.detach().abs()
    elif kind == "mse_to":
        t = (a - 1) ** 2
    else:
        t = 0.5 * (a - b).abs()
    return t.mean(), t.detach()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape",
                         [(3, 517, 64), (3, 517, 60), (1, (SWEEP * 8 + 40) // 8, 8), (1, (SWEEP + 40) // 3, 3)],
                         ids=["vector", "per_element", "vector_wrap", "per_element_wrap"])
def test_gan_terms(gpu, shape, dtype):
    """hinge(a, real / fake) = -mean min(+-a - 1, 0), neg_mean, mse_to, l1_mean on
    (B, C, T) views of channels-last (B, T, C) maps against fp64 torch, values
    and gradients (upstream gradient 2.5).  C % 8 == 0 takes the 16-B vector
    kernels, else the per-element ones; the *_wrap sizes are 40 elements past one
    grid sweep (8192 blocks x 256 threads x 8 elements for the bf16 vector form).

    Value bound: a thread sums its m terms in fp32 (then fp64 across threads):
    (m + 4) 2^-23 x scale x sum |term|, plus the fp32 rounding of the result.
    Gradient bound per element: fp32 4 x 2^-24 |ref| (three roundings), bf16 2^-8
    |ref| (one bf16 rounding, factor 2).  Kinks: the kernels give gradient 0 AT
    the kink (hinge: a = +-1 counts as inactive; L1: a = b); that convention is
    not torch's business, so the inputs stay 2^-6 off the hinge kinks and a != b."""
    from sel import dconvops as DC
    B, T, Cc = shape
    dt = C.BF16 if dtype == "bf16" else C.F32
    gen = torch.Generator(device=gpu).manual_seed(B * 31 + Cc)
    fa = _off_kinks(torch.randn(B, T, Cc, generator=gen, device=gpu).to(dt))
    fb = torch.randn(B, T, Cc, generator=gen, device=gpu).to(dt)
    fb = torch.where(fb == fa, fb + 1, fb)
    a64, b64 = fa.permute(0, 2, 1).double(), fb.permute(0, 2, 1).double()
    n = fa.numel()
    V = 16 // fa.element_size()
    V = V if Cc % V == 0 else 1        # fp32 at C = 60 is a vector case too (4 elements per 16 B)
    units = n // V
    blocks = max(1, min(-(-units // 256), 8192))
    m = -(-units // (blocks * 256)) * V
    assert (units > SWEEP) == (T > 1000)
    for kind in GAN_KINDS:
        a = fa.permute(0, 2, 1).detach().requires_grad_(True)
        out = _gan_call(DC, kind, a, fb.permute(0, 2, 1))
        ar = a64.clone().requires_grad_(True)
        ref_g, terms = _gan_ref(kind, ar, b64)
        ref = ref_g.detach()
        allowed = (m + 4) * C.EPS32 * terms.sum().item() / n + 2.0 ** -24 * abs(ref.item())
        err = abs(out.item() - ref.item())
        print(f"{kind} {dtype} {shape}: value {out.item():.8e} ref {ref.item():.8e} err {err:.2e} "
              f"allowed {allowed:.2e}")
        assert err <= allowed, (kind, out.item(), ref.item(), err, allowed)
        (2.5 * out).backward()
        (2.5 * ref_g).backward()
        tol = 2.0 ** -8 if dt == C.BF16 else 4 * 2.0 ** -24
        diff = (a.grad.double() - ar.grad).abs()
        worst = (diff / (tol * ar.grad.abs()).clamp_min(1e-300)).max().item()
        print(f"{kind} {dtype} {shape}: gradient worst element / allowed {worst:.3f}")
        assert bool((diff <= tol * ar.grad.abs()).all()), (kind, worst)
