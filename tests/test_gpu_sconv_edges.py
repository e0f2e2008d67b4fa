"""GPU checks of the channels-last 2-D conv kernels (sconv2d.hip) where the
layer cases of tests/test_gpu_univnet.py do not reach: several output rows per
weight-gradient split (uneven splits, a split across a sample boundary), Cin !=
Cout, the accepted small kernel geometries, and the writes themselves.  The
cases and their CPU references are tests/sconv_cases.py; that each case has
the shape property it is named for is asserted there (and without a GPU by
tests/test_sconv_cases_host.py).

A  random values against F.conv2d in fp64 on the CPU, at the project's layer
   bounds (fp32 1e-5 forward, 1e-4 gradients; bf16 1e-2 / 2e-2, norm-wise), and
   for the fp32 C -> C forward the derived per-element rounding bound
   |y - ref| <= (n + 2) 2^-24 A + 2^-23 |ref|, n = kh kw Cin, A = conv2d(|x|, |w|, |b|).
B  exact arithmetic: inputs for which every partial sum in any order is an fp32
   number, so the outputs are compared bit for bit, in fp32 and in bf16 (where
   the forward needs both bf16 terms of its weights to get there).
C  the raw entry points writing into NaN-filled regions between sentinel
   guard bands: every element written, nothing beyond.
"""
import ctypes

import pytest
import torch

import sconv_cases as C
from sconv_cases import _cl

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _run(SC, gpu, case, leaky, x, wf, wa, b, gy, slope, dt):
    """forward, data gradient and weight gradient (twice) of one layer case from
    torch-layout CPU tensors"""
    B, H, W, ci, co, k, s = case
    sp = SC.LayerSpec(ci, co, k, s, leaky)
    xg = _cl(x).to(gpu).to(SC._in_dtype(sp, dt))
    gyg = _cl(gy).to(gpu).to(SC._out_dtype(sp, dt))
    wfg, wag = wf.float().to(gpu), wa.float().to(gpu)
    y = SC.conv_fwd(sp, xg, SC._pack_fwd(sp, wfg, dt), b.float().to(gpu), slope, dt)
    gx = SC.conv_bwd_data(sp, gyg, SC._pack_adj(sp, wag, dt), xg if ci != 1 else None, xg.shape, slope, dt)
    gw, gb = SC.conv_wgrad(sp, gyg, xg, slope, dt)
    gw2, gb2 = SC.conv_wgrad(sp, gyg, xg, slope, dt)
    assert y.dtype == SC._out_dtype(sp, dt) and gx.dtype == SC._in_dtype(sp, dt)
    assert gw.dtype == gb.dtype == torch.float32
    return sp, y, gx, gw, gb, gw2, gb2


# ---------------------------------------------------------------------------
# A. random values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(C.EDGE_CASES))
def test_edge_case_matches_conv2d(gpu, name, dtype):
    from sel import sconvops as SC
    case = C.EDGE_CASES[name]
    B, H, W, ci, co, k, s = case
    C.check_properties(name, case)
    r = C.layer_ref(name, case)
    dt = DT[dtype]
    tol_f, tol_g = (1e-5, 1e-4) if dtype == "fp32" else (1e-2, 2e-2)
    sp, y, gx, gw, gb, gw2, gb2 = _run(SC, gpu, case, r["leaky"], r["x"], r["w"], r["w"], r["b"], r["gpre"],
                                       C.SLOPE, dt)
    assert tuple(y.shape) == tuple(_cl(r["y"]).shape) and tuple(gx.shape) == tuple(_cl(r["gx"]).shape)
    assert tuple(gw.shape) == tuple(r["gw"].shape) and tuple(gb.shape) == tuple(r["gb"].shape)
    e = {"fwd": C.rel(y, _cl(r["y"])), "gx": C.rel(gx, _cl(r["gx"])), "gw": C.rel(gw, r["gw"]),
         "gb": C.rel(gb, r["gb"])}
    ratio = None
    if dtype == "fp32" and ci != 1 and co != 1:
        n = k[0] * k[1] * ci
        ref = _cl(r["y"])
        bound = (n + 2) * 2.0 ** -24 * _cl(C.abs_conv(r, case)) + 2.0 ** -23 * ref.abs()
        err = (y.double().cpu() - ref).abs()
        ratio = float((err / bound).max())
    print(name, dtype, {k_: f"{v:.2e}" for k_, v in e.items()},
          "" if ratio is None else f"worst per-element error / bound {ratio:.3f}")
    assert all(bool(torch.isfinite(t).all()) for t in (y, gx, gw, gb))
    assert e["fwd"] <= tol_f, e
    assert e["gx"] <= tol_g and e["gw"] <= tol_g and e["gb"] <= tol_g, e
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)       # fixed-order reduction
    if ratio is not None:
        # (sample, row, column, channel) of the first elements beyond the bound
        assert bool((err <= bound).all()), (ratio, (err > bound).nonzero()[:6].tolist())
    if s[1] == 2 and (W - k[1]) % 2 == 1:                      # the column no tap reads: exactly zero
        assert float(r["gx"][:, :, :, -1].abs().max()) == 0.0
        assert float(gx[:, :, -1, :].float().abs().max()) == 0.0


# ---------------------------------------------------------------------------
# B. exact arithmetic, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(C.EXACT_CASES))
def test_exact_case_is_bit_equal(gpu, name, dtype):
    """Integers in [-2, 2], weights k 2^-12 (forward) and k 2^-7 (data gradient),
    slope 0.25: every partial sum is an fp32 number whatever the split, tile or
    MFMA layout, so any difference from the reference is a wrong or missing
    term, never rounding.  In bf16 the forward's reference is the bf16 rounding
    of the exact value, which one bf16 term of the weights misses on ~40 % of
    the outputs (asserted >= 25 % by sconv_cases.exact_case)."""
    from sel import sconvops as SC
    case = C.EXACT_CASES[name]
    B, H, W, ci, co, k, s = case
    if name in C.EDGE_CASES:
        C.check_properties(name, case)
    e = C.exact_case(name, case)
    dt = DT[dtype]
    sp, y, gx, gw, gb, gw2, gb2 = _run(SC, gpu, case, e["leaky"], e["x"], e["wf"], e["wa"], e["b"], e["gy"],
                                       C.EXACT_SLOPE, dt)
    tag = "32" if dtype == "fp32" else "16"
    pairs = {"y": (y.double().cpu(), _cl(e["y" + tag])), "gx": (gx.double().cpu(), _cl(e["gx" + tag])),
             "gw": (gw.double().cpu(), e["gw"]), "gb": (gb.double().cpu(), e["gb"])}
    report = [C.describe_mismatch(kind, got, ref, case) for kind, (got, ref) in pairs.items()
              if not torch.equal(got, ref)]
    print(name, dtype, "bit-equal" if not report else "\n".join(report))
    assert not report, "\n".join(report)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)


# ---------------------------------------------------------------------------
# C. the writes
# ---------------------------------------------------------------------------
SENTINEL = 12345.0


class _Guarded:
    """An output region of n elements, NaN-filled, between two sentinel bands of
    `guard` elements (a multiple of 64, so the region keeps 16-byte alignment)."""

    def __init__(self, shape, dtype, guard, device):
        self.shape = tuple(shape)
        self.n = 1
        for v in self.shape:
            self.n *= v
        self.guard = (max(guard, 256) + 63) // 64 * 64
        self.buf = torch.full((self.n + 2 * self.guard,), SENTINEL, dtype=dtype, device=device)
        self.buf[self.guard:self.guard + self.n] = float("nan")
        self.sentinel = self.buf[:self.guard].clone()
        assert self.region.data_ptr() % 16 == 0 and bool(torch.isnan(self.region).all())

    @property
    def region(self):
        return self.buf[self.guard:self.guard + self.n]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.region.data_ptr())

    def check(self, what, want):
        out = self.region.view(self.shape)
        assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).sum())} elements not written"
        assert torch.equal(out, want), what
        assert torch.equal(self.buf[:self.guard], self.sentinel), f"{what}: wrote before the tensor"
        assert torch.equal(self.buf[self.guard + self.n:], self.sentinel), f"{what}: wrote beyond the tensor"


def _operands(SC, gpu, name, dt):
    case = C.EDGE_CASES.get(name) or C.LAYER_CASES[name]
    B, H, W, ci, co, k, s = case
    r = C.layer_ref(name, case)
    sp = SC.LayerSpec(ci, co, k, s, r["leaky"])
    x = _cl(r["x"]).to(gpu).to(SC._in_dtype(sp, dt))
    gy = _cl(r["gpre"]).to(gpu).to(SC._out_dtype(sp, dt))
    return case, sp, x, gy, r["w"].to(gpu), r["b"].to(gpu)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tile_plus", "k2x4_s2"])
def test_forward_writes_its_output_and_nothing_else(gpu, name, dtype):
    from sel import _lib as L
    from sel import sconvops as SC
    from sel.convops import _code
    dt = DT[dtype]
    case, sp, x, gy, w, b = _operands(SC, gpu, name, dt)
    B, H, W = case[:3]
    wp = SC._pack_fwd(sp, w, dt)
    want = SC.conv_fwd(sp, x, wp, b, C.SLOPE, dt)
    Ho, Wo = C.out_hw(case)
    assert Wo % C.TILE != 0                                     # the partial last tile
    out = _Guarded(want.shape, want.dtype, Wo * sp.cout, gpu)
    d = sp.desc(B, H, W, C.SLOPE)
    L.call("sel_sconv_fwd", ctypes.byref(d), _code(dt), L.ptr(x), L.ptr(wp), L.ptr(b), out.ptr, L.stream())
    out.check("y", want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["s2_odd_tail", "k1x2_s2", "k2x4_s2", "first_k2x4_s2", "last_k1x1"])
def test_data_gradient_writes_its_output_and_nothing_else(gpu, name, dtype):
    """The stride-2 data gradient is one launch per column phase, each writing
    every second column; the column no tap reads is written too (with zeros)."""
    from sel import _lib as L
    from sel import sconvops as SC
    from sel.convops import _code
    dt = DT[dtype]
    case, sp, x, gy, w, b = _operands(SC, gpu, name, dt)
    B, H, W = case[:3]
    wa = SC._pack_adj(sp, w, dt)
    aux = x if sp.cin != 1 else None
    want = SC.conv_bwd_data(sp, gy, wa, aux, x.shape, C.SLOPE, dt)
    out = _Guarded(want.shape, want.dtype, W * sp.cin, gpu)
    d = sp.desc(B, H, W, C.SLOPE)
    L.call("sel_sconv_bwd_data", ctypes.byref(d), _code(dt), L.ptr(gy), L.ptr(wa), L.ptr(aux), out.ptr, L.stream())
    out.check("gx", want)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["wg_rows_2", "cin_gt_cout", "wg_first_rows", "wg_last_rows"])
def test_weight_gradient_writes_its_outputs_and_nothing_else(gpu, name, dtype, with_bias):
    """gw, gb and the workspace of exactly the stated size, each between guard
    bands; again with gb = None, which must leave gw unchanged."""
    from sel import _lib as L
    from sel import sconvops as SC
    from sel.convops import _code
    dt = DT[dtype]
    case, sp, x, gy, w, b = _operands(SC, gpu, name, dt)
    B, H, W = case[:3]
    want_gw, want_gb = SC.conv_wgrad(sp, gy, x, C.SLOPE, dt)
    d = sp.desc(B, H, W, C.SLOPE)
    nbytes = L.lib().sel_sconv_wgrad_workspace(ctypes.byref(d), _code(dt))
    R, cap, rng = C.wg_ranges(case)
    assert nbytes == len(rng) * (want_gw.numel() + sp.cout) * 4
    gw = _Guarded(want_gw.shape, torch.float32, sp.cin * sp.kh * sp.kw, gpu)
    gb = _Guarded(want_gb.shape, torch.float32, sp.cout, gpu)
    ws = _Guarded((nbytes // 4,), torch.float32, 4096, gpu)
    L.call("sel_sconv_wgrad", ctypes.byref(d), _code(dt), L.ptr(gy), L.ptr(x), gw.ptr, gb.ptr if with_bias else None,
           ws.ptr, nbytes, L.stream())
    gw.check("gw", want_gw)
    if with_bias:
        gb.check("gb", want_gb)
    else:
        assert bool(torch.isnan(gb.region).all())
    # every partial the finishing kernel sums was written, and none beyond the stated size
    assert bool(torch.isfinite(ws.region).all())
    assert torch.equal(ws.buf[:ws.guard], ws.sentinel) and torch.equal(ws.buf[ws.guard + ws.n:], ws.sentinel)
