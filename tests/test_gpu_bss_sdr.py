"""GPU checks of the BSS-eval SDR against the fp64 restatement
tests/bss_sdr_ref.py: the correlations sel_bss_sdr hands to its solve at every
shape edge (T around 1, L and the correlation chunk; L around the wave sizes;
both zero_mean settings under a DC offset, where a sample past T must be zero
and not -mean), the values of the shared recipe, the degenerate rows, the
plumbing (optional outputs, an unaligned view, graph replay, run-to-run bits)
and the Python forms.

Bounds.  Four times the largest deviation seen on the MI355X, rounded up to one
significant figure, and never above the caps of the definition: 1e-12 absolute
on the correlations (values in [-1, 1]; a relative 1e-7 on them moves the value
by up to 0.1 dB, so 1e-12 keeps that under 1e-6 dB) and 1e-3 dB on the values.
The measured figures are in DESIGN §23.5; each test prints its own before it
asserts.
"""
import numpy as np
import pytest
import torch

import bss_sdr_ref as BR

pytestmark = pytest.mark.gpu

# largest |GPU - fp64| seen on the MI355X, x4, one significant figure up:
# correlations 2.554e-15; values 1.853e-06 dB (half an ulp of the fp32 result at 30 dB)
CORR_BOUND = 2e-14
DB_BOUND = 8e-6
assert CORR_BOUND <= 1e-12 and DB_BOUND <= 1e-3

_ROWS = [("white", 10, 0), ("ar2", 30, 1), ("voiced", 0, 0)]    # rows of one batch differ in content


def _L():
    from sel import _lib as L
    return L


def _C():
    return int(_L().load().sel_bss_sdr_chunk())


def _run(pred, target, L, zero_mean=False, load_diag=0.0, want_mean=True, want_corr=True):
    """sel_bss_sdr on (B, T) device tensors -> (vals, mean, corr), the outputs pre-filled with sentinels."""
    S = _L()
    B, T = pred.shape
    dev = pred.device
    ws = S.workspace(S.lib().sel_bss_sdr_workspace(B, T, L), dev)
    vals = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    mean = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    corr = torch.full((B, 2, L), -7.0, dtype=torch.float64, device=dev)
    S.call("sel_bss_sdr", S.ptr(pred), S.ptr(target), B, T, L, int(zero_mean), float(load_diag), S.ptr(vals),
           S.ptr(mean) if want_mean else None, S.ptr(corr) if want_corr else None, S.ptr(ws), ws.numel(), S.stream())
    torch.cuda.synchronize()
    return vals, mean, corr


def _pairs(rows, T, dc=False):
    """(B, T) fp32 numpy (pred, target); with dc the offsets 0.05 and 0.02 are added in fp32."""
    p = np.stack([BR.case(*r, T)[0] for r in rows])
    t = np.stack([BR.case(*r, T)[1] for r in rows])
    if dc:
        p, t = p + np.float32(0.05), t + np.float32(0.02)
    return p, t


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _corr_shapes(L, C):
    Ts = []
    for T in (1, 2, 3, L - 1, L, L + 1, C - 1, C, C + 1, C + L - 2, C + L - 1, C + L, 3 * C + 17):
        if T >= 1 and T not in Ts:
            Ts.append(T)
    return Ts


# ---- correlations ------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 511, 512])
def test_correlations_match_fp64_reference(gpu, L):
    C = _C()
    worst = 0.0
    for T in _corr_shapes(L, C):
        for B in (1, 3):
            p, t = _pairs(_ROWS[:B], T, dc=True)
            pd, td = _dev(p, gpu), _dev(t, gpu)
            for zm in (False, True):
                _, _, corr = _run(pd, td, L, zm)
                got = corr.cpu().numpy()
                for j in range(B):
                    r, b = BR.corr_ref(p[j], t[j], L, zm)
                    dev = max(np.abs(got[j, 0] - r).max(), np.abs(got[j, 1] - b).max())
                    worst = max(worst, dev)
                    assert np.isfinite(got[j]).all() and dev <= CORR_BOUND, (T, B, zm, j, dev)
                if T < L:       # linear correlations: lags at or past T are exactly zero
                    assert not got[:, :, T:].any(), (T, L, zm)
    print(f"BSS-CORR L={L} max|corr - ref|={worst:.3e}")


def test_correlations_with_load_diag(gpu):
    C = _C()
    p, t = _pairs(_ROWS, C + 65, dc=True)
    _, _, c0 = _run(_dev(p, gpu), _dev(t, gpu), 65, True, 0.0)
    vals, _, c1 = _run(_dev(p, gpu), _dev(t, gpu), 65, True, 1e-6)
    got = c1.cpu().numpy()
    for j in range(3):
        r, b = BR.corr_ref(p[j], t[j], 65, True, 1e-6)
        assert max(np.abs(got[j, 0] - r).max(), np.abs(got[j, 1] - b).max()) <= CORR_BOUND
        want = BR.sdr_full(p[j], t[j], 65, True, 1e-6, want_cond=False)["val"]
        assert abs(float(vals[j]) - want) <= DB_BOUND, (j, float(vals[j]), want)
    c0, c1 = c0.cpu(), c1.cpu()
    assert torch.equal(c0[:, 0, 1:], c1[:, 0, 1:]) and torch.equal(c0[:, 1], c1[:, 1])
    assert torch.equal(c1[:, 0, 0], c0[:, 0, 0] + 1e-6)


# ---- values --------------------------------------------------------------------
def _check_values(got, want, what):
    """|GPU - ref| over the finite reference values; a reference of +inf (1 - coh <= 0) asks for +inf or
    at least 120 dB, one of -inf (a silent prediction) for -inf."""
    worst = 0.0
    for g, w in zip(got, want):
        if w == np.inf:
            assert g == np.inf or (np.isfinite(g) and g >= 120.0), (what, g, w)
        elif w == -np.inf:
            assert g == -np.inf, (what, g, w)
        else:
            assert np.isfinite(g), (what, g, w)
            worst = max(worst, abs(float(g) - w))
    return worst


def _value_ids():
    try:
        return BR.value_shapes(_C())
    except Exception:       # no library at collection time: the test itself then fails on it
        return BR.value_shapes(2048)


@pytest.mark.parametrize("T,L", _value_ids())
def test_values_match_fp64_reference(gpu, T, L):
    rows = BR.ALL_CASES
    p, t = _pairs(rows, T)
    vals, mean, _ = _run(_dev(p, gpu), _dev(t, gpu), L)
    want = np.array([BR.case_ref(*r, T, L)["val"] for r in rows])
    got = vals.cpu().numpy().astype(np.float64)
    worst = _check_values(got, want, (T, L))
    if np.isfinite(want).all():
        dm = abs(float(mean.item()) - want.mean())
        print(f"BSS-VAL T={T} L={L} rows={len(rows)} max|dB - ref|={worst:.3e} |mean - ref|={dm:.3e}")
        assert dm <= DB_BOUND, (mean.item(), want.mean())
    else:
        assert (T, L) == (1, 1)
        print(f"BSS-VAL T={T} L={L} rows={len(rows)} max|dB - ref|={worst:.3e} (degenerate rows: {want})")
        assert not np.isfinite(float(mean.item()))
    assert worst <= DB_BOUND, (T, L, worst, got, want)


def test_values_of_a_long_pair_under_zero_mean(gpu):
    T = 100003
    rows = [("voiced", 10, 0), ("ar2", 30, 1)]
    p, t = _pairs(rows, T, dc=True)
    vals, mean, corr = _run(_dev(p, gpu), _dev(t, gpu), 512, True)
    refs = [BR.sdr_full(p[j], t[j], 512, True, want_cond=False) for j in range(2)]
    want = np.array([r["val"] for r in refs])
    got = vals.cpu().numpy().astype(np.float64)
    dc = max(np.abs(corr.cpu().numpy()[j, 0] - refs[j]["r"]).max() for j in range(2))
    dc = max(dc, max(np.abs(corr.cpu().numpy()[j, 1] - refs[j]["b"]).max() for j in range(2)))
    print(f"BSS-LONG max|dB - ref|={np.abs(got - want).max():.3e} max|corr - ref|={dc:.3e} values={got}")
    assert dc <= CORR_BOUND and np.abs(got - want).max() <= DB_BOUND
    assert abs(float(mean.item()) - want.mean()) <= DB_BOUND


def test_degenerate_rows(gpu):
    C = _C()
    T = C + 65
    g = np.random.default_rng(11)
    x = g.standard_normal(T).astype(np.float32)
    p3, t3 = BR.case("ar2", 10, 0, T)
    p = np.stack([x, g.standard_normal(T).astype(np.float32), p3])
    t = np.stack([x, np.zeros(T, np.float32), t3])
    for L in (64, 512):
        vals, mean, _ = _run(_dev(p, gpu), _dev(t, gpu), L)
        v = vals.cpu().numpy().astype(np.float64)
        print(f"BSS-DEGENERATE L={L} values={v} mean={mean.item()}")
        assert v[0] == np.inf or (np.isfinite(v[0]) and v[0] >= 120.0)      # preds equal to target
        assert np.isnan(v[1])                                               # silent target
        assert abs(v[2] - BR.case_ref("ar2", 10, 0, T, L)["val"]) <= DB_BOUND
        assert np.isnan(mean.item())


# ---- mechanics -----------------------------------------------------------------
def test_optional_outputs_offset_view_and_repeat(gpu):
    C = _C()
    p, t = _pairs(_ROWS, C + 513, dc=True)
    pd, td = _dev(p, gpu), _dev(t, gpu)
    v0, m0, c0 = _run(pd, td, 512, True)
    v1, m1, c1 = _run(pd, td, 512, True)            # the same bits on a second run
    assert torch.equal(v0, v1) and torch.equal(m0, m1) and torch.equal(c0, c1)
    v2, m2, c2 = _run(pd, td, 512, True, want_mean=False, want_corr=False)
    assert torch.equal(v0, v2) and bool((m2 == -7).all()) and bool((c2 == -7).all())
    B, T = pd.shape                                 # inputs one float into their allocations
    po = torch.zeros(B * T + 1, dtype=torch.float32, device=gpu)[1:].view(B, T).copy_(pd)
    to = torch.zeros(B * T + 1, dtype=torch.float32, device=gpu)[1:].view(B, T).copy_(td)
    assert po.data_ptr() % 16 == 4 and po.is_contiguous()
    v3, m3, c3 = _run(po, to, 512, True)
    assert torch.equal(v0, v3) and torch.equal(m0, m3) and torch.equal(c0, c3)
    assert abs(m0.item() - v0.double().mean().item()) <= 1e-5


def test_graph_replay_equals_eager(gpu):
    """One captured launch replayed on three staged batches."""
    S = _L()
    C = _C()
    B, T, L = 3, C + 17, 65
    sets = [[(k, q, s) for k in BR.KINDS] for q, s in ((30, 0), (10, 1), (0, 0))]
    pred = torch.zeros(B, T, dtype=torch.float32, device=gpu)
    target = torch.zeros(B, T, dtype=torch.float32, device=gpu)
    ws = S.workspace(S.lib().sel_bss_sdr_workspace(B, T, L), gpu)
    vals = torch.full((B,), -7.0, dtype=torch.float32, device=gpu)
    mean = torch.full((1,), -7.0, dtype=torch.float32, device=gpu)
    corr = torch.full((B, 2, L), -7.0, dtype=torch.float64, device=gpu)

    def launch():
        S.call("sel_bss_sdr", S.ptr(pred), S.ptr(target), B, T, L, 1, 0.0, S.ptr(vals), S.ptr(mean), S.ptr(corr),
               S.ptr(ws), ws.numel(), S.stream())

    eager = []
    for rows in sets:                               # also loads the kernels before the capture
        p, t = _pairs(rows, T, dc=True)
        eager.append(_run(_dev(p, gpu), _dev(t, gpu), L, True))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    torch.cuda.synchronize()
    assert bool((vals == -7).all()) and bool((corr == -7).all())    # capturing ran nothing
    for rows, (ve, me, ce) in zip(sets, eager):
        p, t = _pairs(rows, T, dc=True)
        pred.copy_(_dev(p, gpu))
        target.copy_(_dev(t, gpu))
        vals.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(vals, ve) and torch.equal(mean, me) and torch.equal(corr, ce), rows
    assert not torch.equal(eager[0][0], eager[1][0])


def test_module_and_functional_forms(gpu):
    from sel import metrics as M
    T = _C() + 513
    rows = BR.ALL_CASES[:4]
    p, t = _pairs(rows, T)
    pd, td = _dev(p, gpu), _dev(t, gpu)
    want = np.array([BR.case_ref(*r, T, 512)["val"] for r in rows])
    v = M.sdr(pd.view(2, 2, T), td.view(2, 2, T))
    assert v.shape == (2, 2) and v.dtype == torch.float32 and v.grad_fn is None
    assert np.abs(v.cpu().numpy().reshape(-1) - want).max() <= DB_BOUND
    m = M.SignalDistortionRatio()(pd.clone().requires_grad_(True), td)
    assert m.shape == () and m.grad_fn is None and not m.requires_grad
    assert abs(m.item() - want.mean()) <= DB_BOUND
    p, t = _pairs(rows, T, dc=True)
    pd, td = _dev(p, gpu), _dev(t, gpu)
    w64 = np.array([BR.sdr_full(p[j], t[j], 64, True, 1e-6, want_cond=False)["val"] for j in range(4)])
    v64 = M.sdr(pd, td, filter_length=64, zero_mean=True, load_diag=1e-6)
    assert np.abs(v64.cpu().numpy() - w64).max() <= DB_BOUND
    m64 = M.SignalDistortionRatio(filter_length=64, zero_mean=True, load_diag=1e-6)(pd, td)
    assert abs(m64.item() - w64.mean()) <= DB_BOUND
    with pytest.raises(ValueError, match="shape"):
        M.sdr(pd, td[:, :-1])


def test_measures_with_sdr(gpu):
    from mel_spectrogram import measures
    g = torch.Generator().manual_seed(4)
    clean = 0.1 * torch.randn(1, 24000, generator=g)
    pred = (clean + 0.02 * torch.randn(1, 24000, generator=g)).to(gpu)
    out = measures(pred, clean.to(gpu), sdr=True)
    assert list(out) == ["MAE", "MSE", "SNR", "SDR", "SI-SDR(True)", "SI-SDR(False)", "STOI", "Mel-L1"]
    assert all(torch.is_tensor(v) and v.numel() == 1 and bool(torch.isfinite(v).all()) for v in out.values()), out
    want = BR.sdr_full(pred[0].cpu().numpy(), clean[0].numpy(), 512, want_cond=False)["val"]
    assert abs(out["SDR"].item() - want) <= DB_BOUND and out["SDR"].item() >= out["SI-SDR(False)"].item() - 1e-3
    plain = measures(pred, clean.to(gpu))
    assert list(plain) == ["MAE", "MSE", "SNR", "SI-SDR(True)", "SI-SDR(False)", "STOI", "Mel-L1"]
