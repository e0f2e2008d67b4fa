"""CPU checks of the BSS-eval SDR: every refusal of sel_bss_sdr
through ctypes (before any device work: the pointers below are never
dereferenced), the workspace size, the fp64 restatement tests/bss_sdr_ref.py
against its cross-checks, the conditions that make the shared value cases
meaningful, and the Python argument checks."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import bss_sdr_ref as BR
import metrics_ref as MR

SEL_ERR_ARG, SEL_ERR_WORKSPACE = -1, -4
P = ctypes.c_void_p(0x1000)      # a non-null, 8-byte aligned pointer no refused call may touch
NULL = None

# the value cases must be well inside what fp64 resolves
MIN_ONE_MINUS_COH, MAX_COND = 1e-5, 1e9


def _lib():
    from sel import _lib
    return _lib.load()


def _call(**kw):
    a = dict(pred=P, target=P, B=3, T=5000, L=512, zm=0, load_diag=0.0, vals=P, mean=P, corr=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = 1 << 40
    return _lib().sel_bss_sdr(a["pred"], a["target"], a["B"], a["T"], a["L"], a["zm"], a["load_diag"], a["vals"],
                              a["mean"], a["corr"], a["ws"], a["ws_bytes"], None)


_ids = lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"  # noqa: E731
                          for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(pred=NULL), dict(target=NULL), dict(vals=NULL), dict(ws=NULL), dict(B=0),
                                 dict(B=-1), dict(B=65536), dict(T=0), dict(T=-7), dict(L=0), dict(L=-1),
                                 dict(L=513), dict(zm=2), dict(zm=-1), dict(load_diag=-1e-9),
                                 dict(load_diag=float("inf")), dict(load_diag=float("nan")),
                                 dict(ws=ctypes.c_void_p(0x1004))], ids=_ids)
def test_bss_sdr_refuses(bad):
    assert _call(**bad) == SEL_ERR_ARG
    assert b"sel_bss_sdr" in _lib().sel_last_error()


def test_workspace_one_byte_short_is_refused():
    lib = _lib()
    for B, T, L in ((3, 5000, 512), (1, 1, 1), (2, 2048, 64), (2, 2049, 65)):
        need = lib.sel_bss_sdr_workspace(B, T, L)
        assert need > 0
        assert _call(B=B, T=T, L=L, ws_bytes=need - 1) == SEL_ERR_WORKSPACE
        assert b"sel_bss_sdr" in lib.sel_last_error()


def test_workspace_is_monotone_and_aligned():
    lib = _lib()
    C = lib.sel_bss_sdr_chunk()
    assert C >= 512
    Ts = [1, 2, 511, 512, C - 1, C, C + 1, 2 * C, 2 * C + 1, 96000, 480000]
    Bs = [1, 2, 7, 64, 65535]
    for L in (1, 64, 512):
        for B in Bs:
            sizes = [lib.sel_bss_sdr_workspace(B, T, L) for T in Ts]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (B, L, sizes)
            assert all(s % 8 == 0 for s in sizes)
        for T in Ts:
            sizes = [lib.sel_bss_sdr_workspace(B, T, L) for B in Bs]
            assert all(a < b for a, b in zip(sizes, sizes[1:])), (T, L, sizes)
    # one more chunk at T = C + 1: (2L + 1) more doubles per row
    assert lib.sel_bss_sdr_workspace(3, C + 1, 512) - lib.sel_bss_sdr_workspace(3, C, 512) == 3 * 1025 * 8
    # shapes the call refuses need no workspace
    for B, T, L in ((0, 100, 512), (65536, 100, 512), (1, 0, 512), (1, 100, 0), (1, 100, 513)):
        assert lib.sel_bss_sdr_workspace(B, T, L) == 0


# ---- the reference alone ---------------------------------------------------
@pytest.mark.parametrize("T,L", [(512, 512), (513, 512), (600, 64), (2049, 65), (6161, 512), (24000, 512)])
def test_fft_form_equals_direct_sums_at_T_ge_L(T, L):
    """torchmetrics takes the correlations from an FFT; at T >= L no wrapped lag falls inside [:L]."""
    worst = 0.0
    for kind in BR.KINDS:
        for snr in BR.SNRS:
            p, t = BR.case(kind, snr, 0, T)
            for zm in (False, True):
                worst = max(worst, abs(BR.sdr_fft(p, t, L, zm) - BR.sdr_full(p, t, L, zm, want_cond=False)["val"]))
    print(f"BSS-FFT T={T} L={L} max|fft - direct|={worst:.3e} dB")
    assert worst <= 1e-8


def test_one_tap_is_the_si_sdr():
    """L = 1: coh = (t . p)^2 / (|t|^2 |p|^2), which is the SI-SDR (its eps aside)."""
    p, t = BR.case("white", 10, 0, 4096)
    a = BR.sdr_full(p, t, 1)["val"]
    b = float(MR.sdr_db(p.astype(np.float64)[None], t.astype(np.float64)[None], 1, 0)[0])
    print(f"BSS-L1 {a:.7f} against SI-SDR {b:.7f}")
    assert abs(a - b) <= 1e-5


def test_load_diag_and_zero_mean_in_the_reference():
    p, t = BR.case("ar2", 10, 1, 2049)
    a, b = BR.sdr_full(p, t, 64), BR.sdr_full(p, t, 64, load_diag=1e-6)
    assert b["r"][0] == a["r"][0] + 1e-6 and np.array_equal(a["r"][1:], b["r"][1:]) and a["val"] != b["val"]
    z = BR.sdr_full(p + np.float32(0.05), t + np.float32(0.02), 64, zero_mean=True)
    assert abs(z["val"] - BR.sdr_full(p, t, 64, zero_mean=True)["val"]) < 1e-4
    # linear correlations: lags at or past T are zero
    s = BR.sdr_full(p[:3], t[:3], 8)
    assert np.all(s["r"][3:] == 0) and np.all(s["b"][3:] == 0) and s["r"][2] != 0


_COND_T = (63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2559, 2560, 6161)
_COND_L = (1, 2, 64, 65, 512)


def _conditions(T, L):
    worst_c, worst_m = 0.0, 1.0
    for kind, snr, seed in BR.ALL_CASES:
        r = BR.case_ref(kind, snr, seed, T, L, want_cond=True)
        worst_c, worst_m = max(worst_c, r["cond"]), min(worst_m, 1.0 - r["coh"])
    return worst_c, worst_m


@pytest.mark.parametrize("L", _COND_L)
def test_value_cases_are_well_conditioned(L):
    """Every value case: 1 - coh >= 1e-5 and cond(R) <= 1e9 in the reference."""
    worst_c, worst_m = 0.0, 1.0
    for T in _COND_T:
        c, m = _conditions(T, L)
        assert m >= MIN_ONE_MINUS_COH and c <= MAX_COND, (T, L, m, c)
        worst_c, worst_m = max(worst_c, c), min(worst_m, m)
    print(f"BSS-COND L={L} max cond={worst_c:.3e} min 1-coh={worst_m:.3e}")


def test_value_shapes_derived_from_the_chunk():
    """The GPU test places T around L and the chunk.  Those shapes meet the
    same conditions, but for the two that L = 1 makes tiny: T = 1 (coh is 1
    whatever the signals are, or 0 where the noise cancels the one sample: the
    degenerate rules apply) and T = 2 (R is 1 x 1,
    so cond = 1, and two neighbouring samples of the voiced signal are nearly
    proportional: 1 - coh falls to 5e-6, where one rounding of coh, 1.1e-16,
    still moves the value by only 4.34 * 1.1e-16 / 5e-6 = 1e-10 dB)."""
    C = _lib().sel_bss_sdr_chunk()
    small = []
    for T, L in BR.value_shapes(C):
        if T in _COND_T and L in _COND_L:
            continue
        c, m = _conditions(T, L)
        print(f"BSS-COND T={T} L={L} max cond={c:.3e} min 1-coh={m:.3e}")
        if m >= MIN_ONE_MINUS_COH and c <= MAX_COND:
            continue
        small.append((T, L))
        assert L == 1 and c == 1.0 and (T == 1 or (T == 2 and m >= 1e-6)), (T, L, c, m)
    assert small == [(1, 1), (2, 1)]
    for kind, snr, seed in BR.ALL_CASES:
        coh = BR.case_ref(kind, snr, seed, 1, 1)["coh"]
        assert 1.0 - coh < 1e-12 or coh == 0.0


def test_exact_fit_shapes_are_not_value_cases():
    """T in {2, 3} with L >= 64: the filter fits the prediction exactly, so
    these shapes are checked on their correlations only."""
    for T in (2, 3):
        for L in (64, 512):
            c, m = _conditions(T, L)
            assert m < MIN_ONE_MINUS_COH or c > MAX_COND, (T, L, m, c)


# ---- Python ----------------------------------------------------------------
def test_python_argument_checks():
    from sel import metrics as M
    x = torch.randn(2, 600)
    for bad in (0, -1, 513, 1024, 2.5, True):
        with pytest.raises(ValueError, match="512"):
            M.sdr(x, x, filter_length=bad)
        with pytest.raises(ValueError, match="512"):
            M.SignalDistortionRatio(filter_length=bad)
    for bad in (-1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="load_diag"):
            M.SignalDistortionRatio(load_diag=bad)
    m = M.SignalDistortionRatio()
    assert (m.filter_length, m.zero_mean, m.load_diag) == (512, False, 0.0)
    assert M.SignalDistortionRatio(filter_length=64, zero_mean=True, load_diag=1e-6).load_diag == 1e-6


def test_use_cg_iter_warns_once_and_is_ignored():
    from sel import metrics as M
    M._warned_cg = False
    with pytest.warns(UserWarning, match="use_cg_iter"):
        M.SignalDistortionRatio(use_cg_iter=10)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M.SignalDistortionRatio(use_cg_iter=10)


def test_python_refuses_cpu_tensors_and_shape_mismatch():
    from sel import metrics as M
    from mel_spectrogram import measures
    x = torch.randn(2, 600)
    for f in (lambda: M.sdr(x, x), lambda: M.SignalDistortionRatio()(x, x), lambda: measures(x, x, sdr=True),
              lambda: M.sdr(x, x, filter_length=64, zero_mean=True, load_diag=1e-6)):
        with pytest.raises(RuntimeError, match="CPU"):
            f()
