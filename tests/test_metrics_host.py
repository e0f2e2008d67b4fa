"""CPU checks of the evaluation measures: every refusal of
sel_sdr_fwd / sel_sdr_bwd / sel_stoi through ctypes (before any device work:
the pointers below are never dereferenced), the workspace sizes, the band-edge
table against its formula, and the fp64 restatement tests/metrics_ref.py
against the cross-check figures of its definition, with the condition every
shared case has to meet: a margin of at least 1 dB between each frame energy
and the silent-frame threshold."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_ref as MR

SEL_ERR_ARG, SEL_ERR_WORKSPACE = -1, -4
P = ctypes.c_void_p(0x1000)      # a non-null, 8-byte aligned pointer no refused call may touch
NULL = None


def _lib():
    from sel import _lib
    return _lib.load()


def test_error_codes_match_header():
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "include", "sel.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"\b(SEL_ERR_[A-Z]+)\s*=\s*(-?\d+)", src)}
    assert codes["SEL_ERR_ARG"] == SEL_ERR_ARG and codes["SEL_ERR_WORKSPACE"] == SEL_ERR_WORKSPACE


def _sdr_fwd(**kw):
    a = dict(pred=P, target=P, B=3, T=100, si=1, zm=0, vals=P, mean=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib().sel_sdr_workspace(max(a["B"], 1))
    return _lib().sel_sdr_fwd(a["pred"], a["target"], a["B"], a["T"], a["si"], a["zm"], a["vals"], a["mean"], a["ws"],
                              a["ws_bytes"], None)


def _sdr_bwd(**kw):
    a = dict(pred=P, target=P, B=3, T=100, si=1, zm=0, g_vals=P, g_mean=P, g_pred=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib().sel_sdr_workspace(max(a["B"], 1))
    return _lib().sel_sdr_bwd(a["pred"], a["target"], a["B"], a["T"], a["si"], a["zm"], a["g_vals"], a["g_mean"],
                              a["g_pred"], a["ws"], a["ws_bytes"], None)


def _stoi(**kw):
    a = dict(clean=P, proc=P, B=2, T=4096, extended=0, d=P, mean=P, info=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib().sel_stoi_workspace(max(a["B"], 1), max(a["T"], 256))
    return _lib().sel_stoi(a["clean"], a["proc"], a["B"], a["T"], a["extended"], a["d"], a["mean"], a["info"],
                           a["ws"], a["ws_bytes"], None)


_ids = lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"  # noqa: E731
                          for k, v in b.items())

_SDR_BAD = [dict(pred=NULL), dict(target=NULL), dict(ws=NULL), dict(B=0), dict(B=-1), dict(T=0), dict(T=-5),
            dict(si=2), dict(si=-1), dict(zm=2), dict(zm=-1), dict(ws=ctypes.c_void_p(0x1004))]


@pytest.mark.parametrize("bad", _SDR_BAD + [dict(vals=NULL), dict(mean=NULL)], ids=_ids)
def test_sdr_fwd_refuses(bad):
    assert _sdr_fwd(**bad) == SEL_ERR_ARG
    assert b"sel_sdr_fwd" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", _SDR_BAD + [dict(g_pred=NULL), dict(g_vals=NULL, g_mean=NULL),
                                            dict(B=1 << 20, T=1 << 40)], ids=_ids)
def test_sdr_bwd_refuses(bad):
    assert _sdr_bwd(**bad) == SEL_ERR_ARG
    assert b"sel_sdr_bwd" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", [dict(clean=NULL), dict(proc=NULL), dict(d=NULL), dict(ws=NULL), dict(B=0),
                                 dict(B=-2), dict(B=65536), dict(T=0), dict(T=-4096), dict(T=255),
                                 dict(T=(1 << 30) + 1), dict(extended=2), dict(extended=-1),
                                 dict(ws=ctypes.c_void_p(0x1004))], ids=_ids)
def test_stoi_refuses(bad):
    assert _stoi(**bad) == SEL_ERR_ARG
    assert b"sel_stoi" in _lib().sel_last_error()


def test_workspace_one_byte_short_is_refused():
    lib = _lib()
    assert _sdr_fwd(ws_bytes=lib.sel_sdr_workspace(3) - 1) == SEL_ERR_WORKSPACE
    assert _sdr_bwd(ws_bytes=lib.sel_sdr_workspace(3) - 1) == SEL_ERR_WORKSPACE
    for T in (256, 4096, 30000):
        assert _stoi(T=T, ws_bytes=lib.sel_stoi_workspace(2, T) - 1) == SEL_ERR_WORKSPACE
        assert b"sel_stoi" in lib.sel_last_error()


def test_workspaces_are_monotone():
    lib = _lib()
    Ts = [256, 383, 384, 3968, 4096, 4223, 4224, 8000, 30000, 480000]
    for B in (1, 2, 7, 64):
        sizes = [lib.sel_stoi_workspace(B, T) for T in Ts]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (B, sizes)
        assert lib.sel_sdr_workspace(B) == 48 * B
    for T in Ts:
        sizes = [lib.sel_stoi_workspace(B, T) for B in (1, 2, 7, 64)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (T, sizes)
    # frames F = (T - 256) // 128 + 1: energies and kept list (2F) and counts (3), 4-byte; two band
    # planes of (F - 1) x 15 and one segment sum per possible segment (F - 30), fp64
    for T in Ts:
        F = (T - 256) // 128 + 1
        assert lib.sel_stoi_workspace(3, T) == 3 * (8 * (max(F - 30, 0) + 30 * (F - 1)) + 4 * (2 * F + 3)), T
    assert lib.sel_stoi_workspace(1, 255) == 0 and lib.sel_stoi_workspace(0, 4096) == 0


def test_band_edges_match_formula():
    edges = (ctypes.c_int * 16)()
    assert _lib().sel_stoi_band_edges(edges) == 0
    ref = MR.band_edges()
    assert [(edges[b], edges[b + 1]) for b in range(15)] == ref
    # the formula itself, against the figures of the definition
    assert ref == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69),
                   (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
    assert _lib().sel_stoi_band_edges(None) == SEL_ERR_ARG


def test_window_is_hanning_258_inner():
    w = MR.window()
    assert len(w) == 256 and np.allclose(w, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1, 257) / 257), atol=1e-15)


@pytest.mark.parametrize("name,frames,kept,d,de", [("t4096", 31, 31, 0.944584, 0.159689),
                                                   ("mid_gap", 61, 51, 0.953729, 0.365995)])
def test_restatement_cross_checks(name, frames, kept, d, de):
    """fp64 signals of the recipe, seed 0 at 15 dB: the figures of the definition."""
    T, gaps = MR.CASES[name]
    x = MR.sig(0, T, gaps)
    y = MR.noisy(x, 0, 15)
    r, e = MR.stoi_full(x, y, False), MR.stoi_full(x, y, True)
    assert (r["frames"], r["kept"], r["M"]) == (frames, kept, kept - 1)
    assert abs(r["d"] - d) < 1e-6 and abs(e["d"] - de) < 1e-6, (r["d"], e["d"])


def test_restatement_of_identical_signals_is_one():
    T, gaps = MR.CASES["t4224"]
    x = MR.sig(0, T, gaps)
    assert abs(MR.stoi(x, x) - 1.0) < 1e-9 and abs(MR.stoi(x, x, True) - 1.0) < 1e-9


_FRAMES = {"t3968": (30, 30), "t4096": (31, 31), "t4223": (31, 31), "t4224": (32, 32), "mid_gap": (61, 51),
           "lead_gap": (61, 47), "tail_gap": (61, 51), "two_gaps": (92, 68), "m30_gap": (41, 33), "long": (233, None)}


@pytest.mark.parametrize("name", list(MR.CASES))
def test_case_margins_and_shapes(name):
    """Every case keeps its frame set under fp32: margin >= 1 dB in the
    reference; and the cases are what their names say (seed 0)."""
    for seed in MR.SEEDS:
        for snr in MR.SNRS:
            r = MR.case_ref(name, seed, snr, False)
            assert r["margin"] >= 1.0, (name, seed, snr, r["margin"])
            assert r["M"] == r["kept"] - 1 and r["frames"] == _FRAMES[name][0]
            assert r["kept"] < r["frames"] or not MR.CASES[name][1]
    r = MR.case_ref(name, 0, 15, False)
    if _FRAMES[name][1] is not None:
        assert r["kept"] == _FRAMES[name][1]
    if name == "t3968":
        assert r["M"] == 29 and r["d"] == 1e-5 and MR.case_ref(name, 0, 15, True)["d"] == 1e-5
    if name in ("t4096", "t4223"):
        assert r["M"] == 30
    if name == "t4224":
        assert r["M"] == 31


@pytest.mark.parametrize("name", [n for n in MR.CASES if n != "t3968"])
def test_stoi_falls_with_snr(name):
    for seed in MR.SEEDS:
        for ext in (False, True):
            hi, lo = MR.case_ref(name, seed, 15, ext)["d"], MR.case_ref(name, seed, 0, ext)["d"]
            assert lo < hi <= 1.0, (name, seed, ext, hi, lo)


def test_si_sdr_restatement():
    r = np.random.default_rng(5)
    t = r.standard_normal((3, 1000))
    for zm in (False, True):
        exact = MR.sdr_db(0.37 * t, t, True, zm)
        tc = t - t.mean(-1, keepdims=True) if zm else t
        cap = 10 * np.log10(((0.37 * tc) ** 2).sum(-1) / MR.EPS32)  # no residual: only eps is left, ~90 dB here
        assert (exact > 80).all() and np.allclose(exact, cap, atol=1e-3), (exact, cap)
        p = t + 0.1 * r.standard_normal(t.shape)
        a, b = MR.sdr_db(p, t, True, zm), MR.sdr_db(4.2 * p, t, True, zm)
        assert np.allclose(a, b, atol=1e-6) and (np.abs(a - 20) < 1.5).all(), (a, b)
    # the plain form is not scale invariant, and a DC offset only matters without zero_mean
    assert not np.allclose(MR.sdr_db(p, t, False, False), MR.sdr_db(4.2 * p, t, False, False), atol=1.0)
    assert np.allclose(MR.sdr_db(p + 3.0, t - 1.0, False, True), MR.sdr_db(p, t, False, True), atol=1e-9)
    # the torch form (fp64 autograd reference of the GPU test) is the same function
    tv = MR.sdr_db(torch.from_numpy(p), torch.from_numpy(t), True, True, xp=torch).numpy()
    assert np.allclose(tv, MR.sdr_db(p, t, True, True), atol=1e-10)


def test_eval_measures_config_is_checked():
    from trainer.trainerGAN import EVAL_MEASURES, _check_eval_measures
    from trainer.denoise import Trainer
    assert EVAL_MEASURES == ("SI-SDR", "SNR", "STOI", "ESTOI")
    assert _check_eval_measures({}) == () and _check_eval_measures({"eval_measures": []}) == ()
    assert _check_eval_measures({"eval_measures": ["STOI", "SI-SDR"], "sampling_rate": 24000}) == ("STOI", "SI-SDR")
    with pytest.raises(ValueError, match="eval_measures"):
        _check_eval_measures({"eval_measures": ["SI-SDR", "PESQ"], "sampling_rate": 24000})
    with pytest.raises(ValueError, match="eval_measures"):
        _check_eval_measures({"eval_measures": "STOI", "sampling_rate": 24000})
    with pytest.raises(KeyError, match="sampling_rate"):
        _check_eval_measures({"eval_measures": ["STOI"]})

    class _Gen(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.quantizer = torch.nn.Linear(1, 1)
            self.decoder = torch.nn.Linear(1, 1)

    with pytest.raises(ValueError, match="eval_measures"):
        Trainer(steps=0, epochs=0, data_loader={}, model={"generator": _Gen(), "discriminator": None}, criterion={},
                optimizer={}, scheduler={}, config={"outdir": None, "eval_measures": ["SDR"], "sampling_rate": 24000})


def test_modules_refuse_cpu_tensors():
    from sel import metrics as M
    from mel_spectrogram import measures
    x = torch.randn(2, 4096)
    for f in (lambda: M.SignalNoiseRatio(zero_mean=True)(x, x), lambda: M.ScaleInvariantSignalDistortionRatio()(x, x),
              lambda: M.ShortTimeObjectiveIntelligibility(10000)(x, x), lambda: M.si_sdr(x, x), lambda: M.snr(x, x),
              lambda: M.stoi(x, x, 10000), lambda: measures(x, x)):
        with pytest.raises(RuntimeError):
            f()
