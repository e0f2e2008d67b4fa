"""CPU checks of the ragged-batch layer: every refusal of the new
*_var entry points through ctypes (before any device work: the pointers below
are never dereferenced), their workspace sizes, the ValueErrors for lengths
given on the host, the bucketing of sel.evaluate as pure logic on lengths, and
the condition the shared STOI rows have to meet (a margin of at least 1 dB
between each frame energy and the silent-frame threshold, in fp64)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import ragged_cases as RC

SEL_ERR_ARG, SEL_ERR_UNSUPPORTED, SEL_ERR_WORKSPACE = -1, -3, -4
P = ctypes.c_void_p(0x1000)      # a non-null, 8-byte aligned pointer no refused call may touch
ODD = ctypes.c_void_p(0x1004)
NULL = None


def _lib():
    from sel import _lib
    return _lib.load()


_ids = lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"  # noqa: E731
                          for k, v in b.items())


def _sdr_fwd(**kw):
    a = dict(pred=P, target=P, B=3, T=100, lengths=P, si=1, zm=0, vals=P, mean=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib().sel_sdr_workspace(max(a["B"], 1))
    return _lib().sel_sdr_fwd_var(a["pred"], a["target"], a["B"], a["T"], a["lengths"], a["si"], a["zm"], a["vals"],
                                  a["mean"], a["ws"], a["ws_bytes"], None)


def _sdr_bwd(**kw):
    a = dict(pred=P, target=P, B=3, T=100, lengths=P, si=1, zm=0, g_vals=P, g_mean=P, g_pred=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib().sel_sdr_workspace(max(a["B"], 1))
    return _lib().sel_sdr_bwd_var(a["pred"], a["target"], a["B"], a["T"], a["lengths"], a["si"], a["zm"],
                                  a["g_vals"], a["g_mean"], a["g_pred"], a["ws"], a["ws_bytes"], None)


def _stoi(**kw):
    a = dict(clean=P, proc=P, B=2, T=4096, lengths=P, extended=0, d=P, mean=P, info=P, ws=P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib().sel_stoi_workspace(max(a["B"], 1), max(a["T"], 256))
    return _lib().sel_stoi_var(a["clean"], a["proc"], a["B"], a["T"], a["lengths"], a["extended"], a["d"], a["mean"],
                               a["info"], a["ws"], a["ws_bytes"], None)


def _bss(**kw):
    a = dict(pred=P, target=P, B=2, T=5000, lengths=P, L=512, zm=0, load_diag=0.0, vals=P, mean=P, corr=P, ws=P,
             ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(_lib().sel_bss_sdr_workspace(a["B"], a["T"], a["L"]), 8)
    return _lib().sel_bss_sdr_var(a["pred"], a["target"], a["B"], a["T"], a["lengths"], a["L"], a["zm"],
                                  a["load_diag"], a["vals"], a["mean"], a["corr"], a["ws"], a["ws_bytes"], None)


def _resample(**kw):
    a = dict(x=P, n=2, len=1000, lengths=P, orig=48000, new=10000, lpw=6, rolloff=0.99, table=P, y=P, out_lengths=P)
    a.update(kw)
    return _lib().sel_resample_var(a["x"], a["n"], a["len"], a["lengths"], a["orig"], a["new"], a["lpw"],
                                   a["rolloff"], a["table"], a["y"], a["out_lengths"], None)


def _mel(**kw):
    a = dict(x=P, B=2, T=2200, lengths=P, n_fft=400, hop=200, win=400, window=P, fb=P, krange=P, n_mels=128,
             power=2.0, out=P, frames=P)
    a.update(kw)
    return _lib().sel_power_mel_fwd_var(a["x"], a["B"], a["T"], a["lengths"], a["n_fft"], a["hop"], a["win"],
                                        a["window"], a["fb"], a["krange"], a["n_mels"], a["power"], a["out"],
                                        a["frames"], None)


def _l1l2(**kw):
    a = dict(a=P, b=P, B=3, inner=1, stride=100, n=P, l1=P, l2=P, means=P)
    a.update(kw)
    return _lib().sel_rows_l1_l2_var(a["a"], a["b"], a["B"], a["inner"], a["stride"], a["n"], a["l1"], a["l2"],
                                     a["means"], None)


_SDR_BAD = [dict(pred=NULL), dict(target=NULL), dict(lengths=NULL), dict(ws=NULL), dict(B=0), dict(B=-1), dict(T=0),
            dict(T=-5), dict(si=2), dict(si=-1), dict(zm=2), dict(zm=-1), dict(ws=ODD)]


@pytest.mark.parametrize("bad", _SDR_BAD + [dict(vals=NULL), dict(mean=NULL)], ids=_ids)
def test_sdr_fwd_var_refuses(bad):
    assert _sdr_fwd(**bad) == SEL_ERR_ARG
    assert b"sel_sdr_fwd_var" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", _SDR_BAD + [dict(g_pred=NULL), dict(g_vals=NULL, g_mean=NULL),
                                            dict(B=1 << 20, T=1 << 40)], ids=_ids)
def test_sdr_bwd_var_refuses(bad):
    assert _sdr_bwd(**bad) == SEL_ERR_ARG
    assert b"sel_sdr_bwd_var" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", [dict(clean=NULL), dict(proc=NULL), dict(lengths=NULL), dict(d=NULL), dict(ws=NULL),
                                 dict(B=0), dict(B=-2), dict(B=65536), dict(T=0), dict(T=-4096), dict(T=255),
                                 dict(T=(1 << 30) + 1), dict(extended=2), dict(extended=-1), dict(ws=ODD)], ids=_ids)
def test_stoi_var_refuses(bad):
    assert _stoi(**bad) == SEL_ERR_ARG
    assert b"sel_stoi_var" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", [dict(pred=NULL), dict(target=NULL), dict(lengths=NULL), dict(vals=NULL),
                                 dict(ws=NULL), dict(B=0), dict(B=65536), dict(T=0), dict(T=(1 << 32) + 1),
                                 dict(L=0), dict(L=513), dict(zm=2), dict(load_diag=-1.0),
                                 dict(load_diag=float("nan")), dict(load_diag=float("inf")), dict(ws=ODD)], ids=_ids)
def test_bss_sdr_var_refuses(bad):
    assert _bss(**bad) == SEL_ERR_ARG
    assert b"sel_bss_sdr_var" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", [dict(x=NULL), dict(lengths=NULL), dict(table=NULL), dict(y=NULL),
                                 dict(out_lengths=NULL), dict(n=0), dict(n=-1), dict(len=0), dict(len=-3),
                                 dict(len=(1 << 40) + 1)], ids=_ids)
def test_resample_var_refuses(bad):
    assert _resample(**bad) == SEL_ERR_ARG
    assert b"sel_resample_var" in _lib().sel_last_error()


def test_resample_var_refuses_what_the_plan_refuses():
    assert _resample(n=65536) == SEL_ERR_UNSUPPORTED
    for bad in (dict(orig=0), dict(new=-1), dict(lpw=0), dict(rolloff=0.0), dict(rolloff=1.5)):
        assert _resample(**bad) == SEL_ERR_ARG, bad
    assert _resample(orig=22051, new=24000) == SEL_ERR_UNSUPPORTED      # a tap table beyond the limit


@pytest.mark.parametrize("bad", [dict(x=NULL), dict(lengths=NULL), dict(window=NULL), dict(fb=NULL),
                                 dict(krange=NULL), dict(out=NULL), dict(frames=NULL), dict(B=0), dict(T=0),
                                 dict(hop=0), dict(n_mels=0), dict(win=0), dict(win=401), dict(T=200)], ids=_ids)
def test_power_mel_var_refuses(bad):
    assert _mel(**bad) == SEL_ERR_ARG
    assert b"sel_power_mel_fwd_var" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", [dict(n_fft=6, win=6), dict(n_fft=401), dict(n_fft=2050), dict(n_fft=28, win=28),
                                 dict(power=0.0), dict(power=-1.0)], ids=_ids)
def test_power_mel_var_unsupported(bad):
    assert _mel(**bad) == SEL_ERR_UNSUPPORTED
    assert b"sel_power_mel_fwd_var" in _lib().sel_last_error()


@pytest.mark.parametrize("bad", [dict(a=NULL), dict(b=NULL), dict(n=NULL), dict(l1=NULL), dict(l2=NULL), dict(B=0),
                                 dict(B=-1), dict(inner=0), dict(stride=0), dict(inner=1 << 30, stride=1 << 30),
                                 dict(B=1 << 29, inner=1 << 20, stride=1 << 20)], ids=_ids)
def test_rows_l1_l2_var_refuses(bad):
    assert _l1l2(**bad) == SEL_ERR_ARG
    assert b"sel_rows_l1_l2_var" in _lib().sel_last_error()


def test_workspaces_are_those_of_the_fixed_length_calls():
    """T is the stride: the ragged calls take the workspace of the (B, T) call, and one byte less is refused."""
    lib = _lib()
    assert _sdr_fwd(ws_bytes=lib.sel_sdr_workspace(3) - 1) == SEL_ERR_WORKSPACE
    assert _sdr_bwd(ws_bytes=lib.sel_sdr_workspace(3) - 1) == SEL_ERR_WORKSPACE
    assert lib.sel_sdr_workspace(3) == 48 * 3
    for T in (256, 4096, 12000):
        assert _stoi(T=T, ws_bytes=lib.sel_stoi_workspace(2, T) - 1) == SEL_ERR_WORKSPACE
        assert b"sel_stoi_var" in lib.sel_last_error()
        F = (T - 256) // 128 + 1
        assert lib.sel_stoi_workspace(2, T) == 2 * (8 * (max(F - 30, 0) + 30 * (F - 1)) + 4 * (2 * F + 3))
    C = int(lib.sel_bss_sdr_chunk())
    for T, L in ((1, 1), (C, 512), (RC.BSS_T, 512), (RC.BSS_T, 16)):
        size = lib.sel_bss_sdr_workspace(2, T, L)
        assert size == 2 * (3 + -(-T // C) * (2 * L + 1)) * 8
        assert _bss(T=T, L=L, ws_bytes=size - 1) == SEL_ERR_WORKSPACE
        assert b"sel_bss_sdr_var" in lib.sel_last_error()


# ---- lengths given on the host ------------------------------------------------
def test_check_host_lengths():
    from sel import _lib as L
    got = L.check_host_lengths([3, 7, 10], 3, 10, 1, "t")
    assert got.dtype == torch.int64 and got.tolist() == [3, 7, 10]
    assert L.check_host_lengths(torch.tensor([[5], [6]], dtype=torch.int32), 2, 6, 5, "t").tolist() == [5, 6]
    assert L.check_host_lengths(np.array([256]), 1, 256, 256, "t").tolist() == [256]
    for bad, B, T, lo in (([3, 7], 3, 10, 1), ([0, 7, 10], 3, 10, 1), ([3, 7, 11], 3, 10, 1), ([255], 1, 300, 256),
                          ([3.0, 7.0, 10.0], 3, 10, 1), ([True, False, True], 3, 10, 0), ([-1, 2, 3], 3, 10, 0)):
        with pytest.raises(ValueError, match="lengths"):
            L.check_host_lengths(bad, B, T, lo, "t")


def test_host_lengths_are_checked_before_anything_else():
    """A bad host length is a ValueError even on CPU tensors (where a good one
    reaches the refusal of CPU tensors)."""
    from sel import metrics as M
    from sel.resample import resample
    from mel_spectrogram import MelSpectrogram, measures, measures_rows
    x = torch.randn(2, 4096)
    mel = MelSpectrogram(48000)
    calls = {
        "snr": (lambda n: M.snr(x, x, lengths=n), 1),
        "si_sdr": (lambda n: M.si_sdr(x, x, zero_mean=True, lengths=n), 1),
        "sdr": (lambda n: M.sdr(x, x, lengths=n), 1),
        "stoi": (lambda n: M.stoi(x, x, 10000, lengths=n), 256),
        "stoi16k": (lambda n: M.stoi(x, x, 16000, lengths=n), 409),
        "SignalNoiseRatio": (lambda n: M.SignalNoiseRatio()(x, x, lengths=n), 1),
        "SI-SDR module": (lambda n: M.ScaleInvariantSignalDistortionRatio()(x, x, lengths=n), 1),
        "SDR module": (lambda n: M.SignalDistortionRatio()(x, x, lengths=n), 1),
        "STOI module": (lambda n: M.ShortTimeObjectiveIntelligibility(10000, True)(x, x, lengths=n), 256),
        "mel": (lambda n: mel(x, lengths=n), 201),
        "measures": (lambda n: measures(x, x, 16000, lengths=n), 409),
        "measures_rows": (lambda n: measures_rows(x, x, 48000, lengths=n), 1225),
    }
    for name, (f, lo) in calls.items():
        for bad in ([lo - 1, 4096], [lo, 4097], [lo], [float(lo), 4096.0]):
            with pytest.raises(ValueError, match="lengths"):
                f(bad)
        with pytest.raises(RuntimeError, match="device"):
            f([lo, 4096])
    with pytest.raises(ValueError, match="lengths"):
        resample(x, 48000, 10000, lengths=[-1, 5])
    with pytest.raises(ValueError, match="lengths"):
        resample(x, 48000, 10000, lengths=[0, 4097])
    with pytest.raises(RuntimeError, match="device"):
        resample(x, 48000, 10000, lengths=[0, 4096])
    with pytest.raises(NotImplementedError):
        resample(x, 48000, 10000, lengths=[1, 2], differentiable=True)


def test_stoi_min_length_is_the_first_with_one_frame():
    from sel import metrics as M
    lib = _lib()
    for fs in (8000, 10000, 16000, 22050, 24000, 44100, 48000):
        n = M.stoi_min_length(fs)
        assert lib.sel_resample_out_len(n, fs, 10000) >= 256 > lib.sel_resample_out_len(n - 1, fs, 10000), fs
    assert M.stoi_min_length(10000) == 256 and M.stoi_min_length(16000) == 409 and M.stoi_min_length(48000) == 1225


# ---- the scorer's bucketing ---------------------------------------------------
def test_plan_buckets():
    from sel.evaluate import PAD_QUANTUM, plan_buckets
    assert PAD_QUANTUM == 4096
    rnd = random.Random(3)
    for n, batch in ((1, 1), (11, 1), (11, 4), (11, 16), (64, 16), (33, 7)):
        lengths = [rnd.randint(1, 200000) for _ in range(n)]
        lengths[0] = lengths[-1]                           # a tie
        plan = plan_buckets(lengths, batch)
        seen = [i for idx, _ in plan for i in idx]
        assert sorted(seen) == list(range(n))              # every item exactly once
        assert [lengths[i] for i in seen] == sorted(lengths)
        assert len(plan) == -(-n // batch)
        for idx, T in plan:
            longest = max(lengths[i] for i in idx)
            assert 1 <= len(idx) <= batch and T % 4096 == 0 and longest <= T < longest + 4096
    assert plan_buckets([4096, 4097, 1], 2) == [([2, 0], 4096), ([1], 8192)]
    assert plan_buckets([], 4) == []
    # the plan of a permuted corpus is the permuted plan: the same rows share a bucket
    lengths = [rnd.randint(1, 50000) for _ in range(20)]
    perm = list(range(20))
    rnd.shuffle(perm)
    a = [sorted(lengths[i] for i in idx) for idx, _ in plan_buckets(lengths, 4)]
    b = [sorted(lengths[perm[i]] for i in idx) for idx, _ in plan_buckets([lengths[j] for j in perm], 4)]
    assert a == b
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="batch"):
            plan_buckets([5, 6], bad)
    with pytest.raises(ValueError, match="sample"):
        plan_buckets([5, 0], 2)


def test_score_corpus_refuses_bad_items_before_device_work():
    from sel.evaluate import score_corpus
    x = torch.zeros(5000)
    with pytest.raises(ValueError, match="1-D"):
        score_corpus([("a", x, torch.zeros(4999))], 16000)
    with pytest.raises(ValueError, match="1-D"):
        score_corpus([("a", x.view(1, -1), x.view(1, -1))], 16000)
    with pytest.raises(ValueError, match="duplicate"):
        score_corpus([("a", x, x), ("a", x, x)], 16000)
    with pytest.raises(ValueError, match="batch"):
        score_corpus([("a", x, x)], 16000, batch=0)
    assert score_corpus([], 16000) == ({}, {})


# ---- the shared cases ---------------------------------------------------------
def test_stoi_rows_keep_their_frames_under_fp32():
    want = {256: 1, 4095: 30, 4096: 31, 8448: 65, 11000: 84}
    for ext in (False, True):
        for n, r in zip(RC.STOI_LENGTHS, RC.stoi_refs(ext)):
            assert r["margin"] >= 1.0, (n, r["margin"])
            assert r["frames"] == (n - 256) // 128 + 1 == want[n] and r["M"] == r["kept"] - 1
            if n <= 4096:
                assert r["kept"] == r["frames"]
            if n <= 4095:
                assert r["d"] == 1e-5
            else:
                assert 0.5 < r["d"] <= 1.0 or ext
    assert RC.stoi_refs(False)[3]["kept"] < 65 and RC.stoi_refs(False)[4]["kept"] < 84     # the gaps drop frames
    assert max(RC.STOI_LENGTHS) < RC.STOI_T


def test_case_lengths_sit_at_the_edges():
    lib = _lib()
    assert int(lib.sel_bss_sdr_chunk()) == 2048
    for edge, below in (RC.SDR_LENGTHS, RC.BSS_LENGTHS, RC.MEL_LENGTHS):
        assert len(edge) == len(below) and edge[:-1] == below[:-1]
    assert max(RC.SDR_LENGTHS[0]) == RC.SDR_T and max(RC.SDR_LENGTHS[1]) < RC.SDR_T
    assert max(RC.BSS_LENGTHS[0]) == RC.BSS_T and max(RC.BSS_LENGTHS[1]) < RC.BSS_T
    assert max(RC.MEL_LENGTHS[0]) == RC.MEL_T and max(RC.MEL_LENGTHS[1]) < RC.MEL_T
    assert [1 + n // RC.MEL_HOP for n in RC.MEL_LENGTHS[0]] == [2, 2, 3, 3, 5, 6, 12]
    assert [int(lib.sel_resample_out_len(n, 48000, 10000)) for n in RC.STOI48_LENGTHS] == [257, 4097, 8448, 12000]
    for rows, lengths in ((RC.sdr_rows(RC.SDR_LENGTHS[0]), RC.SDR_LENGTHS[0]),
                          (RC.bss_rows(RC.BSS_LENGTHS[0]), RC.BSS_LENGTHS[0]),
                          (RC.mel_rows(RC.MEL_LENGTHS[0]), RC.MEL_LENGTHS[0])):
        assert [len(p) for p, _ in rows] == lengths
        assert all(np.abs(t).max() > 0 for _, t in rows)   # no silent target
    a, b = RC.pad(RC.sdr_rows(RC.SDR_LENGTHS[1]), RC.SDR_T, float("nan"))
    assert np.isnan(a[:, -1]).all() and np.isnan(b[:, -1]).all() and not np.isnan(a[0, 0])
