"""CPU checks of the STOI / ESTOI gradient: the torch fp64
restatement tests/stoi_grad_ref.py against tests/metrics_ref.py and against a
central difference, the conditions that make the GPU cases meaningful (mask
margin, clip margin, no zero band, enough clipped cells), every refusal of
sel_stoi_bwd and sel_resample_bwd through ctypes (before any device work: the
pointers below are never dereferenced), the workspace size, and the Python
argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_ref as MR
import stoi_grad_ref as GR

SEL_ERR_ARG, SEL_ERR_UNSUPPORTED, SEL_ERR_WORKSPACE = -1, -3, -4
P = ctypes.c_void_p(0x1000)      # a non-null, 8-byte aligned pointer no refused call may touch
NULL = None

GRAD_CASES, SHALLOW_CASES = GR.GRAD_CASES, GR.SHALLOW_CASES


def _lib():
    from sel import _lib
    return _lib.load()


# ---- (a) the restatement's values --------------------------------------------
@pytest.mark.parametrize("name", [n for n in MR.CASES if n != "t3968"])
def test_torch_restatement_equals_numpy_restatement(name):
    worst = 0.0
    for seed in MR.SEEDS:
        for snr in MR.SNRS:
            x, y = MR.case(name, seed, snr)
            for ext in (False, True):
                ref = MR.case_ref(name, seed, snr, ext)
                assert ref["M"] >= 30
                with torch.no_grad():
                    d, info = GR.stoi_torch(x, torch.from_numpy(y.astype(np.float64)), ext, detail=True)
                assert (info["frames"], info["kept"], info["M"]) == (ref["frames"], ref["kept"], ref["M"])
                worst = max(worst, abs(float(d) - ref["d"]))
    print(f"STOI-GRAD-REF {name} max|torch - numpy| = {worst:.3e}")
    assert worst <= 1e-12


def test_restatement_of_a_short_row_is_the_constant():
    x, y = MR.case("t3968", 0, 15)
    p = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
    d = GR.stoi_torch(x, p, False)
    d.backward()
    assert float(d) == 1e-5 and not p.grad.any()


# ---- (b) autograd against a central difference --------------------------------
@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("row", [("t4224", 0, 15), ("mid_gap", 1, 0), ("shallow", 2, 5)], ids=lambda r: r[0])
def test_autograd_matches_central_difference(row, extended):
    h = 1e-6
    x, y = GR.case(*row)
    _, g, _ = GR.case_grad(*row, extended)
    v = np.random.default_rng(77).standard_normal(len(y))
    with torch.no_grad():
        dp = float(GR.stoi_torch(x, torch.from_numpy(y.astype(np.float64) + h * v), extended))
        dm = float(GR.stoi_torch(x, torch.from_numpy(y.astype(np.float64) - h * v), extended))
    fd, ad = (dp - dm) / (2 * h), float(g @ v)
    rel = abs(fd - ad) / abs(ad)
    print(f"STOI-GRAD-FD {row} extended={int(extended)} autograd={ad:.9e} difference={fd:.9e} rel={rel:.3e}")
    assert rel <= 1e-6


# ---- (c) what makes the GPU cases meaningful ----------------------------------
@pytest.mark.parametrize("row", GRAD_CASES + SHALLOW_CASES, ids=lambda r: f"{r[0]}-{r[1]}-{r[2]}")
def test_gpu_cases_keep_their_margins(row):
    _, g, info = GR.case_grad(*row, False)
    assert info["M"] >= 30 and np.isfinite(g).all() and g.any()
    assert info["margin"] >= 1.0, info            # the fp32 mask cannot differ from the fp64 one
    assert info["clip_margin"] >= 1e-6, info      # no cell sits on the clip's kink
    assert info["min_band"] > 0.0, info
    if row[0] == "shallow":
        assert info["kept"] == info["frames"] == 61


def test_shallow_gap_cases_exercise_the_clip():
    clipped = sum(GR.case_grad(*r, False)[2]["clipped"] for r in SHALLOW_CASES)
    cells = sum(GR.case_grad(*r, False)[2]["cells"] for r in SHALLOW_CASES)
    print(f"STOI-GRAD-CLIP shallow-gap cases: {clipped} of {cells} cells clipped ({100.0 * clipped / cells:.1f} %)")
    assert clipped >= 0.05 * cells


# ---- (d) refusals and the workspace -------------------------------------------
def _stoi_bwd(**kw):
    a = dict(clean=P, proc=P, B=2, T=4096, extended=0, g_d=P, g_mean=P, g_proc=P, ws_fwd=P, ws_fwd_bytes=None,
             ws_bwd=P, ws_bwd_bytes=None)
    a.update(kw)
    B, T = max(a["B"], 1), max(a["T"], 256)
    if a["ws_fwd_bytes"] is None:
        a["ws_fwd_bytes"] = _lib().sel_stoi_workspace(B, T)
    if a["ws_bwd_bytes"] is None:
        a["ws_bwd_bytes"] = _lib().sel_stoi_bwd_workspace(B, T)
    return _lib().sel_stoi_bwd(a["clean"], a["proc"], a["B"], a["T"], a["extended"], a["g_d"], a["g_mean"],
                               a["g_proc"], a["ws_fwd"], a["ws_fwd_bytes"], a["ws_bwd"], a["ws_bwd_bytes"], None)


_ids = lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"  # noqa: E731
                          for k, v in b.items())


@pytest.mark.parametrize("bad", [dict(clean=NULL), dict(proc=NULL), dict(g_proc=NULL), dict(ws_fwd=NULL),
                                 dict(ws_bwd=NULL), dict(g_d=NULL, g_mean=NULL), dict(B=0), dict(B=-2),
                                 dict(B=65536), dict(T=0), dict(T=-4096), dict(T=255), dict(T=(1 << 30) + 1),
                                 dict(extended=2), dict(extended=-1), dict(ws_fwd=ctypes.c_void_p(0x1004)),
                                 dict(ws_bwd=ctypes.c_void_p(0x1004))], ids=_ids)
def test_stoi_bwd_refuses(bad):
    assert _stoi_bwd(**bad) == SEL_ERR_ARG
    assert b"sel_stoi_bwd" in _lib().sel_last_error()


def test_stoi_bwd_workspace_one_byte_short_is_refused():
    lib = _lib()
    for T in (256, 4096, 30000):
        assert _stoi_bwd(T=T, ws_fwd_bytes=lib.sel_stoi_workspace(2, T) - 1) == SEL_ERR_WORKSPACE
        assert b"sel_stoi_bwd" in lib.sel_last_error()
        assert _stoi_bwd(T=T, ws_bwd_bytes=lib.sel_stoi_bwd_workspace(2, T) - 1) == SEL_ERR_WORKSPACE
        assert b"sel_stoi_bwd" in lib.sel_last_error()


def test_stoi_bwd_workspace_size():
    lib = _lib()
    Ts = [256, 383, 384, 3968, 4096, 4223, 4224, 8000, 30000, 480000]
    Bs = (1, 2, 3, 7, 64)
    for B in Bs:
        sizes = [lib.sel_stoi_bwd_workspace(B, T) for T in Ts]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (B, sizes)
        assert all(s % 8 == 0 for s in sizes), (B, sizes)
    for T in Ts:
        sizes = [lib.sel_stoi_bwd_workspace(B, T) for B in Bs]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (T, sizes)    # one frame: 4 B bytes, rounded up to 8
        assert T < 384 or all(a < b for a, b in zip(sizes, sizes[1:])), (T, sizes)
        # segment adjoints (F - 30) x 30 x 15 and column adjoints (F - 1) x 256 in fp64, the inverse index F ints
        F = (T - 256) // 128 + 1
        for B in Bs:
            want = B * (8 * (max(F - 30, 0) * 450 + (F - 1) * 256) + 4 * F)
            assert lib.sel_stoi_bwd_workspace(B, T) == (want + 7) // 8 * 8, (B, T)
    assert lib.sel_stoi_bwd_workspace(1, 255) == 0 and lib.sel_stoi_bwd_workspace(0, 4096) == 0
    assert lib.sel_stoi_bwd_workspace(-1, 4096) == 0 and lib.sel_stoi_bwd_workspace(3, 0) == 0


def _resample_bwd(**kw):
    a = dict(gy=P, n_wavs=2, len=4800, orig=24, new=5, lpw=6, rolloff=0.99, table=P, gx=P)
    a.update(kw)
    return _lib().sel_resample_bwd(a["gy"], a["n_wavs"], a["len"], a["orig"], a["new"], a["lpw"], a["rolloff"],
                                   a["table"], a["gx"], None)


@pytest.mark.parametrize("bad,code", [(dict(orig=0), SEL_ERR_ARG), (dict(new=-5), SEL_ERR_ARG),
                                      (dict(lpw=0), SEL_ERR_ARG), (dict(rolloff=0.0), SEL_ERR_ARG),
                                      (dict(rolloff=1.5), SEL_ERR_ARG), (dict(n_wavs=-1), SEL_ERR_ARG),
                                      (dict(len=0), SEL_ERR_ARG), (dict(len=-7), SEL_ERR_ARG),
                                      (dict(orig=2001, new=2000), SEL_ERR_UNSUPPORTED),
                                      (dict(n_wavs=65536), SEL_ERR_UNSUPPORTED)], ids=lambda v: _ids(v) if
                         isinstance(v, dict) else str(v))
def test_resample_bwd_refuses(bad, code):
    assert _resample_bwd(**bad) == code
    assert _lib().sel_last_error()


# ---- (e) the Python argument checks -------------------------------------------
def test_stoi_loss_refuses_cpu_tensors_and_mismatched_shapes():
    from losses import STOILoss
    from sel import metrics as M
    x = torch.randn(2, 4096)
    for f in (lambda: STOILoss(10000)(x, x), lambda: STOILoss(48000, extended=True)(x[:, None], x[:, None]),
              lambda: M.stoi_loss_values(x, x, 10000)):
        with pytest.raises(RuntimeError):
            f()
    for a, b in ((x, x[:, :4000]), (x, x[:1]), (x[:, None], x), (x.reshape(2, 2, 2048), x.reshape(2, 2, 2048)),
                 (x[0], x[0])):
        with pytest.raises(ValueError):
            STOILoss(10000)(a, b)
    with pytest.raises(ValueError):
        STOILoss(0)


def test_denoise_step_needs_the_sampling_rate():
    from train_denoise import DenoiseStep
    with pytest.raises(KeyError, match="sampling_rate"):
        DenoiseStep({"lambda_stoi_loss": 1.0}, torch.device("cpu"))
    with pytest.raises(KeyError, match="sampling_rate"):
        DenoiseStep({"lambda_stoi_loss": 0.5, "stoi_loss_extended": True}, torch.device("cpu"))


def test_resample_default_has_no_differentiable_path():
    import inspect
    from sel.resample import resample
    assert inspect.signature(resample).parameters["differentiable"].default is False
