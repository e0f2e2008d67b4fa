"""The spectral frame kernels (csrc/spectral.hip) at forced multi-pass launch
plans and edge-frame shapes, against the float64 oracle.

Every frame kernel walks `iters` consecutive frame groups per block
(FRAME_LOOP_BEGIN / FramePos::advance; the |X| forward below n_fft 2048 draws
one-wave units from an LDS counter instead, k_stft_mag_fwd / unit_pos).  The
default plan only reaches iters > 1 above ~2000 frame groups; tune key 14 fixes
iters = v for every frame kernel, so the loop bookkeeping (one-ahead prefetch,
signal-boundary carry, inactive tail slots, empty trailing passes, the counter
draw) is reached here on a few thousand samples.

Shapes (B, T, n_fft, hop, win); F = 1 + T // hop frames per signal; FPB =
frames per 256-lane block pass = 16 / 8 / 4 / 2 for n_fft 256 / 512 / 1024 /
2048 (Geo<LOGN>::FPB); groups = ceil(B F / FPB); grid = ceil(groups / v):

  id  shape                      frames groups  what it reaches
  A   (7, 130, 256, 64, 256)       21     2    T = n_fft/2 + 2: every frame touches both reflect pads (both
                                               folds of k_ola_fold land on one sample); F = 3 < FPB = 16: one
                                               pass spans 5+ signals (the while (f >= F) carry runs repeatedly)
  B   (5, 301, 512, 50, 240)       35     5    T < n_fft, F = 7 < FPB = 8, odd T (odd signal offsets), win < n_fft
  C   (3, 1333, 1024, 111, 600)    39    10    odd hop and odd T: interior frames at 4-mod-8 addresses (signal b,
                                               frame f is 8-byte aligned iff b + f is even) -> fetch_frame's
                                               per-sample buffer path on interior frames; last group 3 of 4
  D   (3, 1100, 2048, 240, 1200)   15     8    two-wave frames (block barrier between passes), T < n_fft, F = 5
  E   (2, 4801, 2048, 75, 2048)   130    65    two-wave frames, odd hop, the largest shape
  F   (9, 777, 256, 33, 200)      216    14    four frames per wave: interior, edge, misaligned and inactive
                                               lanes in one wave
  G   (4, 1000, 256, 300, 200)     16     1    hop > win and hop > n_fft: samples no window reaches
  H   shape C, base address = 4 (mod 8)        alignment of every frame flipped against C (aligned iff b + f odd)

Launch plans of the 256-lane kernels (k_stft_mag_bwd, k_stft_loss_fwd/bwd,
k_logmel_fwd/bwd, k_mel_l1; also the |X| forward at n_fft 2048) at v > 0:

  * several blocks, the last with a partly filled pass AND a wholly empty one:
    B v=2 (3 blocks; last: 3 of 8 frames, then empty), B v=3 (2 blocks), C/H
    v=3 (4 blocks; last: 3 of 4 frames, then two empty passes), D v=3 (3
    blocks; last: full, 1 of 2, empty), D v=5 (2 blocks; last: two full, 1 of
    2, two empty), F v=3 (5 blocks; last: full, 8 of 16, empty), F v=5 (3);
  * several blocks, the last with full passes and a wholly empty one: E v=2
    (33 blocks; last 1 of 2 passes), E v=3 (22 blocks; last 2 of 3 passes);
  * several blocks, last pass of the last block partly filled, none empty: C/H
    v=2 (5 blocks), C/H v=5 (2 blocks), D v=2 (4), F v=2 (7); exact fit: E v=5;
  * one block with empty trailing passes: A v=3 (full, 5 of 16, empty), A v=5,
    G v=2/3/5 (16 frames = one pass); one block, last pass partly filled, none
    empty: A v=2, B v=5.

The |X| forward below n_fft 2048 is a 1024-lane block of 16 waves owning
16 v units of 64 / LPF frames (4 / 2 / 1 for n_fft 256 / 512 / 1024); a wave
draws from the counter only when its block owns more than 16 units: B v>=2
(18 units in one block), C/H v=2 (blocks of 32 and 7 units), C/H v=3,5 (39 in
one block), F v=2 (32 + 22), F v=3 (48 + 6), F v=5 (54 in one block).  A and G
(6 and 4 units) check the tail (ue) clamp only.

Which case covers which kernel: test_stft_mag -> k_stft_mag_fwd/bwd (+
k_ola_fold); test_stft_loss -> k_stft_loss_fwd/bwd; test_logmel ->
k_logmel_fwd/bwd; test_mel_loss[fused] -> k_mel_l1, [separate] ->
k_logmel_fwd (paired launch) + k_logmel_bwd with the L1 sign upstream.  T <
n_fft: A, B, D (G: frames past T).  4-mod-8 frame addresses: C, E, F, H (B:
odd signal offsets, no interior frame).

Tolerances are the project's own (tests/test_gpu_spectral.py):
spec_close 1e-4 norm-wise + elementwise with a 1e-5 floor; scalar_close 1e-4;
log-mel values rtol 1e-4 / atol 2e-5; ill-conditioned gradients (log-mag,
log-mel) cond_close = within 3x the oracle's own fp32 error of the fp64 truth.
Across v the per-frame results must be bit-identical (no batch-wide sum feeds
them); loss scalars and the stft_loss gradient (fp32 coefficients from fp64
sums of block partials, whose order follows the grid) agree to 1e-6.

Measured on the MI355X against the fp64 oracle (worst over all shapes and v;
identical across v wherever bit-identity is asserted):

  k_stft_mag_fwd    |X|              1.1e-7 norm-wise (E)
  k_stft_mag_bwd    gradient         3.6e-7 norm-wise (A)
  k_stft_loss_fwd   SC / log-mag     1.8e-7 / 8.2e-8 relative (F); silence target 1.1e-7 / 1.3e-7
  k_stft_loss_bwd   SC gradient      2.7e-7 norm-wise (A); silence target 1.5e-7
                    SC + log-mag     1.9e-4 norm-wise (D) where the oracle's own fp32 gradient is 4.4e-4 off
                                     (the oracle's worst: 6.7e-4 at E, ours 5.6e-5 there)
  k_logmel_fwd      log-mel          2.4e-5 max abs (G, natural log; the fp32 oracle: 2.3e-5)
  k_logmel_bwd      gradient         2.3e-5 norm-wise (G; the fp32 oracle: 9.6e-5)
  k_mel_l1          loss / gradient  1.4e-7 (C) / 2.3e-5 norm-wise (G; the fp32 oracle: 9.4e-5)
  separate mel path loss / gradient  the same figures to the digits shown

No near-tie bin (|d64| < 1e-5) occurs with these seeds, at either log base,
silence target included, so _mel_grad64's sign substitution is idle here (the
cap of TIE_CAP bins is asserted all the same).  No kernel defect was found: all
cases passed as first written.
"""
import contextlib

import numpy as np
import pytest
import torch

from test_gpu_spectral import _mel_grad64, _np, cond_close, scalar_close, spec_close

pytestmark = pytest.mark.gpu

#        B   T    n_fft  hop  win   seed
SHAPES = {
    "A": (7, 130, 256, 64, 256, 101),
    "B": (5, 301, 512, 50, 240, 102),
    "C": (3, 1333, 1024, 111, 600, 103),
    "D": (3, 1100, 2048, 240, 1200, 104),
    "E": (2, 4801, 2048, 75, 2048, 105),
    "F": (9, 777, 256, 33, 200, 106),
    "G": (4, 1000, 256, 300, 200, 107),
    "H": (3, 1333, 1024, 111, 600, 108),
}
SIDS = list(SHAPES)
VS = [0, 2, 3, 5]
LOG_BASES = [None, 10.0]
MEL = dict(fs=24000, num_mels=80, fmin=0, fmax=12000)
TIE_TOL = 1e-5   # _mel_grad64's near-tie threshold
TIE_CAP = 2      # near-tie bins a case may substitute at most
SILENCE_SIDS = ["A", "C", "E"]


def _geom(sid):
    B, T, n, h, w, _ = SHAPES[sid]
    return B, T, n, h, w, 1 + T // h


_INPUTS, _REF, _RUNS, _MODS = {}, {}, {}, {}


def _inputs(sid):
    """x, y = 0.1 randn; gm / up = randn upstreams of |X| and of the log-mel."""
    if sid not in _INPUTS:
        B, T, n, h, w, F = _geom(sid)
        g = torch.Generator().manual_seed(SHAPES[sid][5])
        _INPUTS[sid] = dict(x=0.1 * torch.randn(B, T, generator=g), y=0.1 * torch.randn(B, T, generator=g),
                            gm=torch.randn(B, F, n // 2 + 1, generator=g),
                            up=torch.randn(B, MEL["num_mels"], F, generator=g))
    return _INPUTS[sid]


def _target(sid, silence):
    y = _inputs(sid)["y"]
    return torch.zeros_like(y) if silence else y


def _mel_module(sid, log_base):
    """(MelSpectrogram on the CPU, its fp32 filterbank): the oracle's parameters."""
    from losses import MelSpectrogram
    _, _, n, h, w, _ = _geom(sid)
    key = ("cpu", n, h, w, log_base)
    if key not in _MODS:
        _MODS[key] = MelSpectrogram(fft_size=n, hop_size=h, win_length=w, log_base=log_base, **MEL)
    return _MODS[key]


def _cached(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


# ---- float64 (and fp32) oracle, once per shape ---------------------------------

def _ref_mag(sid):
    def make():
        from oracle import ref_ops as R
        _, _, n, h, w, _ = _geom(sid)
        I = _inputs(sid)
        x = I["x"].double().requires_grad_(True)
        m = R.stft_mag(x, n, h, w, R.hann(w).double())
        m.backward(I["gm"].double())
        return m.detach(), x.grad
    return _cached(_REF, ("mag", sid), make)


def _ref_loss(sid, silence=False):
    def make():
        from oracle import ref_ops as R
        _, _, n, h, w, _ = _geom(sid)
        out = {}
        for dt in (torch.float64, torch.float32):
            win = R.hann(w).to(dt)
            y = _target(sid, silence).to(dt)
            for which in ("sc", "both"):
                x = _inputs(sid)["x"].to(dt, copy=True).requires_grad_(True)
                sc, mg = R.stft_loss(x, y, n, h, w, win)
                (sc if which == "sc" else sc + mg).backward()
                out[which, dt] = x.grad
            out["sc_val", dt], out["mg_val", dt] = sc.detach(), mg.detach()
        return out
    return _cached(_REF, ("loss", sid, silence), make)


def _ref_logmel(sid, log_base):
    def make():
        from oracle import ref_ops as R
        _, _, n, h, w, _ = _geom(sid)
        I, m = _inputs(sid), _mel_module(sid, log_base)
        o64 = R.melspec(I["x"].double(), n, h, w, R.hann(w).double(), m.melmat.double(), 1e-10, log_base)
        x = I["x"].clone().requires_grad_(True)
        R.melspec(x, n, h, w, m.window, m.melmat, 1e-10, log_base).backward(I["up"])
        g64 = _mel_grad64(I["x"], I["x"], [(n, h, w)], [m.melmat], log_base, I["up"])
        return o64, x.grad, g64
    return _cached(_REF, ("logmel", sid, log_base), make)


def _near_ties(sid, log_base, silence=False):
    """Bins of the fp64 log-mel difference under TIE_TOL.  Filters with no
    FFT bin (all-zero melmat columns: the narrow low filters at n_fft 256) are
    left out: both log-mels are log(eps) there in every precision, the
    difference is exactly 0 and sign(0) = 0 with or without the substitution."""
    from oracle import ref_ops as R
    _, _, n, h, w, _ = _geom(sid)
    m = _mel_module(sid, log_base)
    mm, win = m.melmat.double(), R.hann(w).double()
    d = (R.melspec(_inputs(sid)["x"].double(), n, h, w, win, mm, 1e-10, log_base)
         - R.melspec(_target(sid, silence).double(), n, h, w, win, mm, 1e-10, log_base))
    live = (m.melmat != 0).any(0)
    return int((d.abs() < TIE_TOL)[:, live, :].sum())


def _ref_mel(sid, log_base, silence=False):
    def make():
        from oracle import ref_ops as R
        _, _, n, h, w, _ = _geom(sid)
        m = _mel_module(sid, log_base)
        y = _target(sid, silence)
        x = _inputs(sid)["x"].clone().requires_grad_(True)
        R.multi_mel_loss(x, y, [(n, h, w)], [m.window], [m.melmat], 1e-10, log_base).backward()
        x64 = _inputs(sid)["x"].double()
        loss64 = R.multi_mel_loss(x64, y.double(), [(n, h, w)], [R.hann(w).double()], [m.melmat.double()], 1e-10,
                                  log_base)
        g64 = _mel_grad64(_inputs(sid)["x"], y, [(n, h, w)], [m.melmat], log_base)
        return dict(loss64=loss64, g32=x.grad, g64=g64, ties=_near_ties(sid, log_base, silence))
    return _cached(_REF, ("mel", sid, log_base, silence), make)


def _covered(sid):
    """Samples some analysis window reaches: frame f holds padded positions
    f hop + (n_fft - win)//2 + [0, win), and padded position p is sample
    reflect(p - n_fft/2)."""
    _, T, n, h, w, F = _geom(sid)
    p = (np.arange(F)[:, None] * h + (n - w) // 2 + np.arange(w)[None, :] - n // 2).ravel()
    p = np.abs(p)
    p = np.where(p >= T, 2 * (T - 1) - p, p)
    assert p.min() >= 0 and p.max() < T
    cov = np.zeros(T, dtype=bool)
    cov[p] = True
    return cov


# ---- the product's entry points on the GPU, once per (shape, v) ---------------------

@contextlib.contextmanager
def _forced(v):
    from sel import _lib as L
    lib = L.lib()
    prev = lib.sel_tune(14, v)
    try:
        yield
    finally:
        lib.sel_tune(14, prev)


def _dev(sid, t, gpu):
    """The tensor on the GPU; shape H: at a base address of 4 (mod 8)."""
    if sid != "H":
        return t.to(gpu)
    buf = torch.empty(t.numel() + 1, device=gpu)
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 8 == 4
    return d


def _run_mag(sid, v, gpu):
    def make():
        from sel import spectral as S
        _, _, n, h, w, _ = _geom(sid)
        I = _inputs(sid)
        with _forced(v):
            x = _dev(sid, I["x"], gpu).requires_grad_(True)
            m = S.stft_mag(x, n, h, w, torch.hann_window(w).to(gpu))
            m.backward(I["gm"].to(gpu))
            return m.detach().cpu(), x.grad.cpu()
    return _cached(_RUNS, ("mag", sid, v), make)


def _run_loss(sid, v, gpu, silence=False):
    def make():
        from sel import spectral as S
        _, _, n, h, w, _ = _geom(sid)
        out = {}
        with _forced(v):
            win = torch.hann_window(w).to(gpu)
            y = _dev(sid, _target(sid, silence), gpu)
            for which in ("sc", "both"):
                x = _dev(sid, _inputs(sid)["x"], gpu).requires_grad_(True)
                sc, mg = S.stft_loss(x, y, n, h, w, win)
                (sc if which == "sc" else sc + mg).backward()
                out[which] = x.grad.cpu()
            out["sc_val"], out["mg_val"] = sc.detach().cpu(), mg.detach().cpu()
        return out
    return _cached(_RUNS, ("loss", sid, v, silence), make)


def _gpu_mel_module(sid, log_base, gpu):
    from losses import MelSpectrogram
    _, _, n, h, w, _ = _geom(sid)
    key = ("gpu", n, h, w, log_base)
    if key not in _MODS:
        _MODS[key] = MelSpectrogram(fft_size=n, hop_size=h, win_length=w, log_base=log_base, **MEL).to(gpu)
    return _MODS[key]


def _run_logmel(sid, v, log_base, gpu):
    def make():
        m = _gpu_mel_module(sid, log_base, gpu)
        I = _inputs(sid)
        with _forced(v):
            x = _dev(sid, I["x"], gpu).requires_grad_(True)
            o = m(x)
            o.backward(I["up"].to(gpu))
            return o.detach().cpu(), x.grad.cpu()
    return _cached(_RUNS, ("logmel", sid, v, log_base), make)


def _run_mel(sid, v, log_base, fused, gpu, silence=False):
    def make():
        from losses import MultiMelSpectrogramLoss
        from sel import spectral as SP
        _, _, n, h, w, _ = _geom(sid)
        key = ("gpu-loss", n, h, w, log_base)
        if key not in _MODS:
            _MODS[key] = MultiMelSpectrogramLoss(fft_sizes=[n], hop_sizes=[h], win_lengths=[w], window="hann_window",
                                                 log_base=log_base, **MEL).to(gpu)
        ml = _MODS[key]
        prev = SP.MEL_FUSED
        SP.MEL_FUSED = fused
        try:
            with _forced(v):
                x = _dev(sid, _inputs(sid)["x"], gpu).requires_grad_(True)
                y = _dev(sid, _target(sid, silence), gpu)
                loss = ml(x, y)
                loss.backward()
                mt = ml.mel_transfers[0]
                with torch.no_grad():
                    d = (mt(x) - mt(y)).cpu()
                return loss.detach().cpu(), x.grad.cpu(), d
        finally:
            SP.MEL_FUSED = prev
    return _cached(_RUNS, ("mel", sid, v, log_base, fused, silence), make)


def _rel(a, b):
    a, b = _np(a).astype(np.float64), _np(b).astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _report(what, sid, v, **figs):
    print(f"EDGE {what} {sid} v={v} " + " ".join(f"{k}={e:.3e}" for k, e in figs.items()))


# ---- vs the oracle ---------------------------------------------------------------

@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("sid", SIDS)
def test_stft_mag(gpu, sid, v):
    m64, g64 = _ref_mag(sid)
    m, g = _run_mag(sid, v, gpu)
    _report("mag", sid, v, fwd=_rel(m, m64), bwd=_rel(g, g64))
    spec_close(m, m64)
    spec_close(g, g64)


@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("sid", SIDS)
def test_stft_loss(gpu, sid, v):
    ref, got = _ref_loss(sid), _run_loss(sid, v, gpu)
    f64, f32 = torch.float64, torch.float32
    _report("loss", sid, v, sc=_rel(got["sc_val"], ref["sc_val", f64]), mg=_rel(got["mg_val"], ref["mg_val", f64]),
            g_sc=_rel(got["sc"], ref["sc", f64]), g_both=_rel(got["both"], ref["both", f64]),
            g_both_ref32=_rel(ref["both", f32], ref["both", f64]))
    scalar_close(got["sc_val"], ref["sc_val", f64])
    scalar_close(got["mg_val"], ref["mg_val", f64])
    spec_close(got["sc"], ref["sc", f64])  # spectral convergence alone is well conditioned
    cond_close(got["both"], ref["both", f32], ref["both", f64])


@pytest.mark.parametrize("log_base", LOG_BASES)
@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("sid", SIDS)
def test_logmel(gpu, sid, v, log_base):
    o64, g32, g64 = _ref_logmel(sid, log_base)
    o, g = _run_logmel(sid, v, log_base, gpu)
    _report(f"logmel[{log_base}]", sid, v, fwd_maxabs=float((o.double() - o64).abs().max()), bwd=_rel(g, g64),
            bwd_ref32=_rel(g32, g64))
    np.testing.assert_allclose(_np(o), o64.numpy(), rtol=1e-4, atol=2e-5)
    cond_close(g, g32, g64)


def _check_mel(gpu, sid, v, log_base, fused, silence):
    _, _, n, h, w, _ = _geom(sid)
    ref = _ref_mel(sid, log_base, silence)
    # the near-tie substitution below may not carry the comparison
    assert ref["ties"] <= TIE_CAP, ref["ties"]
    loss, g, d = _run_mel(sid, v, log_base, fused, gpu, silence)
    mm = _mel_module(sid, log_base).melmat
    g64_ours = _mel_grad64(_inputs(sid)["x"], _target(sid, silence), [(n, h, w)], [mm], log_base, ours_d=[d])
    _report(f"mel[{log_base},{'fused' if fused else 'separate'}{',silence' if silence else ''}]", sid, v,
            loss=_rel(loss, ref["loss64"]), grad=_rel(g, g64_ours), grad_ref32=_rel(ref["g32"], ref["g64"]))
    scalar_close(loss, ref["loss64"])
    cond_close(g, ref["g32"], g64_ours, ref64_for_ref=ref["g64"])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("log_base", LOG_BASES)
@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("sid", SIDS)
def test_mel_loss(gpu, sid, v, log_base, fused):
    _check_mel(gpu, sid, v, log_base, fused, False)


# ---- across launch plans -----------------------------------------------------------

@pytest.mark.parametrize("v", VS[1:])
@pytest.mark.parametrize("sid", SIDS)
def test_forced_passes_match_default_plan(gpu, sid, v):
    """Same shape and inputs at iters = v against the default plan.  A frame's
    |X|, log-mels and frame gradient depend on nothing outside the frame, and the
    overlap-add is a fixed-order gather: bit-identical.  The loss scalars sum
    block partials in grid order, and the stft_loss gradient takes its two fp32
    coefficients from those fp64 sums: 1e-6."""
    for a, b in zip(_run_mag(sid, v, gpu), _run_mag(sid, 0, gpu)):
        assert torch.equal(a, b), ("stft_mag", _rel(a, b))
    for lb in LOG_BASES:
        for a, b in zip(_run_logmel(sid, v, lb, gpu), _run_logmel(sid, 0, lb, gpu)):
            assert torch.equal(a, b), ("logmel", lb, _rel(a, b))
        for fused in (True, False):
            (la, ga, _), (lb0, gb, _) = _run_mel(sid, v, lb, fused, gpu), _run_mel(sid, 0, lb, fused, gpu)
            assert torch.equal(ga, gb), ("mel grad", lb, fused, _rel(ga, gb))
            scalar_close(la, lb0, 1e-6)
    a, b = _run_loss(sid, v, gpu), _run_loss(sid, 0, gpu)
    scalar_close(a["sc_val"], b["sc_val"], 1e-6)
    scalar_close(a["mg_val"], b["mg_val"], 1e-6)
    for which in ("sc", "both"):
        assert _rel(a[which], b[which]) <= 1e-6, (which, _rel(a[which], b[which]))


# ---- digital silence target ----------------------------------------------------------

@pytest.mark.parametrize("v", [0, 3])
@pytest.mark.parametrize("sid", SILENCE_SIDS)
def test_silence_target(gpu, sid, v):
    """y = 0: every |Y| bin sits on the power floor, sum |Y|^2 = frames x bins x
    1e-7, so one phantom (inactive) frame slot counted in the sums moves SC by
    ~1/(2 frames): percent at these sizes.  (Tried once with a build of
    k_stft_loss_fwd that summed inactive slots too: A and C at both v and E at
    v=3 failed here, E at v=0 has no inactive slot, and every test_stft_loss
    case with an ordinary target still passed.)"""
    ref, got = _ref_loss(sid, True), _run_loss(sid, v, gpu, True)
    f64 = torch.float64
    _report("silence", sid, v, sc=_rel(got["sc_val"], ref["sc_val", f64]), mg=_rel(got["mg_val"], ref["mg_val", f64]),
            g_sc=_rel(got["sc"], ref["sc", f64]))
    scalar_close(got["sc_val"], ref["sc_val", f64])
    scalar_close(got["mg_val"], ref["mg_val", f64])
    spec_close(got["sc"], ref["sc", f64])
    for log_base in LOG_BASES:
        for fused in (True, False):
            _check_mel(gpu, sid, v, log_base, fused, True)


# ---- samples no window reaches --------------------------------------------------------

@pytest.mark.parametrize("v", VS)
def test_uncovered_samples_get_zero_gradient(gpu, v):
    """Shape G (hop > win): 100 of every 300 samples lie under no window (299 of
    the 1000: the first frame's reflected half covers sample 100 too); their
    gradient is exactly 0.0 in every backward (the overlap-add finds no frame)."""
    sid = "G"
    hole = torch.from_numpy(~_covered(sid))
    assert int(hole.sum()) == 299
    assert not _ref_mag(sid)[1][:, hole].any()  # the mask against the oracle
    assert _ref_mag(sid)[1][:, ~hole].ne(0).float().mean() > 0.95
    grads = {"stft_mag": _run_mag(sid, v, gpu)[1], "stft_loss sc": _run_loss(sid, v, gpu)["sc"],
             "stft_loss sc+mag": _run_loss(sid, v, gpu)["both"]}
    for fused in (True, False):
        grads[f"mel fused={fused}"] = _run_mel(sid, v, None, fused, gpu)[1]
    for name, g in grads.items():
        assert g[:, hole].eq(0).all(), (name, float(g[:, hole].abs().max()))
        assert g[:, ~hole].ne(0).float().mean() > 0.95, name
