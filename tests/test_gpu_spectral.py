"""GPU parity of the spectral kernels (libsel.so) against the oracle and goldens.

Tolerance (fp32 on both sides, different FFT algorithms / summation orders):
  * spectra / gradients: norm-wise ||a-b||/||b|| <= 1e-4 and elementwise
    |a-b| <= 1e-4*|b| + 1e-5*max|b|  (low-magnitude bins carry absolute slack:
    torch's own fp32 STFT differs from fp64 by up to 1.7e-3 relative there,
    SURVEY §7 hard part 3);
  * scalar losses: <= 1e-4 relative (north_star).
"""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

RES = [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]


def _np(t):
    return t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def spec_close(a, b, rtol=1e-4, floor=1e-5):
    a, b = _np(a).astype(np.float64), _np(b).astype(np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    nb = np.linalg.norm(b)
    assert np.linalg.norm(a - b) <= rtol * nb + 1e-30, np.linalg.norm(a - b) / nb
    bound = rtol * np.abs(b) + floor * np.abs(b).max()
    bad = np.abs(a - b) > bound
    assert not bad.any(), f"{bad.sum()} elements out of bound; worst {np.abs(a - b)[bad].max()}"


def cond_close(ours, ref32, ref64, slack=3.0, floor=1e-4, ref64_for_ref=None):
    """For ill-conditioned gradients: the log-magnitude / log-mel gradients are
    dominated by bins just above the power floor, where any fp32 FFT (torch's
    included) carries ~1e-3 relative error, amplified by the 1/|X|^2 of the
    log-magnitude adjoint.  The reference's own fp32 gradient is 2.4e-3 (norm)
    away from the fp64 truth on the golden input.  Criterion: ours is within
    `slack` x the reference's own fp32 error of the fp64 truth (fp64 oracle =
    the same restated algorithm in float64).  A numpy float32 emulation of our
    FFT has the same RMS error as torch's (2.3e-7 vs 2.2e-7 on windowed noise),
    so the remaining spread is which near-floor bins each rounding pattern hits."""
    o, r, t = (_np(v).astype(np.float64) for v in (ours, ref32, ref64))
    tr = t if ref64_for_ref is None else _np(ref64_for_ref).astype(np.float64)
    nt = np.linalg.norm(t)
    e_ours = np.linalg.norm(o - t) / nt
    e_ref = np.linalg.norm(r - tr) / np.linalg.norm(tr)
    assert e_ours <= max(slack * e_ref, floor), (e_ours, e_ref)


def scalar_close(a, b, rtol=1e-4):
    a, b = float(_np(a)), float(_np(b))
    assert abs(a - b) <= rtol * abs(b) + 1e-12, (a, b)


@pytest.fixture(scope="module")
def S(gpu):
    from sel import spectral
    return spectral


@pytest.fixture(scope="module")
def stft_g():
    return golden("stft")


@pytest.mark.parametrize("n,h,w", RES)
def test_stft_mag_matches_reference_golden(S, gpu, stft_g, n, h, w):
    x = torch.from_numpy(stft_g["x"]).to(gpu)
    win = torch.hann_window(w).to(gpu)
    spec_close(S.stft_mag(x, n, h, w, win), stft_g[f"mag.{n}"])


def test_stft_mag_short_signal(S, gpu, stft_g):
    x = torch.from_numpy(stft_g["short.x"]).to(gpu)
    spec_close(S.stft_mag(x, 2048, 240, 1200, torch.hann_window(1200).to(gpu)), stft_g["short.mag.2048"])


@pytest.mark.parametrize("n,h,w", RES + [(256, 64, 256), (2048, 300, 2048)])
@pytest.mark.parametrize("B,T", [(1, 4001), (3, 24000)])
def test_stft_mag_fwd_bwd_vs_oracle(S, gpu, n, h, w, B, T):
    from oracle import ref_ops as R
    g = torch.Generator().manual_seed(n + h + B)
    x = 0.1 * torch.randn(B, T, generator=g)
    gm = torch.randn(B, 1 + T // h, n // 2 + 1, generator=g)
    xr = x.clone().requires_grad_(True)
    mr = R.stft_mag(xr, n, h, w, R.hann(w))
    mr.backward(gm)
    xd = x.to(gpu).requires_grad_(True)
    md = S.stft_mag(xd, n, h, w, torch.hann_window(w).to(gpu))
    spec_close(md, mr)
    md.backward(gm.to(gpu))
    spec_close(xd.grad, xr.grad)


def test_stft_errors(S, gpu):
    x = torch.randn(2, 1024, device=gpu)
    with pytest.raises(RuntimeError, match="reflect padding"):
        S.stft_mag(x, 2048, 240, 1200, torch.hann_window(1200, device=gpu))
    with pytest.raises(RuntimeError, match="powers of two"):
        S.stft_mag(torch.randn(2, 4000, device=gpu), 1000, 100, 1000, torch.hann_window(1000, device=gpu))
    with pytest.raises(RuntimeError, match="CPU"):
        S.stft_mag(torch.randn(2, 4000), 1024, 120, 600, torch.hann_window(600))
    # the other host limits of check_frame (spectral.hip)
    x = torch.randn(2, 4000, device=gpu)
    with pytest.raises(RuntimeError, match=r"win_length=1200 must be in \(0, n_fft=1024\]"):
        S.stft_mag(x, 1024, 120, 1200, torch.hann_window(1200, device=gpu))
    for n in (128, 4096):
        with pytest.raises(RuntimeError, match=rf"n_fft={n} outside \[256, 2048\]"):
            S.stft_mag(x, n, n // 4, n, torch.hann_window(n, device=gpu))
    # hop = 0 and a 2^29-sample batch straight through the C entry point (the
    # Python wrapper sizes its output from them); both are refused before any
    # launch, so the buffers are never addressed
    from sel import _lib as L
    win = torch.hann_window(600, device=gpu)
    mag = torch.empty(16, device=gpu)
    with pytest.raises(RuntimeError, match="hop must be > 0"):
        L.call("sel_stft_mag_fwd", L.ptr(x), 2, 4000, 1024, 0, 600, L.ptr(win), 1e-7, L.ptr(mag), L.stream())
    with pytest.raises(RuntimeError, match="exceeds 2 GiB per call"):
        L.call("sel_stft_mag_fwd", L.ptr(x), 1 << 15, 1 << 14, 1024, 120, 600, L.ptr(win), 1e-7, L.ptr(mag),
               L.stream())


def test_stft_losses_match_reference_golden(gpu, stft_g):
    from losses import MultiResolutionSTFTLoss, STFTLoss
    x = torch.from_numpy(stft_g["x"]).to(gpu)
    y = torch.from_numpy(stft_g["y"]).to(gpu)
    for n, h, w in RES:
        sc, mg = STFTLoss(n, h, w).to(gpu)(x, y)
        scalar_close(sc, stft_g[f"sc.{n}"])
        scalar_close(mg, stft_g[f"logmag.{n}"])
    xg = x.clone().requires_grad_(True)
    sc, mg = MultiResolutionSTFTLoss().to(gpu)(xg.unsqueeze(1), y.unsqueeze(1))
    (sc + mg).backward()
    scalar_close(sc, stft_g["mr.sc"])
    scalar_close(mg, stft_g["mr.mag"])
    cond_close(xg.grad, stft_g["mr.grad_x"], _mr_grad64(stft_g))
    # the spectral-convergence part alone is well conditioned: plain 1e-4
    xg = x.clone().requires_grad_(True)
    sc, _ = MultiResolutionSTFTLoss().to(gpu)(xg.unsqueeze(1), y.unsqueeze(1))
    sc.backward()
    spec_close(xg.grad, _mr_grad64(stft_g, "sc"))


def _mr_grad64(g, which="both"):
    from oracle import ref_ops as R
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    y = torch.from_numpy(g["y"]).double()
    sc, mg = R.mr_stft_loss(x.unsqueeze(1), y.unsqueeze(1), RES, [R.hann(w).double() for _, _, w in RES])
    {"both": sc + mg, "sc": sc, "mag": mg}[which].backward()
    return x.grad


def test_mag_pair_modules_vs_oracle(gpu):
    from oracle import ref_ops as R
    from losses import LogSTFTMagnitudeLoss, SpectralConvergenceLoss, stft
    g = torch.Generator().manual_seed(5)
    x, y = 0.1 * torch.randn(4, 9000, generator=g), 0.1 * torch.randn(4, 9000, generator=g)
    win = R.hann(600)
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    xm, ym = R.stft_mag(xr, 1024, 120, 600, win), R.stft_mag(yr, 1024, 120, 600, win)
    lr = 0.7 * R.spectral_convergence(xm, ym) + 1.3 * R.log_stft_magnitude(xm, ym)
    lr.backward()
    xd, yd = x.to(gpu).requires_grad_(True), y.to(gpu).requires_grad_(True)
    wd = win.to(gpu)
    xmd, ymd = stft(xd, 1024, 120, 600, wd), stft(yd, 1024, 120, 600, wd)
    ld = 0.7 * SpectralConvergenceLoss()(xmd, ymd) + 1.3 * LogSTFTMagnitudeLoss()(xmd, ymd)
    ld.backward()
    scalar_close(ld, lr)

    def grad64():
        x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
        w64 = win.double()
        a, b = R.stft_mag(x64, 1024, 120, 600, w64), R.stft_mag(y64, 1024, 120, 600, w64)
        (0.7 * R.spectral_convergence(a, b) + 1.3 * R.log_stft_magnitude(a, b)).backward()
        return x64.grad, y64.grad
    gx64, gy64 = grad64()
    cond_close(xd.grad, xr.grad, gx64)
    cond_close(yd.grad, yr.grad, gy64)


def test_mel_matches_reference_golden(gpu):
    from losses import MultiMelSpectrogramLoss
    g = golden("mel")
    gm = golden("melmat")
    p24 = dict(fs=24000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[None], window="hann_window",
               num_mels=80, fmin=0, fmax=24000, log_base=None)
    ml = MultiMelSpectrogramLoss(**p24).to(gpu)
    np.testing.assert_array_equal(_np(ml.mel_transfers[0].melmat), gm["melmat.24k_fmax24000"])
    yh = torch.from_numpy(g["y_hat"]).to(gpu)
    y = torch.from_numpy(g["y"]).to(gpu)
    mel = ml.mel_transfers[0](yh)
    # log-mel: absolute slack for log of floor-clamped (empty) filters
    np.testing.assert_allclose(_np(mel), g["mel24.y_hat"], rtol=1e-4, atol=1e-4)
    yg = yh.clone().requires_grad_(True)
    loss = ml(yg, y)
    loss.backward()
    scalar_close(loss, g["mel24.loss"])
    mt = ml.mel_transfers[0]
    with torch.no_grad():
        ours_d = [mt(yh) - mt(y)]
    cond_close(yg.grad, g["mel24.grad"], _mel_grad64(g["y_hat"], g["y"], [(2048, 300, 2048)],
                                                     [mt.melmat.cpu()], None, ours_d=ours_d),
               ref64_for_ref=_mel_grad64(g["y_hat"], g["y"], [(2048, 300, 2048)], [mt.melmat.cpu()], None))
    mld = MultiMelSpectrogramLoss().to(gpu)
    yg = yh.clone().requires_grad_(True)
    loss = mld(yg, y)
    loss.backward()
    scalar_close(loss, g["meldef.loss"])
    with torch.no_grad():
        ours_d = [mt(yh) - mt(y) for mt in mld.mel_transfers]
    melmats = [m.melmat.cpu() for m in mld.mel_transfers]
    cond_close(yg.grad, g["meldef.grad"], _mel_grad64(g["y_hat"], g["y"], RES, melmats, 10.0, ours_d=ours_d),
               ref64_for_ref=_mel_grad64(g["y_hat"], g["y"], RES, melmats, 10.0))


def _mel_grad64(yh, y, res, melmats, log_base, up=None, ours_d=None, tie_tol=1e-5):
    """fp64 gradient of the mel loss (or of <melspec, up>).  With `ours_d` (per
    resolution, our fp32 mel(y_hat) - mel(y)), the L1 subgradient at near-ties
    |mel64(y_hat) - mel64(y)| < tie_tol (a few fp32 ulps of the log-mel: the sign
    there is decided by rounding, in the reference's fp32 path as in ours) takes
    our sign, so the comparison checks the backward arithmetic, not the tie-break."""
    from oracle import ref_ops as R
    x = torch.as_tensor(yh).double().requires_grad_(True)
    yy = torch.as_tensor(y).double()
    wins = [R.hann(w).double() for _, _, w in res]
    if up is None and ours_d is not None:
        total = 0.0
        for (n, h, w), win, mm, d32 in zip(res, wins, melmats, ours_d):
            mh = R.melspec(x, n, h, w, win, mm.double(), 1e-10, log_base)
            with torch.no_grad():
                d64 = mh - R.melspec(yy, n, h, w, win, mm.double(), 1e-10, log_base)
                sg = torch.where(d64.abs() < tie_tol, torch.sign(d32.double().cpu()), torch.sign(d64))
            total = total + (mh * sg).sum() / mh.numel()
        (total / len(res)).backward()
    elif up is None:
        R.multi_mel_loss(x, yy, res, wins, [m.double() for m in melmats], 1e-10, log_base).backward()
    else:
        (n, h, w), = res
        R.melspec(x, n, h, w, wins[0], melmats[0].double(), 1e-10, log_base).backward(up.double())
    return x.grad


@pytest.mark.parametrize("log_base", [None, 2.0, 10.0])
def test_logmel_fwd_bwd_vs_oracle(gpu, log_base):
    from oracle import ref_ops as R
    from losses import MelSpectrogram
    m = MelSpectrogram(fs=24000, fft_size=1024, hop_size=256, num_mels=80, fmin=0, fmax=12000,
                       log_base=log_base)
    g = torch.Generator().manual_seed(11)
    x = 0.1 * torch.randn(3, 12000, generator=g)
    up = torch.randn(3, 80, 1 + 12000 // 256, generator=g)
    xr = x.clone().requires_grad_(True)
    o = R.melspec(xr, 1024, 256, 1024, m.window, m.melmat, 1e-10, log_base)
    o.backward(up)
    md = m.to(gpu)
    xd = x.to(gpu).requires_grad_(True)
    od = md(xd)
    np.testing.assert_allclose(_np(od), _np(o), rtol=1e-4, atol=2e-5)
    od.backward(up.to(gpu))
    cond_close(xd.grad, xr.grad, _mel_grad64(x, x, [(1024, 256, 1024)], [m.melmat.cpu()], log_base, up))


def test_mel_loss_large_batch_vs_oracle(gpu):
    """C3-shaped mel loss (B=64, 1 s @ 24 kHz) against the oracle."""
    from oracle import ref_ops as R
    from losses import MultiMelSpectrogramLoss
    p24 = dict(fs=24000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[None], window="hann_window",
               num_mels=80, fmin=0, fmax=24000, log_base=None)
    ml = MultiMelSpectrogramLoss(**p24)
    g = torch.Generator().manual_seed(93)
    yh = 0.1 * torch.randn(64, 1, 24000, generator=g)
    y = 0.1 * torch.randn(64, 1, 24000, generator=g)
    yr = yh.clone().requires_grad_(True)
    mt = ml.mel_transfers[0]
    lr = R.multi_mel_loss(yr, y, [(2048, 300, 2048)], [mt.window], [mt.melmat], 1e-10, None)
    lr.backward()
    mld = ml.to(gpu)
    yd = yh.to(gpu).requires_grad_(True)
    ld = mld(yd, y.to(gpu))
    ld.backward()
    scalar_close(ld, lr)
    cond_close(yd.grad, yr.grad, _mel_grad64(yh, y, [(2048, 300, 2048)], [mt.melmat.cpu()], None))


@pytest.mark.parametrize("res,log_base", [((2048, 300, 2048), None), ((1024, 256, 1024), 10.0),
                                          ((512, 128, 400), 2.0), ((256, 64, 256), None)])
def test_mel_l1_fused_matches_separate_path(gpu, res, log_base):
    """The fused log-mel L1 (sel_mel_l1_fwd_grad: one launch computes both
    log-mels per frame and x's adjoint for a unit upstream, the backward scales
    it) against the separate path (log-mel forwards + L1 + log-mel backward):
    same per-element arithmetic, different summation order of the loss and one
    more rounding of the gradient (unit gradient x upstream)."""
    from losses import MultiMelSpectrogramLoss
    from sel import spectral as SP
    n, h, w = res
    ml = MultiMelSpectrogramLoss(fs=24000, fft_sizes=[n], hop_sizes=[h], win_lengths=[w], window="hann_window",
                                 num_mels=80, fmin=0, fmax=12000, log_base=log_base).to(gpu)
    g = torch.Generator().manual_seed(n + h)
    yh = (0.1 * torch.randn(5, 1, 9000, generator=g)).to(gpu)
    y = (0.1 * torch.randn(5, 1, 9000, generator=g)).to(gpu)
    out = {}
    for fused in (True, False):
        prev = SP.MEL_FUSED
        SP.MEL_FUSED = fused
        try:
            x = yh.clone().requires_grad_(True)
            loss = ml(x, y)
            (3.0 * loss).backward()
            out[fused] = (loss.detach(), x.grad)
        finally:
            SP.MEL_FUSED = prev
    torch.testing.assert_close(out[True][0], out[False][0], rtol=2e-6, atol=0)
    ga, gb = out[True][1], out[False][1]
    assert float((ga - gb).norm() / gb.norm()) < 1e-5
    with torch.no_grad():  # no gradient wanted: the log-mel forwards + L1
        torch.testing.assert_close(ml(yh, y), out[False][0], rtol=0, atol=0)


def test_stft_loss_full_size_properties(gpu):
    """At B=512 (beyond the 256 MB Infinity Cache for the magnitudes): the fused
    loss equals the modular (magnitudes materialised) path, and the backward is
    linear in the upstream gradient."""
    from losses import STFTLoss, stft
    from sel import spectral as S
    g = torch.Generator(device=gpu).manual_seed(3)
    x = 0.1 * torch.randn(512, 24000, device=gpu, generator=g)
    y = 0.1 * torch.randn(512, 24000, device=gpu, generator=g)
    mod = STFTLoss(512, 50, 240).to(gpu)
    sc, mg = mod(x, y)
    xm, ym = stft(x, 512, 50, 240, mod.window), stft(y, 512, 50, 240, mod.window)
    out = S.MagPairLoss.apply(xm, ym)
    scalar_close(sc, out[0], 1e-5)
    scalar_close(mg, out[1], 1e-5)
    xg = x.clone().requires_grad_(True)
    s1, m1 = mod(xg, y)
    (s1 + m1).backward()
    g1 = xg.grad.clone()
    xg.grad = None
    s2, m2 = mod(xg, y)
    (2.0 * s2 + 2.0 * m2).backward()
    spec_close(xg.grad, 2.0 * g1, rtol=1e-6, floor=0)


def test_buffer_b64_loads_at_dword_offsets(gpu):
    """Root cause of round 1's "raw_buffer_load_b64 returned wrong pairs"
    (spectral.hip fetch_frame).  Through the STFT kernels' own buffer resource:
    * 8-byte buffer loads are exact at EVERY dword offset (4-mod-8 included), so
      neither gfx950 nor the descriptor (word3 0x00020000) was at fault;
    * the r1 code took the two floats with __builtin_bit_cast(float, v[i]) on
      the returned ext_vector, which ROCm 7.2's clang lowers to a load from the
      vector's base: element 0 twice (ISA: one buffer_load_dword + v_mov).  Mode
      1 reproduces that form; if a fixed compiler ever makes it exact, this test
      says so instead of failing.
    The kernels now take vector elements as scalars (and keep plain 8-B global
    loads for aligned interior frames)."""
    from sel import _lib as L
    n = 4097
    x = torch.arange(n, dtype=torch.float32, device=gpu) + 0.5
    want = torch.stack([x[:-1], x[1:]], 1).cpu()
    res = {}
    for mode in (0, 1):
        out = torch.full((2 * n,), -1.0, device=gpu)
        L.call("sel_probe_buffer_b64", L.ptr(x), n, mode, L.ptr(out), L.stream())
        res[mode] = out[: 2 * (n - 1)].view(n - 1, 2).cpu()
    assert torch.equal(res[0], want), "b64 buffer loads must be exact at every dword offset"
    dup = torch.equal(res[1][:, 1], want[:, 0]) and torch.equal(res[1][:, 0], want[:, 0])
    assert dup or torch.equal(res[1], want), res[1][:3]
    print(f"bit_cast(float, v[1]) of a buffer_load_b64 result: {'element 0 (miscompiled)' if dup else 'exact'}")


@pytest.mark.parametrize("T,hop,n_fft,win", [(4801, 75, 1024, 600), (3333, 111, 512, 240), (2049, 33, 2048, 1200)])
def test_stft_mag_odd_alignment_vs_oracle(gpu, T, hop, n_fft, win):
    """Frames starting at odd sample offsets (odd hop, odd T: 4-byte-aligned
    frame starts in every signal but the first) through the STFT |X| kernel vs
    the oracle: the fetch must pick the per-dword path for them."""
    from losses import stft
    from oracle import ref_ops as R
    torch.manual_seed(T + hop)
    x = torch.randn(3, T)
    w = torch.hann_window(win)
    got = stft(x.to(gpu), n_fft, hop, win, w.to(gpu))
    ref = R.stft_mag(x.double(), n_fft, hop, win, w.double())
    e = ((got.double().cpu() - ref).norm() / ref.norm()).item()
    assert e < 1e-5, e
