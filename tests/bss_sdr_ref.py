"""fp64 numpy restatement of the BSS-eval SDR of DESIGN §23 (torchmetrics 1.2.0
signal_distortion_ratio with the direct solve).  This is the reference of
tests/test_bss_sdr_host.py and tests/test_gpu_bss_sdr.py, never the code under
test: direct linear correlations and numpy.linalg.solve on the explicit
Toeplitz matrix.  sdr_fft follows torchmetrics' FFT formulation literally, for
the cross-check at T >= L.  It also carries the case recipe both files share."""
import numpy as np


def _prep(pred, target, zero_mean):
    p = np.asarray(pred, np.float64)
    t = np.asarray(target, np.float64)
    if zero_mean:
        p = p - p.mean()
        t = t - t.mean()
    t = t / max(np.linalg.norm(t), 1e-6)
    p = p / max(np.linalg.norm(p), 1e-6)
    return p, t


def correlations(p, t, L):
    """r[k] = sum_n t[n] t[n + k], b[k] = sum_n t[n] p[n + k], k < L; linear: lags k >= T are 0."""
    T = len(t)
    r, b = np.zeros(L), np.zeros(L)
    for k in range(min(L, T)):
        r[k] = np.dot(t[:T - k], t[k:])
        b[k] = np.dot(t[:T - k], p[k:])
    return r, b


def corr_ref(pred, target, L, zero_mean=False, load_diag=None):
    """(r, b) as the solve sees them: after the scaling and load_diag."""
    p, t = _prep(pred, target, zero_mean)
    r, b = correlations(p, t, L)
    if load_diag is not None:
        r[0] += load_diag
    return r, b


def _toeplitz(r):
    i = np.arange(len(r))
    return r[np.abs(i[:, None] - i[None, :])]


def _value(coh):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.inf) if 1.0 - coh <= 0.0 else float(10.0 * np.log10(coh / (1.0 - coh)))


def sdr_full(pred, target, L=512, zero_mean=False, load_diag=None, want_cond=True):
    """One pair of 1-D signals -> dict(val, coh, r, b, cond); cond (the 2-norm
    condition number of R, from its eigenvalues) is None unless asked for."""
    r, b = corr_ref(pred, target, L, zero_mean, load_diag)
    R = _toeplitz(r)
    sol = np.linalg.solve(R, b)
    coh = float(b @ sol)
    cond = None
    if want_cond:
        ev = np.abs(np.linalg.eigvalsh(R))
        cond = float(ev.max() / ev.min())
    return dict(val=_value(coh), coh=coh, r=r, b=b, cond=cond)


def sdr_fft(pred, target, L=512, zero_mean=False, load_diag=None):
    """torchmetrics' formulation: correlations from an FFT of length 2^ceil(log2(2T - 1)), [:L] kept."""
    p, t = _prep(pred, target, zero_mean)
    T = len(t)
    n_fft = 2 ** int(np.ceil(np.log2(2 * T - 1))) if T > 1 else 1
    tf = np.fft.rfft(t, n_fft)
    r = np.fft.irfft(tf.real ** 2 + tf.imag ** 2, n_fft)[:L]
    b = np.fft.irfft(np.conj(tf) * np.fft.rfft(p, n_fft), n_fft)[:L]
    if load_diag is not None:
        r[0] += load_diag
    sol = np.linalg.solve(_toeplitz(r), b)
    return _value(float(b @ sol))


# ---- the shared cases ------------------------------------------------------
KINDS = ("white", "ar2", "voiced")
SNRS = (30, 10, 0)
SEEDS = (0, 1)


def _ar2(e):
    """scipy.signal.lfilter([1], [1, -1.8, 0.9], e)"""
    y = np.zeros(len(e) + 2)
    for n in range(len(e)):
        y[n + 2] = e[n] + 1.8 * y[n + 1] - 0.9 * y[n]
    return y[2:]


def clean(kind, seed, T):
    r = np.random.default_rng(seed)
    if kind == "white":
        return r.standard_normal(T)
    if kind == "ar2":
        return _ar2(r.standard_normal(T))
    if kind == "voiced":
        t = np.arange(T) / 48000
        f0 = r.uniform(100, 180)
        car = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + r.uniform(0, 6.28)) / (h + 1) for h in range(24))
        env = 0.3 + 0.7 * np.sin(2 * np.pi * r.uniform(2, 4) * t + r.uniform(0, 6.28)) ** 2
        return 0.1 * car * env + 1e-4 * r.standard_normal(T)
    raise ValueError(kind)


def noisy(x, seed, snr):
    n = np.random.default_rng(1000 + seed).standard_normal(len(x))
    return x + n * np.linalg.norm(x) / np.linalg.norm(n) * 10 ** (-snr / 20)


_cache = {}


def case(kind, snr, seed, T):
    """-> (pred, target) fp32 arrays (what the GPU is given); cached, read-only."""
    key = (kind, snr, seed, T)
    if key not in _cache:
        x = clean(kind, seed, T)
        y = noisy(x, seed, snr)
        x, y = x.astype(np.float32), y.astype(np.float32)
        x.setflags(write=False)
        y.setflags(write=False)
        _cache[key] = (y, x)
    return _cache[key]


_ref_cache = {}


def case_ref(kind, snr, seed, T, L, want_cond=False):
    """fp64 reference of the fp32 inputs of case(); cached, read-only."""
    key = (kind, snr, seed, T, L)
    if key not in _ref_cache or (want_cond and _ref_cache[key]["cond"] is None):
        _ref_cache[key] = sdr_full(*case(kind, snr, seed, T), L, want_cond=want_cond)
    return _ref_cache[key]


def value_shapes(C):
    """(T, L) of the value cases of the GPU test; C = sel_bss_sdr_chunk()."""
    out = []
    for L in (1, 64, 65, 512):
        for T in (63, L, L + 1, C - 1, C + 1, C + L, 3 * C + 17):
            if (T, L) not in out:
                out.append((T, L))
    return out


ALL_CASES = [(k, q, s) for k in KINDS for q in SNRS for s in SEEDS]
