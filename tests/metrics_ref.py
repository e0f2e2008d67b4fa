"""fp64 numpy restatement of the evaluation measures of DESIGN §22: the SDR
family (torchmetrics 1.2.0 formulas) and STOI / ESTOI at 10 kHz.  This is the
reference of tests/test_metrics_host.py and tests/test_gpu_metrics.py, never
the code under test.  It also carries the case recipe both files share, and
returns each clean signal's margin: the distance in dB of the nearest frame
energy from the silent-frame threshold (a case whose margin is small could keep
a different frame set in fp32 than in fp64)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
EPS = float(np.finfo(np.float64).eps)        # 2.220446049250313e-16
FS, FRAME, HOP, NFFT, NBANDS, NSEG, DYN = 10000, 256, 128, 512, 15, 30, 40.0
BETA = 1.0 + 10.0 ** (15.0 / 20.0)


# ---- SDR family ----------------------------------------------------------
def sdr_db(pred, target, scale_invariant, zero_mean, xp=np):
    """per-row values, (B, T) -> (B).  xp = numpy, or torch for fp64 autograd."""
    p, t = pred, target
    if zero_mean:
        p = p - p.mean(-1, keepdims=True) if xp is np else p - p.mean(-1, keepdim=True)
        t = t - t.mean(-1, keepdims=True) if xp is np else t - t.mean(-1, keepdim=True)
    if scale_invariant:
        alpha = ((p * t).sum(-1) + EPS32) / ((t * t).sum(-1) + EPS32)
        ts = alpha[..., None] * t
        val = ((ts * ts).sum(-1) + EPS32) / (((ts - p) ** 2).sum(-1) + EPS32)
    else:
        val = ((t * t).sum(-1) + EPS32) / (((t - p) ** 2).sum(-1) + EPS32)
    return 10.0 * xp.log10(val)


# ---- STOI / ESTOI ----------------------------------------------------------
def window():
    return np.hanning(FRAME + 2)[1:-1]


def band_edges():
    """(lo, hi) bin pairs of the 15 third-octave bands on the 10000 / 512 grid."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NBANDS, dtype=np.float64)
    lo = 150.0 * 2.0 ** ((2 * k - 1) / 6)
    hi = 150.0 * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi)]


def _frames(x):
    w = window()
    return np.array([w * x[i:i + FRAME] for i in range(0, len(x) - FRAME + 1, HOP)])


def _ola(fr):
    out = np.zeros((len(fr) - 1) * HOP + FRAME)
    for i, f in enumerate(fr):
        out[i * HOP:i * HOP + FRAME] += f
    return out


def _bands(sig):
    w = window()
    fr = np.array([w * sig[i:i + FRAME] for i in range(0, len(sig) - FRAME, HOP)])
    if len(fr) == 0:
        return np.zeros((NBANDS, 0))
    spec = np.abs(np.fft.rfft(fr, NFFT, axis=-1)) ** 2          # (M, 257)
    return np.array([np.sqrt(spec[:, a:b].sum(-1)) for a, b in band_edges()])  # (15, M)


def stoi_full(clean, proc, extended=False):
    """-> dict(d, frames, kept, M, margin) for one pair of 10 kHz signals."""
    clean = np.asarray(clean, np.float64)
    proc = np.asarray(proc, np.float64)
    fx, fy = _frames(clean), _frames(proc)
    e = 20.0 * np.log10(np.linalg.norm(fx, axis=1) + EPS)
    thr = e.max() - DYN
    mask = e > thr
    margin = float(np.abs(e - thr).min())
    kept = int(mask.sum())
    X, Y = _bands(_ola(fx[mask])), _bands(_ola(fy[mask]))
    M = X.shape[1]
    out = dict(frames=len(fx), kept=kept, M=M, margin=margin)
    if M < NSEG:
        out["d"] = 1e-5
        return out
    xs = np.array([X[:, m - NSEG:m] for m in range(NSEG, M + 1)])   # (J, 15, 30)
    ys = np.array([Y[:, m - NSEG:m] for m in range(NSEG, M + 1)])
    J = len(xs)

    def norm(a, ax):
        a = a - a.mean(ax, keepdims=True)
        return a / (np.linalg.norm(a, axis=ax, keepdims=True) + EPS)

    if extended:
        xn, yn = norm(norm(xs, 2), 1), norm(norm(ys, 2), 1)
        out["d"] = float((xn * yn).sum() / (NSEG * J))
    else:
        c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
        yp = np.minimum(c * ys, xs * BETA)
        out["d"] = float((norm(xs, 2) * norm(yp, 2)).sum() / (NBANDS * J))
    return out


def stoi(clean, proc, extended=False):
    return stoi_full(clean, proc, extended)["d"]


# ---- the shared cases ------------------------------------------------------
def sig(seed, T, gaps=()):
    r = np.random.default_rng(seed); t = np.arange(T) / 10000
    f0 = r.uniform(100, 180)
    car = sum(np.sin(2*np.pi*f0*(h+1)*t + r.uniform(0, 6.28)) / (h+1) for h in range(24))
    env = 0.3 + 0.7*np.sin(2*np.pi*r.uniform(2, 4)*t + r.uniform(0, 6.28))**2
    g = np.ones(T)
    for a, b in gaps: g[a:b] = 1e-3
    return 0.1*car*env*g + 1e-5*r.standard_normal(T)


def noisy(x, seed, snr):
    n = np.random.default_rng(1000+seed).standard_normal(len(x))
    return x + n*np.linalg.norm(x)/np.linalg.norm(n)*10**(-snr/20)


CASES = {
    "t3968": (3968, ()),
    "t4096": (4096, ()),
    "t4223": (4223, ()),
    "t4224": (4224, ()),
    "mid_gap": (8000, ((3000, 4500),)),
    "lead_gap": (8000, ((0, 2000),)),
    "tail_gap": (8000, ((6500, 8000),)),
    "two_gaps": (12000, ((2000, 3000), (7000, 9500))),
    "m30_gap": (5376, ((2000, 3280),)),
    "long": (30000, ((5000, 9000), (20000, 21000))),
}
SEEDS = (0, 1, 2)
SNRS = (15, 0)

_cache = {}


def case(name, seed, snr):
    """-> (clean, proc) fp32 arrays (what the GPU is given); cached, read-only."""
    key = (name, seed, snr)
    if key not in _cache:
        T, gaps = CASES[name]
        x = sig(seed, T, gaps)
        y = noisy(x, seed, snr)
        x, y = x.astype(np.float32), y.astype(np.float32)
        x.setflags(write=False)
        y.setflags(write=False)
        _cache[key] = (x, y)
    return _cache[key]


_ref_cache = {}


def case_ref(name, seed, snr, extended):
    """fp64 reference of the fp32 inputs of case(): dict(d, frames, kept, M, margin)."""
    key = (name, seed, snr, bool(extended))
    if key not in _ref_cache:
        x, y = case(name, seed, snr)
        _ref_cache[key] = stoi_full(x, y, extended)
    return _ref_cache[key]
