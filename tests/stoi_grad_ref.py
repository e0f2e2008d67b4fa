"""fp64 reference of the STOI / ESTOI gradient: the definition of
DESIGN §22.1 restated in torch fp64 on the CPU, so that autograd gives the
gradient with respect to the processed signal, and the resampler's transpose
K^T in fp64 numpy, built from sel_resample_kernel's host table.  This is the
reference of tests/test_stoi_grad_host.py and tests/test_gpu_stoi_grad.py, never
the code under test.  The silent-frame mask is computed from the clean signal
in numpy and applied as a constant selection.

It adds the shallow-gap recipe to the shared cases of tests/metrics_ref.py:
metrics_ref.sig's signal with the gaps (2000, 2600) and (5000, 5500) at depth
0.05 instead of 1e-3, T = 8000, noise by metrics_ref.noisy at 10 and 5 dB,
seeds 0-2.  The shared cases barely touch the clip branch of STOI (at most 2 %
of their cells); these clip 5 % to 14 % of theirs and keep all 61 frames."""
import ctypes
import math

import numpy as np
import torch

import metrics_ref as MR
from sel import _lib as _L

# a reference for entry points the library does not declare would compare nothing
for _name in ("sel_stoi_bwd_workspace", "sel_stoi_bwd", "sel_resample_bwd"):
    if _name not in _L.SIGNATURES:
        raise ImportError(f"stoi_grad_ref: the library under test does not declare {_name}")

SHALLOW_T, SHALLOW_GAPS, SHALLOW_DEPTH, SHALLOW_SNRS = 8000, ((2000, 2600), (5000, 5500)), 0.05, (10, 5)
# the rows of the GPU gradient tests: (name, seed, SNR in dB)
GRAD_CASES = [(n, s, q) for n in ("t4096", "t4223", "t4224", "m30_gap", "mid_gap", "lead_gap", "tail_gap", "two_gaps")
              for s, q in ((0, 15), (1, 0), (2, 15))]
SHALLOW_CASES = [("shallow", s, q) for s in MR.SEEDS for q in SHALLOW_SNRS]


def sig_depth(seed, T, gaps, depth):
    """metrics_ref.sig with the gaps at `depth` (same draws in the same order)."""
    r = np.random.default_rng(seed); t = np.arange(T) / 10000
    f0 = r.uniform(100, 180)
    car = sum(np.sin(2*np.pi*f0*(h+1)*t + r.uniform(0, 6.28)) / (h+1) for h in range(24))
    env = 0.3 + 0.7*np.sin(2*np.pi*r.uniform(2, 4)*t + r.uniform(0, 6.28))**2
    g = np.ones(T)
    for a, b in gaps: g[a:b] = depth
    return 0.1*car*env*g + 1e-5*r.standard_normal(T)


_cache = {}


def case(name, seed, snr, crop=None):
    """-> (clean, proc) fp32, read-only: a shared case of metrics_ref, or
    "shallow"; `crop` keeps the first samples (rows of one batch share T)."""
    key = (name, seed, snr, crop)
    if key not in _cache:
        if name == "shallow":
            x = sig_depth(seed, SHALLOW_T, SHALLOW_GAPS, SHALLOW_DEPTH)
            y = MR.noisy(x, seed, snr)
            x, y = x.astype(np.float32), y.astype(np.float32)
        else:
            x, y = MR.case(name, seed, snr)
        if crop is not None:
            x, y = x[:crop].copy(), y[:crop].copy()
        x.setflags(write=False)
        y.setflags(write=False)
        _cache[key] = (x, y)
    return _cache[key]


def stoi_torch(clean, proc, extended, detail=False):
    """d of one pair of 10 kHz signals as a torch fp64 scalar that carries the
    graph to `proc` (a torch fp64 tensor); clean is a numpy array.  With detail,
    also dict(frames, kept, M, margin, mask, clip_margin, clipped, cells, min_band)."""
    x = np.asarray(clean, np.float64)
    w = MR.window()
    fx = np.array([w * x[i:i + MR.FRAME] for i in range(0, len(x) - MR.FRAME + 1, MR.HOP)])
    e = 20.0 * np.log10(np.linalg.norm(fx, axis=1) + MR.EPS)
    thr = e.max() - MR.DYN
    mask = e > thr
    info = dict(frames=len(fx), kept=int(mask.sum()), M=int(mask.sum()) - 1, margin=float(np.abs(e - thr).min()),
                mask=mask)
    wt = torch.from_numpy(w)

    def bands(s):
        fr = (wt * s.unfold(0, MR.FRAME, MR.HOP))[torch.from_numpy(mask)]              # kept frames
        K = fr.shape[0]
        z = torch.zeros(MR.HOP, dtype=torch.float64)
        ola = torch.cat([fr[:, :MR.HOP].reshape(-1), z]) + torch.cat([z, fr[:, MR.HOP:].reshape(-1)])
        cols = ola.unfold(0, MR.FRAME, MR.HOP)[:K - 1] * wt                            # range(0, len - 256, 128)
        spec = torch.fft.rfft(cols, MR.NFFT, dim=-1).abs() ** 2
        return torch.stack([spec[:, a:b].sum(-1).sqrt() for a, b in MR.band_edges()])  # (15, M)

    X, Y = bands(torch.from_numpy(x)), bands(proc)
    M = X.shape[1]
    if M < MR.NSEG:
        d = torch.tensor(1e-5, dtype=torch.float64) + 0.0 * proc.sum()
        return (d, info) if detail else d
    xs = X.unfold(1, MR.NSEG, 1).permute(1, 0, 2)        # (J, 15, 30)
    ys = Y.unfold(1, MR.NSEG, 1).permute(1, 0, 2)
    J = xs.shape[0]

    def norm(a, ax):
        a = a - a.mean(ax, keepdim=True)
        return a / (torch.linalg.norm(a, dim=ax, keepdim=True) + MR.EPS)

    if extended:
        d = (norm(norm(xs, 2), 1) * norm(norm(ys, 2), 1)).sum() / (MR.NSEG * J)
    else:
        c = torch.linalg.norm(xs, dim=2, keepdim=True) / (torch.linalg.norm(ys, dim=2, keepdim=True) + MR.EPS)
        cy, bx = c * ys, xs * MR.BETA
        d = (norm(xs, 2) * norm(torch.minimum(cy, bx), 2)).sum() / (MR.NBANDS * J)
        info.update(clip_margin=float(((cy - bx).abs() / bx).min()), clipped=int((cy >= bx).sum()),
                    cells=int(cy.numel()))
    info["min_band"] = float(min(X.min(), Y.detach().min()))
    return (d, info) if detail else d


_grad_cache = {}


def case_grad(name, seed, snr, extended, crop=None):
    """-> (d, gradient of d with respect to proc as fp64 numpy, info); cached."""
    key = (name, seed, snr, bool(extended), crop)
    if key not in _grad_cache:
        x, y = case(name, seed, snr, crop)
        p = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
        d, info = stoi_torch(x, p, extended, detail=True)
        d.backward()
        g = p.grad.numpy().copy()
        g.setflags(write=False)
        _grad_cache[key] = (float(d), g, info)
    return _grad_cache[key]


# ---- the resampler's transpose ----------------------------------------------
def resample_table(orig, new, lpw=6, rolloff=0.99):
    """-> (o, n, w, table (n, taps) fp64 of the fp32 host table the kernels read)."""
    from sel import _lib
    lib = _lib.load()
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    nph, ntaps = ctypes.c_int(), ctypes.c_int()
    assert lib.sel_resample_plan(o, n, lpw, rolloff, ctypes.byref(nph), ctypes.byref(ntaps)) == 0
    tab = np.empty((nph.value, ntaps.value), np.float32)
    assert lib.sel_resample_kernel(o, n, lpw, rolloff, tab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert nph.value == n and (ntaps.value - o) % 2 == 0
    return o, n, (ntaps.value - o) // 2, tab.astype(np.float64)


def resample_T(gy, length, orig, new):
    """gx (..., length) = K^T gy in fp64: y[f n + p] = sum_i xpad[f o + i] K[p][i], xpad = (w zeros, x, ...)."""
    o, n, w, tab = resample_table(orig, new)
    gy = np.asarray(gy, np.float64)
    out_len = gy.shape[-1]
    assert out_len == -(-n * length // o)
    gx = np.zeros(gy.shape[:-1] + (length,))
    for p in range(n):
        f = np.arange((out_len - p + n - 1) // n)
        for i in range(tab.shape[1]):
            s = f * o + i - w
            ok = (s >= 0) & (s < length)
            gx[..., s[ok]] += gy[..., f[ok] * n + p] * tab[p, i]
    return gx
