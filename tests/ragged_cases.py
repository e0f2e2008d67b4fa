"""The shared cases of the ragged-batch tests: for each measure a
stride T, the row lengths at the kernels' edges, and the rows themselves, made
at each row's own length (so that the fixed-length call on the row alone is the
oracle) and padded into a (B, T) batch whose padding is a fill of the caller's
choice (NaN, then 1e30: padding must be neither read into a result nor masked by
a multiplication).  Host code only: used by tests/test_ragged_host.py and the
two GPU files."""
import numpy as np

import bss_sdr_ref as BR
import metrics_ref as MR

FILLS = (float("nan"), 1e30)

# measure -> (T, lengths at the edges, the same batch with every length below T)
SDR_T = 8200
SDR_LENGTHS = ([1, 255, 256, 257, 4096, 4097, 8200],     # block width 256, the 4096-element backward chunk
               [1, 255, 256, 257, 4096, 4097, 8199])
BSS_T = 6200
BSS_LENGTHS = ([1, 511, 2048, 2049, 4099, 6200],          # below the filter length, the 2048 correlation chunk
               [1, 511, 2048, 2049, 4099, 6100])
BSS_FILTERS = (512, 16)
STOI_T = 12000
STOI_LENGTHS = [256, 4095, 4096, 8448, 11000]             # 1 frame; 30 (1e-5); 31; 65 (the mask's round); all < T
STOI_ROWS = [(0, (), 15), (1, (), 0), (2, (), 15), (3, ((3000, 4500),), 0), (4, ((2000, 3000), (7000, 9500)), 15)]
STOI48_T = 57600                                          # 1.2 s at 48 kHz -> 12000 samples at 10 kHz
STOI48_LENGTHS = [1229, 19661, 40550, 57600]              # -> 257 (1 frame), 4097 (31), 8448 (65), 12000
MEL_T = 2200
MEL_LENGTHS = ([201, 399, 400, 401, 800, 1000, 2200],     # frames 2, 2, 3, 3, 5, 6, 12; four frames per block
               [201, 399, 400, 401, 800, 1000, 2199])
MEL_NFFT, MEL_HOP = 400, 200

_cache = {}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def sdr_rows(lengths):
    """[(pred, target)] fp32, a DC offset on both (zero_mean has something to remove)."""
    key = ("sdr", tuple(lengths))
    if key not in _cache:
        out = []
        for j, n in enumerate(lengths):
            r = np.random.default_rng(100 + j)
            t = (r.standard_normal(n) + 0.3).astype(np.float32)
            p = (t + 0.2 * r.standard_normal(n) - 0.1).astype(np.float32)
            out.append(_ro(p, t))
        _cache[key] = out
    return _cache[key]


def bss_rows(lengths):
    """[(pred, target)] from the recipe of tests/bss_sdr_ref.py, no silent target."""
    kinds = [("white", 10, 0), ("ar2", 30, 1), ("voiced", 0, 0), ("white", 30, 1), ("ar2", 10, 0), ("voiced", 10, 1)]
    return [BR.case(*kinds[j % len(kinds)], n) for j, n in enumerate(lengths)]


def stoi_rows():
    """[(clean, proc)] fp32 at 10 kHz from the recipe of tests/metrics_ref.py, each at its own length."""
    key = "stoi"
    if key not in _cache:
        out = []
        for n, (seed, gaps, snr) in zip(STOI_LENGTHS, STOI_ROWS):
            x = MR.sig(seed, n, gaps)
            y = MR.noisy(x, seed, snr)
            out.append(_ro(x.astype(np.float32), y.astype(np.float32)))
        _cache[key] = out
    return _cache[key]


def stoi_refs(extended):
    key = ("stoi_ref", bool(extended))
    if key not in _cache:
        _cache[key] = [MR.stoi_full(x, y, extended) for x, y in stoi_rows()]
    return _cache[key]


def stoi48_rows():
    """[(clean, proc)] fp32 taken as 48 kHz signals (the recipe's samples, read at 48 kHz)."""
    key = "stoi48"
    if key not in _cache:
        out = []
        for j, n in enumerate(STOI48_LENGTHS):
            x = MR.sig(10 + j, n)
            y = MR.noisy(x, 10 + j, (15, 0)[j % 2])
            out.append(_ro(x.astype(np.float32), y.astype(np.float32)))
        _cache[key] = out
    return _cache[key]


def mel_rows(lengths):
    key = ("mel", tuple(lengths))
    if key not in _cache:
        out = []
        for j, n in enumerate(lengths):
            r = np.random.default_rng(300 + j)
            t = (0.1 * r.standard_normal(n)).astype(np.float32)
            p = (t + 0.02 * r.standard_normal(n)).astype(np.float32)
            out.append(_ro(p, t))
        _cache[key] = out
    return _cache[key]


def pad(rows, T, fill):
    """[(a, b)] at their own lengths -> two (B, T) fp32 arrays, `fill` at and past each row's length."""
    a = np.full((len(rows), T), fill, dtype=np.float32)
    b = np.full((len(rows), T), fill, dtype=np.float32)
    for j, (x, y) in enumerate(rows):
        assert len(x) == len(y) <= T
        a[j, :len(x)] = x
        b[j, :len(y)] = y
    return a, b


def l1_l2_ref(a, b):
    """fp64 mean |a - b| and mean (a - b)^2 of two fp32 arrays."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.abs(d).mean()), float((d * d).mean())


def corpus(n, sample_rate, seed=0, lo=0.3, hi=1.2):
    """n synthetic utterances of lo .. hi seconds: [(utt_id, pred, target)] fp32 numpy, lengths all different."""
    key = ("corpus", n, sample_rate, seed, lo, hi)
    if key not in _cache:
        r = np.random.default_rng(seed)
        lens = np.linspace(lo * sample_rate, hi * sample_rate, n).astype(int) + r.integers(0, 97, n)
        lens = np.minimum(lens, int(hi * sample_rate))
        out = []
        for j, m in enumerate(r.permutation(lens)):
            t = np.arange(m) / sample_rate
            f0 = r.uniform(100, 180)
            car = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + r.uniform(0, 6.28)) / (h + 1) for h in range(12))
            env = 0.3 + 0.7 * np.sin(2 * np.pi * r.uniform(2, 4) * t + r.uniform(0, 6.28)) ** 2
            x = 0.1 * car * env + 1e-4 * r.standard_normal(m)
            y = x + 0.02 * r.standard_normal(m)
            out.append((f"utt{j:02d}",) + _ro(y.astype(np.float32), x.astype(np.float32)))
        _cache[key] = out
    return _cache[key]
