#!/usr/bin/env python
"""Time sel.evaluate.score_corpus against scoring the same utterances one by
one with the fixed-length mel_spectrogram.measures().

64 synthetic utterances of 1 to 4 s at 48 kHz, all eight measures (the BSS-eval
SDR included), batch = 16.  Both sides start from utterances already on the
device and end with the scores on the host; they alternate --rounds times in
one process after one untimed pass of each.  Wall-clock times (the work is
many small launches, so the host is part of what is measured).

    python tools/score_corpus_bench.py --out profiles/score_corpus_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dl-speech-enhancement_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def corpus(n, fs, seed=0):
    r = np.random.default_rng(seed)
    out = []
    for j, m in enumerate(r.integers(fs, 4 * fs + 1, n)):
        t = np.arange(m) / fs
        f0 = r.uniform(100, 180)
        car = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + r.uniform(0, 6.28)) / (h + 1) for h in range(12))
        env = 0.3 + 0.7 * np.sin(2 * np.pi * r.uniform(2, 4) * t + r.uniform(0, 6.28)) ** 2
        x = 0.1 * car * env + 1e-4 * r.standard_normal(m)
        out.append((f"utt{j:02d}", (x + 0.02 * r.standard_normal(m)).astype(np.float32), x.astype(np.float32)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from mel_spectrogram import measures
    from sel.evaluate import score_corpus
    fs = 48000
    dev = torch.device("cuda:0")
    items = [(u, torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)) for u, p, t in corpus(a.utterances, fs)]

    def batched():
        return score_corpus(items, fs, batch=a.batch, sdr=True)[0]

    def one_by_one():
        outs = [measures(p[None], t[None], fs, sdr=True) for _, p, t in items]
        keys = list(outs[0])
        host = torch.stack([torch.stack([o[k] for k in keys]) for o in outs]).cpu()     # one host copy
        return {u: {k: float(host[i, c]) for c, k in enumerate(keys)} for i, (u, _, _) in enumerate(items)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    tb, to = batched(), one_by_one()        # untimed: loads kernels, tables, allocator pools
    same = all(tb[u][k] == to[u][k] for u in tb for k in ("SNR", "SDR", "SI-SDR(True)", "SI-SDR(False)", "STOI"))
    times = {"score_corpus": [], "one_by_one": []}
    for _ in range(a.rounds):
        times["score_corpus"].append(timed(batched)[0])
        times["one_by_one"].append(timed(one_by_one)[0])
    res = {
        "utterances": a.utterances, "sample_rate": fs, "batch": a.batch, "measures": list(next(iter(tb.values()))),
        "seconds_of_audio": sum(len(p) for _, p, _ in items) / fs,
        "kernel_measures_bit_identical": bool(same),
        "ms": times,
        "median_ms": {k: float(np.median(v)) for k, v in times.items()},
    }
    res["speedup_median"] = res["median_ms"]["one_by_one"] / res["median_ms"]["score_corpus"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
