#!/usr/bin/env python
"""Score a directory of predictions against a directory of targets with
sel.evaluate.score_corpus.

    python tools/score_corpus.py PRED_DIR TARGET_DIR --sample-rate 16000 [--out scores.jsonl]

Files are matched by name: .npy (a 1-D array) or PCM-16 .wav (mono, read with
the stdlib wave module; its rate must be --sample-rate).  Output, JSON lines:
one {"utt_id": ..., measure: value, ...} per utterance in name order, then one
{"means": {...}, "utterances": N} line.
"""
import argparse
import json
import os
import sys
import wave

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dl-speech-enhancement_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def read_audio(path, sample_rate):
    if path.endswith(".npy"):
        x = np.load(path)
        if x.ndim != 1:
            raise SystemExit(f"{path}: expected a 1-D array, got shape {x.shape}")
        return x.astype(np.float32)
    with wave.open(path, "rb") as w:
        if w.getnchannels() != 1 or w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise SystemExit(f"{path}: only mono PCM-16 .wav is read")
        if w.getframerate() != sample_rate:
            raise SystemExit(f"{path}: rate {w.getframerate()} is not --sample-rate {sample_rate}")
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return pcm.astype(np.float32) / 32768.0


def list_audio(d):
    return sorted(f for f in os.listdir(d) if f.endswith((".npy", ".wav")))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pred_dir")
    ap.add_argument("target_dir")
    ap.add_argument("--sample-rate", type=int, required=True)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--sdr", action="store_true", help="add the BSS-eval SDR")
    ap.add_argument("--estoi", action="store_true", help="add ESTOI")
    ap.add_argument("--out", default="-", help="JSON-lines file (default: stdout)")
    a = ap.parse_args(argv)
    names = list_audio(a.pred_dir)
    if names != list_audio(a.target_dir):
        raise SystemExit(f"{a.pred_dir} and {a.target_dir} do not hold files of the same names")
    if not names:
        raise SystemExit(f"{a.pred_dir}: no .npy or .wav files")
    import torch
    from sel.evaluate import score_corpus

    def items():
        for f in names:
            p = read_audio(os.path.join(a.pred_dir, f), a.sample_rate)
            t = read_audio(os.path.join(a.target_dir, f), a.sample_rate)
            if p.shape != t.shape:
                raise SystemExit(f"{f}: prediction has {p.shape[0]} samples, target {t.shape[0]}")
            yield f, torch.from_numpy(p), torch.from_numpy(t)

    table, means = score_corpus(items(), a.sample_rate, batch=a.batch, sdr=a.sdr, estoi=a.estoi)
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    try:
        for f in names:
            out.write(json.dumps({"utt_id": f, **table[f]}) + "\n")
        out.write(json.dumps({"means": means, "utterances": len(names)}) + "\n")
    finally:
        if out is not sys.stdout:
            out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
