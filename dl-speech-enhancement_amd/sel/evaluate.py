"""Corpus scoring over ragged batches: what the reference does
file by file in mel_spectrogram.py / testing_denoise.py, on whole utterances of
different lengths, batched.

score_corpus sorts the utterances by length, forms buckets of up to `batch`
rows, pads each bucket with zeros to its longest row rounded up to a multiple
of 4096 samples (so that workspaces and shapes recur), calls
mel_spectrogram.measures_rows with the rows' lengths and keeps every result on
the device; one host copy is made at the end.  A row's values do not depend on
what shares its bucket (each row of a ragged call has the bits of a call on
that row alone), so the table depends on neither `batch` nor the order of
`items`.
"""
import math

import torch

from . import _lib as L

PAD_QUANTUM = 4096


def plan_buckets(lengths, batch, quantum=PAD_QUANTUM):
    """Pure host logic: [(indices, padded length)] covering every index of
    `lengths` exactly once; indices sorted by (length, index), at most `batch`
    per bucket, each bucket padded to its longest row rounded up to a multiple
    of `quantum`."""
    if isinstance(batch, bool) or int(batch) != batch or int(batch) < 1:
        raise ValueError(f"sel.evaluate: batch must be a positive integer, got {batch!r}")
    if int(quantum) < 1:
        raise ValueError(f"sel.evaluate: quantum must be positive, got {quantum!r}")
    lengths = [int(n) for n in lengths]
    if any(n < 1 for n in lengths):
        raise ValueError("sel.evaluate: every utterance needs at least one sample")
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    out = []
    for k in range(0, len(order), int(batch)):
        idx = order[k:k + int(batch)]
        longest = lengths[idx[-1]]
        out.append((idx, (longest + quantum - 1) // quantum * quantum))
    return out


def score_corpus(items, sample_rate, batch=16, sdr=False, estoi=False, device=None):
    """items yields (utt_id, pred, target): 1-D tensors of one length per
    utterance (any length across utterances), on the CPU or the device.  Returns
    (table, means): table = {utt_id: {measure: float}} with the keys of
    mel_spectrogram.measures (SDR with sdr=True; ESTOI after STOI with
    estoi=True), means = {measure: float}, the corpus means over utterances
    accumulated in fp64 (math.fsum: independent of the order).  An utterance too
    short for a measure (STOI needs 256 samples at 10 kHz, Mel-L1 201 samples)
    has NaN there."""
    from mel_spectrogram import measures_rows
    from . import metrics as M
    ids, preds, targets = [], [], []
    for utt_id, pred, target in items:
        pred, target = torch.as_tensor(pred), torch.as_tensor(target)
        if pred.dim() != 1 or pred.shape != target.shape:
            raise ValueError(f"sel.evaluate: {utt_id!r}: pred {tuple(pred.shape)} and target {tuple(target.shape)} "
                             f"must be 1-D and of one length")
        if utt_id in ids:
            raise ValueError(f"sel.evaluate: duplicate utterance id {utt_id!r}")
        ids.append(utt_id)
        preds.append(pred)
        targets.append(target)
    lengths = [int(p.shape[0]) for p in preds]
    plan = plan_buckets(lengths, batch)
    if not ids:
        return {}, {}
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None:
        raise L.SelError("sel.evaluate: no ROCm GPU visible; the MI355X path has no CPU fallback")
    keys, chunks, where = None, [], []
    with torch.no_grad():
        for idx, T in plan:
            w1 = torch.zeros(len(idx), T, dtype=torch.float32, device=device)
            w2 = torch.zeros(len(idx), T, dtype=torch.float32, device=device)
            for r, i in enumerate(idx):
                w1[r, :lengths[i]] = preds[i].to(device=device, dtype=torch.float32)
                w2[r, :lengths[i]] = targets[i].to(device=device, dtype=torch.float32)
            lens = torch.tensor([lengths[i] for i in idx], dtype=torch.int64).to(device)
            rows = measures_rows(w1, w2, sample_rate, sdr=sdr, lengths=lens)
            if estoi:
                rows = dict(rows)
                rows["ESTOI"] = M.stoi(w1, w2, sample_rate, extended=True, lengths=lens)
                rows["Mel-L1"] = rows.pop("Mel-L1")  # ESTOI sits after STOI
            if keys is None:
                keys = list(rows)
            chunks.append(torch.stack([rows[k].double() for k in keys], dim=1))
            where.extend(idx)
        host = torch.cat(chunks, dim=0).cpu()  # the one host copy
    table = {}
    for r, i in enumerate(where):
        table[ids[i]] = {k: float(host[r, c]) for c, k in enumerate(keys)}
    table = {u: table[u] for u in ids}
    means = {k: math.fsum(table[u][k] for u in ids) / len(ids) for k in keys}
    return table, means
