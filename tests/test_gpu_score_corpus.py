"""GPU checks of sel.evaluate.score_corpus and tools/score_corpus.py (DESIGN
§25) on a synthetic corpus of 11 utterances of 0.3 to 1.2 s: the table does not
depend on the batch size or on the order of the items, every entry equals the
solo measures() call on that utterance (the kernel measures bit for bit; MAE,
MSE and Mel-L1, which the solo call reduces in fp32 and the scorer accumulates
in fp64, to 1e-6 relative), also at 48 kHz, where STOI goes through the ragged
resampler; and the command-line tool round-trips a directory of .npy and
PCM-16 .wav files."""
import importlib.util
import json
import math
import os
import random
import wave

import numpy as np
import pytest
import torch

import ragged_cases as RC
from conftest import REPO

pytestmark = pytest.mark.gpu

KERNEL_KEYS = ("SNR", "SDR", "SI-SDR(True)", "SI-SDR(False)", "STOI")
FP64_KEYS = ("MAE", "MSE", "Mel-L1")
KEYS = ["MAE", "MSE", "SNR", "SDR", "SI-SDR(True)", "SI-SDR(False)", "STOI", "Mel-L1"]
REL_BOUND = 1e-6

_solo_cache = {}


def _items(sample_rate, gpu=None):
    out = []
    for utt, p, t in RC.corpus(11, sample_rate):
        p, t = torch.from_numpy(p), torch.from_numpy(t)
        out.append((utt, p.to(gpu), t.to(gpu)) if gpu is not None else (utt, p, t))
    return out


def _solo(sample_rate, gpu):
    """{utt_id: {measure: float}} by today's fixed-length measures(), one utterance at a time; computed once."""
    from mel_spectrogram import measures
    if sample_rate not in _solo_cache:
        table = {}
        for utt, p, t in _items(sample_rate, gpu):
            out = measures(p[None], t[None], sample_rate, sdr=True)
            table[utt] = {k: float(v.item()) for k, v in out.items()}
        _solo_cache[sample_rate] = table
    return _solo_cache[sample_rate]


def _check_against_solo(table, solo):
    worst = 0.0
    for utt, row in table.items():
        assert [k for k in row if k != "ESTOI"] == KEYS
        for k in KERNEL_KEYS:
            assert row[k] == solo[utt][k], (utt, k, row[k], solo[utt][k])
        for k in FP64_KEYS:
            rel = abs(row[k] - solo[utt][k]) / abs(solo[utt][k])
            worst = max(worst, rel)
            assert rel <= REL_BOUND, (utt, k, row[k], solo[utt][k], rel)
    return worst


def test_table_is_independent_of_batch_and_order(gpu):
    from sel.evaluate import score_corpus
    items = _items(16000)
    lengths = [len(p) for _, p, _ in items]
    assert len(items) == 11 and len(set(lengths)) == 11 and 0.3 * 16000 <= min(lengths) and max(lengths) <= 1.2 * 16000
    t1, m1 = score_corpus(items, 16000, batch=1, sdr=True)
    t4, m4 = score_corpus(items, 16000, batch=4, sdr=True)
    shuffled = list(items)
    random.Random(5).shuffle(shuffled)
    ts, ms = score_corpus(shuffled, 16000, batch=4, sdr=True)
    assert list(t1) == [u for u, _, _ in items] and list(ts) == [u for u, _, _ in shuffled]
    assert t1 == t4 and t1 == ts and m1 == m4 and m1 == ms
    assert all(math.isfinite(v) for row in t1.values() for v in row.values())
    for k in KEYS:
        want = math.fsum(t1[u][k] for u in t1) / 11
        assert m1[k] == want
    worst = _check_against_solo(t1, _solo(16000, gpu))
    print(f"SCORER 16 kHz: largest rel dev of MAE / MSE / Mel-L1 from the solo fp32 reductions {worst:.3e}")
    # items on the device, a batch larger than the corpus, ESTOI on request
    t16, _ = score_corpus(_items(16000, gpu), 16000, batch=16, sdr=True, estoi=True)
    assert list(next(iter(t16.values()))) == KEYS[:7] + ["ESTOI", "Mel-L1"]
    assert {u: {k: v for k, v in row.items() if k != "ESTOI"} for u, row in t16.items()} == t1
    from sel import metrics as M
    for utt, p, t in _items(16000, gpu)[:3]:
        assert t16[utt]["ESTOI"] == float(M.stoi(p[None], t[None], 16000, True).item())


def test_scores_at_48k_equal_solo_measures(gpu):
    from sel.evaluate import score_corpus
    table, means = score_corpus(_items(48000), 48000, batch=4, sdr=True)
    worst = _check_against_solo(table, _solo(48000, gpu))
    print(f"SCORER 48 kHz: largest rel dev of MAE / MSE / Mel-L1 from the solo fp32 reductions {worst:.3e}")
    assert all(0.0 < row["STOI"] <= 1.0 for row in table.values())      # below 31 frames: the constant 1e-5
    assert sum(row["STOI"] > 0.1 for row in table.values()) >= 5
    assert means["STOI"] == math.fsum(row["STOI"] for row in table.values()) / 11


def _write_wav(path, x, rate):
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def test_cli_round_trips_npy_and_wav(gpu, tmp_path):
    from sel.evaluate import score_corpus
    spec = importlib.util.spec_from_file_location("score_corpus_cli", os.path.join(REPO, "tools", "score_corpus.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    pd, td = tmp_path / "pred", tmp_path / "target"
    pd.mkdir()
    td.mkdir()
    items = []
    for j, (utt, p, t) in enumerate(RC.corpus(11, 16000)[:5]):
        if j % 2:
            name = utt + ".wav"
            p = _write_wav(str(pd / name), p, 16000)
            t = _write_wav(str(td / name), t, 16000)
        else:
            name = utt + ".npy"
            np.save(str(pd / name), p)
            np.save(str(td / name), t)
        items.append((name, torch.from_numpy(np.ascontiguousarray(p)), torch.from_numpy(np.ascontiguousarray(t))))
    out = tmp_path / "scores.jsonl"
    assert cli.main([str(pd), str(td), "--sample-rate", "16000", "--batch", "2", "--sdr", "--out", str(out)]) == 0
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    table, means = score_corpus(items, 16000, batch=16, sdr=True)
    assert len(lines) == 6 and [x["utt_id"] for x in lines[:5]] == sorted(table)
    for x in lines[:5]:
        assert {k: v for k, v in x.items() if k != "utt_id"} == table[x["utt_id"]]
    assert lines[5] == {"means": means, "utterances": 5}
    # names that do not match, and a .wav at another rate, are refused
    np.save(str(pd / "extra.npy"), np.zeros(5000, np.float32))
    with pytest.raises(SystemExit, match="same names"):
        cli.main([str(pd), str(td), "--sample-rate", "16000"])
    os.remove(str(pd / "extra.npy"))
    with pytest.raises(SystemExit, match="rate"):
        cli.main([str(pd), str(td), "--sample-rate", "8000"])
