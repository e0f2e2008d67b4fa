"""GPU checks of the evaluation measures against the fp64
restatement tests/metrics_ref.py: sel_stoi on every shared case (frame counts
exact, d and the batch mean within the recorded bound, both modes), its
plumbing (optional outputs, an unaligned view, graph replay, run-to-run bits),
the SDR family at its shape edges with its gradient, and the Python modules.

Bounds.  They were set from the first MI355X run as four times the largest
deviation seen, rounded up to one significant figure, and may not exceed the
caps the definition sets (1e-3 for STOI, the third decimal in which it is
reported; 1e-3 dB and 1e-4 relative for the SDR values and gradients).  The
measured figures are in DESIGN §22.5; each test prints its own before it
asserts.
"""
import numpy as np
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu

# largest |GPU - fp64| seen on the MI355X, x4, one significant figure up:
# STOI 2.935e-08, ESTOI 1.487e-08 (half an ulp of the fp32 result), SDR values 1.310e-05 dB,
# gradients 1.776e-07 relative
STOI_BOUND = {False: 2e-7, True: 6e-8}
SDR_DB_BOUND = 6e-5
SDR_GRAD_BOUND = 8e-7
assert max(STOI_BOUND.values()) <= 1e-3 and SDR_DB_BOUND <= 1e-3 and SDR_GRAD_BOUND <= 1e-4

# batches of equal T; rows of a batch differ in seed, SNR and (T = 8000) in the frames kept
GROUPS = {}
for _name, (_T, _gaps) in MR.CASES.items():
    GROUPS.setdefault(_T, []).extend((_name, s, q) for s in MR.SEEDS for q in MR.SNRS)


def _L():
    from sel import _lib as L
    return L


def _batch(rows, gpu):
    x = np.stack([MR.case(*r)[0] for r in rows])
    y = np.stack([MR.case(*r)[1] for r in rows])
    return torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)


def _run_stoi(clean, proc, extended, want_mean=True, want_info=True):
    """sel_stoi on (B, T) device tensors -> (d, mean, info), the outputs pre-filled with sentinels."""
    L = _L()
    B, T = clean.shape
    dev = clean.device
    ws = L.workspace(L.lib().sel_stoi_workspace(B, T), dev)
    d = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    mean = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    info = torch.full((B, 3), -7, dtype=torch.int32, device=dev)
    L.call("sel_stoi", L.ptr(clean), L.ptr(proc), B, T, int(extended), L.ptr(d), L.ptr(mean) if want_mean else None,
           L.ptr(info) if want_info else None, L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return d, mean, info


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("T", sorted(GROUPS))
def test_stoi_matches_fp64_reference(gpu, T, extended):
    rows = GROUPS[T]
    clean, proc = _batch(rows, gpu)
    d, mean, info = _run_stoi(clean, proc, extended)
    refs = [MR.case_ref(*r, extended) for r in rows]
    want_info = np.array([[r["frames"], r["kept"], r["M"]] for r in refs], dtype=np.int32)
    assert np.array_equal(info.cpu().numpy(), want_info), (info.cpu().numpy(), want_info)
    want = np.array([r["d"] for r in refs])
    got = d.cpu().numpy().astype(np.float64)
    dev = np.abs(got - want).max()
    dev_mean = abs(float(mean.item()) - want.mean())
    print(f"STOI-DEV T={T} extended={int(extended)} rows={len(rows)} max|d-ref|={dev:.3e} |mean-ref|={dev_mean:.3e}")
    assert np.isfinite(got).all() and dev <= STOI_BOUND[extended], (dev, got, want)
    assert dev_mean <= STOI_BOUND[extended], (mean.item(), want.mean())
    if T == 3968:   # M = 29: no segment
        assert (want_info[:, 2] == 29).all()
        assert torch.equal(d.cpu(), torch.full((len(rows),), 1e-5, dtype=torch.float32))
        assert mean.item() == np.float32(1e-5)


def test_stoi_of_identical_signals_is_one(gpu):
    clean, _ = _batch(GROUPS[4224][:2], gpu)
    for ext in (False, True):
        d, _, _ = _run_stoi(clean, clean.clone(), ext)
        assert (d.cpu() - 1.0).abs().max().item() <= STOI_BOUND[ext], d


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_stoi_optional_outputs_offset_view_and_repeat(gpu, extended):
    rows = [("mid_gap", 0, 15), ("lead_gap", 1, 0), ("tail_gap", 2, 15)]
    clean, proc = _batch(rows, gpu)
    d0, mean0, info0 = _run_stoi(clean, proc, extended)
    # the same bits on a second run
    d1, mean1, info1 = _run_stoi(clean, proc, extended)
    assert torch.equal(d0, d1) and torch.equal(mean0, mean1) and torch.equal(info0, info1)
    # mean = NULL, info = NULL: accepted, untouched, d unchanged
    d2, mean2, info2 = _run_stoi(clean, proc, extended, want_mean=False, want_info=False)
    assert torch.equal(d0, d2) and bool(torch.isnan(mean2).all()) and bool((info2 == -7).all())
    # inputs one float into their allocations (4-byte aligned only)
    B, T = clean.shape
    co = torch.zeros(B * T + 1, dtype=torch.float32, device=gpu)[1:].view(B, T).copy_(clean)
    po = torch.zeros(B * T + 1, dtype=torch.float32, device=gpu)[1:].view(B, T).copy_(proc)
    assert co.data_ptr() % 16 == 4 and co.is_contiguous()
    d3, mean3, info3 = _run_stoi(co, po, extended)
    assert torch.equal(d0, d3) and torch.equal(mean0, mean3) and torch.equal(info0, info3)


def test_stoi_graph_replay_equals_eager(gpu):
    """One captured launch replayed on three staged batches whose rows keep
    different numbers of frames: kept, M and J are device data."""
    L = _L()
    sets = [[("mid_gap", s, 15), ("lead_gap", s, 0), ("tail_gap", s, 15)] for s in MR.SEEDS]
    B, T = 3, 8000
    clean = torch.zeros(B, T, dtype=torch.float32, device=gpu)
    proc = torch.zeros(B, T, dtype=torch.float32, device=gpu)
    ws = L.workspace(L.lib().sel_stoi_workspace(B, T), gpu)
    d = torch.full((B,), float("nan"), dtype=torch.float32, device=gpu)
    mean = torch.full((1,), float("nan"), dtype=torch.float32, device=gpu)
    info = torch.full((B, 3), -7, dtype=torch.int32, device=gpu)

    def launch():
        L.call("sel_stoi", L.ptr(clean), L.ptr(proc), B, T, 1, L.ptr(d), L.ptr(mean), L.ptr(info), L.ptr(ws),
               ws.numel(), L.stream())

    eager = [_run_stoi(*_batch(rows, gpu), True) for rows in sets]    # also loads the kernels before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    torch.cuda.synchronize()
    assert bool(torch.isnan(d).all()) and bool((info == -7).all())    # capturing ran nothing
    for rows, (de, me, ie) in zip(sets, eager):
        c, p = _batch(rows, gpu)
        clean.copy_(c)
        proc.copy_(p)
        d.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(d, de) and torch.equal(mean, me) and torch.equal(info, ie), rows
    assert len({int(k) for _, _, i in eager for k in i[:, 1]}) > 1


# ---- SDR family ------------------------------------------------------------
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _sdr_inputs(kind, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, T, generator=g)
    if kind == "near":          # about 80 dB
        return t + 1e-4 * torch.randn(B, T, generator=g), t
    if kind == "pred0":
        return torch.zeros(B, T), t
    if kind == "target0":
        return torch.randn(B, T, generator=g), torch.zeros(B, T)
    if kind == "dc":            # a large offset on both, different on each
        t = 0.1 * t
        return t + 0.01 * torch.randn(B, T, generator=g) + 10.0, t + 7.0
    raise ValueError(kind)


def _offset(x, gpu):
    B, T = x.shape
    return torch.zeros(B * T + 1, dtype=torch.float32, device=gpu)[1:].view(B, T).copy_(x)


@pytest.mark.parametrize("B,T,offset", [(1, 1, False), (1, 255, False), (3, 256, False), (2, 257, False),
                                        (5, 100003, False), (2, 257, True)])
def test_sdr_family_matches_fp64(gpu, B, T, offset):
    from sel import metrics as M
    worst_db, worst_g = 0.0, 0.0
    for kind in ("near", "pred0", "target0", "dc"):
        for si, zm in MODES:
            if kind == "dc" and not zm:
                continue
            p, t = _sdr_inputs(kind, B, T, seed=B * 1000 + T)
            w = torch.linspace(0.5, 1.5, B)
            pd = (_offset(p, gpu) if offset else p.to(gpu)).requires_grad_(True)
            td = _offset(t, gpu) if offset else t.to(gpu)
            vals, mean = M._SDRFn.apply(pd, td, bool(si), bool(zm))
            ((vals * w.to(gpu)).sum() + 0.7 * mean).backward()
            pr = p.double().requires_grad_(True)
            vr = MR.sdr_db(pr, t.double(), si, zm, xp=torch)
            ((vr * w.double()).sum() + 0.7 * vr.mean()).backward()
            ddb = max((vals.detach().cpu().double() - vr.detach()).abs().max().item(),
                      abs(mean.item() - vr.mean().item()))
            gn = pr.grad.norm().item()
            dg = (pd.grad.cpu().double() - pr.grad).norm().item() / gn if gn > 0 else pd.grad.abs().max().item()
            worst_db, worst_g = max(worst_db, ddb), max(worst_g, dg)
            assert np.isfinite(ddb) and ddb <= SDR_DB_BOUND, (kind, si, zm, ddb, vals, vr)
            assert np.isfinite(dg) and dg <= SDR_GRAD_BOUND, (kind, si, zm, dg)
    print(f"SDR-DEV B={B} T={T} offset={int(offset)} max|dB-ref|={worst_db:.3e} max grad rel={worst_g:.3e}")


@pytest.mark.parametrize("B,T", [(1, 1), (3, 256), (5, 100003)])
def test_plain_snr_is_sel_snr_bit_for_bit(gpu, B, T):
    L = _L()
    p, t = _sdr_inputs("near", B, T, seed=7)
    p, t = (p + 0.3 * torch.randn(B, T, generator=torch.Generator().manual_seed(8))).to(gpu), t.to(gpu)
    sums = torch.full((2 * B,), float("nan"), dtype=torch.float64, device=gpu)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=gpu)
    L.call("sel_snr_fwd", L.ptr(p), L.ptr(t), B, T, L.ptr(sums), L.ptr(out), L.stream())
    g = torch.tensor([1.7], dtype=torch.float32, device=gpu)
    gp = torch.full((B, T), float("nan"), dtype=torch.float32, device=gpu)
    L.call("sel_snr_bwd", L.ptr(p), L.ptr(t), B, T, L.ptr(sums), L.ptr(g), L.ptr(gp), L.stream())
    ws = torch.full((6 * B,), float("nan"), dtype=torch.float64, device=gpu)
    vals = torch.full((B,), float("nan"), dtype=torch.float32, device=gpu)
    mean = torch.full((1,), float("nan"), dtype=torch.float32, device=gpu)
    L.call("sel_sdr_fwd", L.ptr(p), L.ptr(t), B, T, 0, 0, L.ptr(vals), L.ptr(mean), L.ptr(ws), 48 * B, L.stream())
    gp2 = torch.full((B, T), float("nan"), dtype=torch.float32, device=gpu)
    L.call("sel_sdr_bwd", L.ptr(p), L.ptr(t), B, T, 0, 0, None, L.ptr(g), L.ptr(gp2), L.ptr(ws), 48 * B, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(mean, out) and torch.equal(ws[:2 * B], sums) and torch.equal(gp2, gp)
    assert bool(torch.isfinite(vals).all())
    # and the module keeps using sel_snr_* for zero_mean=False
    from sel.metrics import SignalNoiseRatio
    pm = p.clone().requires_grad_(True)
    v = SignalNoiseRatio()(pm, t)
    v.backward(g[0])
    assert torch.equal(v.reshape(1), out) and torch.equal(pm.grad, gp)


# ---- modules ---------------------------------------------------------------
def test_modules_against_reference(gpu):
    from sel import metrics as M
    rows = GROUPS[4224][:3]
    clean, proc = _batch(rows, gpu)
    x, y = clean.double().cpu().numpy(), proc.double().cpu().numpy()
    for zm in (False, True):
        assert abs(M.ScaleInvariantSignalDistortionRatio(zm)(proc, clean).item()
                   - MR.sdr_db(y, x, True, zm).mean()) <= SDR_DB_BOUND
        assert abs(M.SignalNoiseRatio(zm)(proc, clean).item() - MR.sdr_db(y, x, False, zm).mean()) <= SDR_DB_BOUND
        assert np.abs(M.si_sdr(proc[:, None], clean[:, None], zm).cpu().numpy()[:, 0]
                      - MR.sdr_db(y, x, True, zm)).max() <= SDR_DB_BOUND
        assert np.abs(M.snr(proc, clean, zm).cpu().numpy() - MR.sdr_db(y, x, False, zm)).max() <= SDR_DB_BOUND
    for ext in (False, True):
        want = np.array([MR.case_ref(*r, ext)["d"] for r in rows])
        assert np.abs(M.stoi(proc, clean, 10000, ext).cpu().numpy() - want).max() <= STOI_BOUND[ext]
        m = M.ShortTimeObjectiveIntelligibility(10000, extended=ext)(proc, clean)   # target is the clean signal
        assert abs(m.item() - want.mean()) <= STOI_BOUND[ext]
    p = proc.clone().requires_grad_(True)
    assert not M.ShortTimeObjectiveIntelligibility(10000)(p, clean).requires_grad
    M.ScaleInvariantSignalDistortionRatio()(p, clean).backward()
    assert bool(torch.isfinite(p.grad).all()) and p.grad.abs().max().item() > 0


def test_stoi_at_48k_is_stoi_of_the_resampled_signals(gpu):
    from sel import metrics as M
    from sel.resample import resample
    g = torch.Generator().manual_seed(3)
    clean = 0.1 * torch.randn(2, 1, 24000, generator=g)
    pred = (clean + 0.05 * torch.randn(2, 1, 24000, generator=g)).to(gpu)
    clean = clean.to(gpu)
    for ext in (False, True):
        a = M.stoi(pred, clean, 48000, ext)
        b = M.stoi(resample(pred, 48000, 10000), resample(clean, 48000, 10000), 10000, ext)
        assert a.shape == (2, 1) and torch.equal(a, b) and bool((a > 1e-3).all())


def test_measures_returns_the_seven_keys(gpu):
    from mel_spectrogram import measures
    g = torch.Generator().manual_seed(4)
    clean = 0.1 * torch.randn(1, 24000, generator=g)
    pred = (clean + 0.02 * torch.randn(1, 24000, generator=g)).to(gpu)
    out = measures(pred, clean.to(gpu))
    assert list(out) == ["MAE", "MSE", "SNR", "SI-SDR(True)", "SI-SDR(False)", "STOI", "Mel-L1"]
    assert all(torch.is_tensor(v) and v.numel() == 1 and bool(torch.isfinite(v).all()) for v in out.values()), out
    assert abs(out["SNR"].item() - 14.0) < 1.0 and 0.5 < out["STOI"].item() <= 1.0


def test_trainer_eval_step_records_measures(gpu):
    from models.autoencoder.AudioDec import Generator
    from losses import MultiMelSpectrogramLoss
    from trainer.denoise import Trainer
    gp = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
    torch.manual_seed(0)
    G = Generator(**gp).to(gpu)
    mel = MultiMelSpectrogramLoss(fs=24000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048],
                                  window="hann_window", num_mels=80, fmin=0, fmax=12000, log_base=None).to(gpu)
    base = {"outdir": None, "train_max_steps": 10, "use_mel_loss": True, "use_stft_loss": False,
            "use_shape_loss": False, "lambda_mel_loss": 45.0, "lambda_vq_loss": 1.0, "generator_grad_norm": -1}
    g = torch.Generator().manual_seed(1)
    xc = 0.1 * torch.randn(2, 1, 12000, generator=g)
    xn = xc + 0.05 * torch.randn(2, 1, 12000, generator=g)
    keys = {}
    for label, extra in (("plain", {}), ("measured", {"eval_measures": ["SI-SDR", "STOI", "ESTOI"],
                                                      "sampling_rate": 24000})):
        tr = Trainer(steps=0, epochs=0, data_loader={}, model={"generator": G, "discriminator": None},
                     criterion={"mel": mel}, optimizer={}, scheduler={}, config=dict(base, **extra), device=gpu)
        G.eval()
        tr._eval_step((xn, xc))
        rec = {k: float(v) for k, v in tr.total_eval_loss.items()}
        assert all(np.isfinite(v) for v in rec.values()), rec
        keys[label] = set(rec)
    added = {"eval/SI-SDR", "eval/STOI", "eval/ESTOI"}
    assert "eval/generator_loss" in keys["plain"] and "eval/mel_loss" in keys["plain"]
    assert not (keys["plain"] & {f"eval/{n}" for n in ("SI-SDR", "SNR", "STOI", "ESTOI")})
    assert keys["measured"] == keys["plain"] | added
