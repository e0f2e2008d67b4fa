"""GPU checks of the ragged-batch measures.  The oracle is the
package itself, row by row: row b of a ragged call must have the bits of
today's fixed-length call on x[b:b+1, :L_b].contiguous().  Every batch is run
with its padding filled with NaN and then with 1e30, so padding is neither read
into a result nor masked by a multiplication.  The same rows go against the
fp64 restatements at each row's own length, inside the bounds DESIGN §22.5 and
§23.5 already hold (the rows are bit-identical to calls that meet them); the
fp64-accumulated MAE / MSE / Mel-L1 and every batch mean are held to 1e-6
relative (an fp64 accumulation rounded once to fp32 is good to 6e-8).  Then the
device contract on lengths: one captured call serves batches of other lengths,
a length above T acts as T, a too-short row is NaN and leaves its neighbours
alone, and the bits repeat run to run.
"""
import numpy as np
import pytest
import torch

import bss_sdr_ref as BR
import metrics_ref as MR
import ragged_cases as RC

pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_metrics.py and tests/test_gpu_bss_sdr.py
STOI_BOUND = {False: 2e-7, True: 6e-8}
SDR_DB_BOUND = 6e-5
CORR_BOUND = 2e-14
BSS_DB_BOUND = 8e-6
REL_BOUND = 1e-6      # fp64 accumulation, rounded once


def _L():
    from sel import _lib as L
    return L


def _M():
    from sel import metrics as M
    return M


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _lens(lengths, gpu):
    return torch.tensor(list(lengths), dtype=torch.int64, device=gpu)


def _same(a, b):
    """torch.equal that lets NaN equal NaN."""
    a, b = a.detach(), b.detach()
    if not a.is_floating_point():
        return torch.equal(a, b)
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _solo(x, b, n):
    return x[b:b + 1, :n].detach().contiguous()


# ---- SDR family and its gradient ---------------------------------------------
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _sdr_fn(si):
    return _M().si_sdr if si else _M().snr


@pytest.mark.parametrize("which", [0, 1], ids=["edges", "all_below_T"])
@pytest.mark.parametrize("si,zm", MODES)
def test_sdr_family_rows_and_gradient_equal_solo_calls(gpu, si, zm, which):
    lengths = RC.SDR_LENGTHS[which]
    rows = RC.sdr_rows(lengths)
    B, T = len(rows), RC.SDR_T
    fn = _sdr_fn(si)
    g = torch.linspace(0.5, 2.0, B, device=gpu)
    solo = []
    for b, (p, t) in enumerate(rows):
        ps = _dev(p, gpu)[None].requires_grad_(True)
        v = fn(ps, _dev(t, gpu)[None], bool(zm))
        v.backward(g[b:b + 1])
        solo.append((v.detach(), ps.grad))
    lens = _lens(lengths, gpu)
    first = None
    for fill in RC.FILLS:
        p, t = RC.pad(rows, T, fill)
        pd = _dev(p, gpu).requires_grad_(True)
        vals = fn(pd, _dev(t, gpu), bool(zm), lengths=lens)
        vals.backward(g)
        torch.cuda.synchronize()
        for b, n in enumerate(lengths):
            assert torch.equal(vals[b:b + 1].detach(), solo[b][0]), (fill, b, n, vals[b].item(), solo[b][0].item())
            assert torch.equal(pd.grad[b:b + 1, :n], solo[b][1]), (fill, b, n)
            assert torch.count_nonzero(pd.grad[b, n:]).item() == 0 and not torch.isnan(pd.grad[b, n:]).any()
        if first is None:
            first = (vals.detach().clone(), pd.grad.clone())
        else:       # the fill changes nothing
            assert torch.equal(vals.detach(), first[0]) and torch.equal(pd.grad, first[1])
    want = np.array([MR.sdr_db(p.astype(np.float64)[None], t.astype(np.float64)[None], bool(si), bool(zm))[0]
                     for p, t in rows])
    got = first[0].cpu().numpy().astype(np.float64)
    dev = np.abs(got - want).max()
    print(f"RAGGED-SDR si={si} zm={zm} batch={which} max|dB - ref|={dev:.3e} values={got}")
    assert np.isfinite(got).all() and dev <= SDR_DB_BOUND, (got, want)
    # the module: the mean of the per-row values
    M = _M()
    mod = M.ScaleInvariantSignalDistortionRatio(bool(zm)) if si else M.SignalNoiseRatio(bool(zm))
    p, t = RC.pad(rows, T, float("nan"))
    mean = mod(_dev(p, gpu), _dev(t, gpu), lengths=lens)
    rel = abs(float(mean.item()) - got.mean()) / abs(got.mean())
    print(f"RAGGED-SDR si={si} zm={zm} batch={which} mean rel dev={rel:.3e}")
    assert rel <= REL_BOUND


def test_snr_mean_gradient_is_masked(gpu):
    """(scale_invariant, zero_mean) = (0, 0) from the batch mean alone takes the fp32 SNR gradient kernel."""
    lengths = RC.SDR_LENGTHS[0]
    rows = RC.sdr_rows(lengths)
    B, T = len(rows), RC.SDR_T
    M = _M()
    p, t = RC.pad(rows, T, float("nan"))
    pd = _dev(p, gpu).requires_grad_(True)
    M.SignalNoiseRatio()(pd, _dev(t, gpu), lengths=_lens(lengths, gpu)).backward()
    for b, n in enumerate(lengths):
        ps = _dev(rows[b][0], gpu)[None].requires_grad_(True)
        M.SignalNoiseRatio()(ps, _dev(rows[b][1], gpu)[None]).backward()
        # the solo mean is over one row: its gradient is B times the batch's, and 1 / B is not exact in fp32
        assert torch.allclose(pd.grad[b:b + 1, :n] * B, ps.grad, rtol=1e-6, atol=0), (b, n)
        assert torch.count_nonzero(pd.grad[b, n:]).item() == 0
    # all lengths equal to T: the bits of today's call
    full = RC.sdr_rows([T // 2] * 3)
    p, t = RC.pad(full, T // 2, 0.0)
    a = _dev(p, gpu).requires_grad_(True)
    b_ = _dev(p, gpu).requires_grad_(True)
    ma = M.SignalNoiseRatio()(a, _dev(t, gpu))
    mb = M.SignalNoiseRatio()(b_, _dev(t, gpu), lengths=[T // 2] * 3)
    ma.backward()
    mb.backward()
    assert torch.equal(ma, mb) and torch.equal(a.grad, b_.grad)


# ---- BSS-eval SDR --------------------------------------------------------------
def _bss(pd, td, L, zm, lens=None):
    M = _M()
    B = pd.shape[0]
    corr = torch.full((B, 2, L), -7.0, dtype=torch.float64, device=pd.device)
    vals, mean = M._bss_sdr(pd, td, L, zm, 0.0, lens, corr)
    return vals, mean, corr


@pytest.mark.parametrize("which", [0, 1], ids=["edges", "all_below_T"])
@pytest.mark.parametrize("L", RC.BSS_FILTERS)
def test_bss_sdr_rows_equal_solo_calls(gpu, L, which):
    lengths = RC.BSS_LENGTHS[which]
    rows = RC.bss_rows(lengths)
    T = RC.BSS_T
    lens = _lens(lengths, gpu)
    for zm in (False, True):
        solo = [_bss(_dev(p, gpu)[None], _dev(t, gpu)[None], L, zm) for p, t in rows]
        first = None
        for fill in RC.FILLS:
            p, t = RC.pad(rows, T, fill)
            vals, mean, corr = _bss(_dev(p, gpu), _dev(t, gpu), L, zm, lens)
            torch.cuda.synchronize()
            for b, n in enumerate(lengths):
                assert _same(vals[b:b + 1], solo[b][0]), (fill, zm, b, n, vals[b].item(), solo[b][0].item())
                assert _same(corr[b:b + 1], solo[b][2]), (fill, zm, b, n)
            if first is None:
                first = (vals.clone(), mean.clone(), corr.clone())
            else:
                assert _same(vals, first[0]) and _same(mean, first[1]) and _same(corr, first[2])
        if zm:
            continue    # a one-sample row is silent once centred: the fp64 solve is singular there
        vals, mean, corr = first
        got = vals.cpu().numpy().astype(np.float64)
        worst_c = worst_v = 0.0
        for b, (p, t) in enumerate(rows):
            ref = BR.sdr_full(p, t, L, False, want_cond=False)
            c = corr[b].cpu().numpy()
            worst_c = max(worst_c, np.abs(c[0] - ref["r"]).max(), np.abs(c[1] - ref["b"]).max())
            if ref["val"] == np.inf:
                assert got[b] == np.inf or (np.isfinite(got[b]) and got[b] >= 120.0), (b, got[b])
            else:
                assert np.isfinite(got[b]), (b, got[b], ref["val"])
                worst_v = max(worst_v, abs(got[b] - ref["val"]))
        print(f"RAGGED-BSS L={L} batch={which} max|corr - ref|={worst_c:.3e} max|dB - ref|={worst_v:.3e} values={got}")
        assert worst_c <= CORR_BOUND and worst_v <= BSS_DB_BOUND
        if np.isfinite(got).all():
            rel = abs(float(mean.item()) - got.mean()) / abs(got.mean())
            print(f"RAGGED-BSS L={L} batch={which} mean rel dev={rel:.3e}")
            assert rel <= REL_BOUND
        else:
            assert not np.isfinite(float(mean.item()))


# ---- STOI / ESTOI at 10 kHz -----------------------------------------------------
def _stoi_call(clean, proc, ext, lens=None):
    L = _L()
    B, T = clean.shape
    dev = clean.device
    ws = L.workspace(L.lib().sel_stoi_workspace(B, T), dev)
    d = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    mean = torch.full((1,), -7.0, dtype=torch.float32, device=dev)
    info = torch.full((B, 3), -7, dtype=torch.int32, device=dev)
    if lens is None:
        L.call("sel_stoi", L.ptr(clean), L.ptr(proc), B, T, int(ext), L.ptr(d), L.ptr(mean), L.ptr(info), L.ptr(ws),
               ws.numel(), L.stream())
    else:
        L.call("sel_stoi_var", L.ptr(clean), L.ptr(proc), B, T, L.ptr(lens), int(ext), L.ptr(d), L.ptr(mean),
               L.ptr(info), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return d, mean, info


@pytest.mark.parametrize("ext", [False, True], ids=["stoi", "estoi"])
def test_stoi_rows_equal_solo_calls(gpu, ext):
    lengths, rows, T = RC.STOI_LENGTHS, RC.stoi_rows(), RC.STOI_T
    assert max(lengths) < T     # every length below T
    lens = _lens(lengths, gpu)
    solo = [_stoi_call(_dev(x, gpu)[None], _dev(y, gpu)[None], ext) for x, y in rows]
    first = None
    for fill in RC.FILLS:
        x, y = RC.pad(rows, T, fill)
        xd, yd = _dev(x, gpu), _dev(y, gpu)
        d, mean, info = _stoi_call(xd, yd, ext, lens)
        for b, n in enumerate(lengths):
            assert torch.equal(d[b:b + 1], solo[b][0]), (fill, b, n, d[b].item(), solo[b][0].item())
            assert torch.equal(info[b:b + 1], solo[b][2]), (fill, b, n, info[b], solo[b][2])
        assert torch.equal(_M().stoi(yd, xd, 10000, ext, lengths=lens), d)      # the Python form (preds, target)
        if first is None:
            first = (d.clone(), mean.clone(), info.clone())
        else:
            assert torch.equal(d, first[0]) and torch.equal(mean, first[1]) and torch.equal(info, first[2])
    d, mean, info = first
    refs = RC.stoi_refs(ext)
    want_info = np.array([[r["frames"], r["kept"], r["M"]] for r in refs], dtype=np.int32)
    assert np.array_equal(info.cpu().numpy(), want_info), (info.cpu().numpy(), want_info)
    got = d.cpu().numpy().astype(np.float64)
    dev = np.abs(got - np.array([r["d"] for r in refs])).max()
    rel = abs(float(mean.item()) - got.mean()) / got.mean()
    print(f"RAGGED-STOI extended={int(ext)} max|d - ref|={dev:.3e} mean rel dev={rel:.3e} d={got}")
    assert dev <= STOI_BOUND[ext] and rel <= REL_BOUND
    assert got[0] == np.float32(1e-5) and got[1] == np.float32(1e-5) and got[2] > 0.1


# ---- the ragged resampler, and STOI through it -----------------------------------
@pytest.mark.parametrize("orig,new,T,lengths", [(48000, 10000, RC.STOI48_T, RC.STOI48_LENGTHS),
                                                (8000, 10000, 1000, [1, 5, 7, 100, 999, 1000]),
                                                (22050, 24000, 700, [1, 146, 147, 148, 699])],
                         ids=["48k_10k", "8k_10k", "22k05_24k_table_in_cache"])
def test_resample_rows_equal_solo_calls(gpu, orig, new, T, lengths):
    from sel.resample import resample
    lib = _L().lib()
    r = np.random.default_rng(7)
    rows = [(r.standard_normal(n).astype(np.float32),) * 2 for n in lengths]
    lens = _lens(lengths, gpu)
    want_out = [int(lib.sel_resample_out_len(n, orig, new)) for n in lengths]
    for fill in RC.FILLS:
        x, _ = RC.pad(rows, T, fill)
        xd = _dev(x, gpu)
        y, out_lens = resample(xd, orig, new, lengths=lens)
        torch.cuda.synchronize()
        assert y.shape == (len(rows), int(lib.sel_resample_out_len(T, orig, new)))
        assert out_lens.dtype == torch.int64 and out_lens.tolist() == want_out
        for b, n in enumerate(lengths):
            s = resample(_solo(xd, b, n), orig, new)
            assert s.shape[1] == want_out[b] and torch.equal(y[b:b + 1, :want_out[b]], s), (fill, b, n)
            assert torch.count_nonzero(y[b, want_out[b]:]).item() == 0 and not torch.isnan(y[b]).any()


@pytest.mark.parametrize("ext", [False, True], ids=["stoi", "estoi"])
def test_stoi_at_48k_rows_equal_solo_calls(gpu, ext):
    M = _M()
    lengths, rows, T = RC.STOI48_LENGTHS, RC.stoi48_rows(), RC.STOI48_T
    lens = _lens(lengths, gpu)
    solo = [M.stoi(_dev(y, gpu)[None], _dev(x, gpu)[None], 48000, ext) for x, y in rows]
    for fill in RC.FILLS:
        x, y = RC.pad(rows, T, fill)
        d = M.stoi(_dev(y, gpu), _dev(x, gpu), 48000, ext, lengths=lens)
        for b, n in enumerate(lengths):
            assert torch.equal(d[b:b + 1], solo[b]), (fill, b, n, d[b].item(), solo[b].item())
    got = d.cpu().numpy()
    print(f"RAGGED-STOI48 extended={int(ext)} d={got}")
    assert got[0] == np.float32(1e-5) and (got[1:] > 1e-5).all() and (got[1:] <= 1.0).all()
    x, y = RC.pad(rows, T, float("nan"))
    mean = M.ShortTimeObjectiveIntelligibility(48000, ext)(_dev(y, gpu), _dev(x, gpu), lengths=lens)
    assert abs(float(mean.item()) - got.astype(np.float64).mean()) / got.mean() <= REL_BOUND


# ---- power-mel, Mel-L1, MAE and MSE -----------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["edges", "all_below_T"])
def test_mel_rows_equal_solo_calls_and_mel_l1(gpu, which):
    from mel_spectrogram import MelSpectrogram
    M = _M()
    mel = MelSpectrogram(48000).to(gpu)
    assert (mel.n_fft, mel.hop_length) == (RC.MEL_NFFT, RC.MEL_HOP)
    lengths = RC.MEL_LENGTHS[which]
    rows = RC.mel_rows(lengths)
    T = RC.MEL_T
    lens = _lens(lengths, gpu)
    want_frames = [1 + n // RC.MEL_HOP for n in lengths]
    with torch.no_grad():
        solo = [(mel(_dev(p, gpu)[None]), mel(_dev(t, gpu)[None])) for p, t in rows]
        for fill in RC.FILLS:
            p, t = RC.pad(rows, T, fill)
            m1, f1 = mel(_dev(p, gpu), lengths=lens)
            m2, f2 = mel(_dev(t, gpu), lengths=lens)
            torch.cuda.synchronize()
            assert m1.shape == (len(rows), 128, 1 + T // RC.MEL_HOP)
            assert f1.dtype == torch.int64 and f1.tolist() == want_frames and f2.tolist() == want_frames
            for b, F in enumerate(want_frames):
                assert solo[b][0].shape[-1] == F
                assert torch.equal(m1[b:b + 1, :, :F], solo[b][0]) and torch.equal(m2[b:b + 1, :, :F], solo[b][1]), \
                    (fill, b, lengths[b])
                assert torch.count_nonzero(m1[b, :, F:]).item() == 0 and not torch.isnan(m1[b]).any()
                assert torch.count_nonzero(m2[b, :, F:]).item() == 0 and not torch.isnan(m2[b]).any()
        l1, l2, means = M.rows_l1_l2(m1, m2, f1, means=True)
    a, b_ = m1.cpu().numpy(), m2.cpu().numpy()
    want = np.array([RC.l1_l2_ref(a[b, :, :F], b_[b, :, :F]) for b, F in enumerate(want_frames)])
    r1, r2 = _rel(l1.cpu().numpy(), want[:, 0]), _rel(l2.cpu().numpy(), want[:, 1])
    rm = _rel(means.cpu().numpy(), [l1.double().mean().item(), l2.double().mean().item()])
    print(f"RAGGED-MEL batch={which} Mel-L1 rel dev={r1:.3e} squared rel dev={r2:.3e} means rel dev={rm:.3e}")
    assert max(r1, r2, rm) <= REL_BOUND


@pytest.mark.parametrize("which", [0, 1], ids=["edges", "all_below_T"])
def test_mae_mse_rows_match_fp64(gpu, which):
    M = _M()
    lengths = RC.SDR_LENGTHS[which]
    rows = RC.sdr_rows(lengths)
    lens = _lens(lengths, gpu)
    want = np.array([RC.l1_l2_ref(p, t) for p, t in rows])
    outs = []
    for fill in RC.FILLS:
        p, t = RC.pad(rows, RC.SDR_T, fill)
        outs.append(M.rows_l1_l2(_dev(p, gpu), _dev(t, gpu), lens, means=True))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    l1, l2, means = outs[0]
    r1, r2 = _rel(l1.cpu().numpy(), want[:, 0]), _rel(l2.cpu().numpy(), want[:, 1])
    rm = _rel(means.cpu().numpy(), [l1.double().mean().item(), l2.double().mean().item()])
    print(f"RAGGED-L1L2 batch={which} MAE rel dev={r1:.3e} MSE rel dev={r2:.3e} means rel dev={rm:.3e}")
    assert max(r1, r2, rm) <= REL_BOUND


def test_measures_with_lengths_is_the_mean_of_measures_rows(gpu):
    from mel_spectrogram import measures, measures_rows
    lengths = [4100, 6000, 8192]
    r = np.random.default_rng(21)
    rows = [MR.sig(40 + j, n) for j, n in enumerate(lengths)]
    rows = [((x + 0.02 * r.standard_normal(len(x))).astype(np.float32), x.astype(np.float32)) for x in rows]
    p, t = RC.pad(rows, 8192, float("nan"))
    pd, td, lens = _dev(p, gpu), _dev(t, gpu), _lens(lengths, gpu)
    per_row = measures_rows(pd, td, 10000, sdr=True, lengths=lens)
    out = measures(pd, td, 10000, sdr=True, lengths=lens)
    keys = ["MAE", "MSE", "SNR", "SDR", "SI-SDR(True)", "SI-SDR(False)", "STOI", "Mel-L1"]
    assert list(per_row) == keys and list(out) == keys
    for k in keys:
        assert per_row[k].shape == (3,) and out[k].dim() == 0
        want = per_row[k].double().mean().item()
        rel = abs(out[k].item() - want) / abs(want)
        print(f"RAGGED-MEASURES {k}: rows={per_row[k].tolist()} mean={out[k].item()} rel dev={rel:.3e}")
        assert np.isfinite(want) and rel <= REL_BOUND
    # equal lengths given as lengths: the per-row kernel measures of today's fixed-length calls
    M = _M()
    full = measures_rows(pd[2:], td[2:], 10000, sdr=True, lengths=[8192])
    assert torch.equal(full["SNR"], M.snr(pd[2:], td[2:])) and torch.equal(full["SDR"], M.sdr(pd[2:], td[2:]))
    assert torch.equal(full["STOI"], M.stoi(pd[2:], td[2:], 10000))
    assert torch.equal(full["SI-SDR(True)"], M.si_sdr(pd[2:], td[2:], True))
    assert torch.equal(measures_rows(pd[2:], td[2:], 10000, sdr=True)["SI-SDR(False)"], M.si_sdr(pd[2:], td[2:]))


# ---- device lengths ----------------------------------------------------------------
def _measure_fns(gpu):
    from mel_spectrogram import MelSpectrogram
    from sel.resample import resample
    M = _M()
    mel = MelSpectrogram(48000).to(gpu)

    def mel_l1(p, t, n):
        m1, f = mel(p, lengths=n)
        m2, _ = mel(t, lengths=n)
        return (m1, f) + M.rows_l1_l2(m1, m2, f, means=True)

    # name -> (call, the measure's minimum length)
    return {
        "snr": (lambda p, t, n: M._sdr_family(p, t, False, False, n), 1),
        "si_sdr_zero_mean": (lambda p, t, n: M._sdr_family(p, t, True, True, n), 1),
        "bss_sdr": (lambda p, t, n: M._bss_sdr(p, t, 64, True, 0.0, n), 1),
        "stoi": (lambda p, t, n: M._stoi(p, t, 10000, False, n), 256),
        "estoi_16k": (lambda p, t, n: M._stoi(p, t, 16000, True, n), 409),
        "resample": (lambda p, t, n: resample(p, 16000, 10000, lengths=n), 0),
        "mel_l1": (mel_l1, 201),
        "mae_mse": (lambda p, t, n: M.rows_l1_l2(p, t, n, means=True), 1),
    }


_NAMES = ["snr", "si_sdr_zero_mean", "bss_sdr", "stoi", "estoi_16k", "resample", "mel_l1", "mae_mse"]
_DT = 9000
_STAGES = [[9000, 600, 4500, 7000], [409, 9000, 8191, 8192], [3000, 4097, 1000, 8999]]


def _stage(k, gpu):
    r = np.random.default_rng(50 + k)
    rows = []
    for j, n in enumerate(_STAGES[k]):
        x = MR.sig(60 + 4 * k + j, n)
        rows.append(((x + 0.05 * r.standard_normal(n)).astype(np.float32), x.astype(np.float32)))
    p, t = RC.pad(rows, _DT, float("nan"))
    return _dev(p, gpu), _dev(t, gpu), _lens(_STAGES[k], gpu)


@pytest.mark.parametrize("name", _NAMES)
def test_one_captured_call_serves_other_lengths(gpu, name):
    fn = _measure_fns(gpu)[name][0]
    with torch.no_grad():
        stages = [_stage(k, gpu) for k in range(3)]
        eager = [[o.clone() for o in fn(*s)] for s in stages]       # also loads the kernels and tables
        again = [o.clone() for o in fn(*stages[0])]
        assert all(_same(a, b) for a, b in zip(eager[0], again))    # the same bits run to run
        p, t, n = (torch.zeros_like(x) for x in stages[0])
        n.fill_(_DT)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = fn(p, t, n)
        torch.cuda.synchronize()
        for k, s in enumerate(stages):
            for dst, src in zip((p, t, n), s):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            for o, e in zip(outs, eager[k]):
                assert _same(o, e), (name, k)
    assert not all(_same(a, b) for a, b in zip(eager[0], eager[1]))


@pytest.mark.parametrize("name", _NAMES)
def test_length_above_T_acts_as_T_and_a_short_row_is_nan(gpu, name):
    fn, minimum = _measure_fns(gpu)[name]
    with torch.no_grad():
        p, t, _ = _stage(0, gpu)
        T = _DT
        p, t = torch.nan_to_num(p, nan=0.03), torch.nan_to_num(t, nan=0.02)    # finite padding: rows may grow to T
        good = [T, 600, 4500, 7000]
        ref = [o.clone() for o in fn(p, t, _lens(good, gpu))]
        # a length above T acts as T
        over = [o.clone() for o in fn(p, t, _lens([T + 5, 600, 4500, 1 << 40], gpu))]
        whole = [o.clone() for o in fn(p, t, _lens([T, 600, 4500, T], gpu))]
        assert all(_same(a, b) for a, b in zip(over, whole))
        for a, b in zip(over, ref):
            if a.dim() >= 1 and a.shape[0] == 4:
                assert _same(a[:3], b[:3])
        if minimum == 0:
            return
        # a too-short row (and a negative length) is NaN; its neighbours keep their bits; the mean is NaN
        for short in (minimum - 1, 0, -3):
            bad = [o.clone() for o in fn(p, t, _lens([T, short, 4500, 7000], gpu))]
            rows = [(a, b) for a, b in zip(bad, ref) if a.dim() >= 1 and a.shape[0] == 4 and a.is_floating_point()]
            assert rows
            for a, b in rows:
                assert torch.isnan(a[1]).all(), (name, short, a[1])
                assert _same(a[[0, 2, 3]], b[[0, 2, 3]]), (name, short)
            for a in bad:
                if a.is_floating_point() and (a.dim() == 0 or a.shape[0] != 4):
                    assert torch.isnan(a).all(), (name, short, a)       # the batch mean(s)


def test_gradient_of_a_short_row_is_zero(gpu):
    M = _M()
    p, t, _ = _stage(0, gpu)
    p = torch.nan_to_num(p, nan=1e30).requires_grad_(True)
    vals = M.si_sdr(p, torch.nan_to_num(t, nan=1e30), True, lengths=_lens([_DT, 0, 4500, 7000], gpu))
    assert torch.isnan(vals[1]) and torch.isfinite(vals[[0, 2, 3]]).all()
    vals[[0, 2, 3]].sum().backward()
    assert torch.isfinite(p.grad).all() and torch.count_nonzero(p.grad[1]).item() == 0
    assert torch.count_nonzero(p.grad[2, 4500:]).item() == 0 and torch.count_nonzero(p.grad[2, :4500]).item() > 0
