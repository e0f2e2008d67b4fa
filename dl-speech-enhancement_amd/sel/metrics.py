"""Evaluation measures of the reference's mel_spectrogram.py:47-64 on the
MI355X path, and the SNR loss term of train_denoise.py (:120, :140).

The reference uses torchmetrics 1.2.0 and pystoi (third-party, absent here;
parity unpinned beyond their published formulas, restated in fp64 by
tests/metrics_ref.py):

SignalNoiseRatio(zero_mean=False)
    snr_b = 10 * log10((sum_t target^2 + eps) / (sum_t (target - preds)^2 + eps)),
    eps = finfo(float32).eps, mean over the batch; with zero_mean each row's
    mean is subtracted from preds and target first.  zero_mean=False is computed
    by the sel_snr_fwd / sel_snr_bwd HIP kernels, zero_mean=True by sel_sdr_*.
ScaleInvariantSignalDistortionRatio(zero_mean=False)
    alpha = (sum p t + eps) / (sum t^2 + eps), ts = alpha t,
    10 * log10((sum ts^2 + eps) / (sum (ts - p)^2 + eps)), mean over the batch
    (sel_sdr_fwd / sel_sdr_bwd).
ShortTimeObjectiveIntelligibility(fs, extended=False)
    STOI / ESTOI as DESIGN §22.1 defines them, at 10 kHz (sel_stoi); no
    gradient (stoi_loss_values and losses.STOILoss carry one, through
    sel_stoi_bwd and sel_resample_bwd: DESIGN §24).  Signals at another rate
    go through sel.resample.resample(x, fs, 10000) first; pystoi resamples with its own polyphase filter, so parity
    with it at rates other than 10 kHz is unpinned.

SignalDistortionRatio(use_cg_iter=None, filter_length=512, zero_mean=False, load_diag=None)
    The BSS-eval SDR as DESIGN §23 defines it (sel_bss_sdr): fp64 linear
    correlations of the unit-norm signals, a filter_length-tap symmetric
    Toeplitz solve, 10 log10(coh / (1 - coh)); filter_length in [1, 512].  No
    gradient.  A row whose prediction equals its target up to scale is +inf; a
    silent target row is NaN (torchmetrics raises there).  At T < filter_length
    torchmetrics' FFT reads wrapped lags; here the correlations stay linear.

Ragged batches: snr, si_sdr, sdr and stoi and the four modules'
forward take lengths=None.  With lengths, row b of the (..., T) input is its
first lengths[b] samples and nothing past them is read (the padding may hold
anything); the per-row values have the bits of a call on that row alone and a
module returns the mean of the per-row values.  A device int64 tensor is used as
it is, with no host read, so a captured call serves batches of other lengths: a
value above T counts as T and a row below the measure's minimum (1 sample; 256
for STOI at 10 kHz) is NaN.  A host sequence or CPU tensor is checked against
[minimum, T] (ValueError) and copied.  snr and si_sdr keep autograd with lengths
(exact zeros in the gradient at and past lengths[b]); STOI with lengths is
forward only (stoi_loss_values takes none).

All of them differentiate with respect to preds only (the target is data), and
refuse CPU tensors like the rest of the package.  The functional forms snr,
si_sdr, sdr and stoi return the per-row values (shape preds.shape[:-1]).
"""
import math
import warnings

import torch

from . import _lib as L
from .resample import resample

STOI_FS = 10000
SDR_MAX_FILTER_LENGTH = 512


class _SNRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        L.need_device(pred, target)
        T = pred.shape[-1]
        p = pred.contiguous().float().reshape(-1, T)
        t = target.contiguous().float().reshape(-1, T)
        B = p.shape[0]
        sums = torch.empty(2 * B, dtype=torch.float64, device=p.device)
        out = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("sel_snr_fwd", L.ptr(p), L.ptr(t), B, T, L.ptr(sums), L.ptr(out), L.stream())
        ctx.save_for_backward(p, t, sums)
        ctx.shape = pred.shape
        return out

    @staticmethod
    def backward(ctx, g):
        p, t, sums = ctx.saved_tensors
        B, T = p.shape
        gp = torch.empty_like(p)
        L.call("sel_snr_bwd", L.ptr(p), L.ptr(t), B, T, L.ptr(sums), L.ptr(g.contiguous()), L.ptr(gp), L.stream())
        return gp.view(ctx.shape), None


class _SDRFn(torch.autograd.Function):
    """(per-row values, batch mean) of the SDR family; either output may be differentiated."""

    @staticmethod
    def forward(ctx, pred, target, scale_invariant, zero_mean):
        L.need_device(pred, target)
        if pred.shape != target.shape:
            raise ValueError(f"sel.metrics: preds {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
        T = pred.shape[-1]
        p = pred.contiguous().float().reshape(-1, T)
        t = target.contiguous().float().reshape(-1, T)
        B = p.shape[0]
        ws = L.workspace(L.lib().sel_sdr_workspace(B), p.device)
        vals = torch.empty(B, dtype=torch.float32, device=p.device)
        mean = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("sel_sdr_fwd", L.ptr(p), L.ptr(t), B, T, int(scale_invariant), int(zero_mean), L.ptr(vals),
               L.ptr(mean), L.ptr(ws), ws.numel(), L.stream())
        ctx.save_for_backward(p, t, ws)
        ctx.shape = pred.shape
        ctx.flags = (int(scale_invariant), int(zero_mean))
        ctx.set_materialize_grads(False)
        return vals.view(pred.shape[:-1]), mean

    @staticmethod
    def backward(ctx, g_vals, g_mean):
        p, t, ws = ctx.saved_tensors
        if g_vals is None and g_mean is None:
            return None, None, None, None
        B, T = p.shape
        gv = g_vals.contiguous().float().reshape(-1) if g_vals is not None else None
        gm = g_mean.contiguous().float() if g_mean is not None else None
        gp = torch.empty_like(p)
        L.call("sel_sdr_bwd", L.ptr(p), L.ptr(t), B, T, ctx.flags[0], ctx.flags[1], L.ptr(gv), L.ptr(gm), L.ptr(gp),
               L.ptr(ws), ws.numel(), L.stream())
        return gp.view(ctx.shape), None, None, None


def _rows(preds, target):
    if preds.shape != target.shape:
        raise ValueError(f"sel.metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
    T = preds.shape[-1]
    return (preds.numel() // T if T else 0), T


class _SDRVarFn(torch.autograd.Function):
    """_SDRFn over a ragged batch: lens is the device int64 array of sel_sdr_fwd_var / sel_sdr_bwd_var."""

    @staticmethod
    def forward(ctx, pred, target, lens, scale_invariant, zero_mean):
        T = pred.shape[-1]
        p = pred.contiguous().float().reshape(-1, T)
        t = target.contiguous().float().reshape(-1, T)
        B = p.shape[0]
        ws = L.workspace(L.lib().sel_sdr_workspace(B), p.device)
        vals = torch.empty(B, dtype=torch.float32, device=p.device)
        mean = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("sel_sdr_fwd_var", L.ptr(p), L.ptr(t), B, T, L.ptr(lens), int(scale_invariant), int(zero_mean),
               L.ptr(vals), L.ptr(mean), L.ptr(ws), ws.numel(), L.stream())
        ctx.save_for_backward(p, t, lens, ws)
        ctx.shape = pred.shape
        ctx.flags = (int(scale_invariant), int(zero_mean))
        ctx.set_materialize_grads(False)
        return vals.view(pred.shape[:-1]), mean

    @staticmethod
    def backward(ctx, g_vals, g_mean):
        p, t, lens, ws = ctx.saved_tensors
        if g_vals is None and g_mean is None:
            return None, None, None, None, None
        B, T = p.shape
        gv = g_vals.contiguous().float().reshape(-1) if g_vals is not None else None
        gm = g_mean.contiguous().float() if g_mean is not None else None
        gp = torch.empty_like(p)
        L.call("sel_sdr_bwd_var", L.ptr(p), L.ptr(t), B, T, L.ptr(lens), ctx.flags[0], ctx.flags[1], L.ptr(gv),
               L.ptr(gm), L.ptr(gp), L.ptr(ws), ws.numel(), L.stream())
        return gp.view(ctx.shape), None, None, None, None


def _sdr_family(preds, target, scale_invariant, zero_mean, lengths):
    if lengths is None:
        return _SDRFn.apply(preds, target, scale_invariant, zero_mean)
    B, T = _rows(preds, target)
    lens = L.lengths_arg(lengths, B, T, 1, preds.device, "sel.metrics")
    L.need_device(preds, target)
    return _SDRVarFn.apply(preds, target, lens, scale_invariant, zero_mean)


def snr(preds, target, zero_mean=False, lengths=None):
    """Per-row SNR in dB (torchmetrics.functional.signal_noise_ratio)."""
    return _sdr_family(preds, target, False, bool(zero_mean), lengths)[0]


def si_sdr(preds, target, zero_mean=False, lengths=None):
    """Per-row SI-SDR in dB (torchmetrics.functional.scale_invariant_signal_distortion_ratio)."""
    return _sdr_family(preds, target, True, bool(zero_mean), lengths)[0]


def stoi_min_length(fs):
    """The shortest signal at rate fs that gives one STOI frame (256 samples at 10 kHz)."""
    g = math.gcd(int(fs), STOI_FS)
    o, n = int(fs) // g, STOI_FS // g
    return 255 * o // n + 1  # smallest len with ceil(n len / o) >= 256


def _stoi_var(preds, target, fs, extended, lengths, info=None):
    B, T = _rows(preds, target)
    lens = L.lengths_arg(lengths, B, T, stoi_min_length(fs), preds.device, "sel.metrics")
    L.need_device(preds, target)
    shape = preds.shape[:-1]
    if int(fs) != STOI_FS:  # both signals through the ragged resampler, on the device lengths
        preds, out_lens = resample(preds, int(fs), STOI_FS, lengths=lens)
        target, _ = resample(target, int(fs), STOI_FS, lengths=lens)
        lens = out_lens
    T = preds.shape[-1]
    p = preds.detach().contiguous().float().reshape(-1, T)
    t = target.detach().contiguous().float().reshape(-1, T)
    ws = L.workspace(L.lib().sel_stoi_workspace(B, T), p.device)
    d = torch.empty(B, dtype=torch.float32, device=p.device)
    mean = torch.empty((), dtype=torch.float32, device=p.device)
    L.call("sel_stoi_var", L.ptr(t), L.ptr(p), B, T, L.ptr(lens), int(bool(extended)), L.ptr(d), L.ptr(mean),
           L.ptr(info), L.ptr(ws), ws.numel(), L.stream())
    return d.view(shape), mean


def _stoi(preds, target, fs, extended, lengths=None):
    if lengths is not None:
        return _stoi_var(preds, target, fs, extended, lengths)
    L.need_device(preds, target)
    if preds.shape != target.shape:
        raise ValueError(f"sel.metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
    if int(fs) != STOI_FS:
        preds, target = resample(preds, int(fs), STOI_FS), resample(target, int(fs), STOI_FS)
    T = preds.shape[-1]
    p = preds.detach().contiguous().float().reshape(-1, T)
    t = target.detach().contiguous().float().reshape(-1, T)
    B = p.shape[0]
    ws = L.workspace(L.lib().sel_stoi_workspace(B, T), p.device)
    d = torch.empty(B, dtype=torch.float32, device=p.device)
    mean = torch.empty((), dtype=torch.float32, device=p.device)
    L.call("sel_stoi", L.ptr(t), L.ptr(p), B, T, int(bool(extended)), L.ptr(d), L.ptr(mean), None, L.ptr(ws),
           ws.numel(), L.stream())
    return d.view(preds.shape[:-1]), mean


@torch.no_grad()
def stoi(preds, target, fs, extended=False, lengths=None):
    """Per-row STOI (ESTOI with extended=True); `target` is the clean signal."""
    return _stoi(preds, target, fs, extended, lengths)[0]


class _STOIFn(torch.autograd.Function):
    """(per-row d, batch mean) of STOI / ESTOI at 10 kHz with the gradient with
    respect to preds; either output may be differentiated.  The
    silent-frame mask is a constant selection and target is data."""

    @staticmethod
    def forward(ctx, preds, target, extended):
        L.need_device(preds, target)
        if preds.shape != target.shape:
            raise ValueError(f"sel.metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
        T = preds.shape[-1]
        p = preds.contiguous().float().reshape(-1, T)
        t = target.contiguous().float().reshape(-1, T)
        B = p.shape[0]
        ws = L.workspace(L.lib().sel_stoi_workspace(B, T), p.device)
        d = torch.empty(B, dtype=torch.float32, device=p.device)
        mean = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("sel_stoi", L.ptr(t), L.ptr(p), B, T, int(bool(extended)), L.ptr(d), L.ptr(mean), None, L.ptr(ws),
               ws.numel(), L.stream())
        ctx.save_for_backward(p, t, ws)
        ctx.shape = preds.shape
        ctx.extended = int(bool(extended))
        ctx.set_materialize_grads(False)
        return d.view(preds.shape[:-1]), mean

    @staticmethod
    def backward(ctx, g_d, g_mean):
        p, t, ws = ctx.saved_tensors
        if g_d is None and g_mean is None:
            return None, None, None
        B, T = p.shape
        gd = g_d.contiguous().float().reshape(-1) if g_d is not None else None
        gm = g_mean.contiguous().float() if g_mean is not None else None
        wsb = L.workspace(L.lib().sel_stoi_bwd_workspace(B, T), p.device)
        gp = torch.empty_like(p)
        L.call("sel_stoi_bwd", L.ptr(t), L.ptr(p), B, T, ctx.extended, L.ptr(gd), L.ptr(gm), L.ptr(gp), L.ptr(ws),
               ws.numel(), L.ptr(wsb), wsb.numel(), L.stream())
        return gp.view(ctx.shape), None, None


def _stoi_grad(preds, target, fs, extended):
    L.need_device(preds, target)
    if preds.shape != target.shape:
        raise ValueError(f"sel.metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
    if int(fs) != STOI_FS:
        preds = resample(preds, int(fs), STOI_FS, differentiable=True)
        target = resample(target.detach(), int(fs), STOI_FS)
    return _STOIFn.apply(preds, target.detach(), bool(extended))


def stoi_loss_values(preds, target, fs, extended=False):
    """Per-row STOI (ESTOI with extended=True) that carries the gradient to preds;
    `target` is the clean signal.  At fs != 10000 preds goes through the
    differentiable resampler first (sel_resample / sel_resample_bwd)."""
    return _stoi_grad(preds, target, fs, extended)[0]


def rows_l1_l2(a, b, n, means=False):
    """Per-row mean |a - b| and mean (a - b)^2 of a ragged batch (sel_rows_l1_l2_var):
    a, b (B, stride) or (B, inner, stride) fp32 on the device, of which the first
    n[b] elements of every sub-row count; n a device int64 tensor.  fp64 sums in a
    fixed order.  With means=True also the (2,) batch means of the two."""
    L.need_device(a, b, n)
    if a.shape != b.shape or a.dim() not in (2, 3):
        raise ValueError(f"sel.metrics: rows_l1_l2 needs two (B, stride) or (B, inner, stride) tensors, got "
                         f"{tuple(a.shape)} and {tuple(b.shape)}")
    B, stride = a.shape[0], a.shape[-1]
    inner = a.shape[1] if a.dim() == 3 else 1
    if n.dtype != torch.int64 or n.numel() != B:
        raise ValueError(f"sel.metrics: rows_l1_l2 needs {B} int64 counts")
    a = a.detach().contiguous().float()
    b = b.detach().contiguous().float()
    l1 = torch.empty(B, dtype=torch.float32, device=a.device)
    l2 = torch.empty(B, dtype=torch.float32, device=a.device)
    m = torch.empty(2, dtype=torch.float32, device=a.device) if means else None
    L.call("sel_rows_l1_l2_var", L.ptr(a), L.ptr(b), B, inner, stride, L.ptr(n.contiguous()), L.ptr(l1), L.ptr(l2),
           L.ptr(m), L.stream())
    return (l1, l2, m) if means else (l1, l2)


_warned_cg = False


def _check_sdr_args(use_cg_iter, filter_length, load_diag):
    global _warned_cg
    if isinstance(filter_length, bool) or int(filter_length) != filter_length or \
            not 1 <= int(filter_length) <= SDR_MAX_FILTER_LENGTH:
        raise ValueError(f"sel.metrics: filter_length must be an integer in [1, {SDR_MAX_FILTER_LENGTH}], "
                         f"got {filter_length!r}")
    if load_diag is not None and not (math.isfinite(float(load_diag)) and float(load_diag) >= 0.0):
        raise ValueError(f"sel.metrics: load_diag must be finite and not negative, got {load_diag!r}")
    if use_cg_iter is not None and not _warned_cg:
        _warned_cg = True
        warnings.warn("sel.metrics: use_cg_iter needs fast-bss-eval's conjugate-gradient solve, which is not built; "
                      "the direct solve is used", UserWarning, stacklevel=3)
    return int(filter_length), 0.0 if load_diag is None else float(load_diag)


def _bss_sdr(preds, target, filter_length, zero_mean, load_diag, lengths=None, corr=None):
    lens = None
    if lengths is not None:
        B, T = _rows(preds, target)
        lens = L.lengths_arg(lengths, B, T, 1, preds.device, "sel.metrics")
    L.need_device(preds, target)
    if preds.shape != target.shape:
        raise ValueError(f"sel.metrics: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
    T = preds.shape[-1]
    p = preds.detach().contiguous().float().reshape(-1, T)
    t = target.detach().contiguous().float().reshape(-1, T)
    B = p.shape[0]
    ws = L.workspace(L.lib().sel_bss_sdr_workspace(B, T, filter_length), p.device)
    vals = torch.empty(B, dtype=torch.float32, device=p.device)
    mean = torch.empty((), dtype=torch.float32, device=p.device)
    if lens is None:
        L.call("sel_bss_sdr", L.ptr(p), L.ptr(t), B, T, filter_length, int(bool(zero_mean)), load_diag, L.ptr(vals),
               L.ptr(mean), L.ptr(corr), L.ptr(ws), ws.numel(), L.stream())
    else:
        L.call("sel_bss_sdr_var", L.ptr(p), L.ptr(t), B, T, L.ptr(lens), filter_length, int(bool(zero_mean)),
               load_diag, L.ptr(vals), L.ptr(mean), L.ptr(corr), L.ptr(ws), ws.numel(), L.stream())
    return vals.view(preds.shape[:-1]), mean


@torch.no_grad()
def sdr(preds, target, use_cg_iter=None, filter_length=512, zero_mean=False, load_diag=None, lengths=None):
    """Per-row BSS-eval SDR in dB (torchmetrics.functional.signal_distortion_ratio,
    direct solve).  No autograd: the result carries no grad_fn."""
    filter_length, load_diag = _check_sdr_args(use_cg_iter, filter_length, load_diag)
    return _bss_sdr(preds, target, filter_length, zero_mean, load_diag, lengths)[0]


class SignalNoiseRatio(torch.nn.Module):
    """Drop-in for torchmetrics.audio.SignalNoiseRatio as called by train_denoise.py."""

    def __init__(self, zero_mean=False):
        super().__init__()
        self.zero_mean = bool(zero_mean)

    def forward(self, preds, target, lengths=None):
        if lengths is not None:
            return _sdr_family(preds, target, False, self.zero_mean, lengths)[1]
        if self.zero_mean:
            return _SDRFn.apply(preds, target, False, True)[1]
        return _SNRFn.apply(preds, target)


class ScaleInvariantSignalDistortionRatio(torch.nn.Module):
    """Drop-in for torchmetrics.audio.ScaleInvariantSignalDistortionRatio (batch mean, in dB)."""

    def __init__(self, zero_mean=False):
        super().__init__()
        self.zero_mean = bool(zero_mean)

    def forward(self, preds, target, lengths=None):
        return _sdr_family(preds, target, True, self.zero_mean, lengths)[1]


class SignalDistortionRatio(torch.nn.Module):
    """Drop-in for torchmetrics.audio.SignalDistortionRatio (batch mean, in dB);
    filter_length in [1, 512].  No autograd: the result carries no grad_fn."""

    def __init__(self, use_cg_iter=None, filter_length=512, zero_mean=False, load_diag=None):
        super().__init__()
        self.filter_length, self.load_diag = _check_sdr_args(use_cg_iter, filter_length, load_diag)
        self.zero_mean = bool(zero_mean)

    @torch.no_grad()
    def forward(self, preds, target, lengths=None):
        return _bss_sdr(preds, target, self.filter_length, self.zero_mean, self.load_diag, lengths)[1]


class ShortTimeObjectiveIntelligibility(torch.nn.Module):
    """Drop-in for torchmetrics.audio.ShortTimeObjectiveIntelligibility (batch mean).
    Parity with pystoi is unpinned; at fs != 10000 the resampler differs from pystoi's."""

    def __init__(self, fs, extended=False):
        super().__init__()
        if int(fs) <= 0:
            raise ValueError("sel.metrics: fs must be positive")
        self.fs = int(fs)
        self.extended = bool(extended)

    @torch.no_grad()
    def forward(self, preds, target, lengths=None):
        return _stoi(preds, target, self.fs, self.extended, lengths)[1]
