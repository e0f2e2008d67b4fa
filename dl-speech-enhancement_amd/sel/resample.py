"""On-device band-limited resampling — torchaudio.functional.resample's
sinc_interp_hann path (the call at dataloader/AudioDataset.py:28-33) on the
sel_resample HIP kernel (csrc/resample.hip restates the algorithm)."""
import ctypes
import functools
import math

import torch

from sel import _lib as L


@functools.lru_cache(maxsize=64)
def _table_host(orig_freq, new_freq, lowpass_filter_width, rolloff):
    lib = L.load()
    nph, ntaps = ctypes.c_int(), ctypes.c_int()
    L.check(lib.sel_resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, ctypes.byref(nph),
                                  ctypes.byref(ntaps)), "sel_resample_plan")
    t = torch.empty(nph.value, ntaps.value, dtype=torch.float32)
    L.check(lib.sel_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff,
                                    ctypes.c_void_p(t.data_ptr())), "sel_resample_kernel")
    return t


_DEV_TABLES = {}


def _table_dev(o, n, lowpass_filter_width, rolloff, device):
    key = (o, n, lowpass_filter_width, rolloff, device)
    tab = _DEV_TABLES.get(key)
    if tab is None:
        tab = _table_host(o, n, lowpass_filter_width, rolloff).to(device)
        _DEV_TABLES[key] = tab
    return tab


class _ResampleFn(torch.autograd.Function):
    """y = K x on sel_resample, gx = K^T gy on sel_resample_bwd (same plan, same table)."""

    @staticmethod
    def forward(ctx, waveform, o, n, lowpass_filter_width, rolloff):
        lib = L.lib()
        tab = _table_dev(o, n, lowpass_filter_width, rolloff, waveform.device)
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1]).float().contiguous()
        out_len = lib.sel_resample_out_len(x.shape[1], o, n)
        y = torch.empty(x.shape[0], out_len, dtype=torch.float32, device=x.device)
        L.call("sel_resample", L.ptr(x), x.shape[0], x.shape[1], o, n, lowpass_filter_width, rolloff, L.ptr(tab),
               L.ptr(y), L.stream())
        ctx.cfg = (o, n, lowpass_filter_width, rolloff, tab, shape, waveform.dtype)
        return y.view(*shape[:-1], out_len)

    @staticmethod
    def backward(ctx, gy):
        o, n, lowpass_filter_width, rolloff, tab, shape, dtype = ctx.cfg
        g = gy.reshape(-1, gy.shape[-1]).float().contiguous()
        gx = torch.empty(g.shape[0], shape[-1], dtype=torch.float32, device=g.device)
        L.call("sel_resample_bwd", L.ptr(g), g.shape[0], shape[-1], o, n, lowpass_filter_width, rolloff, L.ptr(tab),
               L.ptr(gx), L.stream())
        return gx.view(shape).to(dtype), None, None, None, None


def _resample_var(waveform, lengths, orig_freq, new_freq, lowpass_filter_width, rolloff):
    shape = waveform.shape
    T = shape[-1]
    B = waveform.numel() // T if T else 0
    lens = L.lengths_arg(lengths, B, T, 0, waveform.device, "sel.resample")
    L.need_device(waveform)
    if orig_freq == new_freq:
        return waveform, lens.view(shape[:-1])
    lib = L.lib()
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    tab = _table_dev(o, n, int(lowpass_filter_width), float(rolloff), waveform.device)
    x = waveform.detach().reshape(-1, T).float().contiguous()
    out_len = lib.sel_resample_out_len(T, o, n)
    y = torch.empty(B, out_len, dtype=torch.float32, device=x.device)
    out_lens = torch.empty(B, dtype=torch.int64, device=x.device)
    L.call("sel_resample_var", L.ptr(x), B, T, L.ptr(lens), o, n, int(lowpass_filter_width), float(rolloff),
           L.ptr(tab), L.ptr(y), L.ptr(out_lens), L.stream())
    return y.view(*shape[:-1], out_len), out_lens.view(shape[:-1])


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99,
             resampling_method="sinc_interp_hann", differentiable=False, lengths=None):
    """Drop-in for torchaudio.functional.resample (sinc_interp_hann): (..., time)
    fp32 on the device -> (..., ceil(time * new / orig)) with the reduced ratio.
    differentiable=True (not in torchaudio's signature): the result carries the
    gradient to `waveform` through sel_resample_bwd; the default has no backward.
    lengths (not in torchaudio's signature): row b is resampled as a
    signal of lengths[b] samples and the call returns (y, out_lengths): y is zero
    at and past out_lengths[b] = ceil(lengths[b] * new / orig), a device int64
    tensor computed on the device.  Device lengths are used as they are (a value
    above time counts as time), host lengths are checked against [0, time].  No
    backward with lengths."""
    if resampling_method not in ("sinc_interp_hann", "sinc_interpolation"):
        raise NotImplementedError(f"sel.resample: {resampling_method} is not implemented")
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if lengths is not None:
        if differentiable:
            raise NotImplementedError("sel.resample: lengths with differentiable=True is not implemented")
        return _resample_var(waveform, lengths, int(orig_freq), int(new_freq), lowpass_filter_width, rolloff)
    if orig_freq == new_freq:
        return waveform
    L.need_device(waveform)
    lib = L.lib()
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    if differentiable:
        return _ResampleFn.apply(waveform, o, n, int(lowpass_filter_width), float(rolloff))
    tab = _table_dev(o, n, int(lowpass_filter_width), float(rolloff), waveform.device)
    shape = waveform.shape
    x = waveform.reshape(-1, shape[-1]).float().contiguous()
    out_len = lib.sel_resample_out_len(x.shape[1], o, n)
    y = torch.empty(x.shape[0], out_len, dtype=torch.float32, device=x.device)
    L.call("sel_resample", L.ptr(x), x.shape[0], x.shape[1], o, n, int(lowpass_filter_width), float(rolloff),
           L.ptr(tab), L.ptr(y), L.stream())
    return y.view(*shape[:-1], out_len)
