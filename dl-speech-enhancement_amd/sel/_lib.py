"""ctypes binding of libsel.so (include/sel.h).

The product path has no CPU fallback: every op requires ROCm device tensors and
the built library; anything else raises.  PyTorch is used only for device
memory (caching allocator), streams and autograd plumbing.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEL_LIB", os.path.join(_HERE, "libsel.so"))

P = ctypes.c_void_p
I64 = ctypes.c_int64
I32 = ctypes.c_int
F32 = ctypes.c_float
F64 = ctypes.c_double
SZ = ctypes.c_size_t

# name -> (restype, argtypes); must cover every function declared in include/sel.h
SIGNATURES = {
    "sel_init": (I32, []),
    "sel_last_error": (ctypes.c_char_p, []),
    "sel_version": (I32, []),
    "sel_tune": (I32, [I32, I32]),
    "sel_tune_get": (I32, [I32]),
    "sel_probe_buffer_b64": (I32, [P, I32, I32, P, P]),
    "sel_probe_copy_f4": (I32, [P, P, I64, I32, P]),
    "sel_stft_mag_fwd": (I32, [P, I64, I64, I32, I32, I32, P, F32, P, P]),
    "sel_stft_bwd_workspace": (SZ, [I64, I64, I32, I32, I32]),
    "sel_stft_mag_bwd": (I32, [P, I64, I64, I32, I32, I32, P, F32, P, P, P, SZ, P]),
    "sel_mag_pair_workspace": (SZ, [I64]),
    "sel_mag_pair_sums": (I32, [P, P, I64, P, P, SZ, P]),
    "sel_mag_pair_bwd": (I32, [P, P, I64, P, P, P, P]),
    "sel_stft_loss_workspace": (SZ, [I64, I64, I32, I32, I32]),
    "sel_stft_loss_fwd": (I32, [P, P, I64, I64, I32, I32, I32, P, P, P, SZ, P]),
    "sel_stft_loss_bwd": (I32, [P, P, I64, I64, I32, I32, I32, P, P, P, P, SZ, P]),
    "sel_stft_loss_finish": (I32, [P, I64, P, P]),
    "sel_stft_loss_coef": (I32, [P, I64, P, P, P, P]),
    "sel_logmel_fwd": (I32, [P, I64, I64, I32, I32, I32, P, P, P, I32, F32, I32, P, P]),
    "sel_l1_workspace": (SZ, [I64]),
    "sel_l1_mean": (I32, [P, P, I64, P, P, SZ, P]),
    "sel_mel_l1_workspace": (SZ, [I64, I64, I32, I32, I32]),
    "sel_mel_l1_fwd_grad": (I32, [P, P, I64, I64, I32, I32, I32, P, P, P, P, I32, F32, I32, P, P, P, SZ, P]),
    "sel_logmel_bwd_workspace": (SZ, [I64, I64, I32, I32, I32]),
    "sel_logmel_bwd": (I32, [P, I64, I64, I32, I32, I32, P, P, P, P, I32, F32, I32,
                             P, P, P, F32, P, P, SZ, P]),
    "sel_conv_fwd_kernel_id": (I32, [P, I32, I32, I32]),
    "sel_conv_fwd": (I32, [P, I32, I32, P, P, P, P, P, P, P]),
    "sel_resunit_fwd": (I32, [P, I32, P, P, P, P, P, P, P, P]),
    "sel_resunit_bwd": (I32, [P, I32, P, P, P, P, P, P, P, P]),
    "sel_resunit_wgrad_splits": (I32, [P, I32]),
    "sel_resunit_bwd_wgrad": (I32, [P, I32, P, P, P, P, P, P, P, P, I32, P]),
    "sel_conv_wgrad_workspace": (SZ, [P]),
    "sel_conv_wgrad": (I32, [P, I32, P, P, P, P, P, SZ, P]),
    "sel_conv_wgrad_partials": (I32, [P, I32, P, P, I32, P, SZ, P, P]),
    "sel_wgrad_finish_many": (I32, [P, I32, P]),
    "sel_pack_weight": (I32, [I32, P, I32, I32, I32, I32, I32, P, P]),
    "sel_pack_dgrad": (I32, [P, I32, I32, I32, I32, P, P]),
    "sel_unpack_wgrad": (I32, [I32, P, I32, I32, I32, I32, P, P]),
    "sel_conv_replicate_fix": (I32, [P, I32, P, P, P, P]),
    "sel_cast": (I32, [P, I32, P, I32, I64, P]),
    "sel_rvq_workspace": (SZ, [I64, I32, I32]),
    "sel_rvq_fwd": (I32, [P, I64, I32, P, I32, I32, P, P, P, P, P, SZ, P]),
    "sel_rvq_finish": (I32, [P, P, I64, I32, I32, I32, F32, P, P, P]),
    "sel_rvq_bwd": (I32, [P, I64, I32, P, I32, P, P, P, F32, P, P]),
    "sel_rvq_step": (I32, [P, I32, I32, I32, P, I32, I32, P, I32, P, P, P]),
    "sel_rvq_lookup_step": (I32, [P, I32, I32, I32, I64, I32, P, P, P, P, I32, P, P]),
    "sel_rvq_step_wire": (I32, [P, I32, I32, I32, P, I32, I32, P, I32, P, P, P, P]),
    "sel_rvq_lookup_wire_step": (I32, [P, I32, I32, I32, I32, I32, P, P, P, P, I32, P, P, P]),
    "sel_rvq_step_dgram": (I32, [P, I32, I32, I32, P, I32, I32, P, P, P, I32, P, P, P, I64, P]),
    "sel_rvq_lookup_dgram_step": (I32, [P, I64, I32, I32, I32, I32, I32, P, P, P, P, P, P, P, I64, I32, I32, P, P, P]),
    "sel_rvq_ema_workspace": (SZ, [I64, I32, I32, I32]),
    "sel_rvq_ema_update": (I32, [P, I64, I32, P, I32, I32, P, P, P, F32, F32, P, SZ, P]),
    "sel_rvq_ema_stats_floats": (SZ, [I32, I32, I32]),
    "sel_rvq_ema_stats_workspace": (SZ, [I64, I32, I32, I32]),
    "sel_rvq_ema_stats": (I32, [P, I64, I32, P, I32, I32, P, I32, P, P, SZ, P]),
    "sel_rvq_ema_apply": (I32, [P, I32, I32, I32, I32, P, F32, F32, P]),
    "sel_add_noise_workspace": (SZ, [I64]),
    "sel_add_noise": (I32, [P, P, I64, F32, P, P, SZ, P]),
    "sel_power_mel_fwd": (I32, [P, I64, I64, I32, I32, I32, P, P, P, I32, F32, P, P]),
    "sel_pack_many": (I32, [P, I32, I64, I32, P]),
    "sel_pack_many_host": (I32, [P, I32, I64, I32, P]),
    "sel_conv_wgrad_unpacked": (I32, [P, I32, P, P, I32, I32, I32, I32, I32, P, P, P, SZ, P]),
    "sel_sumsq2": (I32, [P, P, I64, P, P, SZ, P]),
    "sel_mix_noise": (I32, [P, P, I64, P, F32, P, P]),
    "sel_snr_fwd": (I32, [P, P, I64, I64, P, P, P]),
    "sel_snr_bwd": (I32, [P, P, I64, I64, P, P, P, P]),
    "sel_sdr_workspace": (SZ, [I64]),
    "sel_sdr_fwd": (I32, [P, P, I64, I64, I32, I32, P, P, P, SZ, P]),
    "sel_sdr_bwd": (I32, [P, P, I64, I64, I32, I32, P, P, P, P, SZ, P]),
    "sel_stoi_workspace": (SZ, [I64, I64]),
    "sel_stoi": (I32, [P, P, I64, I64, I32, P, P, P, P, SZ, P]),
    "sel_stoi_band_edges": (I32, [P]),
    "sel_stoi_bwd_workspace": (SZ, [I64, I64]),
    "sel_stoi_bwd": (I32, [P, P, I64, I64, I32, P, P, P, P, SZ, P, SZ, P]),
    "sel_bss_sdr_chunk": (I64, []),
    "sel_bss_sdr_workspace": (SZ, [I64, I64, I32]),
    "sel_bss_sdr": (I32, [P, P, I64, I64, I32, I32, F64, P, P, P, P, SZ, P]),
    "sel_sdr_fwd_var": (I32, [P, P, I64, I64, P, I32, I32, P, P, P, SZ, P]),
    "sel_sdr_bwd_var": (I32, [P, P, I64, I64, P, I32, I32, P, P, P, P, SZ, P]),
    "sel_stoi_var": (I32, [P, P, I64, I64, P, I32, P, P, P, P, SZ, P]),
    "sel_bss_sdr_var": (I32, [P, P, I64, I64, P, I32, I32, F64, P, P, P, P, SZ, P]),
    "sel_resample_var": (I32, [P, I64, I64, P, I32, I32, I32, F32, P, P, P, P]),
    "sel_power_mel_fwd_var": (I32, [P, I64, I64, P, I32, I32, I32, P, P, P, I32, F32, P, P, P]),
    "sel_rows_l1_l2_var": (I32, [P, P, I64, I64, I64, P, P, P, P, P]),
    "sel_batchnorm_workspace": (SZ, [I64, I32]),
    "sel_batchnorm_fwd": (I32, [P, I64, I32, P, P, I32, F32, F32, P, P, P, P, P, P, SZ, P]),
    "sel_batchnorm_bwd": (I32, [P, P, I64, I32, P, P, P, I32, P, P, P, P, SZ, P]),
    "sel_resample_plan": (I32, [I32, I32, I32, F32, P, P]),
    "sel_resample_out_len": (I64, [I64, I32, I32]),
    "sel_resample_kernel": (I32, [I32, I32, I32, F32, P]),
    "sel_resample": (I32, [P, I64, I64, I32, I32, I32, F32, P, P, P]),
    "sel_resample_bwd": (I32, [P, I64, I64, I32, I32, I32, F32, P, P, P]),
    "sel_shape_loss_workspace": (SZ, [I64, I64, I32]),
    "sel_shape_loss_fwd": (I32, [P, P, I64, I64, I32, P, P, P, P, SZ, P]),
    "sel_shape_loss_bwd": (I32, [P, I64, I64, I32, P, P, P, F32, P, P]),
    "sel_dconv_kernel": (I32, [P, I32, ctypes.c_char_p, SZ]),
    "sel_dconv_fwd": (I32, [P, I32, P, P, P, P, P, P, P]),
    "sel_dconv_geometry": (I32, [I32, I32, I32, P, P]),
    "sel_dconv_pack": (I32, [I32, P, P, I32, I32, I32, I32, I32, I32, I32, P, P]),
    "sel_dconv_pack_many": (I32, [P, I32, I32, P]),
    "sel_dconv_wgrad_workspace": (SZ, [P, I32]),
    "sel_dconv_wgrad_kernel": (I32, [P, I32, ctypes.c_char_p, SZ, P]),
    "sel_dconv_w3_instances": (I32, [P, I32]),
    "sel_dconv_wgrad": (I32, [P, I32, P, P, I32, I32, I32, I32, I32, P, P, P, P, P, P, SZ, P]),
    "sel_dconv_wgrad_partials": (I32, [P, I32, P, P, I32, I32, I32, I32, I32, P, P, P, P, P, P, SZ, P, P]),
    "sel_dconv_wgrad_finish_many": (I32, [P, I32, P]),
    "sel_adam_step_many": (I32, [P, I32, F64, F64, F64, F64, F64, F64, P]),
    "sel_adam_step_many_dev": (I32, [P, I32, F64, F64, F64, F64, P, P, P, P]),
    "sel_avgpool1d_fwd": (I32, [P, I32, I32, I32, I32, I32, I32, I32, I32, P, P]),
    "sel_avgpool1d_bwd": (I32, [P, I32, I32, I32, I32, I32, I32, I32, I32, P, P]),
    "sel_mpd_fold": (I32, [P, I32, I32, I32, I32, I32, P, P]),
    "sel_mpd_unfold": (I32, [P, I32, I32, I32, I32, I32, P, P]),
    "sel_gan_workspace": (SZ, []),
    "sel_gan_reduce": (I32, [I32, I32, P, P, P, P, P, P, I32, F32, ctypes.c_double, I32, P, P, SZ, P]),
    "sel_gan_grad": (I32, [I32, I32, P, P, P, P, P, P, I32, F32, P, F32, P, P, I32, P]),
    "sel_hfg_conv_kernel": (I32, [P, I32, I32]),
    "sel_hfg_conv_fwd": (I32, [P, I32, I32, P, P, P, P, P, P]),
    "sel_hfg_reslayer_fwd": (I32, [P, I32, P, P, P, P, P, P, P]),
    "sel_hfg_conv_bwd_kernel": (I32, [P, I32, I32, I32]),
    "sel_hfg_conv_bwd_data": (I32, [P, I32, I32, P, P, P, P, P, F32, P, P]),
    "sel_hfg_conv_wgrad_workspace": (SZ, [P, I32, I32]),
    "sel_hfg_conv_wgrad": (I32, [P, I32, I32, P, P, P, P, P, P, SZ, P]),
    "sel_sconv_check": (I32, [P]),
    "sel_sconv_fwd": (I32, [P, I32, P, P, P, P, P]),
    "sel_sconv_bwd_data": (I32, [P, I32, P, P, P, P, P]),
    "sel_sconv_wgrad_workspace": (SZ, [P, I32]),
    "sel_sconv_wgrad": (I32, [P, I32, P, P, P, P, P, SZ, P]),
    "sel_conv_step": (I32, [P, I32, I32, P, P, P, P, P, P, P, P]),
    "sel_stream_commit": (I32, [P, I32, P]),
    "sel_hfg_conv_step": (I32, [P, I32, I32, P, P, P, P, P, P, P, P]),
    "sel_conv_step_pool": (I32, [P, I32, I32, P, P, I32, P, P, P, P, P, P, P, P]),
    "sel_stream_copy_slots": (I32, [P, I32, I32, P, P, I32, P, P]),
    "sel_hfg_conv_step_pool": (I32, [P, I32, I32, P, P, I32, P, P, P, P, P, P, P, P]),
}

_lock = threading.Lock()
_lib = None
_initialized = False


class SelError(RuntimeError):
    pass


def load():
    """dlopen libsel.so (no GPU needed) and declare every C signature."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise SelError(f"libsel.so not found at {LIB_PATH}: build it with "
                               f"`make -C dl-speech-enhancement_amd/csrc` (hipcc, gfx950)")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def lib():
    """Loaded + initialised library (uploads FFT tables; needs the GPU)."""
    global _initialized
    L = load()
    if not _initialized:
        with _lock:
            if not _initialized:
                if not torch.cuda.is_available():
                    raise SelError("sel: no ROCm GPU visible; the MI355X path has no CPU fallback")
                torch.cuda.init()
                rc = L.sel_init()
                if rc != 0:
                    raise SelError(f"sel_init failed ({rc}): {L.sel_last_error().decode()}")
                # kernel-selection knobs for A/B measurements: SEL_TUNE="4=1,6=1"
                for kv in filter(None, os.environ.get("SEL_TUNE", "").split(",")):
                    k, v = kv.split("=")
                    L.sel_tune(int(k), int(v))
                _initialized = True
    return L


class KernelTimer:
    """Brackets selected C-ABI calls with HIP events on the launching stream
    (torch.cuda.current_stream(), the stream every sel call enqueues on) — used
    by bench.py for the live roofline.  Each record carries the caller's tag
    (kernel instance) and algorithmic bytes / flops of that launch."""

    def __init__(self, names):
        self.names = set(names)
        self.records = []  # (name, tag, bytes, flops, ev0, ev1)

    def add(self, name, meta, ev0, ev1):
        tag, nbytes, flops = meta if meta else (name, 0, 0)
        self.records.append((name, tag, nbytes, flops, ev0, ev1))

    def summary(self):
        """{tag: (launches, total_ms, bytes, flops)}"""
        torch.cuda.synchronize()
        out = {}
        for name, tag, nb, fl, a, b in self.records:
            n, ms, B, F = out.get(tag, (0, 0.0, 0, 0))
            out[tag] = (n + 1, ms + a.elapsed_time(b), B + nb, F + fl)
        return out

    def durations_ms(self, name):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for n, _, _, _, a, b in self.records if n == name]


TIMER = None


def call(name, *args, meta=None):
    """Invoke a C entry point, raise SelError on failure, optionally timed.
    meta = (tag, algorithmic bytes, flops) for the KernelTimer."""
    fn = getattr(lib(), name)
    t = TIMER
    if t is not None and name in t.names:
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        t.add(name, meta() if callable(meta) else meta, a, b)
    else:
        rc = fn(*args)
    check(rc, name)


def check(rc, what):
    if rc != 0:
        raise SelError(f"{what} failed ({rc}): {load().sel_last_error().decode()}")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def need_device(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise SelError("sel: the MI355X path needs ROCm device tensors (got a CPU tensor); "
                           "there is no CPU fallback")


def check_host_lengths(lengths, B, T, minimum, what):
    """Per-row lengths given on the host (a sequence or a CPU tensor): B integers
    in [minimum, T], as a CPU int64 tensor; anything else is a ValueError."""
    t = torch.as_tensor(lengths)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{what}: lengths must be integers, got {t.dtype}")
    t = t.reshape(-1).to(torch.int64)
    if t.numel() != B:
        raise ValueError(f"{what}: {t.numel()} lengths for {B} rows")
    if B and (int(t.min()) < minimum or int(t.max()) > T):
        raise ValueError(f"{what}: lengths must be in [{minimum}, {T}], got [{int(t.min())}, {int(t.max())}]")
    return t


def lengths_arg(lengths, B, T, minimum, device, what):
    """The device int64 array the *_var entry points take.  A device tensor is
    used as it is, with no host read (a captured call then serves batches of
    other lengths; out-of-range values follow the device contract of DESIGN
    §25); host lengths are checked against [minimum, T] and copied."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.dtype != torch.int64 or lengths.numel() != B:
            raise ValueError(f"{what}: device lengths must be {B} int64 values, got {lengths.numel()} of "
                             f"{lengths.dtype}")
        return lengths.reshape(-1).contiguous()
    return check_host_lengths(lengths, B, T, minimum, what).to(device)


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
