"""Shapes, tune settings and readers for the conv stack's host-side decisions
(tests/test_conv_dispatch_host.py; golden made by
tests/golden/make_goldens_conv_dispatch.py from the library SEL_LIB names).

Nothing here needs a GPU: sel_conv_fwd_kernel_id and sel_dconv_kernel are the
launchers' own decisions, read back as numbers.
"""
import ctypes
import itertools

import numpy as np
import torch

from oracle import ref_ops as R
from sel import configs
from sel import convops as CO
from sel import dconvops as DC

# (per-GPU batch, samples per clip): the bench workloads (c2 32 x 1 s and c3
# 64 x 1 s at 24 kHz, c5 16 x 1 s at 48 kHz), the shipped configs' own
# batch_size x batch_length, and one clip of each length
BATCHES = sorted({(32, 24000), (64, 24000), (16, 48000)} |
                 {(c["batch_size"], c["batch_length"]) for c in configs.CONFIGS.values()} |
                 {(1, c["batch_length"]) for c in configs.CONFIGS.values()})


def generator_descs(B, L, g=configs.GENERATOR):
    """Every conv launch shape of the AudioDec generator (encoder, projector,
    decoder; models/autoencoder/modules) on B clips of L samples, as ConvDesc
    field tuples: each layer's forward and its adjoint (the dgrad launch)."""
    out = []

    def layer(kind, T, cin, cout, k, stride=1, dil=1):
        d, To, _ = CO._layer_desc(kind, B, T, cin, cout, k, stride, dil, True)
        out.extend([d, d.adjoint()])
        return To

    def res_units(T, c):
        for dil in (1, 3, 9):
            layer(CO.PACK_FWD, T, c, c, 7, dil=dil)
            out.append(CO.ConvDesc(B * T, T, c, c, 1, 1, 0, CO.PAD_ZERO, 0, c))
            out.append(out[-1].adjoint())

    T, c = L, g["encode_channels"]
    layer(CO.PACK_FWD, T, g["input_channels"], c, 7)
    for ratio, s in zip(g["enc_ratios"], g["enc_strides"]):
        res_units(T, c)
        if T % s:
            return None  # (this clip length does not fold: the model rejects it too)
        T = layer(CO.PACK_FWD_STRIDED, T, c, g["encode_channels"] * ratio, 2 * s, stride=s)
        c = g["encode_channels"] * ratio
    layer(CO.PACK_FWD, T, c, g["code_dim"], 3)
    c = g["decode_channels"] * g["dec_ratios"][0]
    layer(CO.PACK_FWD, T, g["code_dim"], c, 7)
    for i, s in enumerate(g["dec_strides"]):
        cout = g["decode_channels"] * (g["dec_ratios"][i + 1] if i + 1 < len(g["dec_ratios"]) else 1)
        T = layer(CO.PACK_CONVT, T, c, cout, 2 * s, stride=s)
        c = cout
        res_units(T, c)
    layer(CO.PACK_FWD, T, c, g["output_channels"], 7)
    return [tuple(getattr(d, f) for f, _ in CO.ConvDesc._fields_) for d in out]


def edge_descs():
    """Shapes at the dispatch thresholds: widths, taps, row counts just below
    and at the row thresholds, the three clip lengths, the pad forms."""
    out = []
    for N, K, T, thr in itertools.product((32, 64, 96, 128, 256, 512), (1, 2, 3, 7), (80, 400, 2000),
                                          (8192, 16384, 65536)):
        for B in ((thr - 1) // T, -(-thr // T)):
            for pad, mode in ((0, CO.PAD_ZERO), (K - 1, CO.PAD_ZERO), (K - 1, CO.PAD_REPLICATE)):
                out.append((B * T, T, N, N, K, 1, pad, mode, 0, N))
    return out


def conv_cases():
    """Sorted, duplicate-free (rows, T, C, N, K, dil, pad, pad_mode, in_elu,
    bias_period) tuples, each with in_elu 0 and 1."""
    descs = set(edge_descs())
    for B, L in BATCHES:
        descs.update(generator_descs(B, L) or [])
    both = {d[:8] + (e,) + d[9:] for d in descs for e in (0, 1)}
    return sorted(both)


def tune_settings():
    """(key, value) pairs applied one at a time; (0, 0) is the default."""
    bits = [1 << i for i in range(9)]  # per thin-kernel instance
    doc = {0: range(21, 31), 4: [1], 6: bits, 7: bits, 11: [1, 2, 3], 12: bits, 37: [1, 2], 38: [1], 42: [1],
           46: [1], 47: [1, 2], 50: [1, 2], 52: [1, 2], 67: [1, 3]}
    return [(0, 0)] + [(k, v) for k, vs in doc.items() for v in vs]


def forward_ids(lib, cases=None):
    """{"k<key>_v<value>": int32 array over cases x (bf16, fp32 output) x
    (no epilogue, epilogue)} of sel_conv_fwd_kernel_id."""
    cases = conv_cases() if cases is None else cases
    descs = [CO.ConvDesc(*c) for c in cases]
    out = {}
    for key, val in tune_settings():
        prev = lib.sel_tune(key, val)
        try:
            out[f"k{key}_v{val}"] = np.array(
                [lib.sel_conv_fwd_kernel_id(ctypes.byref(d), CO.BF16, od, epi)
                 for d in descs for od in (CO.BF16, CO.F32) for epi in (0, 1)], dtype=np.int32)
        finally:
            lib.sel_tune(key, prev)
    return out


def mpd_descs():
    """The MPD chain's forward and adjoint layer descriptors at C5 sizes
    (test_host_logic's shapes: 16 and 32 clips, every period)."""
    specs = [DC.LayerSpec(ci, co, k, s, p, 1, lk) for (ci, co, k, s, p, lk) in R.period_discriminator_plan()]
    out = []
    for clips in (16, 32):
        for p in (2, 3, 5, 7, 11):
            Lv, Bs = (48000 + p - 1) // p, clips * p
            geo = DC.chain_layout(specs, Lv, DC.period_alloc(Lv, specs))
            for li, (sp, (Ti, Ta, To, Toa)) in enumerate(zip(specs, geo)):
                out.append(DC._fwd_desc(sp, Bs, Ti, Ta, To, Toa, 0.1))
                out.append(DC._dgrad_desc(sp, Bs, Ta, To, Toa, 0.1, li > 0, T_in=Ti))
    return out


def dconv_kernels(lib):
    """"<path> <kernel name>" of sel_dconv_kernel per MPD descriptor, at the
    default and with tune keys 22 and 37 set."""
    out = []
    for key, val in ((0, 0), (22, 1), (37, 1)):
        prev = lib.sel_tune(key, val)
        try:
            for d in mpd_descs():
                buf = ctypes.create_string_buffer(96)
                path = lib.sel_dconv_kernel(ctypes.byref(d), DC._code(torch.bfloat16), buf, 96)
                out.append(f"{path} {buf.value.decode()}")
        finally:
            lib.sel_tune(key, prev)
    return out


def slot_values(lib, cases=None):
    """sel_resunit_wgrad_splits and sel_conv_wgrad_workspace per case: they
    depend on the device's occupancy query (or its fallback without a device),
    so two libraries are compared on the same machine instead of with a golden."""
    cases = conv_cases() if cases is None else cases
    splits, ws = [], []
    for c in cases:
        d = CO.ConvDesc(*c)
        splits.append(int(lib.sel_resunit_wgrad_splits(ctypes.byref(d), CO.BF16)))
        ws.append(int(lib.sel_conv_wgrad_workspace(ctypes.byref(d))))
    return {"resunit_wgrad_splits": splits, "conv_wgrad_workspace": ws}
