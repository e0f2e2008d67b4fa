"""Streaming step primitive (csrc/stream.hip) and the static plan of a hop.

``conv_step`` is the thin binding of ``sel_conv_step`` (include/sel.h): one
causal layer of one streaming hop on channels-last rows, the reference's
``pad_buffer`` (layers/conv_layer.py:144-147, :185-188) as an explicit carry.

``plan`` walks a ``StreamGenerator`` (models/autoencoder*/AudioDec.py) on the
host -- no GPU, no libsel call -- and returns, for ``encode`` and for
``decode``, the ordered list of steps a hop consists of.  ``sel.streaming``
turns a plan into fixed buffers and launches; tests/test_stream_plan_host.py
executes one on the CPU against the oracle.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib as L
from . import convops as CO


class CopyJob(ctypes.Structure):
    """include/sel.h sel_copy_job"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("bytes", ctypes.c_int64)]


def conv_step(desc, carry, x, wp, bias=None, res=None, out=None, carry_out=None):
    """One sel_conv_step launch on the current stream.

    x: (B*T, C) new rows (any leading shape), carry: (B, P, C) or None when
    K = 1, wp: the packed weight (sel.convops.pack), all in one dtype; res and
    out share the output dtype (out's when given, else x's).  Returns
    (out, carry_out); missing ones are allocated.  carry is not written."""
    L.need_device(x, wp, carry, bias, res, out, carry_out)
    P = (desc.K - 1) * desc.dil
    B = desc.rows // max(desc.T, 1)
    if out is None:
        out = torch.empty((desc.rows, desc.N), dtype=x.dtype, device=x.device)
    if P > 0 and carry_out is None and carry is not None:
        carry_out = torch.empty_like(carry)
    for t, n in ((x, desc.rows * desc.C), (out, desc.rows * desc.N), (res, desc.rows * desc.N),
                 (carry, B * P * desc.C), (carry_out, B * P * desc.C), (wp, desc.N * desc.K * desc.C)):
        if t is not None and (not t.is_contiguous() or t.numel() != n):
            raise L.SelError(f"sel: conv_step operand of {t.numel()} elements, expected {n} contiguous")
    if wp.dtype != x.dtype or (carry is not None and carry.dtype != x.dtype) or \
            (carry_out is not None and carry_out.dtype != x.dtype) or (res is not None and res.dtype != out.dtype):
        raise L.SelError("sel: conv_step operands must share the input dtype (res: the output dtype)")
    L.call("sel_conv_step", ctypes.byref(desc), CO._code(x.dtype), CO._code(out.dtype), L.ptr(carry), L.ptr(x),
           L.ptr(wp), L.ptr(bias), L.ptr(res), L.ptr(out), L.ptr(carry_out), L.stream())
    return out, carry_out


def commit(pairs):
    """carry <- carry_out for every (carry_out, carry) pair, one launch per 48."""
    jobs = (CopyJob * len(pairs))(*[CopyJob(s.data_ptr(), d.data_ptr(), s.numel() * s.element_size())
                                    for s, d in pairs])
    L.call("sel_stream_commit", ctypes.cast(jobs, ctypes.c_void_p), len(pairs), L.stream())


@dataclass(frozen=True)
class Step:
    """One sel_conv_step launch of a hop."""
    name: str                 # module path of the layer (generator.get_submodule(name))
    kind: int                 # sel.convops.PACK_*
    stride: int
    weight: str               # parameter names (state_dict keys)
    bias: Optional[str]
    T: int                    # descriptor fields; rows = batch * T
    C: int
    N: int
    K: int
    dil: int
    in_elu: int
    bias_period: int
    src: int                  # index of the step whose output is the input; -1: the method's input
    res: Optional[int]        # index of the step whose output is added, -1: the method's input
    carry_shape: Optional[Tuple[int, int, int]]   # (batch, P, C) or None (K = 1)
    buffer: Optional[str]     # state_dict key of the pad_buffer the carry stands for
    buffer_shape: Optional[Tuple[int, int, int]]  # its shape in the reference: (1, Cin, P_ref)
    out_float: bool           # fp32 output whatever the compute dtype

    @property
    def pad(self):
        return (self.K - 1) * self.dil

    def desc(self, batch):
        return CO.ConvDesc(batch * self.T, self.T, self.C, self.N, self.K, self.dil, self.pad, CO.PAD_ZERO,
                           self.in_elu, self.bias_period)


@dataclass(frozen=True)
class Plan:
    batch: int
    chunk: int                # samples per hop
    frames: int               # code frames per hop (chunk / prod(enc_strides))
    pqc: bool                 # projector / quantizer / decoder.conv1 in the path
    in_channels: int
    enc_channels: int         # channels of encode()'s output
    dec_in_channels: int      # channels of decode()'s input
    out_channels: int
    out_samples: int          # samples decode() returns per hop
    encode: Tuple[Step, ...]
    decode: Tuple[Step, ...]


def _reject(msg):
    raise NotImplementedError(f"sel.streamops.plan: {msg}")


class _Builder:
    def __init__(self, batch):
        self.batch = batch
        self.steps = []

    def conv(self, name, m, T, src, in_elu=0, res=None, out_float=False):
        """CausalConv1d (stride 1 or the k = 2s down-sampling conv) on T input samples."""
        from layers.conv_layer import CausalConv1d
        if not isinstance(m, CausalConv1d):
            _reject(f"{name} is a {type(m).__name__}: a session streams causal layers only (mode='causal')")
        c = m.conv
        s, k, cin, cout = m.stride, m.kernel_size, c.in_channels, c.out_channels
        if c.groups != 1:
            _reject(f"{name} is grouped (groups={c.groups}); grouped layers stay on the module path (*.inference)")
        bias = f"{name}.conv.bias" if c.bias is not None else None
        if s == 1:
            P = (k - 1) * m.dilation
            st = Step(name, CO.PACK_FWD, 1, f"{name}.conv.weight", bias, T, cin, cout, k, m.dilation, in_elu,
                      cout if bias else 0, src, res, (self.batch, P, cin) if P else None,
                      f"{name}.pad_buffer" if P else None, (1, cin, P) if P else None, out_float)
            To = T
        else:
            if k != 2 * s:
                _reject(f"{name} has kernel_size {k} != 2 * stride ({s}); such layers stay on the module path")
            if T % s:
                _reject(f"{name}: {T} input samples per hop are not a multiple of its stride {s}")
            To = T // s
            st = Step(name, CO.PACK_FWD_STRIDED, s, f"{name}.conv.weight", bias, To, s * cin, cout, 3, 1, in_elu,
                      cout if bias else 0, src, res, (self.batch, 2, s * cin), f"{name}.pad_buffer",
                      (1, cin, 2 * s - 1), out_float)
        self.steps.append(st)
        return len(self.steps) - 1, To

    def convt(self, name, m, T, src):
        from layers.conv_layer import CausalConvTranspose1d
        if not isinstance(m, CausalConvTranspose1d):
            _reject(f"{name} is a {type(m).__name__}: a session streams causal layers only (mode='causal')")
        d = m.deconv
        s, k = m.stride, m.kernel_size
        if k != 2 * s or d.groups != 1:
            _reject(f"{name} has kernel_size {k} != 2 * stride ({s}) or groups; such layers stay on the module path")
        bias = f"{name}.deconv.bias" if d.bias is not None else None
        cin, cout = d.in_channels, d.out_channels
        self.steps.append(Step(name, CO.PACK_CONVT, s, f"{name}.deconv.weight", bias, T, cin, s * cout, 2, 1, 0,
                               cout if bias else 0, src, None, (self.batch, 1, cin), f"{name}.pad_buffer",
                               (1, cin, 1), False))
        return len(self.steps) - 1, T * s

    def res_unit(self, name, ru, T, src):
        """residual_unit.py:78-81: x + conv2(ELU(conv1.inference(ELU(x)))); conv1's
        carry holds ELU(x), conv2 is the 1x1 with + x in its epilogue."""
        from layers.conv_layer import Conv1d1x1
        h, _ = self.conv(f"{name}.conv1", ru.conv1, T, src, in_elu=1)
        c2 = ru.conv2
        if not isinstance(c2, Conv1d1x1) or c2.out_channels != ru.conv1.conv.in_channels:
            _reject(f"{name}.conv2 is not the unit's 1x1 conv")
        bias = f"{name}.conv2.bias" if c2.bias is not None else None
        self.steps.append(Step(f"{name}.conv2", CO.PACK_FWD, 1, f"{name}.conv2.weight", bias, T, c2.in_channels,
                               c2.out_channels, 1, 1, 1, c2.out_channels if bias else 0, h, src, None, None, None,
                               False))
        return len(self.steps) - 1


def plan(generator, batch, chunk):
    """The steps of one hop of `chunk` samples at `batch` streams, for a
    StreamGenerator with or without PQC.  Pure Python: reads module attributes
    only.  Raises NotImplementedError for what a session cannot run."""
    if batch < 1 or chunk < 1:
        raise ValueError("sel.streamops.plan: batch and chunk must be positive")
    if getattr(generator, "mode", None) != "causal":
        _reject(f"mode {getattr(generator, 'mode', None)!r}: streaming needs the causal generator")
    enc, dec = generator.encoder, generator.decoder
    pqc = not getattr(dec, "skip_conv1", False)
    hop = 1
    for blk in enc.conv_blocks:
        hop *= getattr(blk.conv, "stride", 1)
    if chunk % hop:
        _reject(f"chunk ({chunk}) is not a multiple of the encoder's total stride ({hop})")

    e = _Builder(batch)
    cur, T = e.conv("encoder.conv", enc.conv, chunk, -1)
    for i, blk in enumerate(enc.conv_blocks):
        for j, ru in enumerate(blk.res_units):
            cur = e.res_unit(f"encoder.conv_blocks.{i}.res_units.{j}", ru, T, cur)
        cur, T = e.conv(f"encoder.conv_blocks.{i}.conv", blk.conv, T, cur)
    if pqc:
        proj = generator.projector.project
        if isinstance(proj, torch.nn.Sequential):
            _reject("the 'conv1d_bn' projector has no streaming step")
        cur, T = e.conv("projector.project", proj, T, cur, out_float=True)
    frames = T

    d = _Builder(batch)
    cur, T = -1, frames
    if pqc:
        cur, T = d.conv("decoder.conv1", dec.conv1, T, cur)
    for i, blk in enumerate(dec.conv_blocks):
        cur, T = d.convt(f"decoder.conv_blocks.{i}.conv", blk.conv, T, cur)
        for j, ru in enumerate(blk.res_units):
            cur = d.res_unit(f"decoder.conv_blocks.{i}.res_units.{j}", ru, T, cur)
    cur, T = d.conv("decoder.conv2", dec.conv2, T, cur, out_float=True)

    return Plan(batch, chunk, frames, pqc, generator.input_channels, e.steps[-1].N, d.steps[0].C,
                d.steps[-1].N, T, tuple(e.steps), tuple(d.steps))
