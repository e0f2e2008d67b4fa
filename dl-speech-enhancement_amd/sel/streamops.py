"""Streaming step primitive (csrc/stream.hip) and the static plan of a hop.

``conv_step`` is the thin binding of ``sel_conv_step`` (include/sel.h): one
causal layer of one streaming hop on channels-last rows, the reference's
``pad_buffer`` (layers/conv_layer.py:144-147, :185-188) as an explicit carry.

``plan`` walks a ``StreamGenerator`` (models/autoencoder*/AudioDec.py) on the
host -- no GPU, no libsel call -- and returns, for ``encode`` and for
``decode``, the ordered list of steps a hop consists of.  ``sel.streaming``
turns a plan into fixed buffers and launches; tests/test_stream_plan_host.py
executes one on the CPU against the oracle.

``hfg_conv_step`` binds ``sel_hfg_conv_step`` (csrc/hfg_step.hip), the grouped
LeakyReLU form of the same step, and ``plan_vocoder`` walks a HiFi-GAN vocoder
``StreamGenerator`` (models/vocoder/HiFiGAN.py) the same way;
tests/test_vocoder_plan_host.py executes its plans against the reference goldens.

``conv_step_pool`` / ``hfg_conv_step_pool`` / ``copy_slots`` bind the
slot-indexed forms for stream pools (``sel.streaming.StreamPool``), and
``SlotTable`` is the host-side record of which slots are open.

``rvq_step`` / ``rvq_lookup_step`` bind the quantizer and the codebook lookup of a
hop as stateless step launches (csrc/vq_step.hip), which
``sel.streaming``'s ``enable_codes`` puts inside the hop's launch list;
``rvq_step_wire`` / ``rvq_lookup_wire_step`` are the same launches writing and
reading the packed records of the wire format (``sel.wire``), and
``rvq_step_dgram`` / ``rvq_lookup_dgram_step`` the ones writing and reading
datagrams (wire version 2): a per-stream stage budget and header on the way
out, the header's stage count and a held record for lost hops on the way in.
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


# ---- stream pools: the slot-indexed forms (include/sel.h sel_conv_step_pool) ------------------
class SlotTable:
    """Which slots of a pool of ``capacity`` are open.  Pure Python, no device:
    the kernels trust the list they are given (distinct, in range), so every
    list passes ``check`` before it is staged."""

    def __init__(self, capacity):
        if capacity < 1:
            raise ValueError("sel.streamops.SlotTable: capacity must be positive")
        self.capacity = int(capacity)
        self._open = set()

    def open(self):
        """The lowest free slot."""
        for s in range(self.capacity):
            if s not in self._open:
                self._open.add(s)
                return s
        raise L.SelError(f"sel: the pool is full ({self.capacity} streams open)")

    def close(self, slot):
        self.check([slot])
        self._open.discard(int(slot))

    def is_open(self, slot):
        return slot in self._open

    def __len__(self):
        return len(self._open)

    def check(self, slots):
        """The list as ints; SelError for a list longer than capacity, a
        duplicate, an id out of range or a closed slot."""
        raw = list(slots)      # once: a one-shot iterator must not slip past the checks below
        out = [int(s) for s in raw]
        if len(out) > self.capacity:
            raise L.SelError(f"sel: {len(out)} slots listed, the pool holds {self.capacity}")
        if len(set(out)) != len(out):
            raise L.SelError(f"sel: duplicate slot in {out}")
        for s, r in zip(out, raw):
            if s != r or not 0 <= s < self.capacity:
                raise L.SelError(f"sel: slot {r!r} is out of range [0, {self.capacity})")
            if s not in self._open:
                raise L.SelError(f"sel: slot {s} is not open")
        return out


def _pool_operands(what, desc, cin, nres, P, carry, carry_out, slots, n_active, x, wp, res, out, nslots):
    B = desc.rows // max(desc.T, 1)
    for t in (slots, n_active):
        if t is None or t.dtype != torch.int32 or not t.is_contiguous():
            raise L.SelError(f"sel: {what} takes contiguous int32 device tensors for slots and n_active")
    if slots.numel() < B or n_active.numel() < 1:
        raise L.SelError(f"sel: {what} needs {B} slot entries (capacity) and one n_active, got "
                         f"{slots.numel()} and {n_active.numel()}")
    if P == 0:
        if nslots is None or nslots < 1:
            raise L.SelError(f"sel: {what} with K = 1 has no carry pool to size the slot range: pass nslots")
    else:
        if carry is None or carry_out is None or carry.shape != carry_out.shape or carry.dim() != 3:
            raise L.SelError(f"sel: {what} with K > 1 needs carry and carry_out pools of one shape (nslots, P, C)")
        if nslots not in (None, carry.shape[0]):
            raise L.SelError(f"sel: {what} nslots {nslots} is not the carry pool's {carry.shape[0]}")
        nslots = carry.shape[0]
        if tuple(carry.shape[1:]) != (P, desc.C):
            raise L.SelError(f"sel: {what} carry pool of shape {tuple(carry.shape)}, expected (nslots, {P}, {desc.C})")
    for t, n in ((x, desc.rows * cin), (out, desc.rows * desc.N), (res, desc.rows * nres)):
        if t is not None and (not t.is_contiguous() or t.numel() != n):
            raise L.SelError(f"sel: {what} operand of {t.numel()} elements, expected {n} contiguous")
    for t in (carry, carry_out):
        if t is not None and not t.is_contiguous():
            raise L.SelError(f"sel: {what} takes contiguous carry pools")
    if wp.dtype != x.dtype or (carry is not None and carry.dtype != x.dtype) or \
            (carry_out is not None and carry_out.dtype != x.dtype) or (res is not None and res.dtype != out.dtype):
        raise L.SelError(f"sel: {what} operands must share the input dtype (res: the output dtype)")
    return nslots


def conv_step_pool(desc, carry, carry_out, slots, n_active, x, wp, bias=None, res=None, out=None, nslots=None):
    """One sel_conv_step_pool launch on the current stream.

    desc.rows = capacity * T.  carry / carry_out: (nslots, P, C) pools (None when
    K = 1); slots (>= capacity int32) and n_active (1 int32): DEVICE tensors the
    kernel reads, so a captured launch follows what is staged into them; x, res,
    out: the capacity-sized dense buffers, of which the first n_active samples
    are read / written.  The list must hold distinct ids (SlotTable.check).
    nslots: the valid slot range when there is no carry pool to take it from (K = 1).
    Returns out (allocated when missing)."""
    L.need_device(x, wp, carry, carry_out, slots, n_active, bias, res, out)
    P = (desc.K - 1) * desc.dil
    if out is None:
        out = torch.empty((desc.rows, desc.N), dtype=x.dtype, device=x.device)
    nslots = _pool_operands("conv_step_pool", desc, desc.C, desc.N, P, carry, carry_out, slots, n_active, x, wp, res,
                            out, nslots)
    if wp.numel() != desc.N * desc.K * desc.C:
        raise L.SelError(f"sel: conv_step_pool weight of {wp.numel()} elements, expected {desc.N * desc.K * desc.C}")
    L.call("sel_conv_step_pool", ctypes.byref(desc), CO._code(x.dtype), CO._code(out.dtype), L.ptr(carry),
           L.ptr(carry_out), nslots, L.ptr(slots), L.ptr(n_active), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(res),
           L.ptr(out), L.stream())
    return out


def hfg_conv_step_pool(desc, carry, carry_out, slots, n_active, x, wp, bias=None, res=None, out=None,
                       nslots=None):
    """One sel_hfg_conv_step_pool launch on the current stream: hfg_conv_step's
    operands with conv_step_pool's slot table (carry pools (nslots, P, C))."""
    L.need_device(x, wp, carry, carry_out, slots, n_active, bias, res, out)
    G = max(desc.groups, 1)
    P = (desc.K - 1) * desc.dil
    if out is None:
        if desc.accumulate:
            raise L.SelError("sel: hfg_conv_step_pool with accumulate needs the out buffer it adds into")
        out = torch.empty((desc.rows, desc.N), dtype=x.dtype, device=x.device)
    cin = desc.C if desc.in_group_stride else desc.C // G
    nres = desc.N if desc.res_group_stride else desc.N // G
    nslots = _pool_operands("hfg_conv_step_pool", desc, cin, nres, P, carry, carry_out, slots, n_active, x, wp, res,
                            out, nslots)
    if wp.numel() != desc.N * desc.K * (desc.C // G):
        raise L.SelError(f"sel: hfg_conv_step_pool weight of {wp.numel()} elements, expected "
                         f"{desc.N * desc.K * (desc.C // G)}")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise L.SelError("sel: hfg_conv_step_pool takes a contiguous fp32 bias")
    L.call("sel_hfg_conv_step_pool", ctypes.byref(desc), CO._code(x.dtype), CO._code(out.dtype), L.ptr(carry),
           L.ptr(carry_out), nslots, L.ptr(slots), L.ptr(n_active), L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(res),
           L.ptr(out), L.stream())
    return out


def copy_slots(pairs, src_slots, dst_slots, n):
    """Slot row src_slots[i] of src -> slot row dst_slots[i] of dst for every
    (src, dst) pair of pools (nslots, ...) and i < n[0], one launch per 48 pairs.
    src_slots / dst_slots / n are int32 DEVICE tensors read by the kernel.  All
    pools share nslots; src may be dst (opening a stream from the template row)."""
    L.need_device(src_slots, dst_slots, n, *[t for p in pairs for t in p])
    for t in (src_slots, dst_slots, n):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise L.SelError("sel: copy_slots takes contiguous int32 device tensors for the slot lists and n")
    nslots = pairs[0][0].shape[0]
    for s, d in pairs:
        if s.shape != d.shape or s.dtype != d.dtype or s.shape[0] != nslots or not s.is_contiguous() \
                or not d.is_contiguous():
            raise L.SelError("sel: copy_slots pairs must be contiguous pools of one shape, dtype and slot count")
    cap = min(src_slots.numel(), dst_slots.numel())
    if cap < 1 or n.numel() < 1:
        raise L.SelError("sel: copy_slots needs non-empty slot lists and a count")
    jobs = (CopyJob * len(pairs))(*[CopyJob(s.data_ptr(), d.data_ptr(), s[0].numel() * s.element_size())
                                    for s, d in pairs])
    L.call("sel_stream_copy_slots", ctypes.cast(jobs, ctypes.c_void_p), len(pairs), nslots, L.ptr(src_slots),
           L.ptr(dst_slots), cap, L.ptr(n), L.stream())


# ---- the residual VQ of a hop as step launches (include/sel.h sel_rvq_step) --------------------
def _count_operand(what, n_active):
    if n_active is not None and (n_active.dtype != torch.int32 or not n_active.is_contiguous()
                                 or n_active.numel() < 1):
        raise L.SelError(f"sel: {what} takes a contiguous int32 device tensor for n_active")


def _rows_per_sample(what, rows, rows_per_sample):
    if rows_per_sample < 1 or rows % rows_per_sample:
        raise L.SelError(f"sel: {what} rows ({rows}) is not a multiple of rows_per_sample ({rows_per_sample})")


def _quantizer_operands(what, z, embeds, idx, zq, rows_per_sample, need_idx=False):
    """The operands the three quantizer launches share -> (S, D, K, rows)."""
    if embeds.dim() != 3 or embeds.dtype != torch.float32 or not embeds.is_contiguous():
        raise L.SelError(f"sel: {what} takes a contiguous fp32 (S, D, K) stack, got {embeds.dtype} "
                         f"{tuple(embeds.shape)}")
    S, D, K = embeds.shape
    if z.dim() != 2 or z.shape[1] != D or z.dtype != torch.float32 or not z.is_contiguous():
        raise L.SelError(f"sel: {what} takes contiguous fp32 rows (rows, {D}), got {z.dtype} {tuple(z.shape)}")
    rows = z.shape[0]
    if (need_idx or idx is not None) and (idx.dtype != torch.int64 or not idx.is_contiguous()
                                          or tuple(idx.shape) != (S, rows)):
        raise L.SelError(f"sel: {what} writes a contiguous int64 idx of shape {(S, rows)}, got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    if zq is not None and (zq.dtype != torch.float32 or not zq.is_contiguous() or zq.shape != z.shape):
        raise L.SelError(f"sel: {what} writes a contiguous fp32 zq of shape {tuple(z.shape)}")
    _rows_per_sample(what, rows, rows_per_sample)
    return S, D, K, rows


def _lookup_codebook(what, codebook, codebooks=None):
    """The flat codebook of the three lookup launches -> (ncodes, D), and with the
    stage count ``codebooks`` of the packed forms -> (S, K, D)."""
    if codebook.dim() != 2 or codebook.dtype != torch.float32 or not codebook.is_contiguous():
        raise L.SelError(f"sel: {what} takes a contiguous fp32 (ncodes, D) codebook, got {codebook.dtype} "
                         f"{tuple(codebook.shape)}")
    ncodes, D = codebook.shape
    if codebooks is None:
        return ncodes, D
    S = int(codebooks)
    if S < 1 or ncodes % S or ncodes < S:
        raise L.SelError(f"sel: {what}: a codebook of {ncodes} rows is not {S} stages of one size")
    return S, ncodes // S, D


def _lookup_outputs(what, out, rows, D, mean, scale, idx_out=None, S=None):
    """out, the optional idx_out and mean / scale of the three lookup launches."""
    if out.dtype not in (torch.float32, torch.bfloat16) or not out.is_contiguous() or out.numel() != rows * D:
        raise L.SelError(f"sel: {what} writes {rows} contiguous fp32 / bf16 rows of {D}, got {out.dtype} "
                         f"{tuple(out.shape)}")
    if idx_out is not None and (idx_out.dtype != torch.int64 or not idx_out.is_contiguous()
                                or tuple(idx_out.shape) != (S, rows)):
        raise L.SelError(f"sel: {what} writes a contiguous int64 idx_out of shape {(S, rows)}")
    if (mean is None) != (scale is None):
        raise L.SelError(f"sel: {what} takes mean and scale together or not at all")
    for t in (mean, scale):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != D):
            raise L.SelError(f"sel: {what} takes contiguous fp32 mean / scale of {D} elements")


def rvq_step(z, embeds, idx, rows_per_sample=1, n_active=None, flatten=True, zq=None):
    """One sel_rvq_step launch on the current stream: z (rows, D) fp32 rows ->
    idx (S, rows) int64 picks (flatten: + s*K, ids into the flat codebook) and,
    when given, zq (rows, D) fp32.  embeds: the (S, D, K) fp32 codebook stack.
    n_active (1 int32, DEVICE) makes the first n_active * rows_per_sample rows
    the only ones read and written.  Nothing is allocated.  Returns idx."""
    L.need_device(z, embeds, idx, n_active, zq)
    S, D, K, rows = _quantizer_operands("rvq_step", z, embeds, idx, zq, rows_per_sample, need_idx=True)
    _count_operand("rvq_step", n_active)
    L.call("sel_rvq_step", L.ptr(z), rows, rows_per_sample, D, L.ptr(embeds), S, K, L.ptr(n_active),
           int(bool(flatten)), L.ptr(idx), L.ptr(zq), L.stream())
    return idx


def rvq_lookup_step(idx, codebook, out, rows_per_sample=1, mean=None, scale=None, n_active=None):
    """One sel_rvq_lookup_step launch on the current stream: idx (S, rows) int64
    ids into codebook (ncodes, D) fp32 (ResidualVQ.initial()'s flat layout) ->
    out (rows, D) fp32 or bf16: the codes summed in fp32 in ascending stage order,
    then (acc - mean) / scale when both are given (D fp32 each), then rounded to
    out's dtype.  n_active as in rvq_step.  Nothing is allocated.  Returns out."""
    L.need_device(idx, codebook, out, mean, scale, n_active)
    ncodes, D = _lookup_codebook("rvq_lookup_step", codebook)
    if idx.dim() != 2 or idx.dtype != torch.int64 or not idx.is_contiguous():
        raise L.SelError(f"sel: rvq_lookup_step takes a contiguous int64 idx (S, rows), got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    S, rows = idx.shape
    _lookup_outputs("rvq_lookup_step", out, rows, D, mean, scale)
    _rows_per_sample("rvq_lookup_step", rows, rows_per_sample)
    _count_operand("rvq_lookup_step", n_active)
    L.call("sel_rvq_lookup_step", L.ptr(idx), rows, rows_per_sample, S, ncodes, D, L.ptr(codebook), L.ptr(mean),
           L.ptr(scale), L.ptr(n_active), CO._code(out.dtype), L.ptr(out), L.stream())
    return out


# ---- the same with the wire format's records (include/sel.h, sel/wire.py) ----------------------
def _wire_operand(what, wire, rows, S, K):
    from .wire import WireFormat
    fb = WireFormat(S, K).frame_bytes
    if wire is None or wire.dtype != torch.uint8 or wire.dim() != 2 or tuple(wire.shape) != (rows, fb) \
            or wire.stride() != (fb, 1):
        raise L.SelError(f"sel: {what} takes a dense uint8 wire buffer of shape {(rows, fb)}, got "
                         f"{None if wire is None else (wire.dtype, tuple(wire.shape), wire.stride())}")


def rvq_step_wire(z, embeds, wire, rows_per_sample=1, n_active=None, flatten=True, idx=None, zq=None):
    """One sel_rvq_step_wire launch on the current stream: rvq_step (same picks,
    idx and zq, both optional here) that also writes every active row's packed
    record into wire (rows, frame_bytes) uint8 -- dense rows, any byte alignment.
    Nothing is allocated.  Returns wire."""
    L.need_device(z, embeds, wire, idx, n_active, zq)
    S, D, K, rows = _quantizer_operands("rvq_step_wire", z, embeds, idx, zq, rows_per_sample)
    _wire_operand("rvq_step_wire", wire, rows, S, K)
    _count_operand("rvq_step_wire", n_active)
    L.call("sel_rvq_step_wire", L.ptr(z), rows, rows_per_sample, D, L.ptr(embeds), S, K, L.ptr(n_active),
           int(bool(flatten)), L.ptr(idx), L.ptr(zq), L.ptr(wire), L.stream())
    return wire


def rvq_lookup_wire_step(wire, codebook, codebooks, out, rows_per_sample=1, mean=None, scale=None, n_active=None,
                         idx_out=None):
    """One sel_rvq_lookup_wire_step launch on the current stream: rvq_lookup_step
    on the ids taken out of wire (rows, frame_bytes) uint8 -- dense rows, any byte
    alignment -- for a codebook (codebooks * K, D) fp32.  A field >= K contributes
    zero.  idx_out (codebooks, rows) int64, when given, receives the flattened
    ids (-1 for such a field).  Nothing is allocated.  Returns out."""
    L.need_device(wire, codebook, out, mean, scale, n_active, idx_out)
    S, K, D = _lookup_codebook("rvq_lookup_wire_step", codebook, codebooks)
    if wire is None or wire.dim() != 2:
        raise L.SelError("sel: rvq_lookup_wire_step takes a (rows, frame_bytes) uint8 wire buffer")
    rows = wire.shape[0]
    _wire_operand("rvq_lookup_wire_step", wire, rows, S, K)
    _lookup_outputs("rvq_lookup_wire_step", out, rows, D, mean, scale, idx_out, S)
    _rows_per_sample("rvq_lookup_wire_step", rows, rows_per_sample)
    _count_operand("rvq_lookup_wire_step", n_active)
    L.call("sel_rvq_lookup_wire_step", L.ptr(wire), rows, rows_per_sample, S, K, D, L.ptr(codebook), L.ptr(mean),
           L.ptr(scale), L.ptr(n_active), CO._code(out.dtype), L.ptr(out), L.ptr(idx_out), L.stream())
    return out


# ---- the same with datagrams: stage budgets, headers, held records (include/sel.h, wire version 2) ----
def _dgram_operand(what, dgram, B, S, K, T):
    """(B, >= 4 + T * fb(S)) uint8 on the device, rows of one stride, bytes adjacent; any start address"""
    from .wire import DatagramFormat
    try:
        need = DatagramFormat(S, K, T).stride
    except ValueError as e:
        raise L.SelError(f"sel: {what}: {e}") from None
    if dgram is None or dgram.dtype != torch.uint8 or dgram.dim() != 2 or dgram.shape[0] != B \
            or dgram.shape[1] < need or dgram.stride(1) != 1 or dgram.stride(0) < dgram.shape[1]:
        raise L.SelError(f"sel: {what} takes a uint8 datagram buffer of shape ({B}, >= {need}), got "
                         f"{None if dgram is None else (dgram.dtype, tuple(dgram.shape), dgram.stride())}")
    return dgram.stride(0)


def _control_operand(what, name, t, B):
    if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < B):
        raise L.SelError(f"sel: {what} takes a contiguous int32 device tensor of {B} entries for {name}")


def rvq_step_dgram(z, embeds, dgram, rows_per_sample=1, n_active=None, stages=None, seq=None, flatten=True, idx=None,
                   zq=None):
    """One sel_rvq_step_dgram launch on the current stream: rvq_step_wire whose
    chain stops, per sample, after ``clamp(stages[i], 1, S)`` stages, writing a
    datagram per sample -- the header {2, s_i, seq[i] as uint16} and the sample's
    rows_per_sample records of s_i fields -- into the front of row i of dgram
    (B, >= 4 + rows_per_sample * fb(S)) uint8.  stages / seq (B int32 each,
    DEVICE; None: S / 0) are read by the kernel, so a captured launch follows what
    is staged into them.  idx (optional) gets -1 in the stages not run, zq is the
    truncated sum.  Nothing is allocated.  Returns dgram."""
    L.need_device(z, embeds, dgram, idx, n_active, stages, seq, zq)
    S, D, K, rows = _quantizer_operands("rvq_step_dgram", z, embeds, idx, zq, rows_per_sample)
    B = rows // rows_per_sample
    stride = _dgram_operand("rvq_step_dgram", dgram, B, S, K, rows_per_sample)
    _count_operand("rvq_step_dgram", n_active)
    _control_operand("rvq_step_dgram", "stages", stages, B)
    _control_operand("rvq_step_dgram", "seq", seq, B)
    L.call("sel_rvq_step_dgram", L.ptr(z), rows, rows_per_sample, D, L.ptr(embeds), S, K, L.ptr(n_active),
           L.ptr(stages), L.ptr(seq), int(bool(flatten)), L.ptr(idx), L.ptr(zq), L.ptr(dgram), stride, L.stream())
    return dgram


def rvq_lookup_dgram_step(dgram, codebook, codebooks, out, rows_per_sample=1, mean=None, scale=None, n_active=None,
                          slots=None, lost=None, hold=None, idx_out=None):
    """One sel_rvq_lookup_dgram_step launch on the current stream: the lookup on
    the records of the datagrams in dgram (B, >= 4 + rows_per_sample * fb(S))
    uint8, each with the stage count its header gives, for a codebook (codebooks
    * K, D) fp32 -> out (B * rows_per_sample, D) fp32 / bf16.  A sample whose
    lost[i] is non-zero, or whose header is not {2, 1..S}, decodes in every row
    the record that hold (nslots, >= 1 + fb(S)) uint8 keeps for its slot
    (slots[i], None: i) from the last valid hop -- the empty sum when there is
    none -- and a valid sample stores its last row's record there.  slots / lost:
    B int32 each, DEVICE.  idx_out (codebooks, rows) int64, when given, receives
    the ids summed.  Nothing is allocated.  Returns out."""
    L.need_device(dgram, codebook, out, mean, scale, n_active, slots, lost, hold, idx_out)
    S, K, D = _lookup_codebook("rvq_lookup_dgram_step", codebook, codebooks)
    if dgram is None or dgram.dim() != 2:
        raise L.SelError("sel: rvq_lookup_dgram_step takes a (B, stride) uint8 datagram buffer")
    B = dgram.shape[0]
    rows = B * rows_per_sample
    _rows_per_sample("rvq_lookup_dgram_step", rows, rows_per_sample)       # rows_per_sample < 1
    stride = _dgram_operand("rvq_lookup_dgram_step", dgram, B, S, K, rows_per_sample)
    _lookup_outputs("rvq_lookup_dgram_step", out, rows, D, mean, scale, idx_out, S)
    nslots, hold_stride = 0, 0
    if hold is not None:
        from .wire import DatagramFormat
        need = 1 + DatagramFormat(S, K).frame_bytes()
        if hold.dtype != torch.uint8 or hold.dim() != 2 or hold.shape[0] < 1 or hold.shape[1] < need \
                or hold.stride(1) != 1 or hold.stride(0) < hold.shape[1]:
            raise L.SelError(f"sel: rvq_lookup_dgram_step takes uint8 hold rows of shape (nslots, >= {need}), got "
                             f"{(hold.dtype, tuple(hold.shape), hold.stride())}")
        nslots, hold_stride = hold.shape[0], hold.stride(0)
    _count_operand("rvq_lookup_dgram_step", n_active)
    _control_operand("rvq_lookup_dgram_step", "slots", slots, B)
    _control_operand("rvq_lookup_dgram_step", "lost", lost, B)
    L.call("sel_rvq_lookup_dgram_step", L.ptr(dgram), stride, rows, rows_per_sample, S, K, D, L.ptr(codebook),
           L.ptr(mean), L.ptr(scale), L.ptr(n_active), L.ptr(slots), L.ptr(lost), L.ptr(hold), hold_stride, nslots,
           CO._code(out.dtype), L.ptr(out), L.ptr(idx_out), L.stream())
    return out


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


# ---- the HiFi-GAN vocoder decoder (models/vocoder/HiFiGAN.py StreamGenerator) ----------------
def hfg_conv_step(desc, carry, x, wp, bias=None, res=None, out=None, carry_out=None):
    """One sel_hfg_conv_step launch on the current stream.

    desc: sel.hfgops.HfgDesc.  x: (B*T, C) new rows, or (B*T, C/G) when
    in_group_stride is 0; carry: (B, P, C) or None when K = 1; wp: the packed
    weight (N, K, C/G), all in one dtype.  res ((B*T, N), or (B*T, N/G) when
    res_group_stride is 0) and out share the output dtype (out's when given,
    else x's).  Returns (out, carry_out); missing ones are allocated (not with
    desc.accumulate, which adds into the given out).  carry is not written."""
    L.need_device(x, wp, carry, bias, res, out, carry_out)
    G = max(desc.groups, 1)
    P = (desc.K - 1) * desc.dil
    B = desc.rows // max(desc.T, 1)
    if out is None:
        if desc.accumulate:
            raise L.SelError("sel: hfg_conv_step with accumulate needs the out buffer it adds into")
        out = torch.empty((desc.rows, desc.N), dtype=x.dtype, device=x.device)
    if P > 0 and carry_out is None and carry is not None:
        carry_out = torch.empty_like(carry)
    cin = desc.C if desc.in_group_stride else desc.C // G
    nres = desc.N if desc.res_group_stride else desc.N // G
    for t, n in ((x, desc.rows * cin), (out, desc.rows * desc.N), (res, desc.rows * nres), (carry, B * P * desc.C),
                 (carry_out, B * P * desc.C), (wp, desc.N * desc.K * (desc.C // G))):
        if t is not None and (not t.is_contiguous() or t.numel() != n):
            raise L.SelError(f"sel: hfg_conv_step operand of {t.numel()} elements, expected {n} contiguous")
    if wp.dtype != x.dtype or (carry is not None and carry.dtype != x.dtype) or \
            (carry_out is not None and carry_out.dtype != x.dtype) or (res is not None and res.dtype != out.dtype):
        raise L.SelError("sel: hfg_conv_step operands must share the input dtype (res: the output dtype)")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise L.SelError("sel: hfg_conv_step takes a contiguous fp32 bias")
    L.call("sel_hfg_conv_step", ctypes.byref(desc), CO._code(x.dtype), CO._code(out.dtype), L.ptr(carry), L.ptr(x),
           L.ptr(wp), L.ptr(bias), L.ptr(res), L.ptr(out), L.ptr(carry_out), L.stream())
    return out, carry_out


@dataclass(frozen=True)
class VocoderStep:
    """One sel_hfg_conv_step launch of a vocoder hop."""
    name: str                 # module path of the layer (it owns pad_buffer), generator.get_submodule(name)
    conv: str                 # module path of the inner nn.Conv1d / nn.ConvTranspose1d: its weight-norm-folded
    #                           weight comes from sel.hfgops.packed(module, kind, stride, dtype), its bias as is
    kind: int                 # sel.convops.PACK_FWD / PACK_CONVT
    stride: int
    T: int                    # descriptor fields; rows = batch * T
    C: int
    N: int
    K: int
    dil: int
    groups: int
    shared_in: bool           # in_group_stride 0: the source has C/G channels every group reads
    shared_res: bool          # res_group_stride 0: the residual has N/G channels
    bias_period: int
    slope: float              # LeakyReLU slope of the prologue on the new rows (1: none)
    tanh: bool
    scale: float
    accumulate: bool
    src: int                  # index of the step whose output buffer is the input; -1: decode's input
    res: Optional[int]        # index of the step whose output buffer is added
    out: int                  # index of the step whose output buffer this step writes (its own unless accumulate)
    carry_shape: Optional[Tuple[int, int, int]]   # (batch, P, C) or None (K = 1)
    buffer: Optional[str]     # state_dict key of the pad_buffer the carry stands for
    buffer_shape: Optional[Tuple[int, int, int]]  # its shape in the reference: (1, C, P)
    out_float: bool           # fp32 output whatever the compute dtype

    @property
    def pad(self):
        return (self.K - 1) * self.dil

    def desc(self, batch):
        from . import hfgops as HF
        return HF.make_desc(batch * self.T, self.T, self.C, self.N, self.K, self.dil, self.pad, CO.PAD_ZERO,
                            self.groups, self.shared_in, self.shared_res, self.bias_period, 0, self.tanh,
                            self.accumulate, self.slope, self.scale)


@dataclass(frozen=True)
class VocoderPlan:
    batch: int
    frames: int               # input frames per hop
    in_channels: int
    out_channels: int
    out_samples: int          # samples decode() returns per hop: frames * prod(upsample_scales)
    steps: Tuple[VocoderStep, ...]


def _vreject(msg):
    raise NotImplementedError(f"sel.streamops.plan_vocoder: {msg}")


def _lrelu_slope(act, where):
    if not isinstance(act, torch.nn.LeakyReLU):
        _vreject(f"{where} is a {type(act).__name__}: the step kernel fuses LeakyReLU only")
    return float(act.negative_slope)


class _VocoderBuilder:
    def __init__(self, batch):
        self.batch = batch
        self.steps = []

    def _add(self, **kw):
        i = len(self.steps)
        kw.setdefault("out", i)
        self.steps.append(VocoderStep(**kw))
        return kw["out"]

    def causal(self, name, m, T, src, slope=1.0, res=None, shared_in=False, shared_res=False, tanh=False, scale=1.0,
               out=None, out_float=False):
        """CausalConv1d.inference fed with act(x) (hfgops.causal_stream)."""
        from layers.conv_layer import CausalConv1d
        if not isinstance(m, CausalConv1d) or m.stride != 1:
            _vreject(f"{name} is no stride-1 CausalConv1d")
        c = m.conv
        K, dil = c.kernel_size[0], c.dilation[0]
        P = (K - 1) * dil
        if P == 0:
            _vreject(f"{name} has kernel_size 1: its pad_buffer grows with every call in the reference")
        kw = {} if out is None else dict(out=out)
        return self._add(name=name, conv=f"{name}.conv", kind=CO.PACK_FWD, stride=1, T=T, C=c.in_channels,
                         N=c.out_channels, K=K, dil=dil, groups=c.groups, shared_in=shared_in, shared_res=shared_res,
                         bias_period=c.out_channels if c.bias is not None else 0, slope=slope, tanh=tanh,
                         scale=scale, accumulate=out is not None, src=src, res=res,
                         carry_shape=(self.batch, P, c.in_channels), buffer=f"{name}.pad_buffer",
                         buffer_shape=(1, c.in_channels, P), out_float=out_float, **kw)

    def upsample(self, name, m, T, src, slope):
        """CausalConvTranspose1d.inference fed with act(x), k = 2s (hfgops.upsample_stream)."""
        from layers.conv_layer import CausalConvTranspose1d
        if not isinstance(m, CausalConvTranspose1d):
            _vreject(f"{name} is a {type(m).__name__}, not a CausalConvTranspose1d")
        d, s = m.deconv, m.stride
        if m.kernel_size != 2 * s or d.groups != 1:
            _vreject(f"{name} has kernel_size {m.kernel_size} != 2 * stride ({s}) or groups; such layers stay on "
                     "the module path")
        i = self._add(name=name, conv=f"{name}.deconv", kind=CO.PACK_CONVT, stride=s, T=T, C=d.in_channels,
                      N=s * d.out_channels, K=2, dil=1, groups=1, shared_in=False, shared_res=False,
                      bias_period=d.out_channels if d.bias is not None else 0, slope=slope, tanh=False, scale=1.0,
                      accumulate=False, src=src, res=None, carry_shape=(self.batch, 1, d.in_channels),
                      buffer=f"{name}.pad_buffer", buffer_shape=(1, d.in_channels, 1), out_float=False)
        return i, T * s

    def pointwise(self, name, c, T, src):
        """Conv1d1x1 (MultiGroupConv1d.conv_out): K = 1, no carry."""
        if not isinstance(c, torch.nn.Conv1d) or c.kernel_size[0] != 1 or c.groups != 1:
            _vreject(f"{name} is no 1x1 conv")
        return self._add(name=name, conv=name, kind=CO.PACK_FWD, stride=1, T=T, C=c.in_channels, N=c.out_channels,
                         K=1, dil=1, groups=1, shared_in=False, shared_res=False,
                         bias_period=c.out_channels if c.bias is not None else 0, slope=1.0, tanh=False, scale=1.0,
                         accumulate=False, src=src, res=None, carry_shape=None, buffer=None, buffer_shape=None,
                         out_float=False)

    def resblock(self, name, blk, T, src, shared_first=False, scale=1.0, out=None):
        """HiFiGANResidualBlock.inference (hfgops.resblock, stream=True); shared_first:
        src has C/G channels (MultiGroupConv1d's repeat, never materialised)."""
        slope = _lrelu_slope(blk.activation, f"{name}.activation")
        n = blk.num_layer
        x = src
        for idx in range(n):
            sh = shared_first and idx == 0
            kw = dict(scale=scale, out=out) if idx == n - 1 else {}
            if blk.use_additional_convs:
                h = self.causal(f"{name}.convs1.{idx}", blk.convs1[idx], T, x, slope, shared_in=sh)
                x = self.causal(f"{name}.convs2.{idx}", blk.convs2[idx], T, h, slope, res=x, shared_res=sh, **kw)
            else:
                x = self.causal(f"{name}.convs1.{idx}", blk.convs1[idx], T, x, slope, res=x, shared_in=sh,
                                shared_res=sh, **kw)
        return x


def plan_vocoder(generator, batch, frames):
    """The steps of one hop of `frames` input frames at `batch` streams for a
    HiFi-GAN StreamGenerator (models/vocoder/HiFiGAN.py), in the order of
    ``decode``: input_conv, per stage the upsampling layer and its block
    (MultiGroupConv1d: the residual block with the shared input / residual on its
    first layer, then conv_out; MultiReceptiveField: every block in turn, the
    first one's last conv writing the fusion buffer at 1/num_blocks, the later
    ones accumulating into it), output_conv with tanh and fp32 output.  Pure
    Python: reads module attributes only.  Raises NotImplementedError for what
    a session cannot run."""
    from models.vocoder.modules.multi_fusion import MultiGroupConv1d, MultiReceptiveField
    if batch < 1 or frames < 1:
        raise ValueError("sel.streamops.plan_vocoder: batch and frames must be positive")
    for attr in ("input_conv", "upsamples", "blocks", "output_conv", "activation_upsamples", "activation_output1"):
        if not hasattr(generator, attr):
            _vreject(f"{type(generator).__name__} is no HiFi-GAN generator (no {attr})")
    b = _VocoderBuilder(batch)
    T = frames
    cur = b.causal("input_conv", generator.input_conv, T, -1)
    up = _lrelu_slope(generator.activation_upsamples, "activation_upsamples")
    for i, (ups, blk) in enumerate(zip(generator.upsamples, generator.blocks)):
        cur, T = b.upsample(f"upsamples.{i}", ups, T, cur, up)
        if isinstance(blk, MultiGroupConv1d):
            y = b.resblock(f"blocks.{i}", blk, T, cur, shared_first=True)
            cur = b.pointwise(f"blocks.{i}.conv_out", blk.conv_out, T, y)
        elif isinstance(blk, MultiReceptiveField):
            nb = len(blk.blocks)
            fused = None
            for j, rb in enumerate(blk.blocks):
                o = b.resblock(f"blocks.{i}.blocks.{j}", rb, T, cur, scale=1.0 / nb, out=fused)
                fused = o if fused is None else fused
            cur = fused
        else:
            _vreject(f"blocks.{i} is a {type(blk).__name__}")
    out_slope = _lrelu_slope(generator.activation_output1, "activation_output1")
    if not isinstance(generator.activation_output2, torch.nn.Tanh):
        _vreject("activation_output2 is not Tanh")
    b.causal("output_conv", generator.output_conv, T, cur, out_slope, tanh=True, out_float=True)
    steps = tuple(b.steps)
    return VocoderPlan(batch, frames, steps[0].C, steps[-1].N, T, steps)
