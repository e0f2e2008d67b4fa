"""Streaming codec sessions: a hop as a fixed list of step launches, replayed
as a HIP graph.

``StreamGenerator.encode/decode`` (models/autoencoder*/AudioDec.py) run every
causal layer through ``*.inference``: a ``cat`` with the pad_buffer, a fresh
buffer tensor per call, the training conv kernel, a slice.  A ``StreamSession``
runs the same hop as one ``sel_conv_step`` launch per layer (csrc/stream.hip)
plus one ``sel_stream_commit``, on buffers allocated once: every activation,
every carry (the pad_buffers, channels-last) and their ``carry_out`` twins live
at fixed addresses, so ``encode`` and ``decode`` are each captured into one
graph (single stream, no parallel branches) and replayed per hop.

The session is opt-in and changes nothing on the module path; the two exchange
state through ``load_state`` / ``store_state``.

``VocoderSession`` is the same for the receiver of the shipped codecs, the
HiFi-GAN vocoder ``StreamGenerator.decode`` (models/vocoder/HiFiGAN.py): one
``sel_hfg_conv_step`` launch per conv (csrc/hfg_step.hip; groups, LeakyReLU,
tanh and the MultiReceptiveField mean inside the kernel), one commit per 48
carries, one graph.

``StreamPool`` / ``VocoderPool`` serve streams that do NOT move in lockstep:
a fixed number of slots, each holding one stream's carries, and per tick one
batched hop over whichever slots have a hop ready, on the slot-indexed step
kernels (``sel_conv_step_pool`` / ``sel_hfg_conv_step_pool``); the active set is
device data, so one captured graph serves every tick.

``enable_codes()`` on any of the four puts the quantizer behind the
transmitter's hop and the codebook lookup in front of the receiver's, as
stateless step launches (``sel_rvq_step`` / ``sel_rvq_lookup_step``,
csrc/vq_step.hip) in second graphs beside the existing ones: ``transmit`` is
then one replay from samples to code indices, ``receive`` one from code
indices to samples.  ``enable_codes(wire=True)`` also puts the bytes of the
wire format (sel/wire.py) inside the hop: ``transmit_packets`` is one replay from
samples to packets, ``receive_packets`` one from packets to samples.
``enable_codes(datagrams=True)`` adds what a sender puts on a network (wire
version 2, ``sel.wire.DatagramFormat``): ``transmit_datagrams`` stops the
quantizer after each stream's stage budget and writes a header with the stage
count and the hop number; ``receive_datagrams`` decodes whatever stage count
arrives and conceals a hop that did not, from the stream's last good record.

Inside, all of these are one mechanism.  A ``_Half`` holds the fixed buffers
and the step launches of ``encode`` or ``decode``, and a dict of named hop
variants (``_Hop``): the plain hop, and whatever ``enable_codes`` added with
``add_hop(name, pre=..., post=..., **buffers)`` -- "codes", "wire", "dgram" --
each a launch list ``pre -> steps -> commit -> post`` with its own graph and
the buffers it owns; ``run(name)`` replays one.  The six ``transmit*`` /
``receive*`` methods are written once, in ``_CodesMixin``, for sessions
(``method(x)``) and pools (``method(slots, x)``); what differs between the two --
the slot list to stage, n of capacity rows, the wording of errors, how a
datagram hop's control words reach the device -- is a handful of hooks, the
session's in ``_CodesMixin``, the pool's in ``_PoolBase``.
"""
import functools

import torch

from . import _lib as L
from . import convops as CO
from . import streamops as SO
from .wire import WireFormat


class _Hop:
    """One named variant of a half's hop: ``pre -> steps -> commit -> post`` as a
    launch list and, for a captured half, a graph of its own.  ``pre`` / ``post``
    are stateless launches in front of the steps (a lookup into ``inp``) or behind
    them (a quantizer on ``outs[-1]``); the plain hop has neither.  Beside them
    the fixed buffers the variant owns -- ``idx`` (S, rows) code indices, ``buf``
    packets (rows, frame_bytes) or datagrams (streams, stride), ``ctl`` the device
    control words a datagram launch reads (staged before every replay), ``hold``
    the receiver's held records -- and the views of them a per-hop method hands
    out, prepared once: ``idx_out`` (S, streams, frames), ``packets`` (streams,
    packet_bytes), ``y`` (streams, out_channels, samples) of the half's output.
    ``staged``: on a session, the control words the device holds (None: unknown)."""

    def __init__(self, pre=None, post=None, idx=None, buf=None, ctl=None, hold=None, idx_out=None, packets=None,
                 y=None):
        self.pre, self.post, self.graph, self.staged = pre, post, None, None
        self.idx, self.buf, self.ctl, self.hold = idx, buf, ctl, hold
        self.idx_out, self.packets, self.y = idx_out, packets, y


class _Half:
    """The launches of one method (encode or decode) on fixed buffers."""
    _step = staticmethod(SO.conv_step)

    def __init__(self, steps, generator, batch, in_channels, dtype, device):
        self.steps = steps
        self.batch = batch
        T0 = steps[0].T * (steps[0].stride if steps[0].kind == CO.PACK_FWD_STRIDED else 1)
        self.inp = torch.zeros((batch, T0, in_channels), dtype=dtype, device=device)
        self.descs, self.wps, self.biases, self.outs = [], [], [], []
        self.carry, self.carry_out = [], []
        for i, st in enumerate(steps):
            wp, bias = self._weights(generator, st, dtype)
            self.descs.append(st.desc(batch))
            self.wps.append(wp)
            self.biases.append(bias)
            if getattr(st, "out", i) != i:
                self.outs.append(self.outs[st.out])    # a vocoder step that accumulates into an earlier one's buffer
            else:
                self.outs.append(torch.zeros((batch * st.T, st.N), dtype=torch.float32 if st.out_float else dtype,
                                             device=device))
            if st.carry_shape is None:
                self.carry.append(None)
                self.carry_out.append(None)
            else:
                self.carry.append(torch.zeros(st.carry_shape, dtype=dtype, device=device))
                self.carry_out.append(torch.zeros(st.carry_shape, dtype=dtype, device=device))
        self.pairs = [(o, c) for o, c in zip(self.carry_out, self.carry) if c is not None]
        self.hops = {None: _Hop()}         # the variants by name; None: the plain hop

    @staticmethod
    def _weights(generator, st, dtype):
        """(packed weight, fp32 bias or None) of a step"""
        w = generator.get_parameter(st.weight)
        L.need_device(w)
        bias = generator.get_parameter(st.bias).detach().float().contiguous() if st.bias else None
        return CO.PACKS.get(st.kind, w, st.stride, dtype)[0], bias

    @property
    def graph(self):
        return self.hops[None].graph

    @property
    def hold(self):
        """the receiver's held records once enable_codes(datagrams=True) ran"""
        hop = self.hops.get("dgram")
        return None if hop is None else hop.hold

    def _buf(self, i):
        return self.inp if i == -1 else self.outs[i]

    def _launch_steps(self):
        step = self._step
        for i, st in enumerate(self.steps):
            step(self.descs[i], self.carry[i], self._buf(st.src), self.wps[i], self.biases[i],
                 None if st.res is None else self._buf(st.res), self.outs[i], self.carry_out[i])
        SO.commit(self.pairs)

    def launch(self, hop=None):
        if hop is not None and hop.pre is not None:
            hop.pre()
        self._launch_steps()
        if hop is not None and hop.post is not None:
            hop.post()

    def capture(self, warmup=2):
        dev = self.inp.device
        # eager warm-up on a side stream, as trainer/graph.py does it
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.launch()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.launch()
        self.hops[None].graph = graph

    def add_hop(self, name, pre=None, post=None, **buffers):
        """A further variant of the hop beside the plain one: a second launch list
        with a stateless launch in front of the steps (``pre``) or behind them
        (``post``) and, for a captured half, a second graph.  Only the new launch is
        warmed up eagerly (it has no state; a pool's runs with ``n_active = 0``); the
        capture itself executes nothing, so no carry moves.  ``buffers``: the fixed
        tensors the variant owns (_Hop)."""
        hop = self.hops[name] = _Hop(pre, post, **buffers)
        if self.graph is not None:
            (pre or post)()
            torch.cuda.synchronize(self.inp.device)
            hop.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(hop.graph):
                self.launch(hop)
        return hop

    def drop_hops(self):
        self.hops = {None: self.hops[None]}

    def run(self, name=None):
        """Replay the variant's graph, or issue its launch list."""
        hop = self.hops[name]
        if hop.graph is not None:
            hop.graph.replay()
        else:
            self.launch(hop)
        return self.outs[-1]

    def zero(self):
        for c in self.carry:
            if c is not None:
                c.zero_()


def _fill_idx(dst, idx, owner, which, n):
    """idx (S, [batch,] frames) int64 -> the fixed (S, rows) buffer (or its first rows); owner._what(which, n)
    names the call when it is refused."""
    L.need_device(idx)
    if idx.dtype != torch.int64 or idx.dim() < 2 or idx.shape[0] != dst.shape[0] or idx.numel() != dst.numel():
        raise L.SelError(f"sel: {owner._what(which, n)} takes int64 indices of {dst.shape[0]} codebooks x {dst.shape[1]} frames, "
                         f"got {idx.dtype} {tuple(idx.shape)}")
    dst.copy_(idx.reshape(dst.shape))


def _fill_packets(dst, p, owner, which, n):
    """p (n, packet_bytes) uint8 -> the fixed packet buffer (or its first n packets)."""
    L.need_device(p)
    if p.dtype != torch.uint8 or tuple(p.shape) != tuple(dst.shape):
        raise L.SelError(f"sel: {owner._what(which, n)} takes uint8 packets of shape {tuple(dst.shape)}, got {p.dtype} {tuple(p.shape)}")
    dst.copy_(p)


class _CodesMixin:
    """``enable_codes`` / ``transmit`` / ``receive`` of sessions and pools: the
    quantizer behind the transmitter's hop and the codebook lookup in front of
    the receiver's, inside the hop's launch list (csrc/vq_step.hip)."""
    _tx = _rx = None          # the halves that carry codes once enable_codes ran
    _codes_enabled = _wire_enabled = _dgram_enabled = False
    wire = None               # the WireFormat once enable_codes(wire=True) gave a half its packets
    datagram = None           # the DatagramFormat once enable_codes(datagrams=True) gave a half its datagrams
    _seq = _dstats = _dgram_stager = None

    @torch.no_grad()
    def enable_codes(self, lookup_generator=None, wire=False, datagrams=False):
        """Put ``quantize`` behind ``encode`` and ``lookup`` in front of ``decode``:
        afterwards ``transmit`` is one replay from samples to code indices and
        ``receive`` one replay from code indices to samples.

        The transmitter half (an AudioDec session / pool with PQC) snapshots its
        own generator's codebook stack (S, D, K); the receiver half snapshots the
        flat (S*K, D) codebook of ``lookup_generator`` (default:
        ``self.lookup_generator``; none known: no receiver half) and, for a
        vocoder with ``stats``, its mean / scale.  The snapshots are private fp32
        copies taken once, like the packed weights: call ``enable_codes`` again
        after the codebooks change.  With ``graph=True`` the extended hops are
        captured as NEW graphs beside the existing ones; ``encode`` / ``decode`` /
        ``quantize`` / ``lookup`` keep their graphs and their bits.  No carry and
        no template row changes (safe after ``load_state()``).

        ``wire=True`` adds the packets of the wire format (sel/wire.py; the layout
        is ``self.wire``): the transmitter's quantizer launch writes them beside
        the indices (``transmit`` keeps its bits, ``transmit_packets`` returns the
        bytes of the same replay), and the receiver gets a third launch list and
        graph that looks the codes up straight out of the packet buffer
        (``receive_packets``), with no int64 buffer in between.

        ``datagrams=True`` adds wire version 2 (``self.datagram``, a
        ``sel.wire.DatagramFormat``) beside whatever the other keywords built: a
        further launch list and graph per half.  The transmitter's ends in
        ``rvq_step_dgram``, whose chain stops after each stream's stage budget
        (``transmit_datagrams(x, stages)``); the receiver's starts with
        ``rvq_lookup_dgram_step``, which takes the stage count from each header and
        conceals a hop that did not arrive by repeating the stream's last good
        record (``receive_datagrams``).  Budgets, hop numbers and loss flags are
        device words staged before the replay, so one graph serves every mix."""
        for half in self._halves:
            half.drop_hops()
        self._tx = self._rx = self.wire = self.datagram = None
        self._seq = self._dstats = None
        self._all = range(self._dec.inp.shape[0])        # a session's streams
        self._codes_enabled = self._wire_enabled = self._dgram_enabled = False
        tx = self._build_transmitter(wire, datagrams)
        rx = self._build_receiver(lookup_generator if lookup_generator is not None else self.lookup_generator, wire,
                                  datagrams)
        for name in ("wire", "dgram"):
            if name in tx and name in rx and (tx[name].codebooks, tx[name].codebook_size) != (rx[name].codebooks,
                                                                                              rx[name].codebook_size):
                raise L.SelError(f"sel: the transmitter packs {tx[name]!r}, the lookup codebook reads {rx[name]!r}")
        fmt = {**rx, **tx}
        self.wire, self.datagram = fmt.get("wire"), fmt.get("dgram")
        if self.datagram is not None:
            streams = self._dec.inp.shape[0]
            self._seq = [0] * streams
            self._dstats = [self._new_stats() for _ in range(streams)]
        self._codes_enabled, self._wire_enabled, self._dgram_enabled = True, bool(wire), bool(datagrams)

    def _build_transmitter(self, wire, datagrams):
        """The variants of the transmitter half (an AudioDec session / pool with PQC):
        "codes", whose quantizer launch writes the indices and, with ``wire``, the
        packets beside them -- ``transmit`` and ``transmit_packets`` are the same
        replay -- and "dgram".  -> {"wire" / "dgram": the format built}."""
        enc = getattr(self, "_enc", None)
        if enc is None or not self.plan.pqc:
            return {}
        dev, frames, fmt = enc.inp.device, self.plan.frames, {}
        rvq = self.generator.quantizer.codebook
        stack = torch.stack([l.embed.detach() for l in rvq.layers]).to(dev, torch.float32).contiguous().clone()
        z = enc.outs[-1]
        if z.dtype != torch.float32 or z.shape[1] != stack.shape[1]:
            raise L.SelError(f"sel: encode's output rows {z.dtype} {tuple(z.shape)} are not the fp32 code vectors "
                             f"of a (S, D, K) = {tuple(stack.shape)} quantizer")
        S, K = stack.shape[0], stack.shape[2]
        idx = torch.zeros((S, z.shape[0]), dtype=torch.int64, device=dev)
        idx_out = self._idx_view(idx.view(S, -1, frames))
        count = getattr(enc, "n_active", None)
        self._prepare_codes(enc)
        if wire:
            fmt["wire"] = WireFormat(S, K, frames)
            buf = torch.zeros((z.shape[0], fmt["wire"].frame_bytes), dtype=torch.uint8, device=dev)
            enc.add_hop("codes", post=functools.partial(SO.rvq_step_wire, z, stack, buf, frames, count, True, idx),
                        idx=idx, idx_out=idx_out, buf=buf, packets=buf.view(-1, fmt["wire"].packet_bytes))
        else:
            enc.add_hop("codes", post=functools.partial(SO.rvq_step, z, stack, idx, frames, count, True), idx=idx,
                        idx_out=idx_out)
        if datagrams:
            fmt["dgram"] = self._datagram_format(S, K, frames)
            B = z.shape[0] // frames
            dbuf = torch.zeros((B, fmt["dgram"].stride), dtype=torch.uint8, device=dev)
            ctl, (stages, seq) = self._dgram_words(enc, B, 2, dev)
            post = functools.partial(SO.rvq_step_dgram, z, stack, dbuf, frames, count, stages, seq, True)
            if count is None:
                # a session (no slot list to stage): the hop numbers advance on the device, behind
                # the launch that read them, so a steady budget needs no control copy per hop
                def post(launch=post, seq=seq):
                    launch()
                    seq.add_(1)
            enc.add_hop("dgram", post=post, buf=dbuf, ctl=ctl)
        self._tx = enc
        return fmt

    def _build_receiver(self, lg, wire, datagrams):
        """The variants of the receiver half for the flat (S*K, D) codebook of ``lg``
        (none: no receiver half): "codes", the lookup out of the index buffer,
        "wire", a list and graph of its own that looks the codes up straight out of
        the packet buffer, and "dgram".  -> {"wire" / "dgram": the format built}."""
        dec = self._dec
        if lg is None or (getattr(self, "_enc", None) is not None and not self.plan.pqc):
            return {}
        dev, frames, fmt = dec.inp.device, self.plan.frames, {}
        rvq = lg.quantizer.codebook
        if not hasattr(rvq, "codebook_size"):
            lg.quantizer.initial()
        flat = rvq.codebook.detach().to(dev, torch.float32).contiguous().clone()
        S = len(rvq.layers)
        if dec.inp.shape[-1] != flat.shape[1]:
            raise L.SelError(f"sel: the lookup codebook has {flat.shape[1]} channels, decode takes "
                             f"{dec.inp.shape[-1]}")
        B = dec.inp.shape[0]
        idx = torch.zeros((S, B * frames), dtype=torch.int64, device=dev)
        y = dec.outs[-1].view(B, self.plan.out_samples, self.plan.out_channels).transpose(1, 2)
        mean = scale = None
        if getattr(self.generator, "norm", False):
            mean = self.generator.mean.detach().to(dev, torch.float32).contiguous().clone()
            scale = self.generator.scale.detach().to(dev, torch.float32).contiguous().clone()
        if (wire or datagrams) and flat.shape[0] % S:
            raise L.SelError(f"sel: the lookup codebook's {flat.shape[0]} rows are not {S} stages of one size")
        count = getattr(dec, "n_active", None)
        self._prepare_codes(dec)
        dec.add_hop("codes", pre=functools.partial(SO.rvq_lookup_step, idx, flat, dec.inp, frames, mean, scale, count),
                    idx=idx, y=y)
        if wire:
            fmt["wire"] = WireFormat(S, flat.shape[0] // S, frames)
            buf = torch.zeros((idx.shape[1], fmt["wire"].frame_bytes), dtype=torch.uint8, device=dev)
            dec.add_hop("wire", pre=functools.partial(SO.rvq_lookup_wire_step, buf, flat, S, dec.inp, frames, mean,
                                                      scale, count),
                        buf=buf, packets=buf.view(B, fmt["wire"].packet_bytes), y=y)
        if datagrams:
            fmt["dgram"] = self._datagram_format(S, flat.shape[0] // S, frames)
            dbuf = torch.zeros((B, fmt["dgram"].stride), dtype=torch.uint8, device=dev)
            # a stream's last good record, at a fixed address: one row per batch stream / pool slot
            hold = torch.zeros((B, 1 + fmt["dgram"].frame_bytes()), dtype=torch.uint8, device=dev)
            ctl, (lost,) = self._dgram_words(dec, B, 1, dev)
            dec.add_hop("dgram", pre=functools.partial(SO.rvq_lookup_dgram_step, dbuf, flat, S, dec.inp, frames, mean,
                                                       scale, count, getattr(dec, "slots", None), lost, hold),
                        buf=dbuf, ctl=ctl, hold=hold, y=y)
        self._rx = dec
        return fmt

    # ---- datagrams: formats, control words, counters ----------------------------------------
    @staticmethod
    def _datagram_format(S, K, frames):
        from .wire import DatagramFormat
        try:
            return DatagramFormat(S, K, frames)
        except ValueError as e:
            raise L.SelError(f"sel: enable_codes(datagrams=True): {e}") from None

    def _dgram_words(self, half, B, arrays, device):
        """The device control words of a half's datagram launch: ``arrays`` int32
        arrays of B entries (one per stream) behind one another, so that one copy
        stages them all -> (the tensor to stage into, the arrays).  A session has no
        control words yet and gets a tensor of its own (pools: _PoolBase)."""
        if self._dgram_stager is None:
            self._dgram_stager = _Stager(2 * B, device)
        ctl = torch.zeros(arrays * B, dtype=torch.int32, device=device)
        return ctl, [ctl[i * B:(i + 1) * B] for i in range(arrays)]

    @staticmethod
    def _new_stats():
        return dict(received=0, lost=0, refused=0, seq_gaps=0, concealed_run=0, stages=None, seq=None)

    def _clear_stream(self, i):
        """Stream i (a batch position, a pool slot) starts over: hop number 0, nothing held, counters at zero."""
        if self._seq is not None:
            self._seq[i] = 0
            self._dstats[i] = self._new_stats()
        if self._rx is not None and self._rx.hold is not None:
            self._rx.hold[i].zero_()

    def _stage_list(self, which, stages, n):
        """``stages``: None (all), an int, or one int per stream, each in [1, S] -> a list of n ints."""
        S = self.datagram.codebooks
        if stages is None:
            return [S] * n
        if isinstance(stages, torch.Tensor):
            if stages.dim() > 1 or stages.dtype not in (torch.int32, torch.int64):
                raise L.SelError(f"sel: {self._what(which, n)} takes stages as an int or {n} ints, got {stages.dtype} "
                                 f"{tuple(stages.shape)}")
            stages = stages.tolist()
        raw = [stages] * n if isinstance(stages, int) and not isinstance(stages, bool) else list(stages) \
            if isinstance(stages, (list, tuple)) else None
        if raw is None or len(raw) != n:
            raise L.SelError(f"sel: {self._what(which, n)} takes stages as an int or {n} ints, got {stages!r}")
        for s in raw:
            if not isinstance(s, int) or isinstance(s, bool) or not 1 <= s <= S:
                raise L.SelError(f"sel: {self._what(which, n)}: a budget of {s!r} stages, the quantizer has 1..{S}")
        return raw

    def _take_datagrams(self, which, dst, p, lost, streams):
        """Fill the fixed buffer's rows ``dst`` (n, stride) from ``p`` and return the n
        loss flags, counting per stream.  ``p``: a device uint8 (n, stride) tensor
        (``lost``: n flags or None), or a list of bytes-like / None entries, which
        goes through ``DatagramFormat.assemble`` and one host-to-device copy."""
        n, fmt = dst.shape[0], self.datagram
        heads = [None] * n
        refused = ()
        if isinstance(p, torch.Tensor):
            L.need_device(p)
            if p.dtype != torch.uint8 or tuple(p.shape) != tuple(dst.shape):
                raise L.SelError(f"sel: {self._what(which, n)} takes uint8 datagrams of shape {tuple(dst.shape)}, got {p.dtype} "
                                 f"{tuple(p.shape)}")
            flags = self._flag_list(which, lost, n)
            dst.copy_(p)
        elif isinstance(p, (list, tuple)):
            if len(p) != n or any(d is not None and not isinstance(d, (bytes, bytearray, memoryview)) for d in p):
                raise L.SelError(f"sel: {self._what(which, n)} takes {n} datagrams, each bytes-like or None")
            buf, gone, refused = fmt.assemble(p)
            flags = [int(a or b) for a, b in zip(gone, self._flag_list(which, lost, n))]
            heads = [None if f else fmt.parse(d) for f, d in zip(gone, p)]
            dst.copy_(buf)
        else:
            raise L.SelError(f"sel: {self._what(which, n)} takes a device uint8 tensor or a list of bytes-like / None entries, got "
                             f"{type(p).__name__}")
        for j, (i, f) in enumerate(zip(streams, flags)):
            st = self._dstats[i]
            if f:
                st["lost"] += 1
                st["refused"] += int(j in refused)
                st["concealed_run"] += 1
                continue
            st["received"] += 1
            st["concealed_run"] = 0
            if heads[j] is not None:                  # a device tensor's headers are not read back
                s, q = heads[j]
                if st["seq"] is not None:
                    st["seq_gaps"] += (q - st["seq"] - 1) & 0xFFFF
                st["stages"], st["seq"] = s, q
        return flags

    def _flag_list(self, which, lost, n):
        if lost is None:
            return [0] * n
        if isinstance(lost, torch.Tensor):
            if lost.dim() != 1 or lost.dtype not in (torch.bool, torch.int32, torch.int64):
                raise L.SelError(f"sel: {self._what(which, n)} takes lost as {n} flags, got {lost.dtype} {tuple(lost.shape)}")
            lost = lost.tolist()
        if not isinstance(lost, (list, tuple)) or len(lost) != n or \
                any(not isinstance(f, (bool, int)) for f in lost):
            raise L.SelError(f"sel: {self._what(which, n)} takes lost as {n} flags, got {lost!r}")
        return [int(bool(f)) for f in lost]

    def _prepare_codes(self, half):
        """Before a half's new launch is warmed up and captured (pools: no active stream)."""

    def _codes_half(self, which):
        if not self._codes_enabled:
            raise L.SelError(f"sel: {which} needs enable_codes() first")
        if which.endswith("_packets") and not self._wire_enabled:
            raise L.SelError(f"sel: {which} needs enable_codes(wire=True) first")
        if which.endswith("_datagrams") and not self._dgram_enabled:
            raise L.SelError(f"sel: {which} needs enable_codes(datagrams=True) first")
        if which.startswith("transmit"):
            if self._tx is None:
                raise L.SelError(f"sel: {which} needs a transmitter with PQC: without it (or on a vocoder) encode's "
                                 "output is not the projector's fp32 code vector")
            return self._tx
        if self._rx is None:
            raise L.SelError(f"sel: {which} knows no lookup codebook: set lookup_generator (the generator whose "
                             "codebooks decode the indices) and call enable_codes() again")
        return self._rx

    # ---- what differs between a session and a pool, as hooks (the pool's: _PoolBase) -----------
    # A per-hop method takes (x) on a session and (slots, x) on a pool.  _begin splits that into
    # (slots, x, optional); a session's slots are None, and so is its n below: every stream, the
    # whole of each fixed buffer, nothing to stage.  A pool's n counts the listed slots.
    def _begin(self, which, args, opt=None, takes_opt=False):
        if len(args) != 1:
            opt = self._optional(which, args, 1, opt, takes_opt)
        return None, args[0], opt

    @staticmethod
    def _optional(which, args, lead, opt, takes_opt):
        """the datagram methods' optional argument given by position, or a TypeError for the arity"""
        if len(args) != lead + 1 or not takes_opt or opt is not None:
            raise TypeError(f"{which}() takes {'a slot list and ' if lead > 1 else ''}one argument"
                            f"{' and an optional one' if takes_opt else ''}, got {len(args)}")
        return args[-1]

    def _what(self, which, n):
        """how a refused call is named"""
        return "session " + which

    @staticmethod
    def _idx_view(idx):
        """the index buffer as (codebooks, streams, frames) -> the view ``transmit`` hands out, prepared once"""
        return idx.squeeze(1)

    def _stage_dgram(self, hop, streams, *arrays):
        """A datagram hop's control words -- budgets and hop numbers, or loss flags --
        staged as a pool's slot list is, unless the device already holds exactly
        these (a receiver that loses nothing stages nothing)."""
        words, = arrays                                  # a session stages one array at a time
        if hop.staged != words:
            self._dgram_stager.stage(hop.ctl, words)
            hop.staged = words

    def _stage_budgets(self, hop, streams, budgets):
        words = budgets + self._seq
        if hop.staged != words:
            self._dgram_stager.stage(hop.ctl, words)
        hop.staged = None                                # unknown until the hop has run

    def _sent(self, hop, budgets):
        # the hop's last launch added 1 to every hop number on the device: with the same budgets the
        # next hop finds its words in place (at the 2^16 wrap they differ, and are staged again)
        hop.staged = budgets + [q + 1 for q in self._seq]
        self._seq = [(q + 1) & 0xFFFF for q in self._seq]

    # ---- the per-hop methods, once for sessions and pools ---------------------------------------
    def _check_input(self, which, slots, x):
        pl = self.plan
        L.need_device(x)
        n = pl.batch if slots is None else len(slots)
        if tuple(x.shape) != (n, pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: {self._what(which, n)} takes {(n, pl.in_channels, pl.chunk)}, got "
                             f"{tuple(x.shape)}")

    def _send(self, which, args):
        """``transmit`` and ``transmit_packets``: the one replay that writes the index
        buffer and, with ``wire=True``, the packet buffer -> (its _Hop, n)"""
        half = self._codes_half(which)
        slots, x, _ = self._begin(which, args)
        self._check_input(which, slots, x)
        if slots is None:
            n = None
            half.inp.copy_(x.transpose(1, 2))
        else:
            n = self._stage(half, slots)
            half.inp[:n].copy_(x.transpose(1, 2))
        half.run("codes")
        return half.hops["codes"], n

    @torch.no_grad()
    def transmit(self, *args):
        """``transmit(x)`` on a session, ``transmit(slots, x)`` on a pool: x (n,
        in_channels, chunk), for all ``batch`` streams or the n listed slots ->
        flattened code indices, int64, what ``quantize(encode(x))`` returns (a
        pool: (codebooks, n, frames)): one replay.  A VIEW of a fixed buffer, valid
        until the next ``transmit``."""
        hop, n = self._send("transmit", args)
        return hop.idx_out if n is None else hop.idx_out[:, :n]

    @torch.no_grad()
    def receive(self, *args):
        """``receive(idx)`` on a session, ``receive(slots, idx)`` on a pool: the indices
        ``transmit`` / ``quantize`` return -> y (n, out_channels, samples), what
        ``decode(lookup(idx))`` returns (the codes summed in stage order): one replay."""
        half = self._codes_half("receive")
        hop = half.hops["codes"]
        slots, idx, _ = self._begin("receive", args)
        n = None if slots is None else self._stage(half, slots)
        _fill_idx(hop.idx if n is None else hop.idx[:, :n * self.plan.frames], idx, self, "receive", n)
        half.run("codes")
        return hop.y if n is None else hop.y[:n]

    # ---- the same in the bytes of the wire format (after enable_codes(wire=True)) -----
    @torch.no_grad()
    def transmit_packets(self, *args):
        """``transmit_packets(x)`` / ``transmit_packets(slots, x)`` -> (n, packet_bytes)
        uint8, ``self.wire``'s packing of what ``transmit`` returns for the same
        arguments, packet i that of stream i / ``slots[i]``: one replay (the one
        ``transmit`` runs).  A VIEW of a fixed buffer, valid until the next
        ``transmit`` / ``transmit_packets``."""
        hop, n = self._send("transmit_packets", args)
        return hop.packets if n is None else hop.packets[:n]

    @torch.no_grad()
    def receive_packets(self, *args):
        """``receive_packets(p)`` / ``receive_packets(slots, p)``: p (n, packet_bytes)
        uint8, packet i for stream i / ``slots[i]`` -> y, what ``receive`` returns
        for the indices in the packets: one replay, with no index tensor in between."""
        half = self._codes_half("receive_packets")
        hop = half.hops["wire"]
        slots, p, _ = self._begin("receive_packets", args)
        n = None if slots is None else self._stage(half, slots)
        _fill_packets(hop.packets if n is None else hop.packets[:n], p, self, "receive_packets", n)
        half.run("wire")
        return hop.y if n is None else hop.y[:n]

    # ---- the same in datagrams, wire version 2 (after enable_codes(datagrams=True)) -----
    @torch.no_grad()
    def transmit_datagrams(self, *args, stages=None):
        """``transmit_datagrams(x, stages=None)`` on a session, ``transmit_datagrams(slots,
        x, stages=None)`` on a pool -> (n, stride) uint8, ``stride =
        self.datagram.stride``: row i starts with the datagram of stream i /
        ``slots[i]`` for this hop -- the header with the stages carried and the
        stream's hop number (0 after construction, ``reset()`` and a pool's
        ``open()``, wrapping at 2^16), then the hop's records of ``stages`` fields
        -- ``self.datagram.datagram_bytes(stages[i])`` bytes; the bytes of a row
        beyond that are not written and keep what an earlier hop left there.
        ``stages``: an int or one int per stream in [1, codebooks], default all; the
        quantizer's chain stops after that many stages.  One replay, whatever the
        budgets: they are device words.  A session stages them in front of the
        replay when they change (its hop numbers advance on the device, behind the
        quantizer's launch); a pool stages them with its slot list, one control
        copy per tick.  A VIEW of a fixed buffer: a call invalidates the view the
        previous ``transmit_datagrams`` returned and, like ``transmit``,
        ``encode``'s; the views of ``transmit`` / ``transmit_packets`` stay valid."""
        half = self._codes_half("transmit_datagrams")
        hop = half.hops["dgram"]
        slots, x, stages = self._begin("transmit_datagrams", args, stages, True)
        self._check_input("transmit_datagrams", slots, x)
        if slots is None:
            n, streams, inp, out = None, self._all, half.inp, hop.buf
        else:
            streams = self.table.check(slots)
            n = len(streams)
            inp, out = half.inp[:n], hop.buf[:n]
        budgets = self._stage_list("transmit_datagrams", stages, len(streams))
        self._stage_budgets(hop, streams, budgets)
        inp.copy_(x.transpose(1, 2))
        half.run("dgram")
        self._sent(hop, budgets)
        return out

    @torch.no_grad()
    def receive_datagrams(self, *args, lost=None):
        """``receive_datagrams(p, lost=None)`` on a session, ``receive_datagrams(slots, p,
        lost=None)`` on a pool: the datagrams of one hop -> y, what ``receive``
        returns for the ids in them (-1 beyond the stages a datagram carries): one
        replay.  ``p``: a device uint8 (n, stride) tensor as ``transmit_datagrams``
        returns it, with ``lost``, one flag per stream, marking rows to disregard;
        or a list of n entries, bytes-like or None for a datagram that did not
        arrive, which ``self.datagram.assemble`` turns into one host-to-device
        copy.  A lost stream -- flagged, None, or with a header this receiver
        refuses -- is concealed: every frame of the hop decodes the last frame's
        record of the stream's last good datagram (nothing held yet, or the slot
        opened since: the empty sum), so the decoder's carried state moves on.
        Nothing is reordered: the caller decides which datagram belongs to which
        hop.  ``datagram_stats()`` counts."""
        half = self._codes_half("receive_datagrams")
        hop = half.hops["dgram"]
        slots, p, lost = self._begin("receive_datagrams", args, lost, True)
        if slots is None:
            streams, dst, y = self._all, hop.buf, hop.y
        else:
            streams = self.table.check(slots)
            dst, y = hop.buf[:len(streams)], hop.y[:len(streams)]
        self._stage_dgram(hop, streams, self._take_datagrams("receive_datagrams", dst, p, lost, streams))
        half.run("dgram")
        return y

    # ---- state: the carries of every half ---------------------------------------------------------
    def _layers(self):
        for half in self._halves:
            for st, c in zip(half.steps, half.carry):
                if c is not None:
                    yield st, c, self.generator.get_submodule(st.name)

    def _pad_rows(self, st, m, batches, holds):
        """a layer's pad_buffer (1 or batch, C, P_ref), checked, channels-last on the carries' device"""
        pb = m.pad_buffer
        if pb.shape[0] not in batches or tuple(pb.shape[1:]) != tuple(st.buffer_shape[1:]):
            raise L.SelError(f"sel: {st.buffer} has shape {tuple(pb.shape)}, {holds.format(st.buffer_shape)}")
        return pb.to(self._dec.inp.device).transpose(1, 2)


def _fill_carry(st, dst, rows):
    """dst ([batch,] P, C), a carry or one slot row of it <- rows ([batch,] P_ref, C),
    the reference's pad_buffer channels-last.  The down-sampling conv keeps its
    2s - 1 samples as 2 phase rows of s samples: 2s rows, the first one zeroed
    (the extra oldest sample meets a zero weight)."""
    if st.kind == CO.PACK_FWD_STRIDED:
        v = dst.view(*dst.shape[:-2], 2 * st.stride, -1)
        v[..., :1, :].zero_()
        v[..., 1:, :].copy_(rows)
    else:
        dst.copy_(rows)


class _SessionBase(_CodesMixin):
    """Capture, counters and state transfer of StreamSession and VocoderSession."""

    def _capture(self, graph):
        self.graphed = bool(graph)
        if graph:
            for half in self._halves:
                half.capture()
            self.reset()   # the warm-up hops ran on zero input; start from zero state

    def datagram_stats(self):
        """Per stream, since construction / ``reset()``: hops ``received``, ``lost``
        (``refused``: of those, the malformed ones), ``seq_gaps`` (hop numbers missing
        between consecutive datagrams seen), ``concealed_run`` (the current run of
        concealed hops) and the last datagram's ``stages`` and ``seq``.  Headers are
        read on the host only: for datagrams given as a device tensor ``refused``,
        ``seq_gaps``, ``stages`` and ``seq`` do not move."""
        if not self._dgram_enabled:
            raise L.SelError("sel: datagram_stats needs enable_codes(datagrams=True) first")
        return [dict(s) for s in self._dstats]

    def carries(self):
        """{pad_buffer key: carry tensor (batch, P, C), channels-last} -- the live state."""
        return {st.buffer: c for st, c, _ in self._layers()}

    @torch.no_grad()
    def reset(self):
        for half in self._halves:
            half.zero()
        for i in range(len(self._seq or ())):
            self._clear_stream(i)

    @torch.no_grad()
    def load_state(self):
        """carries <- the generator's pad_buffers ((1 or batch, C, P), broadcast to batch)."""
        for st, c, m in self._layers():
            rows = self._pad_rows(st, m, (1, c.shape[0]), "the session holds {} per stream")
            _fill_carry(st, c, rows.expand(c.shape[0], -1, -1))

    @torch.no_grad()
    def store_state(self):
        """The generator's pad_buffers <- carries, in the reference's shapes (fp32)."""
        for st, c, m in self._layers():
            v = c.view(c.shape[0], -1, st.buffer_shape[1])
            if st.kind == CO.PACK_FWD_STRIDED:
                v = v[:, 1:]
            m.pad_buffer = v.transpose(1, 2).float().contiguous()


class StreamSession(_SessionBase):
    """One streaming endpoint state: ``batch`` parallel streams, ``chunk`` samples per hop.

    ``encode(x) -> z``, ``quantize(z) -> idx``, ``lookup(idx) -> zq`` and
    ``decode(zq) -> y`` take and return what the ``StreamGenerator`` methods do
    (shapes and dtypes; for ``batch > 1`` ``lookup`` returns (batch, frames, dim),
    the layout ``decode`` takes).

    The tensors ``encode`` and ``decode`` return are VIEWS of the session's fixed
    output buffers: they are valid until the next call of the same method, which
    overwrites them in place (clone what must outlive it).  Inputs are copied
    into fixed input buffers, so the caller's tensors are free after the call.

    State: every causal layer's carry starts at zero (``reset()``);
    ``load_state()`` copies the generator's pad_buffers in -- so the reference's
    warm-up, ``G.initial_encoder(...)`` / ``G.initial_decoder(...)`` on the module
    path followed by ``load_state()``, is the supported one, and
    ``receptive_length`` need not be a multiple of ``chunk`` -- and
    ``store_state()`` writes the carries back as pad_buffers in the reference's
    shapes.  The packed weights are those of the pack cache when the session is
    built; build a new session after the weights change.

    ``graph=True``: ``encode`` and ``decode`` are each one captured graph on a
    single stream (warm-up on a side stream, then capture); ``graph=False``
    issues the same launches eagerly.  Both produce the same bits.
    ``dtype=None`` follows ``sel.convops.compute_dtype()``.
    """

    def __init__(self, generator, batch=1, chunk=300, graph=True, dtype=None):
        self.generator = generator
        # whose codebooks quantize / lookup use (a receiver decodes with one
        # generator and looks codes up in its copy of the encoder's: utils/audiodec.py)
        self.lookup_generator = generator
        self.plan = SO.plan(generator, batch, chunk)
        self.dtype = dtype or CO.compute_dtype()
        p = next(generator.parameters())
        L.need_device(p)
        L.lib()
        dev = p.device
        pl = self.plan
        with torch.no_grad():
            self._enc = _Half(pl.encode, generator, batch, pl.in_channels, self.dtype, dev)
            self._dec = _Half(pl.decode, generator, batch, pl.dec_in_channels, self.dtype, dev)
            self._halves = (self._enc, self._dec)
            if hasattr(generator, "quantizer") and not hasattr(generator.quantizer.codebook, "codebook_size"):
                generator.quantizer.initial()
            self._capture(graph)

    # ---- the four methods of the reference's streamer -------------------------
    @torch.no_grad()
    def encode(self, x):
        """x (batch, in_channels, chunk) -> z (batch, code_dim, frames) fp32 (without
        PQC: the encoder output in the compute dtype)."""
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (pl.batch, pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: session encode takes {(pl.batch, pl.in_channels, pl.chunk)}, got {tuple(x.shape)}")
        self._enc.inp.copy_(x.transpose(1, 2))
        return self._enc.run().view(pl.batch, pl.frames, pl.enc_channels).transpose(1, 2)

    @torch.no_grad()
    def quantize(self, z):
        """z -> flattened code indices (sel_rvq_fwd, as StreamGenerator.quantize)."""
        return self.lookup_generator.quantize(z)

    @torch.no_grad()
    def lookup(self, idx):
        zq = self.lookup_generator.lookup(idx)
        return zq.reshape(self.plan.batch, self.plan.frames, zq.shape[-1])

    @torch.no_grad()
    def decode(self, zq):
        """zq (batch, frames, code_dim) -- without PQC (batch, channels, frames) --
        -> y (batch, out_channels, samples) fp32."""
        pl = self.plan
        L.need_device(zq)
        src = zq if pl.pqc else zq.transpose(1, 2)
        if tuple(src.shape) != (pl.batch, pl.frames, pl.dec_in_channels):
            raise L.SelError(f"sel: session decode takes {pl.frames} frames of {pl.dec_in_channels} channels "
                             f"for {pl.batch} streams, got {tuple(zq.shape)}")
        self._dec.inp.copy_(src)
        return self._dec.run().view(pl.batch, pl.out_samples, pl.out_channels).transpose(1, 2)


class _VocoderHalf(_Half):
    """The launches of a vocoder ``decode`` on fixed buffers: _Half on the grouped step kernel."""
    _step = staticmethod(SO.hfg_conv_step)

    @staticmethod
    def _weights(generator, st, dtype):
        from . import hfgops as HF
        m = generator.get_submodule(st.conv)
        return HF.packed(m, st.kind, st.stride, dtype), m.bias.detach().float().contiguous() if st.bias_period else None


class VocoderSession(_SessionBase):
    """The receiver's streaming state for a HiFi-GAN vocoder ``StreamGenerator``:
    ``batch`` parallel streams, ``frames`` code frames per hop.

    ``decode(c)`` takes what ``StreamGenerator.decode`` takes, (batch, frames,
    in_channels), and returns (batch, out_channels, frames * prod(upsample_scales))
    fp32 -- a VIEW of the session's fixed output buffer, valid until the next
    ``decode`` (clone what must outlive it).  ``decode_norm`` (the generator's
    ``stats``) is applied while the input buffer is filled, outside the graph.
    ``lookup(idx)`` goes through ``lookup_generator`` (the receiver's copy of the
    encoder, set by utils/audiodec.py) and returns (batch, frames, code_dim).

    State as StreamSession: every carry starts at zero (``reset()``);
    ``load_state()`` copies the generator's pad_buffers in (the reference's
    warm-up, ``G.initial_decoder(...)`` on the module path, then ``load_state()``)
    and ``store_state()`` writes the carries back as fp32 pad_buffers in the
    reference's shapes.  The packed weights (weight norm folded) are those of
    sel.hfgops' pack cache when the session is built; build a new session after
    the weights change.

    ``graph=True``: a hop is one captured graph on a single stream -- the three
    independent MultiReceptiveField blocks of v0 are issued in order on it, no
    side streams (warm-up on a side stream, then capture, then ``reset()``);
    ``graph=False`` issues the same launches eagerly.  Both produce the same bits.
    ``dtype=None`` follows ``sel.convops.compute_dtype()``.
    """

    def __init__(self, generator, batch=1, frames=1, graph=True, dtype=None):
        self.generator = generator
        self.lookup_generator = None
        self.plan = SO.plan_vocoder(generator, batch, frames)
        self.dtype = dtype or CO.compute_dtype()
        p = next(generator.parameters())
        L.need_device(p)
        L.lib()
        pl = self.plan
        with torch.no_grad():
            self._dec = _VocoderHalf(pl.steps, generator, batch, pl.in_channels, self.dtype, p.device)
            self._halves = (self._dec,)
            self._capture(graph)

    @torch.no_grad()
    def lookup(self, idx):
        if self.lookup_generator is None:
            raise L.SelError("sel: this VocoderSession has no lookup_generator (the generator whose codebooks "
                             "decode the indices)")
        zq = self.lookup_generator.lookup(idx)
        return zq.reshape(self.plan.batch, self.plan.frames, zq.shape[-1])

    @torch.no_grad()
    def decode(self, c):
        """c (batch, frames, in_channels) -> y (batch, out_channels, samples) fp32."""
        pl = self.plan
        L.need_device(c)
        if tuple(c.shape) != (pl.batch, pl.frames, pl.in_channels):
            raise L.SelError(f"sel: session decode takes {(pl.batch, pl.frames, pl.in_channels)}, got {tuple(c.shape)}")
        self._dec.inp.copy_(self.generator.decode_norm(c))
        return self._dec.run().view(pl.batch, pl.out_samples, pl.out_channels).transpose(1, 2)

# ---- stream pools: independent streams on the slot-indexed step kernels -------------------------
class _Stager:
    """The per-tick control words of a pool: ``[n, slot_0, slot_1, ...]`` goes
    from pinned host memory into a fixed device buffer with one asynchronous
    copy on the current stream, outside the graph.  The pinned side is a small
    ring; an entry is reused only after the event recorded behind its last copy
    has completed, so a pending copy never sees its source overwritten."""
    RING = 4

    def __init__(self, width, device):
        self.width = width
        self.host = [torch.zeros(width, dtype=torch.int32).pin_memory() for _ in range(self.RING)]
        self.events = [None] * self.RING
        self.turn = 0
        self.device = device

    def stage(self, dst, words):
        if len(words) > self.width or dst.numel() > self.width:
            raise L.SelError(f"sel: {len(words)} control words for a staging ring of {self.width}")
        k = self.turn
        self.turn = (k + 1) % self.RING
        if self.events[k] is not None:
            self.events[k].synchronize()
        h = self.host[k]
        h.zero_()
        h[:len(words)] = torch.tensor(words, dtype=torch.int32)
        dst.copy_(h[:dst.numel()], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.events[k] = ev


class _PoolMixin:
    """What _PoolHalf and _VocoderPoolHalf add to their session halves: carry
    pools of capacity + 1 slot rows, the device control words and the
    slot-indexed launches."""

    def _make_pool(self, capacity, device):
        self.capacity = capacity
        self.nslots = capacity + 1          # row `capacity` is the template
        # [n, slots...] and, behind them, room for two per-stream arrays of a datagram
        # tick (budgets and hop numbers, or loss flags): one tensor, so one copy stages a tick
        self.ctl_all = torch.zeros(1 + 3 * capacity, dtype=torch.int32, device=device)
        self.ctl = self.ctl_all[:1 + capacity]
        self.n_active, self.slots = self.ctl[:1], self.ctl[1:]
        for lst in (self.carry, self.carry_out):
            for i, c in enumerate(lst):
                if c is not None:
                    lst[i] = torch.zeros((self.nslots,) + tuple(c.shape[1:]), dtype=c.dtype, device=device)
        self.pairs = [(o, c) for o, c in zip(self.carry_out, self.carry) if c is not None]

    def _launch_steps(self):
        step = self._step
        for i, st in enumerate(self.steps):
            step(self.descs[i], self.carry[i], self.carry_out[i], self.slots, self.n_active, self._buf(st.src),
                 self.wps[i], self.biases[i], None if st.res is None else self._buf(st.res), self.outs[i],
                 nslots=self.nslots)
        SO.copy_slots(self.pairs, self.slots, self.slots, self.n_active)


class _PoolHalf(_PoolMixin, _Half):
    _step = staticmethod(SO.conv_step_pool)

    def __init__(self, steps, generator, capacity, in_channels, dtype, device):
        _Half.__init__(self, steps, generator, capacity, in_channels, dtype, device)
        self._make_pool(capacity, device)


class _VocoderPoolHalf(_PoolMixin, _VocoderHalf):
    _step = staticmethod(SO.hfg_conv_step_pool)

    def __init__(self, steps, generator, capacity, in_channels, dtype, device):
        _VocoderHalf.__init__(self, steps, generator, capacity, in_channels, dtype, device)
        self._make_pool(capacity, device)


class _PoolBase(_CodesMixin):
    """Slots, the template row, staging and opening: shared by StreamPool and VocoderPool."""

    def _init_pool(self, capacity, halves, device):
        self.capacity = int(capacity)
        self.table = SO.SlotTable(capacity)
        self._halves = halves
        # the ring carries a tick's [n, slots...] (1 + capacity words; a datagram tick's
        # two further arrays of capacity words) and open()'s three words below
        self._stager = _Stager(1 + 3 * self.capacity, device)
        self._dgram_stager = self._stager
        # opening a stream: [1, capacity (the template row), the new slot]
        self._open_ctl = torch.zeros(3, dtype=torch.int32, device=device)
        self._carries = [c for h in halves for c in h.carry if c is not None]

    def _capture(self, graph):
        self.graphed = bool(graph)
        if graph:
            # n_active = 0: every block of every launch returns at once, so the
            # warm-up hops and the capture itself leave no state behind
            for h in self._halves:
                h.ctl.zero_()
                h.capture()

    def _stage(self, half, slots):
        slots = self.table.check(slots)
        self._stager.stage(half.ctl, [len(slots)] + slots)
        return len(slots)

    def _prepare_codes(self, half):
        # n_active = 0: the warm-up launch and the capture touch no row
        if half.graph is not None:
            half.ctl.zero_()

    # ---- the hooks of the per-hop methods (_CodesMixin): a slot list in front, n of capacity rows ----
    def _begin(self, which, args, opt=None, takes_opt=False):
        if len(args) != 2:
            opt = self._optional(which, args, 2, opt, takes_opt)
        return args[0], args[1], opt

    def _what(self, which, n):
        return f"pool {which} for {n} slots"

    @staticmethod
    def _idx_view(idx):
        return idx

    def _dgram_words(self, half, B, arrays, device):
        # behind the slot list, in the tensor the half's graphs already read: a tick is one copy
        cap = self.capacity
        views = [half.ctl_all[1 + (1 + i) * cap:1 + (2 + i) * cap] for i in range(arrays)]
        return half.ctl_all[:1 + (1 + arrays) * cap], views

    def _stage_dgram(self, hop, slots, *arrays):
        """[n, slots..., array 0..., array 1...], each padded to capacity, in one copy."""
        pad = [0] * (self.capacity - len(slots))
        words = [len(slots)] + slots + pad
        for a in arrays:
            words += a + pad
        self._stager.stage(hop.ctl, words)

    def _stage_budgets(self, hop, slots, budgets):
        self._stage_dgram(hop, slots, budgets, [self._seq[s] & 0xFFFF for s in slots])
        for s in slots:
            self._seq[s] += 1

    def _sent(self, hop, budgets):
        """the hop numbers are host words, staged with every tick"""

    def datagram_stats(self, slot):
        """The counters of a session's ``datagram_stats()`` for one open slot, since its ``open()``."""
        if not self._dgram_enabled:
            raise L.SelError("sel: datagram_stats needs enable_codes(datagrams=True) first")
        slot, = self.table.check([slot])
        return dict(self._dstats[slot])

    @torch.no_grad()
    def open(self):
        """A free slot (the lowest), its state copied from the template row in one launch."""
        slot = self.table.open()
        try:
            self._stager.stage(self._open_ctl, [1, self.capacity, slot])
            c = self._open_ctl
            SO.copy_slots([(t, t) for t in self._carries], c[1:2], c[2:3], c[0:1])
            self._clear_stream(slot)    # hop number 0, and nothing held from the slot's previous stream
        except BaseException:
            self.table.close(slot)      # the slot is taken only once its state is in place
            raise
        return slot

    def close(self, slot):
        self.table.close(slot)

    def state(self, slot):
        """{pad_buffer key: (P, C) carry of the slot, channels-last} -- a view, for inspection."""
        slot, = self.table.check([slot])
        return {st.buffer: c[slot] for st, c, _ in self._layers()}

    @torch.no_grad()
    def reset_template(self):
        """New streams start from zero state."""
        for c in self._carries:
            c[self.capacity].zero_()

    @torch.no_grad()
    def load_state(self):
        """template <- the generator's pad_buffers ((1, C, P)), as a session's load_state fills a carry."""
        for st, c, m in self._layers():
            _fill_carry(st, c[self.capacity], self._pad_rows(st, m, (1,), "the pool's template holds {}")[0])


class StreamPool(_PoolBase):
    """``capacity`` independent streams of one AudioDec ``StreamGenerator``,
    ``chunk`` samples per hop: streams open and close at any time, and on every
    tick one batched hop runs over whichever slots have a hop ready.  Every
    stream's output equals, bit for bit, what a solo ``batch=1`` session gives
    on the same hops.

    ``slot = open()`` / ``close(slot)``; per tick, for a list ``slots`` of n
    distinct open slots: ``encode(slots, x)`` with x (n, in_channels, chunk) ->
    z (n, code_dim, frames); ``quantize(z)`` -> idx (codebooks, n, frames);
    ``lookup(idx)`` -> (n, frames, dim); ``decode(slots, zq)`` -> y (n,
    out_channels, samples).  Sample i of every tensor belongs to ``slots[i]``.
    The tensors ``encode`` and ``decode`` return are VIEWS of the first n samples
    of the pool's fixed buffers, valid until the next call of the same method.

    The plan is that of a session of ``batch = capacity``.  Every carry and its
    ``carry_out`` twin holds capacity + 1 slot rows; row ``capacity`` is the
    TEMPLATE a newly opened stream starts from: zero after construction and
    ``reset_template()``, the generator's pad_buffers (the reference's warm-up)
    after ``load_state()``.  ``state(slot)`` shows a stream's carries.

    ``graph=True``: each half is one graph captured once at capacity (with no
    active stream, so the capture leaves no state behind).  Per tick the list
    and its length go through pinned host memory (a ring of four entries, each
    guarded by an event) into fixed device words with one asynchronous copy on
    the current stream, before the replay and outside the graph; the kernels
    read them, so one graph serves every active set.  ``graph=False`` issues the
    same launches eagerly; both produce the same bits."""

    def __init__(self, generator, capacity, chunk=300, graph=True, dtype=None):
        self.generator = generator
        self.lookup_generator = generator
        self.plan = SO.plan(generator, capacity, chunk)
        self.dtype = dtype or CO.compute_dtype()
        p = next(generator.parameters())
        L.need_device(p)
        L.lib()
        pl = self.plan
        with torch.no_grad():
            self._enc = _PoolHalf(pl.encode, generator, capacity, pl.in_channels, self.dtype, p.device)
            self._dec = _PoolHalf(pl.decode, generator, capacity, pl.dec_in_channels, self.dtype, p.device)
            if hasattr(generator, "quantizer") and not hasattr(generator.quantizer.codebook, "codebook_size"):
                generator.quantizer.initial()
            self._init_pool(capacity, (self._enc, self._dec), p.device)
            self._capture(graph)

    @torch.no_grad()
    def encode(self, slots, x):
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (len(slots), pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: pool encode takes {(len(slots), pl.in_channels, pl.chunk)} for {len(slots)} "
                             f"slots, got {tuple(x.shape)}")
        n = self._stage(self._enc, slots)
        self._enc.inp[:n].copy_(x.transpose(1, 2))
        out = self._enc.run()
        return out.view(self.capacity, pl.frames, pl.enc_channels)[:n].transpose(1, 2)

    @torch.no_grad()
    def quantize(self, z):
        """z (n, code_dim, frames) -> flattened code indices (codebooks, n, frames)."""
        idx = self.lookup_generator.quantize(z)
        return idx.view(idx.shape[0], z.shape[0], z.shape[2])

    @torch.no_grad()
    def lookup(self, idx):
        zq = self.lookup_generator.lookup(idx)
        return zq.reshape(-1, self.plan.frames, zq.shape[-1])

    @torch.no_grad()
    def decode(self, slots, zq):
        pl = self.plan
        L.need_device(zq)
        src = zq if pl.pqc else zq.transpose(1, 2)
        if tuple(src.shape) != (len(slots), pl.frames, pl.dec_in_channels):
            raise L.SelError(f"sel: pool decode takes {pl.frames} frames of {pl.dec_in_channels} channels for "
                             f"{len(slots)} slots, got {tuple(zq.shape)}")
        n = self._stage(self._dec, slots)
        self._dec.inp[:n].copy_(src)
        out = self._dec.run()
        return out.view(self.capacity, pl.out_samples, pl.out_channels)[:n].transpose(1, 2)


class VocoderPool(_PoolBase):
    """``capacity`` independent streams of one HiFi-GAN vocoder ``StreamGenerator``,
    ``frames`` code frames per hop: StreamPool's slots, template row, staging and
    graph for ``decode(slots, c)`` with c (n, frames, in_channels) -> y (n,
    out_channels, samples) fp32, a VIEW of the first n samples of the fixed output
    buffer.  ``decode_norm`` (the generator's ``stats``) is applied while the
    input buffer is filled; ``lookup(idx)`` goes through ``lookup_generator`` and
    returns (n, frames, code_dim)."""

    def __init__(self, generator, capacity, frames=1, graph=True, dtype=None):
        self.generator = generator
        self.lookup_generator = None
        self.plan = SO.plan_vocoder(generator, capacity, frames)
        self.dtype = dtype or CO.compute_dtype()
        p = next(generator.parameters())
        L.need_device(p)
        L.lib()
        pl = self.plan
        with torch.no_grad():
            self._dec = _VocoderPoolHalf(pl.steps, generator, capacity, pl.in_channels, self.dtype, p.device)
            self._init_pool(capacity, (self._dec,), p.device)
            self._capture(graph)

    @torch.no_grad()
    def lookup(self, idx):
        if self.lookup_generator is None:
            raise L.SelError("sel: this VocoderPool has no lookup_generator (the generator whose codebooks "
                             "decode the indices)")
        zq = self.lookup_generator.lookup(idx)
        return zq.reshape(-1, self.plan.frames, zq.shape[-1])

    @torch.no_grad()
    def decode(self, slots, c):
        pl = self.plan
        L.need_device(c)
        if tuple(c.shape) != (len(slots), pl.frames, pl.in_channels):
            raise L.SelError(f"sel: pool decode takes {(len(slots), pl.frames, pl.in_channels)} for {len(slots)} "
                             f"slots, got {tuple(c.shape)}")
        n = self._stage(self._dec, slots)
        self._dec.inp[:n].copy_(self.generator.decode_norm(c))
        out = self._dec.run()
        return out.view(self.capacity, pl.out_samples, pl.out_channels)[:n].transpose(1, 2)
