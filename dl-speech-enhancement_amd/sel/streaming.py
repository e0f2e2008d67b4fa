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
"""
import functools

import torch

from . import _lib as L
from . import convops as CO
from . import streamops as SO
from .wire import WireFormat


class _Half:
    """The launches of one method (encode or decode) on fixed buffers."""

    def __init__(self, steps, generator, batch, in_channels, dtype, device):
        params = dict(generator.named_parameters())
        self.steps = steps
        self.batch = batch
        T0 = steps[0].T * (steps[0].stride if steps[0].kind == CO.PACK_FWD_STRIDED else 1)
        self.inp = torch.zeros((batch, T0, in_channels), dtype=dtype, device=device)
        self.descs, self.wps, self.biases, self.outs = [], [], [], []
        self.carry, self.carry_out = [], []
        for st in steps:
            w = params[st.weight]
            L.need_device(w)
            self.descs.append(st.desc(batch))
            self.wps.append(CO.PACKS.get(st.kind, w, st.stride, dtype)[0])
            self.biases.append(params[st.bias].detach().float().contiguous() if st.bias else None)
            self.outs.append(torch.zeros((batch * st.T, st.N), dtype=torch.float32 if st.out_float else dtype,
                                         device=device))
            if st.carry_shape is None:
                self.carry.append(None)
                self.carry_out.append(None)
            else:
                self.carry.append(torch.zeros(st.carry_shape, dtype=dtype, device=device))
                self.carry_out.append(torch.zeros(st.carry_shape, dtype=dtype, device=device))
        self.pairs = [(o, c) for o, c in zip(self.carry_out, self.carry) if c is not None]
        self.graph = None

    def _buf(self, i):
        return self.inp if i == -1 else self.outs[i]

    def launch(self):
        for i, st in enumerate(self.steps):
            SO.conv_step(self.descs[i], self.carry[i], self._buf(st.src), self.wps[i], self.biases[i],
                         None if st.res is None else self._buf(st.res), self.outs[i], self.carry_out[i])
        SO.commit(self.pairs)

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
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.launch()

    def run(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self.launch()
        return self.outs[-1]

    def zero(self):
        for c in self.carry:
            if c is not None:
                c.zero_()

    # ---- code indices inside the hop (enable_codes) --------------------------------
    pre = post = codes_graph = idx = None
    pre_wire = wire_graph = wire_buf = None

    def add_codes(self, idx, pre=None, post=None, wire_buf=None, pre_wire=None):
        """Extend the hop by a stateless launch in front of it (``pre``: the lookup
        into ``inp``) or behind it (``post``: the quantizer on ``outs[-1]``), as a
        second launch list beside ``launch`` -- and, for a captured half, a second
        graph beside ``graph``.  Only the new launch is warmed up eagerly (it has
        no state); the capture itself executes nothing, so no carry moves.
        ``wire_buf``: the fixed (rows, frame_bytes) packet buffer -- ``post`` then
        writes it beside ``idx``; ``pre_wire``, the lookup out of it, heads a third
        launch list (and graph) beside ``pre``'s."""
        self.idx, self.pre, self.post = idx, pre, post
        self.wire_buf, self.pre_wire = wire_buf, pre_wire
        self.codes_graph = self.wire_graph = None
        if self.graph is not None:
            (pre or post)()
            if pre_wire is not None:
                pre_wire()
            torch.cuda.synchronize(self.inp.device)
            self.codes_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.codes_graph):
                self.launch_codes(self.pre)
            if pre_wire is not None:
                self.wire_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.wire_graph):
                    self.launch_codes(self.pre_wire)

    def launch_codes(self, pre):
        if pre is not None:
            pre()
        self.launch()
        if self.post is not None:
            self.post()

    def run_codes(self):
        if self.codes_graph is not None:
            self.codes_graph.replay()
        else:
            self.launch_codes(self.pre)
        return self.outs[-1]

    def run_wire(self):
        """The receiver's hop from the packet buffer: lookup_wire_step -> steps -> commit."""
        if self.wire_graph is not None:
            self.wire_graph.replay()
        else:
            self.launch_codes(self.pre_wire)
        return self.outs[-1]

    # ---- datagrams inside the hop (enable_codes(datagrams=True)) ---------------------
    pre_dgram = post_dgram = dgram_graph = dgram_buf = dgram_ctl = hold = None
    dgram_staged = None       # sessions: the control words the device holds (None: unknown)

    def add_datagrams(self, buf, ctl, pre=None, post=None, hold=None):
        """A further launch list beside the others, ``pre -> steps -> commit`` (the
        receiver: lookup_dgram_step out of ``buf``) or ``steps -> commit -> post``
        (the transmitter: rvq_step_dgram into ``buf``), and for a captured half a
        further graph.  ``ctl``: the device control words the new launch reads
        (budgets and hop numbers, or loss flags), staged before every replay.
        ``hold``: the receiver's per-stream held records.  As in ``add_codes`` only
        the new stateless launch is warmed up and the capture executes nothing."""
        self.dgram_buf, self.dgram_ctl, self.pre_dgram, self.post_dgram, self.hold = buf, ctl, pre, post, hold
        self.dgram_graph = self.dgram_staged = None
        if self.graph is not None:
            (pre or post)()
            torch.cuda.synchronize(self.inp.device)
            self.dgram_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.dgram_graph):
                self.launch_dgram()

    def launch_dgram(self):
        if self.pre_dgram is not None:
            self.pre_dgram()
        self.launch()
        if self.post_dgram is not None:
            self.post_dgram()

    def run_dgram(self):
        if self.dgram_graph is not None:
            self.dgram_graph.replay()
        else:
            self.launch_dgram()
        return self.outs[-1]


def _fill_idx(dst, idx, what):
    """idx (S, [batch,] frames) int64 -> the fixed (S, rows) buffer (or its first rows)."""
    L.need_device(idx)
    if idx.dtype != torch.int64 or idx.dim() < 2 or idx.shape[0] != dst.shape[0] or idx.numel() != dst.numel():
        raise L.SelError(f"sel: {what} takes int64 indices of {dst.shape[0]} codebooks x {dst.shape[1]} frames, "
                         f"got {idx.dtype} {tuple(idx.shape)}")
    dst.copy_(idx.reshape(dst.shape))


def _fill_packets(dst, p, what):
    """p (n, packet_bytes) uint8 -> the fixed packet buffer (or its first n packets)."""
    L.need_device(p)
    if p.dtype != torch.uint8 or tuple(p.shape) != tuple(dst.shape):
        raise L.SelError(f"sel: {what} takes uint8 packets of shape {tuple(dst.shape)}, got {p.dtype} {tuple(p.shape)}")
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
        dev = self._dec.inp.device
        frames = self.plan.frames
        self._tx = self._rx = self.wire = self.datagram = None
        self._seq = self._dstats = None
        self._dgram_enabled = False
        fmt, dfmt = [], []
        enc = getattr(self, "_enc", None)
        if enc is not None and self.plan.pqc:
            rvq = self.generator.quantizer.codebook
            stack = torch.stack([l.embed.detach() for l in rvq.layers]).to(dev, torch.float32).contiguous().clone()
            z = enc.outs[-1]
            if z.dtype != torch.float32 or z.shape[1] != stack.shape[1]:
                raise L.SelError(f"sel: encode's output rows {z.dtype} {tuple(z.shape)} are not the fp32 code vectors "
                                 f"of a (S, D, K) = {tuple(stack.shape)} quantizer")
            idx = torch.zeros((stack.shape[0], z.shape[0]), dtype=torch.int64, device=dev)
            count = getattr(enc, "n_active", None)
            self._prepare_codes(enc)
            if wire:
                fmt.append(WireFormat(stack.shape[0], stack.shape[2], frames))
                buf = torch.zeros((z.shape[0], fmt[-1].frame_bytes), dtype=torch.uint8, device=dev)
                enc.add_codes(idx, post=functools.partial(SO.rvq_step_wire, z, stack, buf, frames, count, True, idx),
                              wire_buf=buf)
            else:
                enc.add_codes(idx, post=functools.partial(SO.rvq_step, z, stack, idx, frames, count, True))
            if datagrams:
                dfmt.append(self._datagram_format(stack.shape[0], stack.shape[2], frames))
                B = z.shape[0] // frames
                dbuf = torch.zeros((B, dfmt[-1].stride), dtype=torch.uint8, device=dev)
                ctl, (stages, seq) = self._dgram_words(enc, B, 2, dev)
                post = functools.partial(SO.rvq_step_dgram, z, stack, dbuf, frames, count, stages, seq, True)
                if count is None:
                    # a session (no slot list to stage): the hop numbers advance on the device, behind
                    # the launch that read them, so a steady budget needs no control copy per hop
                    def post(launch=post, seq=seq):
                        launch()
                        seq.add_(1)
                enc.add_datagrams(dbuf, ctl, post=post)
            self._tx = enc
        lg = lookup_generator if lookup_generator is not None else self.lookup_generator
        dec = self._dec
        if lg is not None and (enc is None or self.plan.pqc):
            rvq = lg.quantizer.codebook
            if not hasattr(rvq, "codebook_size"):
                lg.quantizer.initial()
            flat = rvq.codebook.detach().to(dev, torch.float32).contiguous().clone()
            S = len(rvq.layers)
            if dec.inp.shape[-1] != flat.shape[1]:
                raise L.SelError(f"sel: the lookup codebook has {flat.shape[1]} channels, decode takes "
                                 f"{dec.inp.shape[-1]}")
            idx = torch.zeros((S, dec.inp.shape[0] * frames), dtype=torch.int64, device=dev)
            mean = scale = None
            if getattr(self.generator, "norm", False):
                mean = self.generator.mean.detach().to(dev, torch.float32).contiguous().clone()
                scale = self.generator.scale.detach().to(dev, torch.float32).contiguous().clone()
            count = getattr(dec, "n_active", None)
            self._prepare_codes(dec)
            pre = functools.partial(SO.rvq_lookup_step, idx, flat, dec.inp, frames, mean, scale, count)
            if wire:
                if flat.shape[0] % S:
                    raise L.SelError(f"sel: the lookup codebook's {flat.shape[0]} rows are not {S} stages of one size")
                fmt.append(WireFormat(S, flat.shape[0] // S, frames))
                buf = torch.zeros((idx.shape[1], fmt[-1].frame_bytes), dtype=torch.uint8, device=dev)
                dec.add_codes(idx, pre=pre, wire_buf=buf,
                              pre_wire=functools.partial(SO.rvq_lookup_wire_step, buf, flat, S, dec.inp, frames, mean,
                                                         scale, count))
            else:
                dec.add_codes(idx, pre=pre)
            if datagrams:
                if flat.shape[0] % S:
                    raise L.SelError(f"sel: the lookup codebook's {flat.shape[0]} rows are not {S} stages of one size")
                dfmt.append(self._datagram_format(S, flat.shape[0] // S, frames))
                B = dec.inp.shape[0]
                dbuf = torch.zeros((B, dfmt[-1].stride), dtype=torch.uint8, device=dev)
                # a stream's last good record, at a fixed address: one row per batch stream / pool slot
                hold = torch.zeros((B, 1 + dfmt[-1].frame_bytes()), dtype=torch.uint8, device=dev)
                ctl, (lost,) = self._dgram_words(dec, B, 1, dev)
                dec.add_datagrams(dbuf, ctl, hold=hold,
                                  pre=functools.partial(SO.rvq_lookup_dgram_step, dbuf, flat, S, dec.inp, frames, mean,
                                                        scale, count, getattr(dec, "slots", None), lost, hold))
            self._rx = dec
        for f in (fmt, dfmt):
            if len(f) == 2 and (f[0].codebooks, f[0].codebook_size) != (f[1].codebooks, f[1].codebook_size):
                raise L.SelError(f"sel: the transmitter packs {f[0]!r}, the lookup codebook reads {f[1]!r}")
        if fmt:
            self.wire = fmt[0]
        if dfmt:
            self.datagram = dfmt[0]
            streams = self._dec.inp.shape[0]
            self._seq = [0] * streams
            self._dstats = [self._new_stats() for _ in range(streams)]
        self._codes_enabled, self._wire_enabled, self._dgram_enabled = True, bool(wire), bool(datagrams)

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

    def _stage_list(self, what, stages, n):
        """``stages``: None (all), an int, or one int per stream, each in [1, S] -> a list of n ints."""
        S = self.datagram.codebooks
        if stages is None:
            return [S] * n
        if isinstance(stages, torch.Tensor):
            if stages.dim() > 1 or stages.dtype not in (torch.int32, torch.int64):
                raise L.SelError(f"sel: {what} takes stages as an int or {n} ints, got {stages.dtype} "
                                 f"{tuple(stages.shape)}")
            stages = stages.tolist()
        raw = [stages] * n if isinstance(stages, int) and not isinstance(stages, bool) else list(stages) \
            if isinstance(stages, (list, tuple)) else None
        if raw is None or len(raw) != n:
            raise L.SelError(f"sel: {what} takes stages as an int or {n} ints, got {stages!r}")
        for s in raw:
            if not isinstance(s, int) or isinstance(s, bool) or not 1 <= s <= S:
                raise L.SelError(f"sel: {what}: a budget of {s!r} stages, the quantizer has 1..{S}")
        return raw

    def _take_datagrams(self, what, dst, p, lost, streams):
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
                raise L.SelError(f"sel: {what} takes uint8 datagrams of shape {tuple(dst.shape)}, got {p.dtype} "
                                 f"{tuple(p.shape)}")
            flags = self._flag_list(what, lost, n)
            dst.copy_(p)
        elif isinstance(p, (list, tuple)):
            if len(p) != n or any(d is not None and not isinstance(d, (bytes, bytearray, memoryview)) for d in p):
                raise L.SelError(f"sel: {what} takes {n} datagrams, each bytes-like or None")
            buf, gone, refused = fmt.assemble(p)
            flags = [int(a or b) for a, b in zip(gone, self._flag_list(what, lost, n))]
            heads = [None if f else fmt.parse(d) for f, d in zip(gone, p)]
            dst.copy_(buf)
        else:
            raise L.SelError(f"sel: {what} takes a device uint8 tensor or a list of bytes-like / None entries, got "
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

    @staticmethod
    def _flag_list(what, lost, n):
        if lost is None:
            return [0] * n
        if isinstance(lost, torch.Tensor):
            if lost.dim() != 1 or lost.dtype not in (torch.bool, torch.int32, torch.int64):
                raise L.SelError(f"sel: {what} takes lost as {n} flags, got {lost.dtype} {tuple(lost.shape)}")
            lost = lost.tolist()
        if not isinstance(lost, (list, tuple)) or len(lost) != n or \
                any(not isinstance(f, (bool, int)) for f in lost):
            raise L.SelError(f"sel: {what} takes lost as {n} flags, got {lost!r}")
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


class StreamSession(_CodesMixin):
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
            if hasattr(generator, "quantizer") and not hasattr(generator.quantizer.codebook, "codebook_size"):
                generator.quantizer.initial()
            self.graphed = bool(graph)
            if graph:
                self._enc.capture()
                self._dec.capture()
                self.reset()   # the warm-up hops ran on zero input; start from zero state

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

    # ---- the same with the code indices inside the hop (after enable_codes) -----
    @torch.no_grad()
    def transmit(self, x):
        """x (batch, in_channels, chunk) -> flattened code indices, int64, what
        ``quantize(encode(x))`` returns: one replay.  A VIEW of a fixed buffer,
        valid until the next ``transmit``."""
        half = self._codes_half("transmit")
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (pl.batch, pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: session transmit takes {(pl.batch, pl.in_channels, pl.chunk)}, got {tuple(x.shape)}")
        half.inp.copy_(x.transpose(1, 2))
        half.run_codes()
        return half.idx.view(-1, pl.batch, pl.frames).squeeze(1)

    @torch.no_grad()
    def receive(self, idx):
        """The indices ``transmit`` / ``quantize`` return -> y, what
        ``decode(lookup(idx))`` returns (the codes summed in stage order): one replay."""
        half = self._codes_half("receive")
        pl = self.plan
        _fill_idx(half.idx, idx, "session receive")
        return half.run_codes().view(pl.batch, pl.out_samples, pl.out_channels).transpose(1, 2)

    # ---- the same in the bytes of the wire format (after enable_codes(wire=True)) -----
    @torch.no_grad()
    def transmit_packets(self, x):
        """x (batch, in_channels, chunk) -> (batch, packet_bytes) uint8, ``self.wire``'s
        packing of what ``transmit(x)`` returns: one replay (the one ``transmit``
        runs).  A VIEW of a fixed buffer, valid until the next ``transmit`` /
        ``transmit_packets``."""
        half = self._codes_half("transmit_packets")
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (pl.batch, pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: session transmit_packets takes {(pl.batch, pl.in_channels, pl.chunk)}, got "
                             f"{tuple(x.shape)}")
        half.inp.copy_(x.transpose(1, 2))
        half.run_codes()
        return half.wire_buf.view(pl.batch, self.wire.packet_bytes)

    @torch.no_grad()
    def receive_packets(self, p):
        """p (batch, packet_bytes) uint8 -> y, what ``receive`` returns for the
        indices in the packets: one replay, with no index tensor in between."""
        half = self._codes_half("receive_packets")
        pl = self.plan
        _fill_packets(half.wire_buf.view(pl.batch, self.wire.packet_bytes), p, "session receive_packets")
        return half.run_wire().view(pl.batch, pl.out_samples, pl.out_channels).transpose(1, 2)

    # ---- the same in datagrams, wire version 2 (after enable_codes(datagrams=True)) -----
    @torch.no_grad()
    def transmit_datagrams(self, x, stages=None):
        """x (batch, in_channels, chunk) -> (batch, stride) uint8, ``stride =
        self.datagram.stride``: row i starts with stream i's datagram for this hop
        -- the header with the stages carried and the stream's hop number (0 after
        construction and ``reset()``, wrapping at 2^16), then the hop's records of
        ``stages`` fields -- ``self.datagram.datagram_bytes(stages[i])`` bytes; the
        bytes of a row beyond that are not written and keep what an earlier hop
        left there.  ``stages``: an int or one int per stream in [1, codebooks],
        default all; the quantizer's chain stops after that many stages.  One
        replay, whatever the budgets: they are device words, staged in front of it
        when they change (the hop numbers advance on the device, behind the
        quantizer's launch).  A VIEW of a fixed buffer: a call invalidates the view the previous
        ``transmit_datagrams`` returned and, like ``transmit``, ``encode``'s; the
        views of ``transmit`` / ``transmit_packets`` stay valid."""
        half = self._codes_half("transmit_datagrams")
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (pl.batch, pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: session transmit_datagrams takes {(pl.batch, pl.in_channels, pl.chunk)}, got "
                             f"{tuple(x.shape)}")
        budgets = self._stage_list("session transmit_datagrams", stages, pl.batch)
        self._stage_words(half, budgets + self._seq)
        half.dgram_staged = None                         # unknown until the hop has run
        half.inp.copy_(x.transpose(1, 2))
        half.run_dgram()
        # the hop's last launch added 1 to every hop number on the device: with the same budgets the
        # next hop finds its words in place (at the 2^16 wrap they differ, and are staged again)
        half.dgram_staged = budgets + [q + 1 for q in self._seq]
        self._seq = [(q + 1) & 0xFFFF for q in self._seq]
        return half.dgram_buf

    @torch.no_grad()
    def receive_datagrams(self, p, lost=None):
        """The datagrams of one hop -> y, what ``receive`` returns for the ids in
        them (-1 beyond the stages a datagram carries): one replay.  ``p``: a
        device uint8 (batch, stride) tensor as ``transmit_datagrams`` returns it,
        with ``lost``, one flag per stream, marking rows to disregard; or a list
        of ``batch`` entries, bytes-like or None for a datagram that did not
        arrive, which ``self.datagram.assemble`` turns into one host-to-device
        copy.  A lost stream -- flagged, None, or with a header this receiver
        refuses -- is concealed: every frame of the hop decodes the last frame's
        record of the stream's last good datagram (nothing held yet: the empty
        sum), so the decoder's carried state moves on.  Nothing is reordered: the
        caller decides which datagram belongs to which hop.  ``datagram_stats()``
        counts."""
        half = self._codes_half("receive_datagrams")
        pl = self.plan
        flags = self._take_datagrams("session receive_datagrams", half.dgram_buf, p, lost, range(pl.batch))
        self._stage_words(half, flags)
        return half.run_dgram().view(pl.batch, pl.out_samples, pl.out_channels).transpose(1, 2)

    def _stage_words(self, half, words):
        """A session half's control words, staged as a pool's slot list is -- unless the
        device already holds exactly these (a receiver that loses nothing stages nothing)."""
        if half.dgram_staged != words:
            self._dgram_stager.stage(half.dgram_ctl, words)
            half.dgram_staged = words

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

    def _reset_datagrams(self):
        for i in range(len(self._seq or ())):
            self._clear_stream(i)

    # ---- state ------------------------------------------------------------------
    def _layers(self):
        for half in (self._enc, self._dec):
            for st, c in zip(half.steps, half.carry):
                if c is not None:
                    yield st, c, self.generator.get_submodule(st.name)

    def carries(self):
        """{pad_buffer key: carry tensor (batch, P, C), channels-last} -- the live state."""
        return {st.buffer: c for st, c, _ in self._layers()}

    @torch.no_grad()
    def reset(self):
        self._enc.zero()
        self._dec.zero()
        self._reset_datagrams()

    @torch.no_grad()
    def load_state(self):
        """carries <- the generator's pad_buffers ((1 or batch, C, P), broadcast to batch)."""
        for st, c, m in self._layers():
            pb = m.pad_buffer
            if pb.shape[0] not in (1, c.shape[0]) or tuple(pb.shape[1:]) != tuple(st.buffer_shape[1:]):
                raise L.SelError(f"sel: {st.buffer} has shape {tuple(pb.shape)}, the session holds "
                                 f"{st.buffer_shape} per stream")
            rows = pb.to(c.device).transpose(1, 2).expand(c.shape[0], -1, -1)      # (batch, P_ref, Cin)
            if st.kind == CO.PACK_FWD_STRIDED:
                # 2s samples as 2 phase rows; the extra oldest sample meets a zero weight
                v = c.view(c.shape[0], 2 * st.stride, -1)
                v[:, :1].zero_()
                v[:, 1:].copy_(rows)
            else:
                c.copy_(rows)

    @torch.no_grad()
    def store_state(self):
        """The generator's pad_buffers <- carries, in the reference's shapes (fp32)."""
        for st, c, m in self._layers():
            v = c.view(c.shape[0], -1, st.buffer_shape[1])
            if st.kind == CO.PACK_FWD_STRIDED:
                v = v[:, 1:]
            m.pad_buffer = v.transpose(1, 2).float().contiguous()


class _VocoderHalf(_Half):
    """The launches of a vocoder ``decode`` on fixed buffers (capture / run / zero as _Half)."""

    def __init__(self, steps, generator, batch, in_channels, dtype, device):
        from . import hfgops as HF
        self.steps = steps
        self.batch = batch
        self.inp = torch.zeros((batch, steps[0].T, in_channels), dtype=dtype, device=device)
        self.descs, self.wps, self.biases, self.outs = [], [], [], []
        self.carry, self.carry_out = [], []
        for i, st in enumerate(steps):
            m = generator.get_submodule(st.conv)
            self.descs.append(st.desc(batch))
            self.wps.append(HF.packed(m, st.kind, st.stride, dtype))
            self.biases.append(m.bias.detach().float().contiguous() if st.bias_period else None)
            if st.out != i:
                self.outs.append(self.outs[st.out])    # accumulates into an earlier step's buffer
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
        self.graph = None

    def launch(self):
        for i, st in enumerate(self.steps):
            SO.hfg_conv_step(self.descs[i], self.carry[i], self._buf(st.src), self.wps[i], self.biases[i],
                             None if st.res is None else self._buf(st.res), self.outs[i], self.carry_out[i])
        SO.commit(self.pairs)


class VocoderSession(_CodesMixin):
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
            self.graphed = bool(graph)
            if graph:
                self._dec.capture()
                self.reset()   # the warm-up hops ran on zero input; start from zero state

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

    # after enable_codes(): lookup, decode_norm and decode as one replay (transmit: always a SelError)
    transmit = StreamSession.transmit
    receive = StreamSession.receive
    transmit_packets = StreamSession.transmit_packets
    receive_packets = StreamSession.receive_packets
    transmit_datagrams = StreamSession.transmit_datagrams
    receive_datagrams = StreamSession.receive_datagrams
    datagram_stats = StreamSession.datagram_stats
    _reset_datagrams = StreamSession._reset_datagrams
    _stage_words = StreamSession._stage_words

    # ---- state ------------------------------------------------------------------
    def _layers(self):
        for st, c in zip(self._dec.steps, self._dec.carry):
            if c is not None:
                yield st, c, self.generator.get_submodule(st.name)

    def carries(self):
        """{pad_buffer key: carry tensor (batch, P, C), channels-last} -- the live state."""
        return {st.buffer: c for st, c, _ in self._layers()}

    @torch.no_grad()
    def reset(self):
        self._dec.zero()
        self._reset_datagrams()

    @torch.no_grad()
    def load_state(self):
        """carries <- the generator's pad_buffers ((1 or batch, C, P), broadcast to batch)."""
        for st, c, m in self._layers():
            pb = m.pad_buffer
            if pb.shape[0] not in (1, c.shape[0]) or tuple(pb.shape[1:]) != tuple(st.buffer_shape[1:]):
                raise L.SelError(f"sel: {st.buffer} has shape {tuple(pb.shape)}, the session holds "
                                 f"{st.buffer_shape} per stream")
            c.copy_(pb.to(c.device).transpose(1, 2).expand(c.shape[0], -1, -1))

    @torch.no_grad()
    def store_state(self):
        """The generator's pad_buffers <- carries, in the reference's shapes (fp32)."""
        for _, c, m in self._layers():
            m.pad_buffer = c.transpose(1, 2).float().contiguous()


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

    def launch(self):
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

    @torch.no_grad()
    def transmit(self, slots, x):
        """x (n, in_channels, chunk) for the n listed slots -> flattened code indices
        (codebooks, n, frames), what ``quantize(encode(slots, x))`` returns: one
        replay.  A VIEW of a fixed buffer, valid until the next ``transmit``."""
        half = self._codes_half("transmit")
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (len(slots), pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: pool transmit takes {(len(slots), pl.in_channels, pl.chunk)} for {len(slots)} "
                             f"slots, got {tuple(x.shape)}")
        n = self._stage(half, slots)
        half.inp[:n].copy_(x.transpose(1, 2))
        half.run_codes()
        return half.idx.view(-1, self.capacity, pl.frames)[:, :n]

    @torch.no_grad()
    def receive(self, slots, idx):
        """idx (codebooks, n, frames), what ``transmit`` / ``quantize`` return, for the
        n listed slots -> y (n, out_channels, samples), what ``decode(slots,
        lookup(idx))`` returns (the codes summed in stage order): one replay."""
        half = self._codes_half("receive")
        pl = self.plan
        n = self._stage(half, slots)
        _fill_idx(half.idx[:, :n * pl.frames], idx, f"pool receive for {n} slots")
        out = half.run_codes()
        return out.view(self.capacity, pl.out_samples, pl.out_channels)[:n].transpose(1, 2)

    @torch.no_grad()
    def transmit_packets(self, slots, x):
        """x (n, in_channels, chunk) for the n listed slots -> (n, packet_bytes) uint8,
        ``self.wire``'s packing of what ``transmit(slots, x)`` returns, packet i that
        of ``slots[i]``: one replay.  A VIEW of a fixed buffer, valid until the next
        ``transmit`` / ``transmit_packets``."""
        half = self._codes_half("transmit_packets")
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (len(slots), pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: pool transmit_packets takes {(len(slots), pl.in_channels, pl.chunk)} for "
                             f"{len(slots)} slots, got {tuple(x.shape)}")
        n = self._stage(half, slots)
        half.inp[:n].copy_(x.transpose(1, 2))
        half.run_codes()
        return half.wire_buf.view(self.capacity, self.wire.packet_bytes)[:n]

    @torch.no_grad()
    def receive_packets(self, slots, p):
        """p (n, packet_bytes) uint8, packet i for ``slots[i]`` -> y (n, out_channels,
        samples), what ``receive`` returns for the indices in the packets: one replay."""
        half = self._codes_half("receive_packets")
        pl = self.plan
        n = self._stage(half, slots)
        _fill_packets(half.wire_buf.view(self.capacity, self.wire.packet_bytes)[:n], p,
                      f"pool receive_packets for {n} slots")
        out = half.run_wire()
        return out.view(self.capacity, pl.out_samples, pl.out_channels)[:n].transpose(1, 2)

    # ---- the same in datagrams (after enable_codes(datagrams=True)) ------------------------------
    def _dgram_words(self, half, B, arrays, device):
        # behind the slot list, in the tensor the half's graphs already read: a tick is one copy
        cap = self.capacity
        views = [half.ctl_all[1 + (1 + i) * cap:1 + (2 + i) * cap] for i in range(arrays)]
        return half.ctl_all[:1 + (1 + arrays) * cap], views

    def _stage_dgram(self, half, slots, *arrays):
        """[n, slots..., array 0..., array 1...], each padded to capacity, in one copy."""
        pad = [0] * (self.capacity - len(slots))
        words = [len(slots)] + slots + pad
        for a in arrays:
            words += a + pad
        self._stager.stage(half.dgram_ctl, words)
        return len(slots)

    @torch.no_grad()
    def transmit_datagrams(self, slots, x, stages=None):
        """x (n, in_channels, chunk) for the n listed slots -> (n, stride) uint8, row i
        starting with the datagram of ``slots[i]`` for this hop, as a session's
        ``transmit_datagrams`` writes it; ``stages``: an int or one int per listed
        slot.  A slot's hop number starts at 0 at ``open()``.  One replay and one
        control copy, whatever the slots and budgets.  A VIEW of a fixed buffer: a
        call invalidates the view of the previous ``transmit_datagrams`` (and
        ``encode``'s); those of ``transmit`` / ``transmit_packets`` stay valid."""
        half = self._codes_half("transmit_datagrams")
        pl = self.plan
        L.need_device(x)
        if tuple(x.shape) != (len(slots), pl.in_channels, pl.chunk):
            raise L.SelError(f"sel: pool transmit_datagrams takes {(len(slots), pl.in_channels, pl.chunk)} for "
                             f"{len(slots)} slots, got {tuple(x.shape)}")
        slots = self.table.check(slots)
        budgets = self._stage_list("pool transmit_datagrams", stages, len(slots))
        n = self._stage_dgram(half, slots, budgets, [self._seq[s] & 0xFFFF for s in slots])
        for s in slots:
            self._seq[s] += 1
        half.inp[:n].copy_(x.transpose(1, 2))
        half.run_dgram()
        return half.dgram_buf[:n]

    @torch.no_grad()
    def receive_datagrams(self, slots, p, lost=None):
        """The datagrams of one tick, entry i for ``slots[i]`` -> y (n, out_channels,
        samples): a session's ``receive_datagrams`` per listed slot, each slot
        concealing its own lost hops from its own held record (cleared at
        ``open()``).  ``p``: a device uint8 (n, stride) tensor with optional
        ``lost`` flags, or a list of n bytes-like / None entries.  One replay."""
        half = self._codes_half("receive_datagrams")
        pl = self.plan
        slots = self.table.check(slots)
        n = len(slots)
        flags = self._take_datagrams(f"pool receive_datagrams for {n} slots", half.dgram_buf[:n], p, lost, slots)
        self._stage_dgram(half, slots, flags)
        out = half.run_dgram()
        return out.view(self.capacity, pl.out_samples, pl.out_channels)[:n].transpose(1, 2)

    def datagram_stats(self, slot):
        """The counters of a session's ``datagram_stats()`` for one open slot, since its ``open()``."""
        if not self._dgram_enabled:
            raise L.SelError("sel: datagram_stats needs enable_codes(datagrams=True) first")
        slot, = self.table.check([slot])
        return dict(self._dstats[slot])

    def _layers(self):
        for half in self._halves:
            for st, c in zip(half.steps, half.carry):
                if c is not None:
                    yield st, c, self.generator.get_submodule(st.name)

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

    def _template_rows(self, st, c, m):
        pb = m.pad_buffer
        if pb.shape[0] != 1 or tuple(pb.shape[1:]) != tuple(st.buffer_shape[1:]):
            raise L.SelError(f"sel: {st.buffer} has shape {tuple(pb.shape)}, the pool's template holds "
                             f"{st.buffer_shape}")
        return pb.to(c.device).transpose(1, 2)[0]      # (P_ref, Cin)


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

    @torch.no_grad()
    def load_state(self):
        """template <- the generator's pad_buffers ((1, C, P)), as StreamSession.load_state fills a carry."""
        for st, c, m in self._layers():
            rows = self._template_rows(st, c, m)
            t = c[self.capacity]
            if st.kind == CO.PACK_FWD_STRIDED:
                # 2s samples as 2 phase rows; the extra oldest sample meets a zero weight
                v = t.view(2 * st.stride, -1)
                v[:1].zero_()
                v[1:].copy_(rows)
            else:
                t.copy_(rows)


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

    @torch.no_grad()
    def load_state(self):
        """template <- the generator's pad_buffers ((1, C, P))."""
        for st, c, m in self._layers():
            c[self.capacity].copy_(self._template_rows(st, c, m))
