"""The wire format of the code indices, version 1 (include/sel.h): what a
transmitter sends per hop and a receiver takes, as bytes.

One record per code frame holds the S un-flattened codes ``k_s`` in ``[0, K)``:
field ``s`` occupies bits ``[s * bits, (s + 1) * bits)`` of the record, read as
a little-endian bit string (bit ``i`` of the record is bit ``i % 8`` of byte
``i // 8``), with ``bits = max(1, ceil(log2 K))``; the record is
``ceil(S * bits / 8)`` bytes and its pad bits are zero.  A stream's packet for
one hop is its ``frames`` records back to back.  No header, no sequence number.

On the GPU the records are written and read inside the hop
(``sel.streamops.rvq_step_wire`` / ``rvq_lookup_wire_step``,
``transmit_packets`` / ``receive_packets`` of sessions and pools).  ``pack`` and
``unpack`` here are the same format on CPU tensors, for the peer without a GPU.

Version 2, the datagram (``DatagramFormat``), is what goes on a network: a
4-byte header -- version, stages carried, hop number -- in front of the hop's
records truncated to the first ``s <= S`` stages.
"""
import torch

WIRE_VERSION = 1
DGRAM_VERSION = 2
DGRAM_HEADER_BYTES = 4


def field_bits(codebook_size):
    """max(1, ceil(log2 K)) in integers."""
    if codebook_size < 1:
        raise ValueError("sel.wire: codebook_size must be positive")
    return max(1, (int(codebook_size) - 1).bit_length())


class WireFormat:
    """The packet layout of ``codebooks`` stages of ``codebook_size`` codes at
    ``frames`` code frames per hop."""
    version = WIRE_VERSION

    def __init__(self, codebooks, codebook_size, frames=1):
        if codebooks < 1 or frames < 1:
            raise ValueError("sel.wire: codebooks and frames must be positive")
        self.codebooks, self.codebook_size, self.frames = int(codebooks), int(codebook_size), int(frames)
        self.bits = field_bits(codebook_size)
        if self.bits > 31:
            raise ValueError(f"sel.wire: {codebook_size} codes need more than 31 bits per field")
        self.frame_bytes = (self.codebooks * self.bits + 7) // 8
        self.packet_bytes = self.frames * self.frame_bytes

    def __repr__(self):
        return (f"WireFormat(v{self.version}: {self.codebooks} x {self.bits} bits, {self.frame_bytes} bytes / frame, "
                f"{self.frames} frames / packet)")

    def bitrate(self, sample_rate, chunk):
        """Bits per second of one stream sending a packet per hop of ``chunk`` samples."""
        return 8 * self.packet_bytes * sample_rate / chunk

    def _weights(self):
        return (torch.arange(self.codebooks, dtype=torch.int64) * self.codebook_size).view(-1, 1)

    def pack(self, idx, flattened=True):
        """idx (codebooks, ...) int64 on the CPU, ``n * frames`` entries per stage
        (what ``transmit`` / ``quantize`` return; ``flattened``: ids ``s * K + k_s``)
        -> (n, packet_bytes) uint8.  ValueError for a code outside [0, K)."""
        S, K, b = self.codebooks, self.codebook_size, self.bits
        if idx.dtype != torch.int64 or idx.device.type != "cpu" or idx.dim() < 2 or idx.shape[0] != S \
                or (idx.numel() // S) % self.frames:
            raise ValueError(f"sel.wire: pack takes CPU int64 indices of {S} codebooks x n * {self.frames} frames, got "
                             f"{idx.dtype} {tuple(idx.shape)} on {idx.device}")
        k = idx.reshape(S, -1)
        if flattened:
            k = k - self._weights()
        if k.numel() and (int(k.min()) < 0 or int(k.max()) >= K):
            raise ValueError(f"sel.wire: a code outside [0, {K})")
        rows = k.shape[1]
        # (rows, S, bits) bit planes, lowest bit first -> the record's bit string
        planes = (k.t().unsqueeze(2) >> torch.arange(b, dtype=torch.int64)) & 1
        string = torch.zeros((rows, 8 * self.frame_bytes), dtype=torch.int64)
        string[:, :S * b] = planes.reshape(rows, S * b)
        by = (string.view(rows, self.frame_bytes, 8) << torch.arange(8, dtype=torch.int64)).sum(2)
        return by.to(torch.uint8).view(rows // self.frames, self.packet_bytes)

    def unpack(self, packets, flatten=True):
        """packets (n, packet_bytes) uint8 on the CPU -> idx (codebooks, n, frames)
        int64 (``flatten``: ids ``s * K + k_s``).  Pad bits are ignored; a field
        >= K gives -1, as the receiving kernel reports it."""
        S, K, b = self.codebooks, self.codebook_size, self.bits
        if packets.dtype != torch.uint8 or packets.device.type != "cpu" or packets.dim() != 2 \
                or packets.shape[1] != self.packet_bytes:
            raise ValueError(f"sel.wire: unpack takes CPU uint8 packets (n, {self.packet_bytes}), got {packets.dtype} "
                             f"{tuple(packets.shape)} on {packets.device}")
        n = packets.shape[0]
        by = packets.reshape(n * self.frames, self.frame_bytes, 1).to(torch.int64)
        string = ((by >> torch.arange(8, dtype=torch.int64)) & 1).view(n * self.frames, 8 * self.frame_bytes)
        planes = string[:, :S * b].reshape(-1, S, b)
        k = (planes << torch.arange(b, dtype=torch.int64)).sum(2).t()          # (S, rows)
        ok = k < K
        if flatten:
            k = k + self._weights()
        return torch.where(ok, k, torch.full_like(k, -1)).reshape(S, n, self.frames).contiguous()


class DatagramFormat:
    """Wire version 2 (include/sel.h): what one stream puts on a network per hop,
    for ``codebooks`` stages of ``codebook_size`` codes at ``frames`` code frames
    per hop.

    A datagram is a 4-byte header -- the version (2), the number ``s`` of stages
    it carries (``1 <= s <= codebooks``: a residual VQ's first ``s`` stages are a
    coarser code of the same frame), the stream's hop number as a wrapping
    little-endian uint16 -- and ``frames`` records of ``s`` fields each, version
    1's record with ``codebooks`` replaced by ``s``.  ``frames`` is not in the
    header: a receiver knows its own and refuses other lengths.

    On the GPU the datagrams are written and read inside the hop
    (``sel.streamops.rvq_step_dgram`` / ``rvq_lookup_dgram_step``) in
    ``(n, stride)`` uint8 buffers, one region of ``stride`` bytes per stream of
    which a datagram fills the front.  The methods here are the same format on
    the CPU: for the peer without a GPU and for the host side of a socket
    (``split`` after the transmitter, ``assemble`` in front of the receiver)."""
    version = DGRAM_VERSION
    header_bytes = DGRAM_HEADER_BYTES

    def __init__(self, codebooks, codebook_size, frames=1):
        if codebooks < 1 or frames < 1:
            raise ValueError("sel.wire: codebooks and frames must be positive")
        if codebooks > 255:
            raise ValueError(f"sel.wire: {codebooks} codebooks do not fit the datagram's stage byte (<= 255)")
        self.codebooks, self.codebook_size, self.frames = int(codebooks), int(codebook_size), int(frames)
        self.bits = field_bits(codebook_size)
        if self.bits > 31:
            raise ValueError(f"sel.wire: {codebook_size} codes need more than 31 bits per field")
        self.stride = self.datagram_bytes(self.codebooks)
        self._records = {}

    def __repr__(self):
        return (f"DatagramFormat(v{self.version}: up to {self.codebooks} x {self.bits} bits, {self.frames} frames, "
                f"{self.datagram_bytes(1)}..{self.stride} bytes)")

    def _stages(self, stages):
        s = self.codebooks if stages is None else int(stages)
        if not 1 <= s <= self.codebooks:
            raise ValueError(f"sel.wire: {stages} stages, a datagram carries 1..{self.codebooks}")
        return s

    def _record(self, stages):
        """the record layout of ``stages`` fields: version 1's, with its pack / unpack"""
        if stages not in self._records:
            self._records[stages] = WireFormat(stages, self.codebook_size, self.frames)
        return self._records[stages]

    def frame_bytes(self, stages=None):
        return (self._stages(stages) * self.bits + 7) // 8

    def datagram_bytes(self, stages=None):
        return self.header_bytes + self.frames * self.frame_bytes(stages)

    def bitrate(self, sample_rate, chunk, stages=None):
        """Bits per second of one stream sending a datagram of ``stages`` stages per
        hop of ``chunk`` samples, the header counted."""
        return 8 * self.datagram_bytes(stages) * sample_rate / chunk

    def pack(self, idx, stages=None, seq=0, flattened=True):
        """idx (codebooks, ...) int64 on the CPU, ``n * frames`` entries per stage;
        stages and seq: an int or one per stream (seq wraps at 2^16) -> a list of
        n ``bytes``.  Only the first ``stages[i]`` rows of stream i's columns are
        looked at (``transmit_datagrams`` leaves -1 in the others)."""
        S, K = self.codebooks, self.codebook_size
        if idx.dtype != torch.int64 or idx.device.type != "cpu" or idx.dim() < 2 or idx.shape[0] != S \
                or (idx.numel() // S) % self.frames:
            raise ValueError(f"sel.wire: pack takes CPU int64 indices of {S} codebooks x n * {self.frames} frames, got "
                             f"{idx.dtype} {tuple(idx.shape)} on {idx.device}")
        k = idx.reshape(S, -1, self.frames)
        n = k.shape[1]
        per = lambda v: [int(v)] * n if not hasattr(v, "__len__") else [int(e) for e in v]  # noqa: E731
        stages = per(S if stages is None else stages)
        seq = per(seq)
        if len(stages) != n or len(seq) != n:
            raise ValueError(f"sel.wire: pack of {n} streams with {len(stages)} stage counts and {len(seq)} hop numbers")
        out = []
        for i in range(n):
            s = self._stages(stages[i])
            body = self._record(s).pack(k[:s, i].contiguous(), flattened=flattened)
            out.append(bytes([self.version, s]) + (seq[i] & 0xFFFF).to_bytes(2, "little")
                       + bytes(body.reshape(-1).tolist()))
        return out

    def parse(self, datagram):
        """bytes-like -> (stages, seq).  ValueError for a wrong version, a stage
        byte outside [1, codebooks] or a length that is not this receiver's."""
        d = bytes(datagram)
        if len(d) < self.header_bytes:
            raise ValueError(f"sel.wire: a datagram of {len(d)} bytes has no header")
        if d[0] != self.version:
            raise ValueError(f"sel.wire: datagram version {d[0]}, expected {self.version}")
        if not 1 <= d[1] <= self.codebooks:
            raise ValueError(f"sel.wire: the datagram says {d[1]} stages, this receiver takes 1..{self.codebooks}")
        if len(d) != self.datagram_bytes(d[1]):
            raise ValueError(f"sel.wire: a datagram of {d[1]} stages x {self.frames} frames is "
                             f"{self.datagram_bytes(d[1])} bytes, got {len(d)}")
        return d[1], int.from_bytes(d[2:4], "little")

    def unpack(self, datagram, flatten=True):
        """bytes-like -> idx (codebooks, frames) int64 (``flatten``: ids ``s * K +
        k_s``), -1 for a field >= K and for the stages the datagram does not carry."""
        d = bytes(datagram)
        s, _ = self.parse(d)
        body = torch.tensor(list(d[self.header_bytes:]), dtype=torch.uint8).view(1, -1)
        out = torch.full((self.codebooks, self.frames), -1, dtype=torch.int64)
        out[:s] = self._record(s).unpack(body, flatten=flatten).view(s, self.frames)
        return out

    def assemble(self, datagrams):
        """A list whose entries are bytes-like or None (nothing arrived) -> (buffer,
        lost, refused): a CPU uint8 ``(n, stride)`` buffer for ``receive_datagrams``
        / ``rvq_lookup_dgram_step`` (zero where nothing valid stands), one lost flag
        per stream, and the positions of entries that arrived malformed (they
        count as lost)."""
        n = len(datagrams)
        buf = torch.zeros((n, self.stride), dtype=torch.uint8)
        lost, refused = [], []
        for i, d in enumerate(datagrams):
            if d is not None:
                try:
                    d = bytes(d)
                    self.parse(d)
                except ValueError:
                    refused.append(i)
                    d = None
            lost.append(d is None)
            if d is not None:
                buf[i, :len(d)] = torch.tensor(list(d), dtype=torch.uint8)
        return buf, lost, refused

    def split(self, buffer):
        """A CPU uint8 ``(n, stride' >= stride)`` buffer as the transmitter wrote it
        -> a list of n ``bytes``, each cut to the length its header gives."""
        if buffer.dtype != torch.uint8 or buffer.device.type != "cpu" or buffer.dim() != 2 \
                or buffer.shape[1] < self.stride:
            raise ValueError(f"sel.wire: split takes a CPU uint8 buffer (n, >= {self.stride}), got {buffer.dtype} "
                             f"{tuple(buffer.shape)} on {buffer.device}")
        out = []
        for row in buffer.tolist():
            if row[0] != self.version or not 1 <= row[1] <= self.codebooks:
                raise ValueError(f"sel.wire: split met a header of version {row[0]} and {row[1]} stages")
            out.append(bytes(row[:self.datagram_bytes(row[1])]))
        return out
