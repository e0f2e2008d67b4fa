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
"""
import torch

WIRE_VERSION = 1


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
