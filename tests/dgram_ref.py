"""The datagram, wire version 2 (include/sel.h), restated in plain Python
integers: the reference of tests/test_rvq_dgram_host.py and
tests/test_gpu_rvq_dgram.py.  Independent of sel/wire.py and of the kernels.

    byte 0      2
    byte 1      s, 1 <= s <= S: the stages this datagram carries
    bytes 2..3  seq & 0xFFFF, little-endian
    bytes 4..   `frames` records of s fields each: ONE Python int per record,
                field j shifted to bit j * bits, int.to_bytes(fb(s), "little")

A plain helper: nothing here needs a GPU.
"""
import torch

VERSION = 2
HEADER = 4


def bits_of(K):
    """max(1, ceil(log2 K)) without floating point"""
    b = 0
    while (1 << b) < K:
        b += 1
    return max(1, b)


def fb(s, K):
    """bytes of a record of s fields"""
    return -(-s * bits_of(K) // 8)


def dgram_bytes(s, K, frames):
    return HEADER + frames * fb(s, K)


def clamp(budget, S):
    return min(max(int(budget), 1), S)


def pack_record(codes, K):
    b = bits_of(K)
    rec = 0
    for j, k in enumerate(codes):
        assert 0 <= k < K, (j, k, K)
        rec |= int(k) << (j * b)
    return rec.to_bytes(fb(len(codes), K), "little")


def pack_datagram(codes, s, seq, K):
    """codes: `frames` lists of at least s un-flattened codes -> bytes"""
    assert 1 <= s <= 255
    out = bytes([VERSION, s]) + (int(seq) & 0xFFFF).to_bytes(2, "little")
    for rec in codes:
        out += pack_record(list(rec)[:s], K)
    return out


def pack(idx, stages, seq, K, frames):
    """idx (S, n * frames) un-flattened int64, stages / seq one int per sample
    (stages already in [1, S]) -> list of n bytes objects"""
    S, rows = idx.shape
    cols = idx.t().tolist()
    n = rows // frames
    return [pack_datagram([cols[i * frames + r] for r in range(frames)], stages[i], seq[i], K) for i in range(n)]


def parse(data, S, K, frames):
    """bytes -> (s, seq), or None for what a receiver refuses"""
    data = bytes(data)
    if len(data) < HEADER or data[0] != VERSION or not 1 <= data[1] <= S:
        return None
    if len(data) != dgram_bytes(data[1], K, frames):
        return None
    return data[1], int.from_bytes(data[2:4], "little")


def unpack(data, S, K, frames, flatten=False):
    """bytes of a valid datagram -> (S, frames) int64: -1 for a field >= K and for stages not carried"""
    s, _ = parse(data, S, K, frames)
    b, n = bits_of(K), fb(s, K)
    out = torch.full((S, frames), -1, dtype=torch.int64)
    for r in range(frames):
        rec = int.from_bytes(bytes(data[HEADER + r * n:HEADER + (r + 1) * n]), "little")
        for j in range(s):
            k = (rec >> (j * b)) & ((1 << b) - 1)
            if k < K:
                out[j, r] = k + (j * K if flatten else 0)
    return out


def buffer(datagrams, stride, fill=0xFF):
    """list of bytes -> (n, stride) uint8, the bytes past each datagram's length = fill"""
    out = torch.full((len(datagrams), stride), fill, dtype=torch.uint8)
    for i, d in enumerate(datagrams):
        assert len(d) <= stride
        out[i, :len(d)] = torch.tensor(list(d), dtype=torch.uint8)
    return out


def set_pad_bits(data, S, K, frames):
    """a copy of a valid datagram with every pad bit of every record set"""
    s, _ = parse(data, S, K, frames)
    n, pad = fb(s, K), 8 * fb(s, K) - s * bits_of(K)
    out = bytearray(data)
    if pad:
        for r in range(frames):
            out[HEADER + (r + 1) * n - 1] |= (0xFF << (8 - pad)) & 0xFF
    return bytes(out)
