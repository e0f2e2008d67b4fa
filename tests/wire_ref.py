"""The wire format of the code indices, version 1 (include/sel.h), restated in
plain Python integers: the reference of tests/test_rvq_wire_host.py,
tests/test_gpu_rvq_wire.py and tests/test_gpu_stream_wire.py.  Independent of
sel/wire.py and of the kernels: a record is built as ONE Python int, field s
shifted to bit s * bits, and written out with int.to_bytes(..., "little"), which
is the format's byte order by definition (bit i of the record is bit i % 8 of
byte i // 8).  A plain helper: nothing here needs a GPU.
"""
import torch


def bits_of(K):
    """max(1, ceil(log2 K)) without floating point"""
    b = 0
    while (1 << b) < K:
        b += 1
    return max(1, b)


def frame_bytes(S, K):
    return -(-S * bits_of(K) // 8)


def pack_record(codes, K):
    """the S un-flattened codes of one row -> bytes"""
    b = bits_of(K)
    rec = 0
    for s, k in enumerate(codes):
        assert 0 <= k < K, (s, k, K)
        rec |= int(k) << (s * b)
    return rec.to_bytes(frame_bytes(len(codes), K), "little")


def unpack_record(data, S, K):
    """bytes of one record -> the S field values (pad bits ignored, nothing refused)"""
    b = bits_of(K)
    assert len(data) == frame_bytes(S, K)
    rec = int.from_bytes(bytes(data), "little")
    return [(rec >> (s * b)) & ((1 << b) - 1) for s in range(S)]


def pack(idx, K, flattened=False):
    """idx (S, rows) int64 (flattened: s * K + k_s) -> (rows, frame_bytes) uint8"""
    S, rows = idx.shape
    cols = idx.tolist()
    out = []
    for r in range(rows):
        out.append(list(pack_record([cols[s][r] - (s * K if flattened else 0) for s in range(S)], K)))
    return torch.tensor(out, dtype=torch.uint8).view(rows, frame_bytes(S, K))


def unpack(wire, S, K, flatten=False):
    """(rows, frame_bytes) uint8 -> (S, rows) int64; a field >= K gives -1"""
    rows = wire.shape[0]
    out = torch.empty((S, rows), dtype=torch.int64)
    for r, data in enumerate(wire.tolist()):
        for s, k in enumerate(unpack_record(data, S, K)):
            out[s, r] = -1 if k >= K else k + (s * K if flatten else 0)
    return out


def set_pad_bits(wire, S, K):
    """a copy with every pad bit of every record set"""
    used = S * bits_of(K)
    out = wire.clone()
    pad = 8 * out.shape[1] - used
    if pad:
        out[:, -1] |= (0xFF << (8 - pad)) & 0xFF
    return out
