"""CPU checks of the datagram (include/sel.h, wire version 2): every refusal of
sel_rvq_step_dgram / sel_rvq_lookup_dgram_step through ctypes (SEL_ERR_ARG
before any device work: the pointers below are never dereferenced), the
format's arithmetic, sel.wire.DatagramFormat against the plain-integer
restatement tests/dgram_ref.py, and the property the stage budget rests on:
the truncated chain's picks are the first picks of the full chain.  Every
comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import dgram_ref as DR
import rvq_step_ref as SR
from conftest import golden

SEL_ERR_ARG = -1
P = ctypes.c_void_p(0x1000)      # a non-null pointer no refused call may touch
NULL = None


def _lib():
    from sel import _lib
    return _lib.load()


# rows = 4, T = 2, S = 8, K = 1024: fb(S) = 10, a full datagram 24 bytes, a hold row 11
def _step(**kw):
    a = dict(z=P, rows=4, T=2, D=64, embeds=P, S=8, K=1024, n_active=NULL, stages=NULL, seq=NULL, flatten=1, idx=P,
             zq=NULL, dgram=P, stride=24)
    a.update(kw)
    return _lib().sel_rvq_step_dgram(a["z"], a["rows"], a["T"], a["D"], a["embeds"], a["S"], a["K"], a["n_active"],
                                     a["stages"], a["seq"], a["flatten"], a["idx"], a["zq"], a["dgram"], a["stride"],
                                     None)


def _lookup(**kw):
    a = dict(dgram=P, stride=24, rows=4, T=2, S=8, K=1024, D=64, codebook=P, mean=NULL, scale=NULL, n_active=NULL,
             slots=NULL, lost=NULL, hold=NULL, hold_stride=0, nslots=0, out_dtype=0, out=P, idx_out=NULL)
    a.update(kw)
    return _lib().sel_rvq_lookup_dgram_step(a["dgram"], a["stride"], a["rows"], a["T"], a["S"], a["K"], a["D"],
                                            a["codebook"], a["mean"], a["scale"], a["n_active"], a["slots"], a["lost"],
                                            a["hold"], a["hold_stride"], a["nslots"], a["out_dtype"], a["out"],
                                            a["idx_out"], None)


_ids = lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"  # noqa: E731
                          for k, v in b.items())


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-4), dict(T=0), dict(T=-2), dict(rows=5, T=2), dict(D=0), dict(D=257), dict(K=0),
    dict(K=-1), dict(S=0), dict(S=-1), dict(z=NULL), dict(embeds=NULL), dict(dgram=NULL), dict(dgram=NULL, idx=NULL),
    dict(zq=P),                                             # zq aliases z
    dict(S=256, stride=4 + 2 * 320),                        # the stage byte
    dict(S=(1 << 31) - 1, K=(1 << 31) - 1, stride=1 << 62),
    dict(stride=23), dict(stride=0), dict(stride=-24),      # one byte short of 4 + 2 * 10, and nonsense
    dict(S=255, K=2, T=1, rows=4, stride=4 + 31),           # 255 bits: 32 bytes per record
], ids=_ids)
def test_rvq_step_dgram_refuses(bad):
    lib = _lib()
    assert _step(**bad) == SEL_ERR_ARG
    assert b"sel_rvq_step_dgram" in lib.sel_last_error()


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-4), dict(T=0), dict(rows=5, T=2), dict(S=0), dict(S=-1), dict(D=0), dict(D=-3),
    dict(K=0), dict(K=-1), dict(dgram=NULL), dict(codebook=NULL), dict(out=NULL), dict(mean=P), dict(scale=P),
    dict(out_dtype=2), dict(out_dtype=-1),
    dict(S=256, stride=4 + 2 * 320),
    dict(stride=23), dict(stride=0),
    dict(hold=P, hold_stride=10, nslots=2),                 # a hold row is 1 + fb(S) = 11 bytes
    dict(hold=P, hold_stride=0, nslots=2), dict(hold=P, hold_stride=-11, nslots=2),
    dict(hold=P, hold_stride=11, nslots=0), dict(hold=P, hold_stride=11, nslots=-1),
    dict(rows=(1 << 31) - 1, T=1, D=1 << 20, S=1, K=2),
], ids=_ids)
def test_rvq_lookup_dgram_step_refuses(bad):
    lib = _lib()
    assert _lookup(**bad) == SEL_ERR_ARG
    assert b"sel_rvq_lookup_dgram_step" in lib.sel_last_error()


def test_header_constants():
    import re
    from pathlib import Path
    from sel import wire
    text = (Path(__file__).resolve().parent.parent / "include" / "sel.h").read_text()
    assert int(re.search(r"#define SEL_DGRAM_VERSION (\d+)", text).group(1)) == wire.DGRAM_VERSION == DR.VERSION == 2
    assert int(re.search(r"#define SEL_DGRAM_HEADER_BYTES (\d+)", text).group(1)) == wire.DGRAM_HEADER_BYTES \
        == DR.HEADER == 4
    assert wire.WIRE_VERSION == 1 and wire.WireFormat.version == 1


# ---------------------------------------------------------------------------
# the format's arithmetic
# ---------------------------------------------------------------------------
def test_record_bytes_of_the_product_shape():
    from sel.wire import DatagramFormat
    f = DatagramFormat(8, 1024, 1)
    assert f.version == 2 and f.header_bytes == 4 and f.bits == 10
    assert [f.frame_bytes(s) for s in range(1, 9)] == [DR.fb(s, 1024) for s in range(1, 9)] == [2, 3, 4, 5, 7, 8, 9, 10]
    assert [f.datagram_bytes(s) for s in (1, 8)] == [6, 14] and f.stride == 14 and f.frame_bytes() == 10
    f4 = DatagramFormat(8, 1024, 4)
    assert f4.stride == 44 and f4.datagram_bytes(3) == 4 + 4 * 4 == DR.dgram_bytes(3, 1024, 4)
    # the header costs 4 bytes per hop: 5.12 kbit/s at 48 kHz and chunk 300, 1.28 at chunk 1200
    assert f.bitrate(48000, 300) == 12800.0 + 5120.0 and f4.bitrate(48000, 1200) == 12800.0 + 1280.0
    assert f.bitrate(48000, 300, 1) == 8 * 6 * 160 and f.bitrate(48000, 300, 4) == 8 * 9 * 160
    for s in (0, 9, -1):
        with pytest.raises(ValueError):
            f.frame_bytes(s)
    for args in ((0, 4), (256, 4), (2, 0), (2, 1 << 32), (2, 4, 0)):
        with pytest.raises(ValueError):
            DatagramFormat(*args)
    assert DatagramFormat(255, 2).stride == 4 + 32


@pytest.mark.parametrize("S,K,s,used,nbytes,pad", [
    (1, 1, 1, 1, 1, 7),              # K = 1: one bit
    (2, 2050, 1, 12, 2, 4),          # 12 bits: the field straddles a byte
    (2, 2050, 2, 24, 3, 0),
    (17, 16, 17, 68, 9, 4),          # 17 x 4: more than one 64-bit accumulator
    (17, 16, 1, 4, 1, 4), (17, 16, 2, 8, 1, 0), (17, 16, 16, 64, 8, 0),
    (3, 1000, 2, 20, 3, 4),
])
def test_record_edges(S, K, s, used, nbytes, pad):
    from sel.wire import DatagramFormat
    f = DatagramFormat(S, K, 1)
    assert s * f.bits == s * DR.bits_of(K) == used and f.frame_bytes(s) == DR.fb(s, K) == nbytes
    assert 8 * nbytes - used == pad
    top = DR.pack_record([K - 1] * s, K)
    assert len(top) == nbytes and (pad == 0 or top[-1] >> (8 - pad) == 0)
    for j in range(s):
        one = [0] * s
        one[j] = K - 1
        assert int.from_bytes(DR.pack_record(one, K), "little") == (K - 1) << (j * f.bits)
    d = DR.pack_datagram([[K - 1] * S], s, 0x1234, K)
    assert d[:4] == bytes([2, s, 0x34, 0x12]) and d[4:] == top and DR.parse(d, S, K, 1) == (s, 0x1234)


# ---------------------------------------------------------------------------
# sel.wire.DatagramFormat against the reference
# ---------------------------------------------------------------------------
def _random_codes(name):
    rows, T, D, K, S = SR.CASES[name]
    g = torch.Generator().manual_seed(2000 + list(SR.CASES).index(name))
    k = torch.randint(0, K, (S, rows), generator=g)
    k[0, 0], k[-1, -1] = K - 1, K - 1
    n = rows // T
    stages = [1 + (3 * i + S - 1) % S for i in range(n)]            # mixed budgets, the first one S
    seq = [(65534 + 7 * i) for i in range(n)]                       # across the wrap
    return k, stages, seq


@pytest.mark.parametrize("name", list(SR.CASES))
def test_datagram_format_equals_the_reference(name):
    from sel.wire import DatagramFormat
    rows, T, D, K, S = SR.CASES[name]
    f = DatagramFormat(S, K, T)
    k, stages, seq = _random_codes(name)
    n = rows // T
    flat = k + K * torch.arange(S).view(-1, 1)
    want = DR.pack(k, stages, seq, K, T)
    assert [len(d) for d in want] == [f.datagram_bytes(s) for s in stages] and stages[0] == S
    assert f.pack(k, stages, seq, flattened=False) == want and f.pack(flat, stages, seq) == want
    assert f.pack(k, None, 0, flattened=False) == DR.pack(k, [S] * n, [0] * n, K, T)
    assert f.pack(k, 1, 65536 + 5, flattened=False) == DR.pack(k, [1] * n, [5] * n, K, T)
    # what the transmitter leaves in idx beyond a budget (-1) is never looked at
    cut = flat.clone().view(S, n, T)
    for i, s in enumerate(stages):
        cut[s:, i] = -1
    assert f.pack(cut.view(S, rows), stages, seq) == want
    for i, d in enumerate(want):
        assert f.parse(d) == DR.parse(d, S, K, T) == (stages[i], seq[i] & 0xFFFF)
        ref = DR.unpack(d, S, K, T)
        assert torch.equal(ref[:stages[i]], k.view(S, n, T)[:stages[i], i]) and bool((ref[stages[i]:] == -1).all())
        assert torch.equal(f.unpack(d, flatten=False), ref)
        assert torch.equal(f.unpack(d), DR.unpack(d, S, K, T, flatten=True))
        assert torch.equal(f.unpack(d), cut[:, i])
        dirty = DR.set_pad_bits(d, S, K, T)
        assert (8 * f.frame_bytes(stages[i]) == stages[i] * f.bits) == (dirty == d)
        assert f.parse(dirty) == f.parse(d) and torch.equal(f.unpack(dirty), f.unpack(d))
    # the round trip through buffers: assemble -> split is the identity on what arrived
    buf, lost, refused = f.assemble(want)
    assert buf.dtype == torch.uint8 and tuple(buf.shape) == (n, f.stride) and lost == [False] * n and refused == []
    assert torch.equal(buf, DR.buffer(want, f.stride, fill=0))
    assert f.split(buf) == want and f.split(DR.buffer(want, f.stride + 3)) == want
    for bad in (k.int(), torch.zeros((S + 1, rows), dtype=torch.int64), torch.full((S, rows), K)):
        with pytest.raises(ValueError):
            f.pack(bad, stages, seq, flattened=False)
    for bad_stages in (0, S + 1, [S] * (n + 1)):
        with pytest.raises(ValueError):
            f.pack(k, bad_stages, seq, flattened=False)


def test_a_field_beyond_K_unpacks_to_minus_one():
    from sel.wire import DatagramFormat
    S, K, s = 3, 1000, 2                            # a truncated record: 20 bits in 3 bytes
    rec = 5 | (1023 << 10)
    d = bytes([2, s, 9, 0]) + rec.to_bytes(3, "little")
    want = torch.tensor([[5], [-1], [-1]])
    assert torch.equal(DR.unpack(d, S, K, 1, flatten=True), want)
    assert torch.equal(DatagramFormat(S, K).unpack(d), want)


def test_assemble_counts_what_did_not_arrive_and_what_is_malformed():
    from sel.wire import DatagramFormat
    S, K, T = 8, 1024, 2
    f = DatagramFormat(S, K, T)
    g = torch.Generator().manual_seed(5)
    k = torch.randint(0, K, (S, 7 * T), generator=g)
    good = DR.pack(k, [8, 3, 1, 8, 2, 5, 8], list(range(7)), K, T)
    v3, s0, s9 = bytearray(good[4]), bytearray(good[5]), bytearray(good[6])
    v3[0], s0[1], s9[1] = 3, 0, S + 1
    entries = [good[0], None, good[2][:-1], memoryview(good[3]), bytes(v3), bytes(s0), bytes(s9)]
    for bad in entries[2], entries[4], entries[5], entries[6], b"", b"\x02", good[1] + b"\x00":
        assert DR.parse(bad, S, K, T) is None
        with pytest.raises(ValueError):
            f.parse(bad)
        with pytest.raises(ValueError):
            f.unpack(bad)
    buf, lost, refused = f.assemble(entries)
    assert lost == [False, True, True, False, True, True, True] and refused == [2, 4, 5, 6]
    assert torch.equal(buf[0], DR.buffer([good[0]], f.stride, 0)[0])
    assert torch.equal(buf[3], DR.buffer([good[3]], f.stride, 0)[0])
    assert not bool(buf[[1, 2, 4, 5, 6]].any())          # nothing of a refused datagram reaches the device
    assert f.split(buf[[0, 3]]) == [good[0], good[3]]
    with pytest.raises(ValueError):
        f.split(buf)                                     # a zero row has no header
    for bad in (buf.int(), buf[:, :-1], buf[0]):
        with pytest.raises(ValueError):
            f.split(bad)


# ---------------------------------------------------------------------------
# the scalable code: stopping the chain after s stages gives the full chain's first s picks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.CASES))
def test_truncated_chain_gives_the_first_picks(name):
    rows, T, D, K, S = SR.CASES[name]
    z, embeds = SR.inputs(name)
    full, _ = SR.rvq_step(z, embeds)
    for s in sorted({1, (S + 1) // 2, S}):
        idx, zq = SR.rvq_step(z, embeds[:s])
        assert torch.equal(idx, full[:s])
        # and zq is the ascending sum of the picked codes' straight-through values: for s = 1, e[pick]
        if s == 1:
            q = embeds[0][:, idx[0]].t()
            assert torch.equal(zq, z + (q - z))


def test_golden_stream_indices_come_out_as_datagrams():
    from sel.wire import DatagramFormat
    g = golden("stream")
    S, K = 2, g["sd.quantizer.codebook.layers.0.embed"].shape[1]
    assert K == 64
    f = DatagramFormat(S, K, 2)                               # chunk 600: two records per datagram
    assert (f.bits, f.frame_bytes(1), f.frame_bytes(2), f.stride) == (6, 1, 2, 8)
    for c in range(6):
        idx = torch.from_numpy(np.asarray(g[f"idx.{c}"]))     # (S, frames), flattened ids
        for s in (S, 1):
            (d,) = f.pack(idx, s, c)
            assert d == DR.pack(idx - K * torch.arange(S).view(-1, 1), [s], [c], K, 2)[0]
            assert f.parse(d) == (s, c) and torch.equal(f.unpack(d)[:s], idx[:s])
            assert bool((f.unpack(d)[s:] == -1).all())
