"""CPU checks of the wire format (include/sel.h, wire version 1): every refusal
of sel_rvq_step_wire / sel_rvq_lookup_wire_step through ctypes (SEL_ERR_ARG
before any device work: the pointers below are never dereferenced), the edge
each case of tests/rvq_step_ref.py contributes to the format, and sel.wire's
pack / unpack against the plain-integer restatement tests/wire_ref.py.  Every
comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import rvq_step_ref as SR
import wire_ref as WR
from conftest import golden

SEL_ERR_ARG = -1
P = ctypes.c_void_p(0x1000)      # a non-null pointer no refused call may touch
NULL = None


def _lib():
    from sel import _lib
    return _lib.load()


def _step(**kw):
    a = dict(z=P, rows=4, T=2, D=64, embeds=P, S=8, K=1024, n_active=NULL, flatten=1, idx=P, zq=NULL, wire=P)
    a.update(kw)
    return _lib().sel_rvq_step_wire(a["z"], a["rows"], a["T"], a["D"], a["embeds"], a["S"], a["K"], a["n_active"],
                                    a["flatten"], a["idx"], a["zq"], a["wire"], None)


def _lookup(**kw):
    a = dict(wire=P, rows=4, T=2, S=8, K=1024, D=64, codebook=P, mean=NULL, scale=NULL, n_active=NULL, out_dtype=0,
             out=P, idx_out=NULL)
    a.update(kw)
    return _lib().sel_rvq_lookup_wire_step(a["wire"], a["rows"], a["T"], a["S"], a["K"], a["D"], a["codebook"],
                                           a["mean"], a["scale"], a["n_active"], a["out_dtype"], a["out"],
                                           a["idx_out"], None)


_ids = lambda b: ",".join(f"{k}={'null' if v is None else 'ptr' if isinstance(v, ctypes.c_void_p) else v}"  # noqa: E731
                          for k, v in b.items())


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-4), dict(T=0), dict(T=-2), dict(rows=5, T=2), dict(D=0), dict(D=-1), dict(D=257),
    dict(K=0), dict(K=-1), dict(S=0), dict(S=-1), dict(z=NULL), dict(embeds=NULL), dict(wire=NULL),
    dict(wire=NULL, idx=NULL),
    dict(zq=P),                                  # zq aliases z
    dict(S=1 << 30, K=1 << 11),                  # S * K beyond 2^40
    dict(S=(1 << 31) - 1, K=(1 << 31) - 1),
], ids=_ids)
def test_rvq_step_wire_refuses(bad):
    lib = _lib()
    assert _step(**bad) == SEL_ERR_ARG
    assert b"sel_rvq_step_wire" in lib.sel_last_error()


@pytest.mark.parametrize("bad", [
    dict(rows=0), dict(rows=-4), dict(T=0), dict(rows=5, T=2), dict(S=0), dict(S=-1), dict(D=0), dict(D=-3),
    dict(K=0), dict(K=-1), dict(S=1 << 20, K=1 << 20, D=256), dict(S=1 << 30, K=1 << 11, D=1),
    dict(S=(1 << 31) - 1, K=(1 << 31) - 1, D=1), dict(wire=NULL), dict(codebook=NULL),
    dict(out=NULL), dict(mean=P), dict(scale=P), dict(out_dtype=2), dict(out_dtype=-1),
    dict(rows=(1 << 31) - 1, T=1, D=1 << 20, S=1, K=2),
], ids=_ids)
def test_rvq_lookup_wire_step_refuses(bad):
    lib = _lib()
    assert _lookup(**bad) == SEL_ERR_ARG
    assert b"sel_rvq_lookup_wire_step" in lib.sel_last_error()


# (S * bits, frame_bytes, pad bits) each case must have, and what it adds to the format's edges
EDGES = {
    "hop": (80, 10, 0), "pool": (80, 10, 0),     # the product shape: no padding
    "one": (1, 1, 7),                            # K = 1 -> bits = 1, one byte
    "d60": (30, 4, 2),                           # 3 x 10 bits: 2 pad bits
    "d255": (12, 2, 4),                          # 2 x 6 bits
    "k2050": (24, 3, 0),                         # 2 x 12 bits: a field straddling a byte
    "s17": (68, 9, 4),                           # 17 x 4 bits: more than one 64-bit accumulator
    "dup": (20, 3, 4), "dup_col": (20, 3, 4),
}


@pytest.mark.parametrize("name", list(SR.CASES))
def test_case_edges_of_the_format(name):
    from sel.wire import WireFormat
    rows, T, D, K, S = SR.CASES[name]
    used, fb, pad = EDGES[name]
    f = WireFormat(S, K, T)
    assert f.bits == WR.bits_of(K) and (1 << f.bits) >= K and (f.bits == 1 or (1 << (f.bits - 1)) < K)
    assert S * f.bits == used and f.frame_bytes == WR.frame_bytes(S, K) == fb and 8 * fb - used == pad
    assert f.packet_bytes == T * fb and f.version == 1
    if name in ("hop", "pool"):
        assert f.bits == 10 and pad == 0 and f.bitrate(48000, 300 * T) == 12800.0    # hop 300: T frames per chunk
    elif name == "one":
        assert K == 1 and f.bits == 1 and fb == 1
    elif name == "k2050":
        assert f.bits == 12 and f.bits % 8           # field 0 ends inside byte 1
    elif name == "s17":
        assert used > 64
    # the reference itself on the case's extreme records: all zero, all K - 1, and one field at a time
    assert WR.pack_record([0] * S, K) == bytes(fb)
    top = WR.pack_record([K - 1] * S, K)
    assert WR.unpack_record(top, S, K) == [K - 1] * S and (pad == 0 or top[-1] >> (8 - pad) == 0)
    for s in range(S):
        one = [0] * S
        one[s] = K - 1
        rec = int.from_bytes(WR.pack_record(one, K), "little")
        assert rec == (K - 1) << (s * f.bits)


def _random_codes(name):
    rows, T, D, K, S = SR.CASES[name]
    g = torch.Generator().manual_seed(1000 + list(SR.CASES).index(name))
    k = torch.randint(0, K, (S, rows), generator=g)
    k[0, 0], k[-1, -1] = K - 1, K - 1
    return k


@pytest.mark.parametrize("name", list(SR.CASES))
def test_sel_wire_equals_the_reference(name):
    from sel.wire import WireFormat
    rows, T, D, K, S = SR.CASES[name]
    f = WireFormat(S, K, T)
    k = _random_codes(name)
    flat = k + K * torch.arange(S).view(-1, 1)
    want = WR.pack(k, K)
    assert want.dtype == torch.uint8 and tuple(want.shape) == (rows, f.frame_bytes)
    for idx, flattened in ((k, False), (flat, True)):
        got = f.pack(idx, flattened=flattened)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (rows // T, f.packet_bytes)
        assert torch.equal(got.view(rows, f.frame_bytes), want)
        assert torch.equal(WR.pack(idx, K, flattened=flattened), want)
    packets = want.view(rows // T, f.packet_bytes)
    # the round trip is the identity, through either side, and set pad bits change nothing
    assert torch.equal(f.unpack(packets, flatten=False).view(S, rows), k)
    assert torch.equal(f.unpack(packets, flatten=True).view(S, rows), flat)
    assert torch.equal(WR.unpack(want, S, K), k) and torch.equal(WR.unpack(want, S, K, flatten=True), flat)
    dirty = WR.set_pad_bits(want, S, K)
    assert (8 * f.frame_bytes == S * f.bits) == torch.equal(dirty, want)
    assert torch.equal(f.unpack(dirty.view(rows // T, f.packet_bytes), flatten=False).view(S, rows), k)
    assert torch.equal(WR.unpack(dirty, S, K), k)


def test_a_field_beyond_K_unpacks_to_minus_one():
    from sel.wire import WireFormat
    S, K = 3, 1000
    rec = 5 | (1023 << 10) | (999 << 20)
    data = torch.tensor(list(rec.to_bytes(4, "little")), dtype=torch.uint8).view(1, 4)
    want = torch.tensor([[5], [-1], [2999]])
    assert torch.equal(WR.unpack(data, S, K, flatten=True), want)
    assert torch.equal(WireFormat(S, K).unpack(data).view(S, 1), want)


def test_sel_wire_refuses_bad_operands():
    from sel.wire import WireFormat
    f = WireFormat(2, 64, 2)
    good = torch.zeros(2, 4, dtype=torch.int64)
    for bad in (good.int(), good[:1], good[:, :3], torch.full((2, 2), 64), torch.full((2, 2), -1)):
        with pytest.raises(ValueError):
            f.pack(bad, flattened=False)
    for bad in (torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.uint8),
                torch.zeros(4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            f.unpack(bad)
    for args in ((0, 4), (2, 0), (2, 1 << 32), (2, 4, 0)):
        with pytest.raises(ValueError):
            WireFormat(*args)


def test_golden_stream_indices_pack_and_unpack_to_themselves():
    from sel.wire import WireFormat
    g = golden("stream")
    S, K = 2, g["sd.quantizer.codebook.layers.0.embed"].shape[1]
    assert K == 64
    f = WireFormat(S, K, 2)                                  # chunk 600: two records per packet
    assert (f.bits, f.frame_bytes, f.packet_bytes) == (6, 2, 4)
    for c in range(6):
        idx = torch.from_numpy(np.asarray(g[f"idx.{c}"]))    # (S, frames), flattened ids
        p = f.pack(idx)
        assert tuple(p.shape) == (1, 4) and torch.equal(p.view(2, 2), WR.pack(idx, K, flattened=True))
        assert torch.equal(f.unpack(p).view(S, 2), idx)
