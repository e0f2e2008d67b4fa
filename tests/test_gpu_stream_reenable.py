"""The hop variants of one object beside one another, and ``enable_codes`` called
twice (sel.streaming) on the GPU.

What the other stream tests leave open: that ``transmit`` and ``transmit_packets``
of a ``wire=True`` object are ONE replay writing both fixed buffers; that the
three ``transmit*`` and the three ``receive*`` of an ``enable_codes(wire=True,
datagrams=True)`` object agree on twin objects fed the same hops; that a second
``enable_codes`` takes a new snapshot of the codebooks, discards the variants
of the first and moves no carry; and the same three receivers on a vocoder.
Golden width, bf16, batch 2 (a session) and two of three slots (a pool), eager
and graph.  Every comparison is bitwise: the oracle is a twin object."""
import pytest
import torch

from conftest import golden
from test_gpu_stream_codes import _gen, _vocoder
from test_gpu_stream_pool import _same
from test_gpu_stream_session import GP, _stream_model

pytestmark = pytest.mark.gpu

DTYPE = torch.bfloat16
BATCH, CHUNK, CAPACITY = 2, 300, 3
S, K = GP["codebook_num"], GP["codebook_size"]
GRAPH = pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
KIND = pytest.mark.parametrize("kind", ["session", "pool"])


def _make(kind, G, graph, vocoder=False, **codes):
    """-> (object, the leading arguments of its per-hop methods): a session of BATCH
    streams, or a pool of CAPACITY slots of which BATCH run, listed out of order"""
    from sel.streaming import StreamPool, StreamSession, VocoderPool, VocoderSession
    if kind == "session":
        o = (VocoderSession(G, BATCH, 1, graph=graph, dtype=DTYPE) if vocoder else
             StreamSession(G, BATCH, CHUNK, graph=graph, dtype=DTYPE))
        lead = ()
    else:
        o = (VocoderPool(G, CAPACITY, 1, graph=graph, dtype=DTYPE) if vocoder else
             StreamPool(G, CAPACITY, CHUNK, graph=graph, dtype=DTYPE))
        slots = [o.open() for _ in range(CAPACITY)]
        lead = ([slots[2], slots[0]],)
    if codes:
        o.enable_codes(**codes)
    return o, lead


def _state(o):
    """every carry row the object holds (a pool: all slot rows and the template row)"""
    torch.cuda.synchronize()
    return list(o._carries) if hasattr(o, "table") else list(o.carries().values())


def _state_equal(a, b):
    sa, sb = _state(a), _state(b)
    assert len(sa) == len(sb) > 0
    return all(_same(x, y) for x, y in zip(sa, sb))


def _hops(gpu, seed, n=3):
    return 0.1 * torch.randn(n, BATCH, 1, CHUNK, generator=torch.Generator().manual_seed(seed)).to(gpu)


def _from_datagrams(f, d):
    """the device buffer transmit_datagrams returns -> flattened ids (S, BATCH, frames) on the CPU"""
    return torch.stack([f.unpack(e) for e in f.split(d.cpu())], 1)


@GRAPH
@KIND
def test_transmit_and_transmit_packets_are_one_replay(gpu, kind, graph):
    G = _gen("golden")
    obj, lead = _make(kind, G, graph, wire=True, datagrams=True)
    twin, _ = _make(kind, G, graph, wire=True, datagrams=True)
    x = _hops(gpu, 31, 2)
    p = obj.transmit_packets(*lead, x[0])               # a view of the fixed packet buffer
    twin.transmit(*lead, x[0])
    idx = obj.transmit(*lead, x[1])                     # the same replay fills that buffer again ...
    assert torch.equal(obj.wire.unpack(p.cpu()).view(idx.shape), idx.cpu())
    assert torch.equal(idx, twin.transmit(*lead, x[1]))
    assert _state_equal(obj, twin)                      # ... and has moved the state by one hop, not two


@GRAPH
@KIND
def test_the_three_variants_agree(gpu, kind, graph):
    G = _gen("golden")
    (a, lead), (b, _), (c, _) = (_make(kind, G, graph, wire=True, datagrams=True) for _ in range(3))
    x = _hops(gpu, 32)
    for h in range(3):
        idx = a.transmit(*lead, x[h]).clone()
        p = b.transmit_packets(*lead, x[h]).clone()
        d = c.transmit_datagrams(*lead, x[h]).clone()
        assert tuple(idx.shape) == (S, BATCH, 1)
        assert torch.equal(b.wire.unpack(p.cpu()).view(idx.shape), idx.cpu()), h
        assert torch.equal(_from_datagrams(c.datagram, d), idx.cpu()), h
        assert [c.datagram.parse(e) for e in c.datagram.split(d.cpu())] == [(S, h)] * BATCH
        y = a.receive(*lead, idx).clone()
        assert tuple(y.shape) == (BATCH, 1, CHUNK)
        assert _same(b.receive_packets(*lead, p), y), h
        assert _same(c.receive_datagrams(*lead, d), y), h
    assert _state_equal(a, b) and _state_equal(a, c)


@GRAPH
@KIND
def test_enable_codes_again_takes_a_new_snapshot(gpu, kind, graph):
    from sel import SelError
    G = _stream_model(gpu, golden("stream"))            # its own generator: a codebook entry changes below
    x = _hops(gpu, 33, 2)
    idx = torch.tensor([5, 9]).view(S, 1, 1) + K * torch.arange(S).view(S, 1, 1)
    idx = idx.expand(S, BATCH, 1).contiguous().to(gpu)

    zq = torch.randn(BATCH, 1, GP["code_dim"], generator=torch.Generator().manual_seed(35)).to(gpu)

    def warm(o, lead):                                  # one hop of each half, whatever the codebooks hold:
        o.encode(*lead, x[0])                           # the carries are not zero
        o.decode(*lead, zq)

    obj, lead = _make(kind, G, graph)
    stale, _ = _make(kind, G, graph)
    for o in (obj, stale):
        warm(o, lead)
    before = [c.clone() for c in _state(obj)]
    assert sum(float(c.float().abs().sum()) for c in before) > 0
    obj.enable_codes(wire=True, datagrams=True)
    stale.enable_codes()
    assert obj.wire is not None and obj.datagram is not None
    assert all(_same(c, d) for c, d in zip(_state(obj), before))
    with torch.no_grad():
        G.quantizer.codebook.codebook[5] += 0.5         # an entry the indices below pick
    obj.enable_codes()
    assert obj.wire is None and obj.datagram is None
    assert all(_same(c, d) for c, d in zip(_state(obj), before))
    fresh, _ = _make(kind, G, graph)
    warm(fresh, lead)
    fresh.enable_codes()
    y = obj.receive(*lead, idx).clone()
    assert _same(y, fresh.receive(*lead, idx))
    assert not _same(y, stale.receive(*lead, idx))      # the first snapshot is a private copy
    assert torch.equal(obj.transmit(*lead, x[1]), fresh.transmit(*lead, x[1]))
    assert _state_equal(obj, fresh)
    with pytest.raises(SelError, match="wire=True"):
        obj.transmit_packets(*lead, x[1])
    with pytest.raises(SelError, match="datagrams=True"):
        obj.receive_datagrams(*lead, [None] * BATCH)


@GRAPH
@KIND
def test_vocoder_variants_agree(gpu, tmp_path, kind, graph):
    from sel import SelError
    V, E = _vocoder(gpu, True, tmp_path), _gen("golden")
    (a, lead), (b, _), (c, _) = (_make(kind, V, graph, vocoder=True, lookup_generator=E, wire=True, datagrams=True)
                                 for _ in range(3))
    gen = torch.Generator().manual_seed(34)
    for h in range(3):
        idx = torch.randint(0, K, (S, BATCH, 1), generator=gen) + K * torch.arange(S).view(S, 1, 1)
        y = a.receive(*lead, idx.to(gpu)).clone()
        assert tuple(y.shape) == (BATCH, 1, CHUNK) and y.dtype == torch.float32
        assert _same(b.receive_packets(*lead, b.wire.pack(idx).to(gpu)), y), h
        assert _same(c.receive_datagrams(*lead, c.datagram.pack(idx, S, h)), y), h
    assert _state_equal(a, b) and _state_equal(a, c)
    x = torch.zeros(BATCH, 1, CHUNK, device=gpu)
    for call in (a.transmit, a.transmit_packets, a.transmit_datagrams):
        with pytest.raises(SelError, match="PQC"):
            call(*lead, x)
