"""sel.streaming.StreamPool / VocoderPool on the GPU.

The oracle is existing code: a solo ``session(1, ..., graph=False)`` per stream,
fed only that stream's hops.  A pool runs a schedule in which streams open on
different ticks, skip ticks, tick in changing list orders, one closes and a new
one takes the freed slot; every stream's z, idx and y of every hop must equal
its solo session's BITWISE.  The golden stream (tests/golden/stream.npz) runs in
one slot among noise streams at the bounds of tests/test_gpu_stream_session.py.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_stream_session import GP, _stream_model, nclose
from test_gpu_vocoder_session import MODELS, V1, _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]

# (opens, closes, tick lists) per tick, by stream name; capacity 4.  B closes
# before tick 4 and D opens into its slot (1); tick 6 has no active stream.
SCHEDULE = [
    (["A"], [], [["A"]]),
    (["B"], [], [["B", "A"]]),
    (["C"], [], [["A", "C"]]),                  # B skips
    ([], [], [["C", "B", "A"]]),
    (["D"], ["B"], [["D", "A"]]),               # close B, then D opens into slot 1; C skips
    (["E"], [], [["E", "C", "D", "A"]]),        # all four slots
    ([], [], [[], ["D"]]),                      # an empty tick, then one stream
    ([], [], [["A", "D", "E", "C"]]),
]
EXPECT_SLOT = {"A": 0, "B": 1, "C": 2, "D": 1, "E": 3}


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return torch.equal(a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16),
                       b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int16))


def _run_schedule(pool, solo, hop, step_pool, step_solo):
    """hop(name, k): the k-th input hop of a stream (1, ...).  step_pool(slots, x)
    and step_solo(session, x) return the tuple of tensors to compare, the pool's
    with the sample axis first."""
    slot, sessions, count, hops = {}, {}, {}, 0
    for opens, closes, ticks in SCHEDULE:
        for name in closes:
            pool.close(slot.pop(name))
        for name in opens:
            slot[name] = pool.open()
            assert slot[name] == EXPECT_SLOT[name], (name, slot[name])
            sessions[name] = solo()
            count[name] = 0
        for names in ticks:
            xs = [hop(n, count[n]) for n in names]
            x = torch.cat(xs) if xs else hop("A", 0)[:0]
            got = step_pool([slot[n] for n in names], x)
            for i, n in enumerate(names):
                want = step_solo(sessions[n], xs[i])
                for j, (g, w) in enumerate(zip(got, want)):
                    assert _same(g[i:i + 1], w), (n, count[n], j)
                count[n] += 1
                hops += 1
    # the carried state, at the end: every open stream's slot holds its solo session's carries
    for n, s in slot.items():
        st, ca = pool.state(s), sessions[n].carries()
        assert st.keys() == ca.keys() and len(st) > 0
        for k in st:
            assert _same(st[k], ca[k][0]), (n, k)
    assert hops == 19 and count["A"] == 7 and count["D"] == 4 and count["B"] == 2
    return slot


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_pool_schedule_equals_solo_sessions(gpu, dtype, graph):
    from sel.streaming import StreamPool, StreamSession
    G = _stream_model(gpu)
    pool = StreamPool(G, 4, 300, graph=graph, dtype=dtype)
    assert pool.graphed == graph
    gen = torch.Generator().manual_seed(5)
    data = {n: 0.1 * torch.randn(8, 1, 1, 300, generator=gen).to(gpu) for n in "ABCDE"}

    def step_pool(slots, x):
        z = pool.encode(slots, x).clone()
        if not slots:
            assert z.shape[0] == 0 and pool.decode(slots, torch.zeros(0, 1, 64, device=gpu)).shape[0] == 0
            return ()
        idx = pool.quantize(z)
        y = pool.decode(slots, pool.lookup(idx))
        assert tuple(z.shape) == (len(slots), 64, 1) and tuple(y.shape) == (len(slots), 1, 300)
        return z, idx.transpose(0, 1), y

    def step_solo(S, x):
        z = S.encode(x).clone()
        idx = S.quantize(z)
        return z, idx.view(1, idx.shape[0], -1), S.decode(S.lookup(idx))

    _run_schedule(pool, lambda: StreamSession(G, 1, 300, graph=False, dtype=dtype), lambda n, k: data[n][k],
                  step_pool, step_solo)


def test_golden_stream_among_noise_streams(gpu):
    """After the reference's warm-up and load_state(), the golden stream runs in
    slot 2 while slots 0 and 1 carry noise and the list order changes per hop."""
    g = golden("stream")
    G = _stream_model(gpu, g)
    G.initial_decoder(G.initial_encoder(600, gpu))
    pool = G.pool(4, 600)
    pool.load_state()
    assert [pool.open() for _ in range(3)] == [0, 1, 2]
    x = torch.from_numpy(g["x"]).to(gpu)
    noise = 0.1 * torch.randn(6, 2, 1, 600, generator=torch.Generator().manual_seed(8)).to(gpu)
    orders = [[2, 0, 1], [0, 2], [1, 0, 2], [2], [0, 1, 2], [2, 1]]
    for c, slots in enumerate(orders):
        at = slots.index(2)
        xs = torch.cat([x[:, :, 600 * c:600 * (c + 1)] if s == 2 else noise[c, s:s + 1] for s in slots])
        z = pool.encode(slots, xs)
        nclose(z[at:at + 1], g[f"z.{c}"], 1e-5, f"z.{c}")
        idx = pool.quantize(z)
        np.testing.assert_array_equal(idx[:, at].cpu().numpy(), g[f"idx.{c}"])
        zq = pool.lookup(idx)
        nclose(zq[at:at + 1], g[f"zq.{c}"], 1e-5, f"zq.{c}")
        y = pool.decode(slots, zq)
        nclose(y[at:at + 1], g[f"y.{c}"], 1e-5, f"y.{c}")
    # reset_template: the next stream starts from zero state, slot 2 keeps its own
    pool.reset_template()
    s3 = pool.open()
    assert s3 == 3 and all(float(v.abs().sum()) == 0.0 for v in pool.state(3).values())
    assert float(sum(v.abs().sum() for v in pool.state(2).values())) > 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name,params", MODELS)
def test_vocoder_pool_schedule_equals_solo_sessions(gpu, name, params, dtype, graph):
    from sel.streaming import VocoderPool, VocoderSession
    G, _ = _model(name, params, gpu)
    pool = VocoderPool(G, 4, 1, graph=graph, dtype=dtype)
    gen = torch.Generator().manual_seed(6)
    data = {n: torch.randn(8, 1, 1, 64, generator=gen).to(gpu) for n in "ABCDE"}

    def step_pool(slots, x):
        y = pool.decode(slots, x)
        assert tuple(y.shape) == (len(slots), 1, 300) and y.dtype == torch.float32
        return (y,)

    _run_schedule(pool, lambda: VocoderSession(G, 1, 1, graph=False, dtype=dtype), lambda n, k: data[n][k],
                  step_pool, lambda S, x: (S.decode(x),))


@pytest.mark.parametrize("capacity", [1, 3])
@pytest.mark.parametrize("decoder", ["symAudioDec", "HiFiGAN"])
def test_audiodec_open_pool_equals_open_session(gpu, tmp_path, decoder, capacity):
    """utils.audiodec.AudioDec.open_pool on checkpoints written to tmp_path: one
    stream through (tx_pool, rx_pool) equals open_session(batch=1) bitwise.
    Capacity 3 leaves slot 0 idle and runs the stream in slot 1; capacity 1 is
    the smallest pool (its control words are shorter than open()'s three)."""
    import yaml
    from models.autoencoder.AudioDec import StreamGenerator as Encoder
    from sel.streaming import StreamPool, VocoderPool
    from utils.audiodec import AudioDec
    ga = golden("audiodec_baseline")
    enc_dir, dec_dir = tmp_path / "enc", tmp_path / "dec"
    enc_dir.mkdir()
    dec_dir.mkdir()
    E = Encoder(**GP)
    E.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in ga.items() if k.startswith("sd.")}, strict=True)
    torch.save({"model": {"generator": E.state_dict()}}, enc_dir / "checkpoint-1steps.pkl")
    (enc_dir / "config.yml").write_text(yaml.safe_dump({"model_type": "symAudioDec", "generator_params": dict(GP)}))
    if decoder == "HiFiGAN":
        V, _ = _model("vocoder_v1", V1, "cpu")
        V.reset_buffer()
        torch.save({"model": {"generator": V.state_dict()}}, dec_dir / "checkpoint-1steps.pkl")
        (dec_dir / "config.yml").write_text(yaml.safe_dump({"model_type": "HiFiGAN", "generator_params": dict(V1)}))
        dec_ckpt = dec_dir / "checkpoint-1steps.pkl"
    else:
        dec_ckpt = enc_dir / "checkpoint-1steps.pkl"
    codec = AudioDec(tx_device=str(gpu), rx_device=str(gpu), receptive_length=900)
    codec.load_transmitter(str(enc_dir / "checkpoint-1steps.pkl"))
    codec.load_receiver(str(enc_dir / "checkpoint-1steps.pkl"), str(dec_ckpt))
    tx, rx = codec.open_session(batch=1, chunk=300)
    ptx, prx = codec.open_pool(capacity=capacity, chunk=300)
    assert isinstance(ptx, StreamPool) and isinstance(prx, VocoderPool if decoder == "HiFiGAN" else StreamPool)
    assert prx.lookup_generator is codec.rx_encoder
    if capacity > 1:
        for p in (ptx, prx):
            p.open()                  # slot 0 stays idle
    st, sr = ptx.open(), prx.open()
    assert (st, sr) == ((1, 1) if capacity > 1 else (0, 0))
    assert float(sum(v.abs().sum() for v in prx.state(sr).values())) > 0   # the warm-up state came with open()
    x = torch.from_numpy(ga["x"]).to(gpu)
    for c in range(3):
        xc = x[:, :, 300 * c:300 * (c + 1)]
        z, zp = tx.encode(xc), ptx.encode([st], xc)
        assert _same(z, zp), c
        idx, idxp = tx.quantize(z), ptx.quantize(zp)
        assert torch.equal(idx.view(idxp.shape), idxp), c
        y, yp = rx.decode(rx.lookup(idx)), prx.decode([sr], prx.lookup(idxp))
        assert tuple(yp.shape) == (1, 1, 300) and _same(y, yp), c


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_capacity_one_pool(gpu, graph):
    """The smallest pool: one slot and the template.  Open, three hops, close,
    reopen: both streams equal fresh solo sessions bitwise; a second open raises."""
    from sel import SelError
    from sel.streaming import StreamSession
    G = _stream_model(gpu)
    pool = G.pool(1, 300, graph=graph)
    x = 0.1 * torch.randn(2, 3, 1, 1, 300, generator=torch.Generator().manual_seed(9)).to(gpu)
    for stream in range(2):
        assert pool.open() == 0
        with pytest.raises(SelError, match="full"):
            pool.open()
        S = StreamSession(G, 1, 300, graph=False)
        for c in range(3):
            z, zs = pool.encode([0], x[stream, c]), S.encode(x[stream, c])
            assert _same(z, zs), (stream, c)
            idx = S.quantize(zs)
            assert torch.equal(pool.quantize(z).view(idx.shape), idx)
            assert _same(pool.decode([0], pool.lookup(idx)), S.decode(S.lookup(idx))), (stream, c)
        assert pool.encode([], x[0, 0][:0]).shape[0] == 0
        pool.close(0)


def test_failed_open_releases_the_slot(gpu, monkeypatch):
    """open() takes the slot only once its state is in place: if the template
    copy fails, the slot is free again and the next open() returns it."""
    from sel import streamops as SO
    G = _stream_model(gpu)
    pool = G.pool(2, 300, graph=False)
    assert pool.open() == 0

    def boom(*a, **k):
        raise RuntimeError("copy failed")
    monkeypatch.setattr(SO, "copy_slots", boom)
    with pytest.raises(RuntimeError, match="copy failed"):
        pool.open()
    monkeypatch.undo()
    assert len(pool.table) == 1 and not pool.table.is_open(1)
    assert pool.open() == 1


def test_pool_errors(gpu):
    from sel import SelError
    G = _stream_model(gpu)
    pool = G.pool(2, 300, graph=False)
    a, b = pool.open(), pool.open()
    with pytest.raises(SelError, match="full"):
        pool.open()
    x = torch.zeros(1, 1, 300, device=gpu)
    pool.encode([a], x)
    pool.close(a)
    with pytest.raises(SelError, match="not open"):
        pool.encode([a], x)
    with pytest.raises(SelError, match="not open"):
        pool.decode([a], torch.zeros(1, 1, 64, device=gpu))
    with pytest.raises(SelError, match="takes"):
        pool.encode([b], torch.zeros(1, 1, 299, device=gpu))
    with pytest.raises(SelError, match="takes"):
        pool.encode([b], torch.zeros(2, 1, 300, device=gpu))
    with pytest.raises(SelError, match="takes"):
        pool.decode([b], torch.zeros(1, 2, 64, device=gpu))
    with pytest.raises(SelError, match="duplicate"):
        pool.encode([b, b], torch.zeros(2, 1, 300, device=gpu))
    with pytest.raises(SelError, match="out of range"):
        pool.encode([2], x)           # the template row is no stream
    with pytest.raises(SelError, match="device"):
        pool.encode([b], x.cpu())
    assert pool.open() == a
