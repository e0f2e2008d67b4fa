"""Packets inside the hop: ``enable_codes(wire=True)`` / ``transmit_packets`` /
``receive_packets`` of the streaming sessions and pools (sel.streaming,
csrc/vq_step.hip) on the GPU.

The references are tests/wire_ref.py (the format in plain Python integers) and
a TWIN object in the same state that runs the existing ``transmit`` /
``receive``: ``transmit_packets(x)`` must equal wire_ref.pack of the twin's
``transmit(x)`` byte for byte (carries afterwards equal), ``receive_packets(p)``
must be bitwise the twin's ``receive(idx)``.  Fixtures as
tests/test_gpu_stream_codes.py: golden width with the golden's weights at B = 1
and 3, full width at B = 1, fp32 and bf16, eager and graph; the golden stream at
chunk 600 (two records per packet; ``y`` within that file's 1e-5); the v1
vocoder with and without stats; pools on the schedule of
tests/test_gpu_stream_pool.py against solo eager sessions; the facade; errors."""
import numpy as np
import pytest
import torch

import wire_ref as WR
from conftest import golden
from test_gpu_stream_codes import _carries_equal, _gen, _vocoder
from test_gpu_stream_pool import _run_schedule, _same
from test_gpu_stream_session import GP, _stream_model, nclose
from test_gpu_vocoder_session import V1, _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _sk(G):
    rvq = G.quantizer.codebook
    return len(rvq.layers), rvq.layers[0].embed.shape[1]


def _packets_of(idx, S, K, batch):
    """wire_ref's packets (batch, packet_bytes) of flattened ids (S, [batch,] frames)"""
    rows = WR.pack(idx.reshape(S, -1).cpu(), K, flattened=True)
    return rows.view(batch, idx.shape[-1] * rows.shape[1])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width,batch", [("golden", 1), ("full", 1), ("golden", 3)])
def test_session_transmit_and_receive_packets(gpu, width, batch, dtype, graph):
    from sel.streaming import StreamSession
    G = _gen(width)
    S, K = _sk(G)
    new = StreamSession(G, batch, 300, graph=graph, dtype=dtype)
    new.enable_codes(wire=True)
    twin = StreamSession(G, batch, 300, graph=graph, dtype=dtype)
    twin.enable_codes()
    w = new.wire
    assert twin.wire is None and (w.codebooks, w.codebook_size, w.frames, w.version) == (S, K, 1, 1)
    assert w.frame_bytes == WR.frame_bytes(S, K) == w.packet_bytes
    x = 0.1 * torch.randn(3, batch, 1, 300, generator=torch.Generator().manual_seed(17)).to(gpu)
    for c in range(3):
        idx = twin.transmit(x[c]).clone()
        p = new.transmit_packets(x[c])
        assert p.dtype == torch.uint8 and tuple(p.shape) == (batch, w.packet_bytes) and p.is_cuda
        want = _packets_of(idx, S, K, batch)
        assert torch.equal(p.cpu(), want), (c, p.cpu(), want)
        assert torch.equal(w.unpack(p.cpu()).view(idx.shape), idx.cpu())
        y = new.receive_packets(p.clone())
        assert tuple(y.shape) == (batch, 1, 300) and _same(y, twin.receive(idx)), c
    _carries_equal(new, twin)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wire_object_keeps_the_bits_of_transmit_and_receive(gpu, dtype, graph):
    """transmit / receive on a wire=True object against a wire=False object, and the
    two receiver graphs of one object taking turns on one state"""
    from sel.streaming import StreamSession
    G = _gen("golden")
    new = StreamSession(G, 3, 300, graph=graph, dtype=dtype)
    new.enable_codes(wire=True)
    old = StreamSession(G, 3, 300, graph=graph, dtype=dtype)
    old.enable_codes()
    x = 0.1 * torch.randn(4, 3, 1, 300, generator=torch.Generator().manual_seed(18)).to(gpu)
    for c in range(4):
        want = old.transmit(x[c]).clone()
        idx = new.transmit(x[c]).clone()
        assert torch.equal(idx, want), c
        y_want = old.receive(want)
        y = new.receive(idx) if c % 2 == 0 else new.receive_packets(new.wire.pack(idx.cpu()).to(gpu))
        assert _same(y, y_want), c
    _carries_equal(new, old)


def test_golden_stream_packets_come_out_exactly(gpu):
    g = golden("stream")
    G = _stream_model(gpu, g)
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=True, codes=True, wire=True)
    S.load_state()
    assert (S.wire.frames, S.wire.frame_bytes, S.wire.packet_bytes) == (2, 2, 4)
    x = torch.from_numpy(g["x"]).to(gpu)
    for c in range(6):
        p = S.transmit_packets(x[:, :, 600 * c:600 * (c + 1)])
        want = WR.pack(torch.from_numpy(np.asarray(g[f"idx.{c}"])), GP["codebook_size"], flattened=True).view(1, 4)
        assert torch.equal(p.cpu(), want), (c, p.cpu(), want)
        nclose(S.receive_packets(p), g[f"y.{c}"], 1e-5, f"y.{c}")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
def test_vocoder_session_receive_packets(gpu, tmp_path, stats, dtype, graph):
    from sel.streaming import VocoderSession
    V, E = _vocoder(gpu, stats, tmp_path), _gen("golden")
    new = VocoderSession(V, 2, 1, graph=graph, dtype=dtype)
    new.enable_codes(lookup_generator=E, wire=True)
    twin = VocoderSession(V, 2, 1, graph=graph, dtype=dtype)
    twin.enable_codes(lookup_generator=E)
    K, S = GP["codebook_size"], GP["codebook_num"]
    assert (new.wire.codebooks, new.wire.codebook_size, new.wire.frames) == (S, K, 1)
    gen = torch.Generator().manual_seed(23)
    for c in range(3):
        idx = torch.randint(0, K, (S, 2, 1), generator=gen) + K * torch.arange(S).view(-1, 1, 1)
        p = _packets_of(idx, S, K, 2).to(gpu)
        y = new.receive_packets(p)
        assert tuple(y.shape) == (2, 1, 300) and y.dtype == torch.float32
        assert _same(y, twin.receive(idx.to(gpu))), c
    _carries_equal(new, twin)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_pool_packets_equal_solo_sessions(gpu, dtype, graph):
    from sel.streaming import StreamPool, StreamSession
    G = _gen("golden")
    S, K = _sk(G)
    pool = StreamPool(G, 4, 300, graph=graph, dtype=dtype)
    pool.enable_codes(wire=True)
    nb = pool.wire.packet_bytes
    gen = torch.Generator().manual_seed(5)
    data = {n: 0.1 * torch.randn(8, 1, 1, 300, generator=gen).to(gpu) for n in "ABCDE"}

    def solo():
        s = StreamSession(G, 1, 300, graph=False, dtype=dtype)
        s.enable_codes()
        return s

    def step_pool(slots, x):
        p = pool.transmit_packets(slots, x)
        assert tuple(p.shape) == (len(slots), nb) and p.dtype == torch.uint8
        p = p.clone()
        y = pool.receive_packets(slots, p)
        assert tuple(y.shape) == (len(slots), 1, 300)
        return () if not slots else (p.long(), y)

    def step_solo(s, x):
        idx = s.transmit(x).clone()
        return _packets_of(idx, S, K, 1).long().to(gpu), s.receive(idx)

    _run_schedule(pool, solo, lambda n, k: data[n][k], step_pool, step_solo)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vocoder_pool_packets_equal_solo_sessions(gpu, tmp_path, dtype, graph):
    from sel.streaming import VocoderPool, VocoderSession
    V, E = _vocoder(gpu, True, tmp_path), _gen("golden")
    pool = VocoderPool(V, 4, 1, graph=graph, dtype=dtype)
    pool.enable_codes(lookup_generator=E, wire=True)
    K, S = GP["codebook_size"], GP["codebook_num"]
    gen = torch.Generator().manual_seed(6)
    data = {n: torch.randint(0, K, (8, 1, S, 1), generator=gen) + K * torch.arange(S).view(1, 1, S, 1) for n in "ABCDE"}

    def solo():
        s = VocoderSession(V, 1, 1, graph=False, dtype=dtype)
        s.enable_codes(lookup_generator=E)
        return s

    def step_pool(slots, idx):                     # idx (n, S, 1) on the CPU
        p = _packets_of(idx.transpose(0, 1), S, K, len(slots)).to(gpu)
        y = pool.receive_packets(slots, p)
        assert tuple(y.shape) == (len(slots), 1, 300) and y.dtype == torch.float32
        return (y,)

    _run_schedule(pool, solo, lambda n, k: data[n][k], step_pool, lambda s, idx: (s.receive(idx[0].to(gpu)),))


def test_enable_codes_wire_after_load_state_moves_no_state(gpu):
    G = _stream_model(gpu, golden("stream"))
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=True)
    S.load_state()
    before = {k: v.clone() for k, v in S.carries().items()}
    assert sum(float(v.abs().sum()) for v in before.values()) > 0
    S.enable_codes(wire=True)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in S.carries().items())
    pool = G.pool(3, 600, graph=True)
    pool.load_state()
    a, b = pool.open(), pool.open()
    x = 0.1 * torch.randn(2, 1, 1, 600, generator=torch.Generator().manual_seed(2)).to(gpu)
    pool.encode([b], x[0])
    torch.cuda.synchronize()
    before = [c.clone() for c in pool._carries]             # every slot row and the template row
    assert sum(float(c[pool.capacity].abs().sum()) for c in before) > 0
    pool.enable_codes(wire=True)
    torch.cuda.synchronize()
    assert all(torch.equal(c, d) for c, d in zip(pool._carries, before))
    # and the pool goes on where it was: slot b's next hop equals a pool that never enabled codes
    ref = G.pool(3, 600, graph=False)
    ref.load_state()
    ref.open()
    rb = ref.open()
    ref.encode([rb], x[0])
    want = ref.quantize(ref.encode([rb], x[1]))
    assert torch.equal(pool.transmit_packets([b], x[1]).cpu(), _packets_of(want, 2, GP["codebook_size"], 1))


@pytest.mark.parametrize("decoder", ["symAudioDec", "HiFiGAN"])
def test_facade_opens_sessions_and_pools_with_wire(gpu, tmp_path, decoder):
    import yaml
    from models.autoencoder.AudioDec import StreamGenerator as Encoder
    from utils.audiodec import AudioDec
    ga = golden("audiodec_baseline")
    enc_dir, dec_dir = tmp_path / "enc", tmp_path / "dec"
    enc_dir.mkdir()
    dec_dir.mkdir()
    E = Encoder(**GP)
    E.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in ga.items() if k.startswith("sd.")}, strict=True)
    torch.save({"model": {"generator": E.state_dict()}}, enc_dir / "checkpoint-1steps.pkl")
    (enc_dir / "config.yml").write_text(yaml.safe_dump({"model_type": "symAudioDec", "generator_params": dict(GP)}))
    dec_ckpt = enc_dir / "checkpoint-1steps.pkl"
    if decoder == "HiFiGAN":
        V, _ = _model("vocoder_v1", V1, "cpu")
        V.reset_buffer()
        torch.save({"model": {"generator": V.state_dict()}}, dec_dir / "checkpoint-1steps.pkl")
        (dec_dir / "config.yml").write_text(yaml.safe_dump({"model_type": "HiFiGAN", "generator_params": dict(V1)}))
        dec_ckpt = dec_dir / "checkpoint-1steps.pkl"
    codec = AudioDec(tx_device=str(gpu), rx_device=str(gpu), receptive_length=900)
    codec.load_transmitter(str(enc_dir / "checkpoint-1steps.pkl"))
    codec.load_receiver(str(enc_dir / "checkpoint-1steps.pkl"), str(dec_ckpt))
    tx0, rx0 = codec.open_session(batch=1, chunk=300, codes=True)       # the twin: indices
    assert tx0.wire is None and rx0.wire is None
    tx, rx = codec.open_session(batch=1, chunk=300, codes=True, wire=True)
    ptx, prx = codec.open_pool(capacity=2, chunk=300, codes=True, wire=True)
    S, K = GP["codebook_num"], GP["codebook_size"]
    for o in (tx, rx, ptx, prx):
        assert (o.wire.codebooks, o.wire.codebook_size, o.wire.frames) == (S, K, 1)
    for p in (ptx, prx):
        p.open()                      # slot 0 stays idle
    st, sr = ptx.open(), prx.open()
    x = torch.from_numpy(ga["x"]).to(gpu)
    for c in range(3):
        xc = x[:, :, 300 * c:300 * (c + 1)]
        idx = tx0.transmit(xc).clone()
        want = _packets_of(idx, S, K, 1)
        p = tx.transmit_packets(xc).clone()
        pp = ptx.transmit_packets([st], xc).clone()
        assert torch.equal(p.cpu(), want) and torch.equal(pp.cpu(), want), c
        y_want = rx0.receive(idx)
        y, yp = rx.receive_packets(p), prx.receive_packets([sr], pp)
        assert tuple(y.shape) == tuple(yp.shape) == (1, 1, 300)
        assert _same(y, y_want) and _same(yp, y_want), c


def test_error_paths(gpu):
    from models.autoencoder_without_PQC.AudioDec import StreamGenerator as NoPQC
    from sel import SelError
    G = _gen("golden")
    x = torch.zeros(1, 1, 300, device=gpu)
    p = torch.zeros(1, 2, dtype=torch.uint8, device=gpu)
    S = G.session(1, 300, graph=False)
    with pytest.raises(SelError, match="enable_codes"):
        S.transmit_packets(x)
    with pytest.raises(SelError, match="enable_codes"):
        S.receive_packets(p)
    S.enable_codes()                                     # codes, but no wire
    with pytest.raises(SelError, match="wire=True"):
        S.transmit_packets(x)
    with pytest.raises(SelError, match="wire=True"):
        S.receive_packets(p)
    pool = G.pool(2, 300, graph=False, codes=True)
    a = pool.open()
    with pytest.raises(SelError, match="wire=True"):
        pool.transmit_packets([a], x)
    with pytest.raises(SelError, match="wire=True"):
        pool.receive_packets([a], p)
    # a plan without PQC: encode's output is no code vector
    torch.manual_seed(3)
    N = NoPQC(encode_channels=8, decode_channels=8, code_dim=64, codebook_num=2, codebook_size=64).to(gpu).eval()
    Sn = N.session(1, 1200, graph=False, codes=True, wire=True)
    with pytest.raises(SelError, match="PQC"):
        Sn.transmit_packets(torch.zeros(1, 1, 1200, device=gpu))
    # a vocoder: no transmitter, and no lookup codebook known
    V, _ = _model("vocoder_v1", V1, gpu)
    Sv = V.session(1, 1, graph=False, codes=True, wire=True)
    with pytest.raises(SelError, match="PQC"):
        Sv.transmit_packets(x)
    with pytest.raises(SelError, match="lookup"):
        Sv.receive_packets(p)
    Pv = V.pool(2, 1, graph=False, codes=True, wire=True)
    with pytest.raises(SelError, match="lookup"):
        Pv.receive_packets([Pv.open()], p)
    # operand checks of the enabled methods
    S.enable_codes(wire=True)
    assert S.wire.packet_bytes == 2
    with pytest.raises(SelError, match="takes"):
        S.transmit_packets(torch.zeros(1, 1, 299, device=gpu))
    with pytest.raises(SelError, match="takes"):
        S.receive_packets(p.int())
    with pytest.raises(SelError, match="takes"):
        S.receive_packets(torch.zeros(1, 3, dtype=torch.uint8, device=gpu))
    with pytest.raises(SelError, match="takes"):
        S.receive_packets(p.view(2))
    with pytest.raises(SelError, match="device"):
        S.receive_packets(p.cpu())
    pool.enable_codes(wire=True)
    with pytest.raises(SelError, match="takes"):
        pool.receive_packets([a], torch.zeros(2, 2, dtype=torch.uint8, device=gpu))
