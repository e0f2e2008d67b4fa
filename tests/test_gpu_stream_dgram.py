"""Datagrams inside the hop: ``enable_codes(datagrams=True)`` /
``transmit_datagrams`` / ``receive_datagrams`` of the streaming sessions and
pools (sel.streaming, csrc/vq_step.hip) on the GPU.

The references are tests/dgram_ref.py (wire version 2 in plain Python integers)
and a TWIN object in the same state that runs the existing ``transmit`` /
``receive``: a datagram must equal dgram_ref's of the twin's ``transmit(x)[:s]``
byte for byte, ``receive_datagrams`` must be bitwise the twin's ``receive`` on
the ids padded with -1 beyond the stages carried, and on a lost hop the twin's
``receive`` on the last good record's ids repeated over the frames (nothing
held: all -1).  Fixtures as tests/test_gpu_stream_wire.py."""
import numpy as np
import pytest
import torch

import dgram_ref as DR
from conftest import golden
from test_gpu_stream_codes import _carries_equal, _gen, _vocoder
from test_gpu_stream_pool import _run_schedule, _same
from test_gpu_stream_session import GP, _stream_model, nclose
from test_gpu_vocoder_session import V1, _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
LOST = [0, 0, 1, 1, 0]                                   # the receiver's five hops: ok, ok, lost, lost, ok


def _sk(G):
    rvq = G.quantizer.codebook
    return len(rvq.layers), rvq.layers[0].embed.shape[1]


def _budgets(S):
    return [min(b, S) for b in (S, 3, 1, S, 2)]          # the transmitter's five hops


def _codes(idx, S, K, batch):
    """flattened ids (S, [batch,] frames) -> un-flattened codes (S, batch, frames) on the CPU"""
    return idx.reshape(S, batch, -1).cpu() - K * torch.arange(S).view(-1, 1, 1)


def _cut(codes, K, stages):
    """un-flattened codes (S, batch, frames) -> flattened ids with -1 beyond each stream's stages"""
    S = codes.shape[0]
    ids = codes + K * torch.arange(S).view(-1, 1, 1)
    for i, s in enumerate(stages):
        ids[s:, i] = -1
    return ids


class _Concealer:
    """What a receiver must decode, hop by hop, from the references alone."""

    def __init__(self, S, batch, frames):
        self.held = [torch.full((S, frames), -1, dtype=torch.int64) for _ in range(batch)]

    def ids(self, cut, lost):
        out = cut.clone()
        for i, gone in enumerate(lost):
            if gone:
                out[:, i] = self.held[i]
            else:
                self.held[i] = cut[:, i, -1:].expand(-1, cut.shape[2]).clone()
        return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width,batch", [("golden", 1), ("full", 1), ("golden", 3)])
def test_session_five_hop_schedule(gpu, width, batch, dtype, graph):
    from sel.streaming import StreamSession
    G = _gen(width)
    S, K = _sk(G)
    new = StreamSession(G, batch, 300, graph=graph, dtype=dtype)
    new.enable_codes(datagrams=True)
    twin = StreamSession(G, batch, 300, graph=graph, dtype=dtype)
    twin.enable_codes()
    f = new.datagram
    assert twin.datagram is None and new.wire is None
    assert (f.codebooks, f.codebook_size, f.frames, f.version, f.stride) == (S, K, 1, 2, DR.dgram_bytes(S, K, 1))
    x = 0.1 * torch.randn(5, batch, 1, 300, generator=torch.Generator().manual_seed(17)).to(gpu)
    budgets, conceal = _budgets(S), _Concealer(S, batch, 1)
    count = [dict(received=0, lost=0, run=0) for _ in range(batch)]
    for c in range(5):
        st = [budgets[(c + i) % 5] for i in range(batch)]             # stream i runs the schedule i hops ahead
        lost = [LOST[(c + 2 * i) % 5] for i in range(batch)]          # stream 1 loses its very first hop
        idx = twin.transmit(x[c]).clone()
        p = new.transmit_datagrams(x[c], st[0] if batch == 1 else st)
        assert p.dtype == torch.uint8 and tuple(p.shape) == (batch, f.stride) and p.is_cuda
        codes = _codes(idx, S, K, batch)
        want = DR.pack(codes.reshape(S, -1), st, [c] * batch, K, 1)
        got = f.split(p.cpu())
        assert got == want, (c, got, want)
        assert [f.parse(d) for d in got] == [(s, c) for s in st]
        ids = conceal.ids(_cut(codes, K, st), lost)
        if c % 2 == 0:                                                # a device tensor with flags ...
            y = new.receive_datagrams(p.clone(), lost if any(lost) or c else None)
        else:                                                         # ... a list with None, through the CPU
            y = new.receive_datagrams([None if gone else d for d, gone in zip(got, lost)])
        y_want = twin.receive(ids.reshape(idx.shape).to(gpu))
        assert tuple(y.shape) == (batch, 1, 300) and _same(y, y_want), c
        for i, gone in enumerate(lost):
            count[i]["lost" if gone else "received"] += 1
            count[i]["run"] = count[i]["run"] + 1 if gone else 0
    _carries_equal(new, twin)
    stats = new.datagram_stats()
    assert len(stats) == batch
    for i, s in enumerate(stats):
        assert (s["received"], s["lost"], s["concealed_run"]) == (count[i]["received"], count[i]["lost"],
                                                                  count[i]["run"]), (i, s)
        assert s["refused"] == 0 and s["received"] + s["lost"] == 5
    # headers are read on the host: stream 0's last datagram given as bytes was hop 1's (hop 3 was lost)
    assert stats[0]["stages"] == budgets[1] and stats[0]["seq"] == 1 and stats[0]["seq_gaps"] == 0
    # reset(): hop numbers, counters and the held records start over
    new.reset()
    twin.reset()
    assert new.datagram_stats()[0] == dict(received=0, lost=0, refused=0, seq_gaps=0, concealed_run=0, stages=None,
                                           seq=None)
    y = new.receive_datagrams([None] * batch)
    assert _same(y, twin.receive(torch.full_like(idx, -1)))
    assert [f.parse(d)[1] for d in f.split(new.transmit_datagrams(x[0]).cpu())] == [0] * batch


def test_receiver_counts_gaps_and_refusals(gpu):
    G = _gen("golden")
    S, K = _sk(G)
    rx = G.session(2, 300, graph=True, codes=True, datagrams=True)
    twin = G.session(2, 300, graph=True, codes=True)
    f = rx.datagram
    gen = torch.Generator().manual_seed(3)
    conceal = _Concealer(S, 2, 1)
    hops = [([65534, 10], [S, 1], None), ([65535, 11], [1, S], None), ([2, 12], [S, S], "version"),
            ([3, 13], [S, S], "short"), ([4, 20], [1, 1], None)]
    for seq, st, damage in hops:
        codes = torch.randint(0, K, (S, 2, 1), generator=gen)
        d = DR.pack(codes.reshape(S, -1), st, seq, K, 1)
        lost = [0, 0]
        if damage:                                        # stream 0's datagram arrives damaged
            d[0] = bytes([3]) + d[0][1:] if damage == "version" else d[0][:-1]
            lost[0] = 1
        y = rx.receive_datagrams(d)
        ids = conceal.ids(_cut(codes, K, st), lost)
        assert _same(y, twin.receive(ids.to(gpu)))
    a, b = rx.datagram_stats()
    assert a == dict(received=3, lost=2, refused=2, seq_gaps=4, concealed_run=0, stages=1, seq=4)     # 65535 -> 4
    assert b == dict(received=5, lost=0, refused=0, seq_gaps=6, concealed_run=0, stages=1, seq=20)    # 13 -> 20
    assert f.stride == DR.dgram_bytes(S, K, 1)


def test_golden_stream_datagrams_come_out_exactly(gpu):
    g = golden("stream")
    G = _stream_model(gpu, g)
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=True, codes=True, datagrams=True)
    S.load_state()
    f, K = S.datagram, GP["codebook_size"]
    assert (f.frames, f.frame_bytes(), f.stride) == (2, 2, 8)
    x = torch.from_numpy(g["x"]).to(gpu)
    for c in range(6):
        p = S.transmit_datagrams(x[:, :, 600 * c:600 * (c + 1)])
        idx = torch.from_numpy(np.asarray(g[f"idx.{c}"]))                 # (S, frames), flattened
        want = DR.pack(idx - K * torch.arange(2).view(-1, 1), [2], [c], K, 2)
        assert f.split(p.cpu()) == want, (c, p.cpu(), want)
        nclose(S.receive_datagrams(p), g[f"y.{c}"], 1e-5, f"y.{c}")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_datagram_object_keeps_the_bits_of_the_other_methods(gpu, dtype, graph):
    """transmit / receive / *_packets on a datagrams=True object against a plain one, and
    the three receiver graphs of one object taking turns on one state"""
    from sel.streaming import StreamSession
    G = _gen("golden")
    S, K = _sk(G)
    new = StreamSession(G, 3, 300, graph=graph, dtype=dtype)
    new.enable_codes(wire=True, datagrams=True)
    old = StreamSession(G, 3, 300, graph=graph, dtype=dtype)
    old.enable_codes(wire=True)
    x = 0.1 * torch.randn(6, 3, 1, 300, generator=torch.Generator().manual_seed(18)).to(gpu)
    for c in range(6):
        want = old.transmit(x[c]).clone()
        if c % 3 == 0:
            idx = new.transmit(x[c]).clone()
        elif c % 3 == 1:
            idx = new.wire.unpack(new.transmit_packets(x[c]).cpu()).view(want.shape).to(gpu)
        else:
            d = new.datagram.split(new.transmit_datagrams(x[c]).cpu())
            # the second call finds its control words in place: the hop number advanced on the device
            assert [new.datagram.parse(e) for e in d] == [(S, c // 3)] * 3
            idx = torch.stack([new.datagram.unpack(e) for e in d], 1).to(gpu)
        assert torch.equal(idx, want), c
        y_want = old.receive(want)
        if c % 3 == 0:
            y = new.receive(idx)
        elif c % 3 == 1:
            y = new.receive_packets(new.wire.pack(idx.cpu()).to(gpu))
        else:
            y = new.receive_datagrams(new.datagram.pack(idx.cpu(), S, c))
        assert _same(y, y_want), c
    _carries_equal(new, old)
    assert torch.equal(new.transmit_packets(x[0]), old.transmit_packets(x[0]))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
def test_vocoder_session_receive_datagrams(gpu, tmp_path, stats, dtype, graph):
    from sel.streaming import VocoderSession
    V, E = _vocoder(gpu, stats, tmp_path), _gen("golden")
    new = VocoderSession(V, 2, 1, graph=graph, dtype=dtype)
    new.enable_codes(lookup_generator=E, datagrams=True)
    twin = VocoderSession(V, 2, 1, graph=graph, dtype=dtype)
    twin.enable_codes(lookup_generator=E)
    K, S = GP["codebook_size"], GP["codebook_num"]
    f = new.datagram
    assert (f.codebooks, f.codebook_size, f.frames) == (S, K, 1)
    gen = torch.Generator().manual_seed(23)
    conceal = _Concealer(S, 2, 1)
    for c, (st, lost) in enumerate([([S, 1], [0, 1]), ([1, S], [0, 0]), ([S, S], [1, 0]), ([1, 1], [1, 1])]):
        codes = torch.randint(0, K, (S, 2, 1), generator=gen)
        d = DR.pack(codes.reshape(S, -1), st, [c, c], K, 1)
        ids = conceal.ids(_cut(codes, K, st), lost)                  # hop 0, stream 1: nothing held, the empty sum
        if c % 2:
            y = new.receive_datagrams(DR.buffer(d, f.stride).to(gpu), lost)
        else:
            y = new.receive_datagrams([None if gone else e for e, gone in zip(d, lost)])
        assert tuple(y.shape) == (2, 1, 300) and y.dtype == torch.float32
        assert _same(y, twin.receive(ids.to(gpu))), c
    _carries_equal(new, twin)


def _knobs(v, S):
    """a budget and a loss flag per stream and hop, read off the hop's own data so that the
    pool and the solo side agree without sharing state"""
    n = int(v)
    return 1 + n % S, n % 3 == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_pool_datagrams_equal_solo_sessions(gpu, dtype, graph):
    from sel.streaming import StreamPool, StreamSession
    G = _gen("golden")
    S, K = _sk(G)
    pool = StreamPool(G, 4, 300, graph=graph, dtype=dtype)
    pool.enable_codes(datagrams=True)
    f = pool.datagram
    gen = torch.Generator().manual_seed(5)
    data = {n: 0.1 * torch.randn(8, 1, 1, 300, generator=gen).to(gpu) for n in "ABCDE"}

    def knobs(x):                                                  # x (n, 1, 300)
        return [_knobs(abs(float(v)) * 1e4, S) for v in x[:, 0, 0].tolist()]

    def solo():
        s = StreamSession(G, 1, 300, graph=False, dtype=dtype)
        s.enable_codes()
        s.t_conceal, s.t_hop = _Concealer(S, 1, 1), 0
        return s

    def step_pool(slots, x):
        kn = knobs(x)
        p = pool.transmit_datagrams(slots, x, [b for b, _ in kn])
        assert tuple(p.shape) == (len(slots), f.stride) and p.dtype == torch.uint8
        d = f.split(p.cpu())
        y = pool.receive_datagrams(slots, [None if gone else e for e, (_, gone) in zip(d, kn)])
        assert tuple(y.shape) == (len(slots), 1, 300)
        return () if not slots else (DR.buffer(d, f.stride, 0).long().to(gpu), y)

    def step_solo(s, x):
        (budget, gone), = knobs(x)
        codes = _codes(s.transmit(x), S, K, 1)
        d = DR.pack(codes.reshape(S, -1), [budget], [s.t_hop], K, 1)
        s.t_hop += 1
        ids = s.t_conceal.ids(_cut(codes, K, [budget]), [gone])
        return DR.buffer(d, f.stride, 0).long().to(gpu), s.receive(ids.reshape(S, 1).to(gpu))

    slot = _run_schedule(pool, solo, lambda n, k: data[n][k], step_pool, step_solo)
    st = pool.datagram_stats(slot["A"])
    assert st["received"] + st["lost"] == 7 and st["refused"] == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vocoder_pool_datagrams_equal_solo_sessions(gpu, tmp_path, dtype, graph):
    from sel.streaming import VocoderPool, VocoderSession
    V, E = _vocoder(gpu, True, tmp_path), _gen("golden")
    pool = VocoderPool(V, 4, 1, graph=graph, dtype=dtype)
    pool.enable_codes(lookup_generator=E, datagrams=True)
    K, S = GP["codebook_size"], GP["codebook_num"]
    f = pool.datagram
    gen = torch.Generator().manual_seed(6)
    data = {n: torch.randint(0, K, (8, 1, S, 1), generator=gen) for n in "ABCDE"}      # un-flattened codes

    def solo():
        s = VocoderSession(V, 1, 1, graph=False, dtype=dtype)
        s.enable_codes(lookup_generator=E)
        s.t_conceal = _Concealer(S, 1, 1)
        return s

    def step_pool(slots, codes):                   # codes (n, S, 1) on the CPU
        kn = [_knobs(v, S) for v in codes[:, 0, 0].tolist()]
        d = DR.pack(codes[:, :, 0].t().contiguous(), [b for b, _ in kn], [7] * len(slots), K, 1)
        lost = [int(gone) for _, gone in kn]
        if len(slots) % 2:
            y = pool.receive_datagrams(slots, DR.buffer(d, f.stride).to(gpu), lost)
        else:
            y = pool.receive_datagrams(slots, [None if gone else e for e, gone in zip(d, lost)])
        assert tuple(y.shape) == (len(slots), 1, 300) and y.dtype == torch.float32
        return (y,)

    def step_solo(s, codes):
        (budget, gone), = [_knobs(v, S) for v in codes[:, 0, 0].tolist()]
        ids = s.t_conceal.ids(_cut(codes.transpose(0, 1), K, [budget]), [gone])
        return (s.receive(ids.to(gpu)),)

    _run_schedule(pool, solo, lambda n, k: data[n][k], step_pool, step_solo)


def test_reopened_slot_starts_from_nothing(gpu):
    G = _gen("golden")
    S, K = _sk(G)
    pool = G.pool(2, 300, graph=True, codes=True, datagrams=True)
    f = pool.datagram
    x = 0.1 * torch.randn(3, 1, 1, 300, generator=torch.Generator().manual_seed(8)).to(gpu)
    a = pool.open()
    for c in range(2):
        p = pool.transmit_datagrams([a], x[c]).clone()
        assert f.parse(f.split(p.cpu())[0]) == (S, c)
        pool.receive_datagrams([a], p)
    assert int(pool._rx.hold[a, 0]) == S and pool.datagram_stats(a)["received"] == 2
    pool.close(a)
    b = pool.open()
    assert b == a and int(pool._rx.hold[b, 0]) == 0
    assert pool.datagram_stats(b) == dict(received=0, lost=0, refused=0, seq_gaps=0, concealed_run=0, stages=None,
                                          seq=None)
    fresh = G.session(1, 300, graph=False, codes=True)
    y = pool.receive_datagrams([b], [None])                       # its first hop is lost: the empty sum
    assert _same(y, fresh.receive(torch.full((S, 1), -1, dtype=torch.int64, device=gpu)))
    assert pool.datagram_stats(b)["concealed_run"] == 1
    assert f.parse(f.split(pool.transmit_datagrams([b], x[2], 1).cpu())[0]) == (1, 0)      # hop number 0 again


def test_enable_codes_datagrams_after_load_state_moves_no_state(gpu):
    G = _stream_model(gpu, golden("stream"))
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=True)
    S.load_state()
    before = {k: v.clone() for k, v in S.carries().items()}
    assert sum(float(v.abs().sum()) for v in before.values()) > 0
    S.enable_codes(datagrams=True)
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
    pool.enable_codes(datagrams=True)
    torch.cuda.synchronize()
    assert all(torch.equal(c, d) for c, d in zip(pool._carries, before))
    # and the pool goes on where it was: slot b's next hop equals a pool that never enabled codes
    ref = G.pool(3, 600, graph=False)
    ref.load_state()
    ref.open()
    rb = ref.open()
    ref.encode([rb], x[0])
    want = ref.quantize(ref.encode([rb], x[1]))
    K = GP["codebook_size"]
    got = pool.datagram.split(pool.transmit_datagrams([b], x[1], 1).cpu())
    assert got == DR.pack(_codes(want, 2, K, 1).reshape(2, -1), [1], [0], K, 2)


@pytest.mark.parametrize("decoder", ["symAudioDec", "HiFiGAN"])
def test_facade_opens_sessions_and_pools_with_datagrams(gpu, tmp_path, decoder):
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
    assert tx0.datagram is None and rx0.datagram is None
    tx, rx = codec.open_session(batch=1, chunk=300, codes=True, datagrams=True)
    ptx, prx = codec.open_pool(capacity=2, chunk=300, codes=True, datagrams=True)
    S, K = GP["codebook_num"], GP["codebook_size"]
    for o in (tx, rx, ptx, prx):
        assert (o.datagram.codebooks, o.datagram.codebook_size, o.datagram.frames) == (S, K, 1) and o.wire is None
    for p in (ptx, prx):
        p.open()                      # slot 0 stays idle
    st, sr = ptx.open(), prx.open()
    x = torch.from_numpy(ga["x"]).to(gpu)
    conceal = _Concealer(S, 1, 1)
    for c, (budget, gone) in enumerate([(S, 0), (1, 0), (S, 1)]):
        xc = x[:, :, 300 * c:300 * (c + 1)]
        codes = _codes(tx0.transmit(xc), S, K, 1)
        want = DR.pack(codes.reshape(S, -1), [budget], [c], K, 1)
        p = tx.transmit_datagrams(xc, budget).clone()
        pp = ptx.transmit_datagrams([st], xc, [budget]).clone()
        assert tx.datagram.split(p.cpu()) == want and ptx.datagram.split(pp.cpu()) == want, c
        y_want = rx0.receive(conceal.ids(_cut(codes, K, [budget]), [gone]).reshape(S, 1).to(gpu))
        y, yp = rx.receive_datagrams(p, [gone]), prx.receive_datagrams([sr], pp, [gone])
        assert tuple(y.shape) == tuple(yp.shape) == (1, 1, 300)
        assert _same(y, y_want) and _same(yp, y_want), c


def test_error_paths(gpu):
    from models.autoencoder_without_PQC.AudioDec import StreamGenerator as NoPQC
    from sel import SelError
    G = _gen("golden")
    x = torch.zeros(1, 1, 300, device=gpu)
    p = torch.zeros(1, 6, dtype=torch.uint8, device=gpu)           # S = 2, K = 64: 4 + 2 bytes
    S = G.session(1, 300, graph=False)
    for call in (lambda: S.transmit_datagrams(x), lambda: S.receive_datagrams(p), S.datagram_stats):
        with pytest.raises(SelError, match="enable_codes"):
            call()
    S.enable_codes(wire=True)                            # codes and packets, but no datagrams
    for call in (lambda: S.transmit_datagrams(x), lambda: S.receive_datagrams(p), S.datagram_stats):
        with pytest.raises(SelError, match="datagrams=True"):
            call()
    pool = G.pool(2, 300, graph=False, codes=True)
    a = pool.open()
    with pytest.raises(SelError, match="datagrams=True"):
        pool.transmit_datagrams([a], x)
    with pytest.raises(SelError, match="datagrams=True"):
        pool.receive_datagrams([a], p)
    # a plan without PQC: encode's output is no code vector
    torch.manual_seed(3)
    N = NoPQC(encode_channels=8, decode_channels=8, code_dim=64, codebook_num=2, codebook_size=64).to(gpu).eval()
    Sn = N.session(1, 1200, graph=False, codes=True, datagrams=True)
    with pytest.raises(SelError, match="PQC"):
        Sn.transmit_datagrams(torch.zeros(1, 1, 1200, device=gpu))
    # a vocoder: no transmitter, and no lookup codebook known
    V, _ = _model("vocoder_v1", V1, gpu)
    Sv = V.session(1, 1, graph=False, codes=True, datagrams=True)
    with pytest.raises(SelError, match="PQC"):
        Sv.transmit_datagrams(x)
    with pytest.raises(SelError, match="lookup"):
        Sv.receive_datagrams(p)
    Pv = V.pool(2, 1, graph=False, codes=True, datagrams=True)
    with pytest.raises(SelError, match="lookup"):
        Pv.receive_datagrams([Pv.open()], p)
    # a lookup codebook of another (S, K) than the transmitter's
    other = _gen("full")
    with pytest.raises(SelError, match="transmitter packs|lookup codebook"):
        G.session(1, 300, graph=False).enable_codes(lookup_generator=other, datagrams=True)
    # operand checks of the enabled methods
    S.enable_codes(datagrams=True)
    assert S.datagram.stride == 6
    with pytest.raises(SelError, match="takes"):
        S.transmit_datagrams(torch.zeros(1, 1, 299, device=gpu))
    for stages in (0, 3, -1, [1, 2], [], 1.0, True, "2", torch.tensor([1.0]), torch.tensor([[1]])):
        with pytest.raises(SelError, match="stages"):
            S.transmit_datagrams(x, stages)
    assert S.datagram_stats()[0]["received"] == 0
    for bad in (p.int(), torch.zeros(1, 7, dtype=torch.uint8, device=gpu), p.view(6)):
        with pytest.raises(SelError, match="takes"):
            S.receive_datagrams(bad)
    with pytest.raises(SelError, match="device"):
        S.receive_datagrams(p.cpu())
    for bad in ([], [None, None], ["ab"], [3], 7, None):
        with pytest.raises(SelError, match="takes"):
            S.receive_datagrams(bad)
    for lost in ([0, 1], [], 1, ["x"], torch.tensor([0.5]), torch.zeros(1, 1, dtype=torch.int32)):
        with pytest.raises(SelError, match="lost"):
            S.receive_datagrams(p, lost)
    pool.enable_codes(datagrams=True)
    with pytest.raises(SelError, match="takes"):
        pool.receive_datagrams([a], torch.zeros(2, 6, dtype=torch.uint8, device=gpu))
    with pytest.raises(SelError, match="stages"):
        pool.transmit_datagrams([a], x, [1, 1])
    with pytest.raises(SelError):
        pool.datagram_stats(1)                               # not open
    # S > 255 does not fit the stage byte
    from sel.streaming import _CodesMixin
    with pytest.raises(SelError, match="255"):
        _CodesMixin._datagram_format(256, 4, 1)
