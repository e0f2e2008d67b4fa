"""Code indices inside the hop: ``enable_codes`` / ``transmit`` / ``receive`` of
the streaming sessions and pools (sel.streaming, csrc/vq_step.hip) on the GPU.

The oracle is existing code on a second session in the same state: ``transmit(x)``
must equal ``quantize(encode(x))`` (torch.equal, the carries afterwards too), and
``receive(idx)`` must equal ``decode(ordered_lookup(idx))`` BITWISE, where
ordered_lookup adds the codes one stage after the other in fp32 (the kernel's
contract; ``lookup`` itself uses torch.sum, whose order is torch's).  Against
today's ``decode(lookup(idx))`` the bound is the project's conv-stack one: 1e-5
norm-wise in fp32, 5e-2 in bf16.  Golden width with the golden's weights and
full width, fp32 and bf16, eager and graph; the golden stream's indices exactly;
the v1 vocoder with and without stats; pools on the schedule of
tests/test_gpu_stream_pool.py against solo eager sessions; the facade."""
import functools

import numpy as np
import pytest
import torch

import rvq_step_ref as SR
from conftest import golden
from test_gpu_stream_pool import _run_schedule, _same
from test_gpu_stream_session import FULL, GP, _stream_model, nclose
from test_gpu_vocoder_session import V1, _model

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
TOL = {torch.float32: 1e-5, torch.bfloat16: 5e-2}


@functools.lru_cache(maxsize=None)
def _gen(width):
    """golden: the golden-width generator with the golden's weights; full: full width, seed 93"""
    gpu = torch.device("cuda:0")
    return _stream_model(gpu, golden("stream")) if width == "golden" else _stream_model(gpu, None, **FULL)


def _flat(G):
    return G.quantizer.codebook.codebook          # (S*K, D), ResidualVQ.initial()'s layout


def _ordered(S, G, idx):
    """decode's input from indices: the ascending-order torch loop"""
    zq = SR.ordered_lookup(idx.reshape(idx.shape[0], -1), _flat(G))
    return zq.reshape(S.plan.batch, S.plan.frames, -1)


def _carries_equal(a, b):
    ca, cb = a.carries(), b.carries()
    assert ca.keys() == cb.keys() and len(ca) > 0
    for k in ca:
        assert _same(ca[k], cb[k]), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("width,batch", [("golden", 1), ("full", 1), ("golden", 3)])
def test_session_transmit_and_receive(gpu, width, batch, dtype, graph):
    from sel.streaming import StreamSession
    G = _gen(width)
    new = StreamSession(G, batch, 300, graph=graph, dtype=dtype)
    new.enable_codes()
    old = StreamSession(G, batch, 300, graph=False, dtype=dtype)      # decodes the ordered lookup
    today = StreamSession(G, batch, 300, graph=False, dtype=dtype)    # decode(lookup(idx)) as it is
    S = len(G.quantizer.codebook.layers)
    x = 0.1 * torch.randn(3, batch, 1, 300, generator=torch.Generator().manual_seed(17)).to(gpu)
    for c in range(3):
        want = old.quantize(old.encode(x[c]))
        idx = new.transmit(x[c])
        assert idx.dtype == torch.int64 and tuple(idx.shape) == tuple(want.shape) == ((S, 1) if batch == 1 else
                                                                                    (S, batch, 1))
        assert torch.equal(idx, want), (c, idx, want)
        idx = idx.clone()
        y = new.receive(idx)
        y_ordered = old.decode(_ordered(old, G, idx))
        assert tuple(y.shape) == (batch, 1, 300) and _same(y, y_ordered), c
        nclose(y, today.decode(today.lookup(idx)), TOL[dtype], f"y.{c}")
    _carries_equal(new, old)
    # encode / decode / quantize / lookup keep their own graphs and bits beside the new ones
    z = new.encode(x[0]).clone()
    assert _same(z, old.encode(x[0])) and torch.equal(new.quantize(z), old.quantize(z))


def test_golden_stream_indices_come_out_exactly(gpu):
    g = golden("stream")
    G = _stream_model(gpu, g)
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=True, codes=True)
    S.load_state()
    x = torch.from_numpy(g["x"]).to(gpu)
    for c in range(6):
        idx = S.transmit(x[:, :, 600 * c:600 * (c + 1)])
        np.testing.assert_array_equal(idx.cpu().numpy(), g[f"idx.{c}"])
        nclose(S.receive(idx), g[f"y.{c}"], 1e-5, f"y.{c}")


def _vocoder(gpu, stats, tmp_path):
    extra = {}
    if stats:
        g = torch.Generator().manual_seed(41)
        table = np.stack([torch.randn(64, generator=g).numpy(), (0.5 + torch.rand(64, generator=g)).numpy()])
        np.save(tmp_path / "stats.npy", table.astype(np.float32))
        extra["stats"] = str(tmp_path / "stats.npy")
    G, _ = _model("vocoder_v1", V1, gpu, **extra)
    assert bool(G.norm) == stats
    return G


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
def test_vocoder_session_receive(gpu, tmp_path, stats, dtype, graph):
    from sel.streaming import VocoderSession
    V, E = _vocoder(gpu, stats, tmp_path), _gen("golden")
    new = VocoderSession(V, 2, 1, graph=graph, dtype=dtype)
    new.enable_codes(lookup_generator=E)
    old = VocoderSession(V, 2, 1, graph=False, dtype=dtype)
    today = VocoderSession(V, 2, 1, graph=False, dtype=dtype)
    today.lookup_generator = E
    K, S = GP["codebook_size"], GP["codebook_num"]
    gen = torch.Generator().manual_seed(23)
    for c in range(3):
        idx = (torch.randint(0, K, (S, 2, 1), generator=gen) + K * torch.arange(S).view(-1, 1, 1)).to(gpu)
        y = new.receive(idx)
        assert tuple(y.shape) == (2, 1, 300) and y.dtype == torch.float32
        assert _same(y, old.decode(_ordered(old, E, idx))), c     # decode applies decode_norm itself
        nclose(y, today.decode(today.lookup(idx)), TOL[dtype], f"y.{c}")
    _carries_equal(new, old)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stream_pool_codes_equal_solo_sessions(gpu, dtype, graph):
    from sel.streaming import StreamPool, StreamSession
    G = _gen("golden")
    pool = StreamPool(G, 4, 300, graph=graph, dtype=dtype)
    pool.enable_codes()
    S = GP["codebook_num"]
    gen = torch.Generator().manual_seed(5)
    data = {n: 0.1 * torch.randn(8, 1, 1, 300, generator=gen).to(gpu) for n in "ABCDE"}

    def solo():
        s = StreamSession(G, 1, 300, graph=False, dtype=dtype)
        s.enable_codes()
        return s

    def step_pool(slots, x):
        idx = pool.transmit(slots, x)
        assert tuple(idx.shape) == (S, len(slots), 1) and idx.dtype == torch.int64
        idx = idx.clone()
        # flattened ids: stage s picks from [s K, (s + 1) K)
        assert torch.equal(idx // GP["codebook_size"], torch.arange(S, device=gpu).view(S, 1, 1).expand_as(idx))
        y = pool.receive(slots, idx)
        assert tuple(y.shape) == (len(slots), 1, 300)
        return () if not slots else (idx.transpose(0, 1), y)

    def step_solo(s, x):
        idx = s.transmit(x).clone()
        return idx.view(1, S, 1), s.receive(idx)

    _run_schedule(pool, solo, lambda n, k: data[n][k], step_pool, step_solo)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vocoder_pool_codes_equal_solo_sessions(gpu, tmp_path, dtype, graph):
    from sel.streaming import VocoderPool, VocoderSession
    V, E = _vocoder(gpu, True, tmp_path), _gen("golden")
    pool = VocoderPool(V, 4, 1, graph=graph, dtype=dtype)
    pool.enable_codes(lookup_generator=E)
    K, S = GP["codebook_size"], GP["codebook_num"]
    gen = torch.Generator().manual_seed(6)
    data = {n: (torch.randint(0, K, (8, 1, S, 1), generator=gen) + K * torch.arange(S).view(1, 1, S, 1)).to(gpu)
            for n in "ABCDE"}

    def solo():
        s = VocoderSession(V, 1, 1, graph=False, dtype=dtype)
        s.enable_codes(lookup_generator=E)
        return s

    def step_pool(slots, idx):
        y = pool.receive(slots, idx.transpose(0, 1).contiguous())
        assert tuple(y.shape) == (len(slots), 1, 300) and y.dtype == torch.float32
        return (y,)

    _run_schedule(pool, solo, lambda n, k: data[n][k], step_pool, lambda s, idx: (s.receive(idx[0]),))


def test_enable_codes_after_load_state_moves_no_state(gpu):
    G = _stream_model(gpu, golden("stream"))
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=True)
    S.load_state()
    before = {k: v.clone() for k, v in S.carries().items()}
    assert sum(float(v.abs().sum()) for v in before.values()) > 0
    S.enable_codes()
    assert all(torch.equal(v, before[k]) for k, v in S.carries().items())
    pool = G.pool(3, 600, graph=True)
    pool.load_state()
    a, b = pool.open(), pool.open()
    x = 0.1 * torch.randn(2, 1, 1, 600, generator=torch.Generator().manual_seed(2)).to(gpu)
    pool.encode([b], x[0])
    torch.cuda.synchronize()
    before = [c.clone() for c in pool._carries]             # every slot row and the template row
    assert sum(float(c[pool.capacity].abs().sum()) for c in before) > 0
    pool.enable_codes()
    torch.cuda.synchronize()
    assert all(torch.equal(c, d) for c, d in zip(pool._carries, before))
    # and the pool goes on where it was: slot b's next hop equals a pool that never enabled codes
    ref = G.pool(3, 600, graph=False)
    ref.load_state()
    ref.open()
    rb = ref.open()
    ref.encode([rb], x[0])
    assert torch.equal(pool.transmit([b], x[1]), ref.quantize(ref.encode([rb], x[1])))


@pytest.mark.parametrize("decoder", ["symAudioDec", "HiFiGAN"])
def test_facade_opens_sessions_and_pools_with_codes(gpu, tmp_path, decoder):
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
    tx0, rx0 = codec.open_session(batch=1, chunk=300, graph=False)      # today's objects
    assert not tx0._codes_enabled and not rx0._codes_enabled
    tx, rx = codec.open_session(batch=1, chunk=300, codes=True)
    ptx, prx = codec.open_pool(capacity=2, chunk=300, codes=True)
    for p in (ptx, prx):
        p.open()                      # slot 0 stays idle
    st, sr = ptx.open(), prx.open()
    x = torch.from_numpy(ga["x"]).to(gpu)
    for c in range(3):
        xc = x[:, :, 300 * c:300 * (c + 1)]
        want = tx0.quantize(tx0.encode(xc))
        idx = tx.transmit(xc).clone()
        assert torch.equal(idx, want), c
        idxp = ptx.transmit([st], xc).clone()
        assert torch.equal(idxp.view(idx.shape), idx), c
        y_ordered = rx0.decode(_ordered(rx0, codec.rx_encoder, idx))
        y, yp = rx.receive(idx), prx.receive([sr], idxp)
        assert tuple(y.shape) == tuple(yp.shape) == (1, 1, 300)
        assert _same(y, y_ordered) and _same(yp, y_ordered), c


def test_error_paths(gpu):
    from models.autoencoder_without_PQC.AudioDec import StreamGenerator as NoPQC
    from sel import SelError
    from sel.streaming import VocoderSession
    G = _gen("golden")
    S = G.session(1, 300, graph=False)
    x = torch.zeros(1, 1, 300, device=gpu)
    idx = torch.zeros(2, 1, dtype=torch.int64, device=gpu)
    with pytest.raises(SelError, match="enable_codes"):
        S.transmit(x)
    with pytest.raises(SelError, match="enable_codes"):
        S.receive(idx)
    pool = G.pool(2, 300, graph=False)
    a = pool.open()
    with pytest.raises(SelError, match="enable_codes"):
        pool.transmit([a], x)
    with pytest.raises(SelError, match="enable_codes"):
        pool.receive([a], idx.view(2, 1, 1))
    # a plan without PQC: encode's output is no code vector
    torch.manual_seed(3)
    N = NoPQC(encode_channels=8, decode_channels=8, code_dim=64, codebook_num=2, codebook_size=64).to(gpu).eval()
    Sn = N.session(1, 1200, graph=False, codes=True)
    with pytest.raises(SelError, match="PQC"):
        Sn.transmit(torch.zeros(1, 1, 1200, device=gpu))
    # no lookup codebook known
    V, _ = _model("vocoder_v1", V1, gpu)
    Sv = V.session(1, 1, graph=False, codes=True)
    assert isinstance(Sv, VocoderSession) and Sv.lookup_generator is None
    with pytest.raises(SelError, match="lookup"):
        Sv.receive(idx)
    with pytest.raises(SelError, match="PQC"):
        Sv.transmit(x)
    Pv = V.pool(2, 1, graph=False, codes=True)
    with pytest.raises(SelError, match="lookup"):
        Pv.receive([Pv.open()], idx.view(2, 1, 1))
    # operand checks of the enabled methods
    S.enable_codes()
    with pytest.raises(SelError, match="takes"):
        S.transmit(torch.zeros(1, 1, 299, device=gpu))
    with pytest.raises(SelError, match="takes"):
        S.receive(idx.int())
    with pytest.raises(SelError, match="takes"):
        S.receive(torch.zeros(3, 1, dtype=torch.int64, device=gpu))
    with pytest.raises(SelError, match="device"):
        S.receive(idx.cpu())
