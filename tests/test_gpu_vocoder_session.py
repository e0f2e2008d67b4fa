"""sel.streaming.VocoderSession on the GPU: the reference goldens
(tests/golden/vocoder_v1.npz MultiGroupConv1d, vocoder_v0.npz
MultiReceptiveField), graph replay against eager launches, batch invariance,
state exchange with the module path, the full-width generators against the
module path, bf16, input statistics, and the codec facade (utils/audiodec.py).
fp32: <= 1e-5 norm-wise per hop, the project's fp32 bound; the bf16 bound is
explained at BF16_BOUND."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

SCALES = dict(upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6])
V1 = dict(in_channels=64, channels=64, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3, **SCALES)
V0 = dict(in_channels=64, channels=32, resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3,
          groups=1, **SCALES)
GP = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
MODELS = [("vocoder_v1", V1), ("vocoder_v0", V0)]
NCARRY = {"vocoder_v1": 30, "vocoder_v0": 78}

# bf16 (v1 golden weights, seven streamed 1-frame chunks from zero state against
# the fp32 golden chunks, the largest norm-wise error over the chunks), measured
# on the MI355X: MODULE_BF16 is the module path (StreamGenerator.decode under
# precision(bfloat16), the code as it was before the session existed),
# SESSION_BF16 the bf16 VocoderSession.  The session's bound is twice the
# module-path error rounded up to one digit, capped at 3e-2: the rule and the cap
# of tests/test_gpu_vocoder.py (BF16_BOUND there).
MODULE_BF16 = 1.489e-2
SESSION_BF16 = 1.489e-2   # the same roundings (operand, output) on both paths; only the fp32 summation order differs
BF16_BOUND = 3e-2   # 2 x 1.489e-2 = 2.98e-2 -> 3e-2 (one digit, rounded up), which is also the cap


def rel(a, b):
    a, b = (v.detach().double().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)).double()
            for v in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model(name, params, dev, **extra):
    from models.vocoder.HiFiGAN import StreamGenerator
    g = golden(name)
    G = StreamGenerator(**params, **extra)
    sd = {k[3:]: torch.from_numpy(v.astype(np.float32)) for k, v in g.items() if k.startswith("sd.")}
    missing = G.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"mean", "scale"}
    return G.to(dev).eval(), g


def _chunk(g, c, dev):
    return torch.from_numpy(g["x"][:1, :, c:c + 1]).transpose(2, 1).contiguous().to(dev)


@pytest.mark.parametrize("name,params", MODELS)
def test_session_matches_reference_golden(gpu, name, params):
    from sel.streaming import VocoderSession
    G, g = _model(name, params, gpu)
    S = VocoderSession(G, 1, 1, graph=False, dtype=torch.float32)
    assert len(S.carries()) == NCARRY[name]
    for c in range(7):
        y = S.decode(_chunk(g, c, gpu))
        assert y.dtype == torch.float32 and tuple(y.shape) == (1, 1, 300)
        e = rel(y, g[f"y.{c}"])
        assert e <= 1e-5, (c, e)
    G.reset_buffer()
    S.store_state()
    sd = G.state_dict()
    bufs = [k for k in g if k.startswith("buf.")]
    assert len(bufs) == len(S.carries()) == sum(k.endswith("pad_buffer") for k in sd)
    for k in bufs:
        assert sd[k[4:]].dtype == torch.float32 and rel(sd[k[4:]], g[k]) <= 1e-5, k
    S.reset()
    assert all(float(c.abs().sum()) == 0.0 for c in S.carries().values())


@pytest.mark.parametrize("name,params", MODELS)
def test_graph_replay_is_bitwise_eager(gpu, name, params):
    G, _ = _model(name, params, gpu)
    Sg = G.session(2, 1, graph=True)
    Se = G.session(2, 1, graph=False)
    assert Sg.graphed and not Se.graphed
    x = torch.randn(5, 2, 1, 64, generator=torch.Generator().manual_seed(12)).to(gpu)
    ptr = None
    for c in range(5):
        yg, ye = Sg.decode(x[c]), Se.decode(x[c])
        assert tuple(yg.shape) == (2, 1, 300) and torch.equal(yg, ye), c
        cg, ce = Sg.carries(), Se.carries()
        assert cg.keys() == ce.keys() and len(cg) == NCARRY[name]
        for k in cg:
            assert torch.equal(cg[k], ce[k]), (c, k)
        assert float(sum(v.abs().sum() for v in cg.values())) > 0
        assert ptr is None or ptr == yg.data_ptr()
        ptr = yg.data_ptr()


@pytest.mark.parametrize("name,params", MODELS)
def test_batch_of_streams(gpu, name, params):
    """A B = 3 session equals three B = 1 sessions bitwise."""
    G, _ = _model(name, params, gpu)
    S3 = G.session(3, 1, graph=False)
    S1 = [G.session(1, 1, graph=False) for _ in range(3)]
    x = torch.randn(3, 3, 1, 64, generator=torch.Generator().manual_seed(31)).to(gpu)
    for c in range(3):
        y3 = S3.decode(x[c])
        for b in range(3):
            assert torch.equal(S1[b].decode(x[c][b:b + 1]), y3[b:b + 1]), (c, b)
            for k, v in S1[b].carries().items():
                assert torch.equal(v[0], S3.carries()[k][b]), (c, b, k)


@pytest.mark.parametrize("name,params", MODELS)
def test_load_state_continues_the_module_path(gpu, name, params):
    """Three golden chunks on the module path, load_state(), chunks 3-6 in the session."""
    G, g = _model(name, params, gpu)
    S = G.session(1, 1, graph=True)
    G.reset_buffer()
    for c in range(3):
        G.decode(_chunk(g, c, gpu))
    S.load_state()
    for c in range(3, 7):
        e = rel(S.decode(_chunk(g, c, gpu)), g[f"y.{c}"])
        assert e <= 1e-5, (c, e)


def _full_width(cfg, gpu, seed):
    """The full-width generator with the parameters redrawn as
    tests/golden/make_goldens_vocoder.py does: v ~ N(0, 1/fan_in),
    g = ||v|| * U(0.5, 1.5), bias ~ N(0, 0.1)."""
    from models.vocoder.HiFiGAN import StreamGenerator
    gen = torch.Generator().manual_seed(seed)
    G = StreamGenerator(**cfg)
    with torch.no_grad():
        for m in G.modules():
            v, wg = getattr(m, "weight_v", None), getattr(m, "weight_g", None)
            if v is None:
                continue
            if isinstance(m, torch.nn.ConvTranspose1d):
                fan_in = v.shape[0] * v.shape[2] // m.stride[0]
            else:
                fan_in = v.shape[1] * v.shape[2]
            v.copy_(torch.randn(v.shape, generator=gen) / fan_in ** 0.5)
            wg.copy_(v.norm(2, dim=(1, 2), keepdim=True) * (0.5 + torch.rand(wg.shape, generator=gen)))
            if m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
    return G.to(gpu).eval(), gen


@pytest.mark.parametrize("which,hops", [("VOCODER_V1", 3), ("VOCODER_V0", 2)])
def test_full_width_matches_the_module_path(gpu, which, hops):
    """B = 1, one frame per hop, fp32: the only test that runs the 768-channel
    G = 3 block-0 layers (v1) and the 256-channel K = 3 / 7 / 11 blocks (v0)
    through the step kernel."""
    from sel import configs
    from sel.streaming import VocoderSession
    G, gen = _full_width(getattr(configs, which), gpu, 11)
    S = VocoderSession(G, 1, 1, graph=False, dtype=torch.float32)
    G.reset_buffer()
    ys = []
    for c in range(hops):
        x = torch.randn(1, 1, 64, generator=gen).to(gpu)
        ym = G.decode(x)
        e = rel(S.decode(x), ym)
        print(f"{which} hop {c}: session vs module {e:.2e}")
        assert e <= 1e-5, (c, e)
        ys.append(ym)
    y = torch.cat(ys, -1).double()
    rms, std = float(y.pow(2).mean().sqrt()), float(y.std(dim=-1).mean())
    print(f"{which}: module output std over time {std:.3f}, rms {rms:.3f}")
    assert std >= 0.3 * rms, (std, rms)


def test_bf16_session_vs_fp32_golden(gpu):
    """v1 golden weights, bf16 session against the fp32 golden chunks; the module
    path's error on the same chunks is printed beside it (MODULE_BF16)."""
    from sel import convops as CO
    from sel.streaming import VocoderSession
    G, g = _model("vocoder_v1", V1, gpu)
    S = VocoderSession(G, 1, 1, graph=False, dtype=torch.bfloat16)
    assert all(c.dtype == torch.bfloat16 for c in S.carries().values())
    G.reset_buffer()
    es, em = [], []
    for c in range(7):
        y = S.decode(_chunk(g, c, gpu))
        assert y.dtype == torch.float32
        es.append(rel(y, g[f"y.{c}"]))
        with CO.precision(torch.bfloat16):
            em.append(rel(G.decode(_chunk(g, c, gpu)), g[f"y.{c}"]))
    print(f"v1 bf16 streamed vs fp32 golden, max over 7 chunks: session {max(es):.3e}, module path {max(em):.3e}")
    assert max(es) <= BF16_BOUND, es


def test_stats_are_applied_outside_the_graph(gpu, tmp_path):
    g = torch.Generator().manual_seed(41)
    stats = np.stack([torch.randn(64, generator=g).numpy(), (0.5 + torch.rand(64, generator=g)).numpy()])
    path = tmp_path / "stats.npy"
    np.save(path, stats.astype(np.float32))
    G, gd = _model("vocoder_v1", V1, gpu, stats=str(path))
    assert G.norm
    S = G.session(1, 1, graph=True)
    G.reset_buffer()
    for c in range(3):
        x = _chunk(gd, c, gpu) + 0.5
        e = rel(S.decode(x), G.decode(x))
        print(f"stats hop {c}: session vs module {e:.2e}")
        assert e <= 1e-6, (c, e)


def test_audiodec_facade_opens_a_vocoder_session(gpu, tmp_path):
    """utils.audiodec.AudioDec with a HiFiGAN decoder: open_session returns
    (StreamSession, VocoderSession); rx.decode(rx.lookup(idx)) equals
    decoder.decode(rx_encoder.lookup(idx)) over 3 hops."""
    import yaml
    from models.autoencoder.AudioDec import StreamGenerator as Encoder
    from sel.streaming import StreamSession, VocoderSession
    from utils.audiodec import AudioDec
    ga, gv = golden("audiodec_baseline"), golden("vocoder_v1")
    enc_dir, dec_dir = tmp_path / "enc", tmp_path / "dec"
    enc_dir.mkdir()
    dec_dir.mkdir()
    E = Encoder(**GP)
    E.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in ga.items() if k.startswith("sd.")}, strict=True)
    V, _ = _model("vocoder_v1", V1, "cpu")
    V.reset_buffer()
    torch.save({"model": {"generator": E.state_dict()}}, enc_dir / "checkpoint-1steps.pkl")
    torch.save({"model": {"generator": V.state_dict()}}, dec_dir / "checkpoint-1steps.pkl")
    (enc_dir / "config.yml").write_text(yaml.safe_dump({"model_type": "symAudioDec", "generator_params": dict(GP)}))
    (dec_dir / "config.yml").write_text(yaml.safe_dump({"model_type": "HiFiGAN", "generator_params": dict(V1)}))
    codec = AudioDec(tx_device=str(gpu), rx_device=str(gpu), receptive_length=900)
    codec.load_transmitter(str(enc_dir / "checkpoint-1steps.pkl"))
    codec.load_receiver(str(enc_dir / "checkpoint-1steps.pkl"), str(dec_dir / "checkpoint-1steps.pkl"))
    tx, rx = codec.open_session(batch=1, chunk=300)
    assert isinstance(tx, StreamSession) and isinstance(rx, VocoderSession)
    assert rx.lookup_generator is codec.rx_encoder and rx.plan.frames == 1
    assert float(sum(c.abs().sum() for c in rx.carries().values())) > 0   # the warm-up state was loaded
    x = torch.from_numpy(ga["x"]).to(gpu)
    for c in range(3):
        idx = tx.quantize(tx.encode(x[:, :, 300 * c:300 * (c + 1)]))
        y = rx.decode(rx.lookup(idx))
        yr = codec.decoder.decode(codec.rx_encoder.lookup(idx))
        assert tuple(y.shape) == tuple(yr.shape) == (1, 1, 300)
        e = rel(y, yr)
        assert e <= 1e-5, (c, e)
