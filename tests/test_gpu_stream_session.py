"""sel.streaming.StreamSession on the GPU: the reference golden
(tests/golden/stream.npz), the oracle restatement at full width and without PQC,
graph replay against eager launches, batch invariance, bf16, and the codec
facade (utils/audiodec.py).  fp32: <= 1e-5 norm-wise per hop, VQ indices exact;
bf16: <= 5e-2 norm-wise against the fp32 oracle."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

GP = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
FULL = dict(encode_channels=32, decode_channels=32, code_dim=64, codebook_num=8, codebook_size=1024)
FULL_SEED = 0     # input seed of the full-width run: see test_full_width_vs_oracle
FULL_HOPS = 8


def nclose(a, b, rtol, name=""):
    a, b = (v.detach().float().cpu().numpy().astype(np.float64) if torch.is_tensor(v) else np.asarray(v, np.float64)
            for v in (a, b))
    assert a.shape == b.shape, (name, a.shape, b.shape)
    e = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    assert e <= rtol, (name, e)


def _stream_model(gpu, g=None, **gp):
    """The setup of tests/test_gpu_stream.py: seed 93, optionally the golden's weights."""
    from models.autoencoder.AudioDec import StreamGenerator
    torch.manual_seed(93)
    G = StreamGenerator(**(gp or GP))
    if g is not None:
        G.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return G.to(gpu).eval() if gpu is not None else G.eval()


def vq_gaps(z, embeds):
    """(stages, frames) relative fp64 gap between the best and the second-best
    code distance of every row and stage, along the fp64 residual chain."""
    from oracle import ref_ops as R
    r = z.double().transpose(2, 1).reshape(-1, z.shape[1])
    gaps = []
    for e in embeds:
        e = e.double()
        d2 = R.vq_distance(r, e).topk(2, dim=1, largest=False)
        gaps.append((d2.values[:, 1] - d2.values[:, 0]) / d2.values[:, 1].abs())
        r = r - e.t()[d2.indices[:, 0]]
    return torch.stack(gaps)


@functools.lru_cache(maxsize=None)
def full_oracle(seed=FULL_SEED, hops=FULL_HOPS, chunk=300):
    """The oracle's stream over `hops` chunks of the full-width seed-93 model, once."""
    from oracle import ref_ops as R
    G = _stream_model(None, None, **FULL)
    P = {k: v.detach().clone() for k, v in G.state_dict().items()}
    geo = R.generator_geometry()
    embeds = [P[f"quantizer.codebook.layers.{i}.embed"] for i in range(FULL["codebook_num"])]
    x = 0.1 * torch.randn(1, 1, hops * chunk, generator=torch.Generator().manual_seed(seed))
    S, out = {}, []
    for c in range(hops):
        xc = x[:, :, chunk * c:chunk * (c + 1)]
        z = R.stream_encode(P, S, xc, geo)
        idx = R.stream_quantize(z, embeds)
        zq = R.stream_lookup(idx, embeds)
        y = R.stream_decode(P, S, zq, geo)
        out.append(dict(x=xc, z=z, idx=idx, zq=zq, y=y, gaps=vq_gaps(z, embeds)))
    return out


def test_session_matches_reference_golden(gpu):
    g = golden("stream")
    G = _stream_model(gpu, g)
    G.initial_decoder(G.initial_encoder(600, gpu))
    S = G.session(1, 600, graph=False)
    S.load_state()
    x = torch.from_numpy(g["x"]).to(gpu)
    for c in range(6):
        z = S.encode(x[:, :, 600 * c:600 * (c + 1)])
        nclose(z, g[f"z.{c}"], 1e-5, f"z.{c}")
        idx = S.quantize(z)
        np.testing.assert_array_equal(idx.cpu().numpy(), g[f"idx.{c}"])
        zq = S.lookup(idx)
        nclose(zq, g[f"zq.{c}"], 1e-5, f"zq.{c}")
        nclose(S.decode(zq), g[f"y.{c}"], 1e-5, f"y.{c}")
    S.store_state()
    sd = G.state_dict()
    nbuf = 0
    for k, v in g.items():
        if k.startswith("buf."):
            nclose(sd[k[4:]], v, 1e-5, k)
            nbuf += 1
    assert nbuf == len(S.carries()) > 0
    S.reset()
    assert all(float(c.abs().sum()) == 0.0 for c in S.carries().values())


def test_full_width_vs_oracle(gpu):
    """32 channels, 8 x 1024 codes, B = 1, chunk 300, 8 hops, fp32; input
    0.1 * randn with seed FULL_SEED = 0.  The oracle's own fp64 gap between the
    best and the second-best code is at least 1.0656e-2 relative over the 64
    (hop, stage) choices at that seed (computed on the CPU before the seed was
    fixed; asserted below), so no index sits on a near-tie and the comparison is
    in effect exact: an index may differ only where that gap is below 1e-5, and
    at most 1% of the 64 may."""
    ora = full_oracle()
    assert min(float(h["gaps"].min()) for h in ora) > 1e-3
    G = _stream_model(gpu, None, **FULL)
    S = G.session(1, 300, graph=False)
    excused = total = 0
    for c, h in enumerate(ora):
        z = S.encode(h["x"].to(gpu))
        nclose(z, h["z"], 1e-5, f"z.{c}")
        idx = S.quantize(z).cpu()
        assert idx.shape == h["idx"].shape
        diff = idx != h["idx"]
        assert bool((h["gaps"][diff] < 1e-5).all()), (c, idx, h["idx"])
        excused += int(diff.sum())
        total += idx.numel()
        zq = S.lookup(h["idx"].to(gpu))
        nclose(zq, h["zq"], 1e-6, f"zq.{c}")
        nclose(S.decode(zq), h["y"], 1e-5, f"y.{c}")
    assert total == 64 and excused <= 0.01 * total


def test_without_pqc_vs_oracle(gpu):
    from oracle import ref_ops as R
    from models.autoencoder_without_PQC.AudioDec import StreamGenerator
    torch.manual_seed(3)
    G = StreamGenerator(encode_channels=8, decode_channels=8, code_dim=64, codebook_num=2,
                        codebook_size=64).to(gpu).eval()
    P = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    geo = R.generator_geometry(encode_channels=8, decode_channels=8)
    S = G.session(1, 1200, graph=False)
    St = {}
    x = 0.1 * torch.randn(1, 1, 3600, generator=torch.Generator().manual_seed(9))
    for c in range(3):
        xc = x[:, :, 1200 * c:1200 * (c + 1)]
        h = S.encode(xc.to(gpu))
        hr = R.stream_encode(P, St, xc, geo, project=False)
        nclose(h, hr, 1e-5, f"h.{c}")
        nclose(S.decode(h), R.stream_decode(P, St, hr.transpose(2, 1), geo, pqc=False), 1e-5, f"y.{c}")


def test_graph_replay_is_bitwise_eager(gpu):
    G = _stream_model(gpu, None, **FULL)
    Sg = G.session(2, 300, graph=True)
    Se = G.session(2, 300, graph=False)
    assert Sg.graphed and not Se.graphed
    x = 0.1 * torch.randn(2, 1, 1500, generator=torch.Generator().manual_seed(12)).to(gpu)
    ptrs = None
    for c in range(5):
        xc = x[:, :, 300 * c:300 * (c + 1)]
        zg, ze = Sg.encode(xc), Se.encode(xc)
        assert torch.equal(zg, ze), c
        zq = Se.lookup(Se.quantize(ze))
        assert tuple(zq.shape) == (2, 1, 64)
        yg, ye = Sg.decode(zq), Se.decode(zq)
        assert torch.equal(yg, ye), c
        assert tuple(zg.shape) == (2, 64, 1) and tuple(yg.shape) == (2, 1, 300)
        cg, ce = Sg.carries(), Se.carries()
        assert cg.keys() == ce.keys() and len(cg) == 36
        for k in cg:
            assert torch.equal(cg[k], ce[k]), (c, k)
        assert float(sum(v.abs().sum() for v in cg.values())) > 0
        now = (zg.data_ptr(), yg.data_ptr())
        assert ptrs is None or ptrs == now
        ptrs = now


def test_batch_of_streams(gpu):
    """A B = 3 session equals three B = 1 sessions bitwise, and the module path
    (G.encode / G.decode on the same chunks) to 1e-5."""
    G = _stream_model(gpu, None, **FULL)
    S3 = G.session(3, 300, graph=False)
    S1 = [G.session(1, 300, graph=False) for _ in range(3)]
    x = 0.1 * torch.randn(3, 1, 900, generator=torch.Generator().manual_seed(31)).to(gpu)
    zqs = torch.randn(3, 3, 1, 64, generator=torch.Generator().manual_seed(32)).to(gpu)
    G.reset_buffer()
    for c in range(3):
        xc = x[:, :, 300 * c:300 * (c + 1)].contiguous()
        z3 = S3.encode(xc)
        y3 = S3.decode(zqs[c])
        for b in range(3):
            assert torch.equal(S1[b].encode(xc[b:b + 1]), z3[b:b + 1]), (c, b)
            assert torch.equal(S1[b].decode(zqs[c][b:b + 1]), y3[b:b + 1]), (c, b)
            for k, v in S1[b].carries().items():
                assert torch.equal(v[0], S3.carries()[k][b]), (c, b, k)
        nclose(z3, G.encode(xc), 1e-5, f"z.{c}")
        nclose(y3, G.decode(zqs[c]), 1e-5, f"y.{c}")


def test_bf16_session_vs_fp32_oracle(gpu):
    ora = full_oracle()
    G = _stream_model(gpu, None, **FULL)
    from sel.streaming import StreamSession
    S = StreamSession(G, 1, 300, graph=False, dtype=torch.bfloat16)
    assert all(c.dtype == torch.bfloat16 for c in S.carries().values())
    for c, h in enumerate(ora):
        z = S.encode(h["x"].to(gpu))
        assert z.dtype == torch.float32
        nclose(z, h["z"], 5e-2, f"z.{c}")
        y = S.decode(h["zq"].to(gpu))
        assert y.dtype == torch.float32
        nclose(y, h["y"], 5e-2, f"y.{c}")


def test_audiodec_facade_sessions(gpu, tmp_path):
    """utils.audiodec.AudioDec: checkpoint + config.yml of the golden-width
    generator -> load_transmitter / load_receiver / open_session; tx.encode ->
    quantize, rx.lookup -> decode over 3 hops equals the bare StreamGenerator
    sequence (same warm-up) to 1e-5, indices exact."""
    import yaml
    from utils.audiodec import AudioDec, assign_model
    g = golden("stream")
    G0 = _stream_model(None, g)
    ckpt = tmp_path / "checkpoint-1steps.pkl"
    torch.save({"model": {"generator": G0.state_dict()}}, ckpt)
    (tmp_path / "config.yml").write_text(yaml.safe_dump({"model_type": "symAudioDec", "generator_params": dict(GP)}))
    codec = AudioDec(tx_device=str(gpu), rx_device=str(gpu), receptive_length=1000)
    codec.load_transmitter(str(ckpt))
    codec.load_receiver(str(ckpt), str(ckpt))
    tx, rx = codec.open_session(batch=1, chunk=600)

    G = _stream_model(gpu, g)
    G.initial_decoder(G.initial_encoder(1000, gpu))
    x = torch.from_numpy(g["x"]).to(gpu)
    for c in range(3):
        xc = x[:, :, 600 * c:600 * (c + 1)]
        z, zr = tx.encode(xc), G.encode(xc)
        nclose(z, zr, 1e-5, f"z.{c}")
        idx, ir = tx.quantize(z), G.quantize(zr)
        assert torch.equal(idx, ir), c
        zq, zqr = rx.lookup(idx), G.lookup(ir)
        nclose(zq, zqr, 1e-5, f"zq.{c}")
        nclose(rx.decode(zq), G.decode(zqr), 1e-5, f"y.{c}")
    assert assign_model("vctk_sym")[0] == 48000
    with pytest.raises(NotImplementedError):
        assign_model("nope")
