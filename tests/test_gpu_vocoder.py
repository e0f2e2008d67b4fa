"""The HiFi-GAN vocoder generator (models/vocoder/HiFiGAN.py Generator /
StreamGenerator) on the GPU against goldens recorded from the reference on the
CPU (tests/golden/make_goldens_vocoder.py): reduced-width models in the
MultiGroupConv1d form (v1: groups 3, K = 11) and the MultiReceptiveField form
(v0: K = 3, 7, 11), and the AudioDec baseline chain of testing_denoise.py:97-101.

fp32 bounds are the project's fp32 conv bound, 1e-5 norm-wise
(tests/test_gpu_stream.py).  The bf16 bound is explained at BF16_BOUND.
"""
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

# bf16 end to end (v1 golden weights, 13 convs deep at 4 widths) against the
# fp32 golden output, norm-wise.  MEASURED_BF16 is the value of the MI355X run
# recorded in DESIGN.md; the bound is twice that, rounded up to one digit (tile
# choice changes the summation order), capped at 3e-2, the project's bf16
# forward bound for a conv stack of this depth (tests/test_gpu_c3.py).
MEASURED_BF16 = 1.363e-2
BF16_BOUND = 3e-2   # 2 x 1.363e-2 = 2.73e-2 -> 3e-2 (one digit, rounded up), which is also the cap


def rel(a, b):
    a, b = (v.detach().double().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)).double()
            for v in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model(name, params, dev):
    from models.vocoder.HiFiGAN import StreamGenerator
    g = golden(name)
    G = StreamGenerator(**params)
    sd = {k[3:]: torch.from_numpy(v.astype(np.float32)) for k, v in g.items() if k.startswith("sd.")}
    G.load_state_dict(sd, strict=True)
    return G.to(dev).eval(), g


@pytest.mark.parametrize("name,params", MODELS)
def test_one_shot_matches_reference_golden(gpu, name, params):
    G, g = _model(name, params, gpu)
    with torch.no_grad():
        y = G(torch.from_numpy(g["x"]).to(gpu))
    assert y.dtype == torch.float32 and y.shape == g["y"].shape
    e = rel(y, g["y"])
    print(f"{name} one-shot fp32: {e:.2e}")
    assert e <= 1e-5, e


@pytest.mark.parametrize("name,params", MODELS)
def test_streaming_matches_reference_golden(gpu, name, params):
    """every streamed chunk and every final pad_buffer (they are state_dict
    entries: the ACTIVATED tails, as the reference keeps them)"""
    G, g = _model(name, params, gpu)
    x = torch.from_numpy(g["x"]).to(gpu)
    G.reset_buffer()
    for c in range(7):
        y = G.decode(x[:1, :, c:c + 1].transpose(2, 1).contiguous())
        e = rel(y, g[f"y.{c}"])
        assert e <= 1e-5, (c, e)
    sd = G.state_dict()
    bufs = [k for k in g if k.startswith("buf.")]
    assert len(bufs) == sum(k.endswith("pad_buffer") for k in sd)
    for k in bufs:
        assert rel(sd[k[4:]], g[k]) <= 1e-5, k
    G.reset_buffer()
    assert all(float(v.abs().sum()) == 0.0 for k, v in G.state_dict().items() if k.endswith("pad_buffer"))


def test_remove_weight_norm_keeps_outputs(gpu):
    G, g = _model("vocoder_v0", V0, gpu)
    x = torch.from_numpy(g["x"]).to(gpu)
    with torch.no_grad():
        y0 = G(x)
        G.remove_weight_norm()
        assert not any(k.endswith("weight_g") for k in G.state_dict())
        y1 = G(x)
    assert rel(y1, y0) <= 1e-6
    assert rel(y1, g["y_no_weight_norm"]) <= 1e-5


def _reach(params):
    """output samples the transposed convs' replicate-versus-zero start can reach:
    each upsampling's first output step differs, and every later causal conv
    carries a difference (K - 1) * dil rows on"""
    r = 0
    for s in params["upsample_scales"]:
        r = (r + 1) * s
        r += max(sum((k - 1) * (d + 1) for d in ds)
                 for k, ds in zip(params["resblock_kernel_sizes"], params["resblock_dilations"]))
    return r + 6


@pytest.mark.parametrize("name,params", MODELS)
def test_stream_chunks_equal_one_shot(gpu, name, params):
    """1-frame chunks equal the one-shot forward once the start of the stream has
    left the receptive field (zero buffer in front of the transposed convs while
    the one-shot forward replicates its first frame), the property of
    test_stream_encoder_chunks_equal_one_shot.  With the K = 11 blocks at 5 rows
    per frame that takes 9501 samples (the reference on the CPU still differs
    at sample 8638 and agrees to 1e-6 after), so 40 frames are streamed; over
    the goldens' 7 frames the reference itself differs by 1.4e-1 (v1) from
    sample 600 on, which the golden comparison above covers."""
    G, g = _model(name, params, gpu)
    n = 40
    reach = _reach(params)
    assert reach < 300 * n - 1500
    x = torch.randn(1, 64, n, generator=torch.Generator().manual_seed(7)).to(gpu)
    with torch.no_grad():
        y = G(x)
    G.reset_buffer()
    ys = torch.cat([G.decode(x[:, :, c:c + 1].transpose(2, 1).contiguous()) for c in range(n)], -1)
    e = rel(ys[..., reach:], y[..., reach:])
    print(f"{name} stream vs one-shot from sample {reach}: {e:.2e}")
    assert e <= 1e-5, e
    assert rel(ys[..., :300], y[..., :300]) > 1e-3   # the start does differ


def test_audiodec_baseline_chain(gpu):
    """encoder -> projector -> quantizer -> HiFi-GAN vocoder (testing_denoise.py:97-101)"""
    from models.autoencoder.AudioDec import Generator as AutoEncoder
    g = golden("audiodec_baseline")
    E = AutoEncoder(**GP)
    E.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    E = E.to(gpu).eval()
    V, _ = _model("vocoder_v1", V1, gpu)
    with torch.no_grad():
        z = E.projector(E.encoder(torch.from_numpy(g["x"]).to(gpu)))
        assert rel(z, g["z"]) <= 1e-5
        _, idx = E.quantizer.inference(z)
        np.testing.assert_array_equal(idx.cpu().numpy(), g["idx"])
        zq, _, _ = E.quantizer(z)
        assert rel(zq, g["zq"]) <= 1e-5
        y = V(zq)
    e = rel(y, g["y"])
    print(f"audiodec baseline chain fp32: {e:.2e}")
    assert e <= 1e-5, e


def test_bf16_end_to_end(gpu):
    """v1 golden weights under precision(bfloat16) against the fp32 golden output.
    Measured on the MI355X: 1.363e-2 (MEASURED_BF16)."""
    from sel import convops as CO
    G, g = _model("vocoder_v1", V1, gpu)
    with torch.no_grad(), CO.precision(torch.bfloat16):
        y = G(torch.from_numpy(g["x"]).to(gpu))
    assert y.dtype == torch.float32
    e = rel(y, g["y"])
    print(f"v1 bf16 end to end vs fp32 golden: {e:.3e}")
    assert e <= BF16_BOUND, e


def test_full_width_bf16_against_fp32(gpu):
    """VOCODER_V1 at full width (B = 1, 2 latent frames -> 600 samples): the only
    test that runs C = 256 / 128, G = 3 through the module.  Both bf16 paths --
    the default dispatch (fused residual layers at C/G = 64 / 32) and the
    two-launch path forced by sel_tune key 71 = 1 -- agree within the bf16
    bound (they are bit-identical by construction, see
    tests/test_gpu_hfg_kernels.py, which the test prints but does not require
    here), and each is within it of the fp32 instance on the same weights."""
    from models.vocoder.HiFiGAN import Generator
    from sel import configs
    from sel import convops as CO
    gen = torch.Generator().manual_seed(11)
    G = Generator(**configs.VOCODER_V1)
    with torch.no_grad():
        # as constructed (normal_(0, 0.01)) the output is a near-constant: redraw as the fixtures do
        for m in G.modules():
            v, wg = getattr(m, "weight_v", None), getattr(m, "weight_g", None)
            if v is None:
                continue
            fan_in = v.shape[0] * 2 if isinstance(m, torch.nn.ConvTranspose1d) else v.shape[1] * v.shape[2]
            v.copy_(torch.randn(v.shape, generator=gen) / fan_in ** 0.5)
            wg.copy_(v.norm(2, dim=(1, 2), keepdim=True) * (0.5 + torch.rand(wg.shape, generator=gen)))
            if m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
    G = G.to(gpu).eval()
    x = torch.randn(1, 64, 2, generator=gen).to(gpu)
    with torch.no_grad():
        y32 = G(x)
        with CO.precision(torch.bfloat16):
            y16 = G(x)
            prev = CO.L.lib().sel_tune(71, 1)
            try:
                y16_two = G(x)
            finally:
                CO.L.lib().sel_tune(71, prev)
    assert y32.shape == (1, 1, 600)
    assert float(y32.std()) > 0.05
    e, e2, ab = rel(y16, y32), rel(y16_two, y32), rel(y16, y16_two)
    print(f"full-width v1 bf16 vs fp32: default {e:.3e}, two-launch {e2:.3e}; default vs two-launch {ab:.3e} "
          f"(bit-identical: {torch.equal(y16, y16_two)})")
    assert e <= BF16_BOUND and e2 <= BF16_BOUND and ab <= BF16_BOUND, (e, e2, ab)


def test_grad_required_raises(gpu):
    G, g = _model("vocoder_v1", V1, gpu)
    x = torch.from_numpy(g["x"]).to(gpu)
    with pytest.raises(NotImplementedError):
        G(x)                                   # parameters require grad, grad mode on
    G.requires_grad_(False)
    with pytest.raises(NotImplementedError):
        G(x.clone().requires_grad_(True))
    y = G(x)                                   # nothing requires grad: fine without no_grad
    assert rel(y, g["y"]) <= 1e-5
