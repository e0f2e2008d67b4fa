"""Training the HiFi-GAN vocoder generator (models/vocoder/HiFiGAN.py with
enable_training(), sel.hfgops.generator_train, trainer/vocoder.py) on the GPU
against goldens recorded from the reference on the CPU in FP64
(tests/golden/make_goldens_vocoder_train.py).

fp32: y <= 1e-5 (the project's fp32 bound); gx and every parameter gradient
<= max(1e-5, 3 x e32.<name>), e32 being the reference's own recorded fp32 noise
against fp64 for that tensor (the row-split tree of the weight gradient sums in
another order than torch does).  bf16: see BF16_GRAD_BOUND.
"""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

UP = dict(upsample_scales=[5, 3], upsample_kernel_sizes=[10, 6])
T1 = dict(in_channels=16, channels=64, resblock_kernel_sizes=[7], resblock_dilations=[[1, 3]], groups=3, **UP)
T0 = dict(in_channels=16, channels=64, resblock_kernel_sizes=[3, 7], resblock_dilations=[[1, 3]] * 2, groups=1, **UP)
SCALES = dict(upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6])
V1 = dict(in_channels=64, channels=64, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3, **SCALES)
TG = dict(in_channels=64, channels=32, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3, **SCALES)
GP = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
MODELS = [("vocoder_train_v1", T1), ("vocoder_train_v0", T0)]

# bf16 end to end (t1 fixture: 11 convs deep, forward and backward in bf16)
# against the FP64 fixture, norm-wise over all parameter gradients concatenated
# and over gx.  MEASURED_* are the values of the MI355X run recorded in
# DESIGN.md; the bound is twice that, rounded up to one digit, never above the
# cap 1.5e-1, the project's bf16 end-to-end gradient bound (tests/test_gpu_c3.py).
BF16_GRAD_CAP = 1.5e-1
MEASURED_BF16_GPARAM = 7.035e-2
MEASURED_BF16_GX = 8.936e-2
BF16_GPARAM_BOUND = 1.5e-1   # 2 x 7.035e-2 = 1.41e-1 -> 2e-1 (one digit, rounded up), capped at 1.5e-1
BF16_GX_BOUND = 1.5e-1       # 2 x 8.936e-2 = 1.79e-1 -> 2e-1, capped at 1.5e-1


def rel(a, b):
    a, b = (v.detach().double().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)).double()
            for v in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _sd(g, prefix="sd."):
    return {k[len(prefix):]: torch.from_numpy(v.astype(np.float32)) for k, v in g.items() if k.startswith(prefix)}


def _model(name, params, dev, cls=None):
    from models.vocoder.HiFiGAN import Generator
    g = golden(name)
    G = (cls or Generator)(**params)
    G.load_state_dict(_sd(g), strict=True)
    return G.to(dev).train().enable_training(), g


def _step(G, g, dev):
    """loss = sum(y * r), backward; returns (y, gx)"""
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    G.zero_grad(set_to_none=True)
    y = G(x)
    (y * torch.from_numpy(g["r"]).to(dev)).sum().backward()
    return y.detach(), x.grad


@pytest.mark.parametrize("name,params", MODELS)
def test_fp32_gradients_match_fp64_reference(gpu, name, params):
    G, g = _model(name, params, gpu)
    y, gx = _step(G, g, gpu)
    assert y.dtype == torch.float32 and rel(y, g["y"]) <= 1e-5, rel(y, g["y"])
    worst = 0.0
    for k, got in [("gx", gx)] + [("g." + n, p.grad) for n, p in G.named_parameters()]:
        assert got is not None, k
        e, bound = rel(got, g[k]), max(1e-5, 3.0 * float(g["e32." + (k[2:] if k != "gx" else k)]))
        worst = max(worst, e / bound)
        assert e <= bound, (k, e, bound)
    print(f"{name} fp32: y {rel(y, g['y']):.2e}, gx {rel(gx, g['gx']):.2e}, worst error / bound {worst:.2f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,params", MODELS)
def test_training_forward_is_bit_identical_to_inference(gpu, name, params, dtype):
    """the training path issues the launches of the no-grad forward with two
    launches per residual layer (sel_tune key 71 = 1)"""
    from sel import convops as CO
    G, g = _model(name, params, gpu)
    x = torch.from_numpy(g["x"]).to(gpu)
    lib = CO.L.lib()
    with CO.precision(dtype):
        y_train = G(x)
        assert y_train.requires_grad
        prev = lib.sel_tune(71, 1)
        try:
            with torch.no_grad():
                y_inf = G(x)
        finally:
            lib.sel_tune(71, prev)
    assert torch.equal(y_train.detach(), y_inf)


def test_bf16_end_to_end_gradients(gpu):
    """Measured on the MI355X: MEASURED_BF16_GPARAM / MEASURED_BF16_GX."""
    from sel import convops as CO
    G, g = _model("vocoder_train_v1", T1, gpu)
    with CO.precision(torch.bfloat16):
        y, gx = _step(G, g, gpu)
    names = [n for n, _ in G.named_parameters()]
    got = torch.cat([dict(G.named_parameters())[n].grad.flatten().double().cpu() for n in names])
    ref = torch.cat([torch.from_numpy(g["g." + n]).flatten().double() for n in names])
    ep, ex = rel(got, ref), rel(gx, g["gx"])
    print(f"t1 bf16 end to end vs fp64: parameter gradients {ep:.3e}, gx {ex:.3e}, y {rel(y, g['y']):.3e}")
    assert BF16_GPARAM_BOUND <= BF16_GRAD_CAP and BF16_GX_BOUND <= BF16_GRAD_CAP
    assert ep <= BF16_GPARAM_BOUND, ep
    assert ex <= BF16_GX_BOUND, ex


def test_remove_weight_norm_then_train(gpu, monkeypatch):
    """after remove_weight_norm() the gradients land on ``weight`` and equal the
    gW the kernels hand to the weight-norm formula of the weight-normed model
    (same effective weight) to 1e-5"""
    from sel import hfgops as HF
    G, g = _model("vocoder_train_v0", T0, gpu)
    kept = []
    plain = HF.effective_weight_train

    def keep(m):
        w = plain(m)
        w.retain_grad()
        kept.append((m, w))
        return w

    monkeypatch.setattr(HF, "effective_weight_train", keep)
    y0, gx0 = _step(G, g, gpu)
    monkeypatch.setattr(HF, "effective_weight_train", plain)
    gws = [(m, w.grad.clone()) for m, w in kept]
    assert gws and all(hasattr(m, "weight_g") for m, _ in gws)
    G.remove_weight_norm()
    assert not any(k.endswith("weight_g") for k in G.state_dict())
    y1, gx1 = _step(G, g, gpu)
    assert rel(y1, y0) <= 1e-6 and rel(gx1, gx0) <= 1e-5
    for m, gw in gws:
        assert isinstance(m.weight, torch.nn.Parameter) and m.weight.grad is not None
        assert rel(m.weight.grad, gw) <= 1e-5, rel(m.weight.grad, gw)
        assert m.bias.grad is not None


def test_enable_training_keeps_state_and_streaming(gpu):
    """no state_dict key appears, and a StreamGenerator with training enabled
    still streams under decode exactly as vocoder_v1.npz records"""
    from models.vocoder.HiFiGAN import StreamGenerator
    g = golden("vocoder_v1")
    G = StreamGenerator(**V1)
    keys = list(G.state_dict())
    G.load_state_dict(_sd(g), strict=True)
    G = G.to(gpu).eval().enable_training()
    assert list(G.state_dict()) == keys
    x = torch.from_numpy(g["x"]).to(gpu)
    G.reset_buffer()
    for c in range(7):
        y = G.decode(x[:1, :, c:c + 1].transpose(2, 1).contiguous())
        assert not y.requires_grad
        assert rel(y, g[f"y.{c}"]) <= 1e-5, c
    for k in [k for k in g if k.startswith("buf.")]:
        assert rel(G.state_dict()[k[4:]], g[k]) <= 1e-5, k
    G.reset_buffer()
    y = G(x.clone().requires_grad_(True))       # the same module trains
    assert y.requires_grad and rel(y, g["y"]) <= 1e-5


def test_vocoder_trainer_steps_match_reference_golden(gpu):
    """trainer/vocoder.Trainer._train_step (:48-111) against the reference CLASS
    ITSELF (tests/golden/vocoder_trainer_step.npz): frozen reduced PQC analyzer
    and reduced MSD + MPD discriminator (regenerated by seed 93, checksummed),
    48 kHz mel loss, lambda 45 / 1 / 2, Adam(2e-4, (0.5, 0.9)) -- fused here --
    two steps from steps = 1 with both start steps 0.  Logged keys equal; values
    1e-5 (step 0) / 1e-4 (step 1); gradient norms after step 0 1e-4 (a wrong
    lambda or a missing 1/#blocks hides behind Adam's sign-like update); the
    two-step parameter delta: at most 2 % of the entries off by more than
    0.5 lr and <= 0.10 norm-wise (the reference's own fp32 run against fp64:
    0 % and 2.3e-5)."""
    from losses import (DiscriminatorAdversarialLoss, FeatureMatchLoss, GeneratorAdversarialLoss,
                        MultiMelSpectrogramLoss)
    from models.autoencoder.AudioDec import Generator as AutoEncoder
    from models.vocoder.HiFiGAN import Discriminator, Generator
    from trainer.vocoder import Trainer
    g = golden("vocoder_trainer_step")
    d_params = dict(
        scales=3, scale_downsample_pooling="AvgPool1d",
        scale_downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 2},
        scale_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [15, 41, 5, 3],
                                    "channels": 16, "max_downsample_channels": 32, "max_groups": 16, "bias": True,
                                    "downsample_scales": [4, 4, 4, 4, 1], "nonlinear_activation": "LeakyReLU",
                                    "nonlinear_activation_params": {"negative_slope": 0.1}},
        follow_official_norm=True, periods=[2, 3, 5, 7, 11],
        period_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": 4,
                                     "downsample_scales": [3, 3, 3, 3, 1], "max_downsample_channels": 32,
                                     "bias": True, "nonlinear_activation": "LeakyReLU",
                                     "nonlinear_activation_params": {"negative_slope": 0.1},
                                     "use_weight_norm": True, "use_spectral_norm": False})
    torch.manual_seed(93)
    A = AutoEncoder(**GP)
    torch.manual_seed(93)
    D = Discriminator(**d_params)
    for m, key in ((A, "chk.analyzer"), (D, "chk.discriminator")):
        chk = sum(float(p.double().abs().sum()) for p in m.parameters())
        assert abs(chk - float(g[key])) <= 1e-9 * float(g[key]), key
    G = Generator(**TG)
    sd0 = _sd(g)
    G.load_state_dict(sd0, strict=True)
    A, D, G = A.to(gpu), D.to(gpu), G.to(gpu)
    lr = 2e-4
    crit = {"mel": MultiMelSpectrogramLoss(fs=48000, fft_sizes=[2048], hop_sizes=[300], win_lengths=[2048],
                                           window="hann_window", num_mels=80, fmin=0, fmax=24000,
                                           log_base=None).to(gpu),
            "gen_adv": GeneratorAdversarialLoss(average_by_discriminators=False),
            "dis_adv": DiscriminatorAdversarialLoss(average_by_discriminators=False),
            "feat_match": FeatureMatchLoss(average_by_discriminators=False, average_by_layers=False,
                                           include_final_outputs=False)}
    cfg = {"outdir": None, "train_max_steps": 10, "use_mel_loss": True, "use_stft_loss": False,
           "use_shape_loss": False, "lambda_mel_loss": 45.0, "lambda_adv": 1.0, "lambda_feat_match": 2.0,
           "use_feat_match_loss": True, "generator_grad_norm": -1, "discriminator_grad_norm": -1,
           "generator_train_start_steps": 0, "discriminator_train_start_steps": 0}
    og = torch.optim.Adam(G.parameters(), lr=lr, betas=(0.5, 0.9), weight_decay=0.0, fused=True)
    od = torch.optim.Adam(D.parameters(), lr=lr, betas=(0.5, 0.9), weight_decay=0.0, fused=True)
    sg = torch.optim.lr_scheduler.MultiStepLR(og, milestones=[200000], gamma=0.5)
    sdd = torch.optim.lr_scheduler.MultiStepLR(od, milestones=[200000], gamma=0.5)
    tr = Trainer(steps=1, epochs=0, data_loader={}, model={"analyzer": A, "generator": G, "discriminator": D},
                 criterion=crit, optimizer={"generator": og, "discriminator": od},
                 scheduler={"generator": sg, "discriminator": sdd}, config=cfg, device=gpu)
    assert G._training_enabled
    a_before = {k: p.detach().clone() for k, p in A.named_parameters()}
    x = torch.from_numpy(g["x"])
    for s in range(2):
        tr._train_step(x)
        tol = 1e-5 if s == 0 else 1e-4
        rec = {k: float(v) for k, v in tr.total_train_loss.items()}
        ref = {k[len(f"rec.{s}."):]: float(v) for k, v in g.items() if k.startswith(f"rec.{s}.")}
        assert set(rec) == set(ref), set(rec) ^ set(ref)
        for k, v in ref.items():
            print(f"step {s} {k}: {rec[k]:.8g} (reference {v:.8g})")
        for k, v in ref.items():
            assert abs(rec[k] - v) <= tol * abs(v) + 1e-7, (s, k, rec[k], v)
        tr.total_train_loss.clear()
        if s == 0:
            for k, p in G.named_parameters():
                want = float(g["gnorm." + k])
                assert abs(float(p.grad.double().norm()) - want) <= 1e-4 * want, (k, float(p.grad.norm()), want)
    flips, tot, num, den = 0, 0, 0.0, 0.0
    for k, p in G.named_parameters():
        refd = torch.from_numpy(g["sd2." + k]).double() - sd0[k].double()
        d = p.detach().double().cpu() - sd0[k].double()
        flips += ((d - refd).abs() > 0.5 * lr).sum().item()
        tot += d.numel()
        num += ((d - refd) ** 2).sum().item()
        den += (refd ** 2).sum().item()
    print(f"two-step delta: {flips} of {tot} entries off by > 0.5 lr, norm-wise {(num / den) ** 0.5:.2e}")
    assert flips <= 0.02 * tot, (flips, tot)
    assert (num / den) ** 0.5 <= 0.10, (num / den) ** 0.5
    for k, p in A.named_parameters():
        assert not p.requires_grad and torch.equal(p.detach(), a_before[k]), k
    assert not A.training
