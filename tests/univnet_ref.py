"""CPU restatement of the UnivNet discriminator (reference models/vocoder/UnivNet.py
and the two UnivNet* classes of models/vocoder/modules/discriminator.py:450-638),
as pure functions over a state dict: the spectrogram (torchaudio.functional.
spectrogram(pad=win // 2, power=1.0, normalized=False) restated as a zero pad and
torch.stft(center=True, reflect).abs()), F.conv2d / leaky_relu with weight norm
applied by hand, and the period discriminators of oracle.ref_ops.  Pinned to
tests/golden/univnet_disc.npz by tests/test_univnet_host.py, as the oracle is to
its goldens.  Also the seeded parameter redraw and cotangents the golden script
and the tests share (the golden stores a checksum, not the tensors)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_ops as R

KERNELS = [(3, 9), (3, 9), (3, 9), (3, 9), (3, 3), (3, 3)]
STRIDES = [(1, 1), (1, 2), (1, 2), (1, 2), (1, 1), (1, 1)]
SPEC = {"channels": 32, "kernel_sizes": KERNELS, "strides": STRIDES, "bias": True,
        "nonlinear_activation": "LeakyReLU", "nonlinear_activation_params": {"negative_slope": 0.2}}
# the recipe's spectral settings with the reduced period discriminators of discriminator.npz
D_PARAMS = dict(
    fft_sizes=[1024, 2048, 512], hop_sizes=[120, 240, 50], win_lengths=[600, 1200, 240], window="hann_window",
    spectral_discriminator_params=SPEC, periods=[2, 3, 5, 7, 11],
    period_discriminator_params={"in_channels": 1, "out_channels": 1, "kernel_sizes": [5, 3], "channels": 4,
                                 "downsample_scales": [3, 3, 3, 3, 1], "max_downsample_channels": 32,
                                 "bias": True, "nonlinear_activation": "LeakyReLU",
                                 "nonlinear_activation_params": {"negative_slope": 0.1},
                                 "use_weight_norm": True, "use_spectral_norm": False})
SEED = 101
T_GOLDEN = 1800


def spectrogram(x, n_fft, hop, win, window):
    """x (..., T) -> |STFT| (..., bins, frames) of the signal zero-padded by win // 2."""
    shape = x.shape
    xp = F.pad(x.reshape(-1, shape[-1]), (win // 2, win // 2))
    s = torch.stft(xp, n_fft, hop, win, window.to(x.dtype), center=True, pad_mode="reflect", normalized=False,
                   onesided=True, return_complex=True).abs()
    return s.reshape(shape[:-1] + s.shape[-2:])


def frames(T, win, hop):
    return 1 + (T + 2 * (win // 2)) // hop


def geometry(T, n_fft, hop, win, kernels=KERNELS, strides=STRIDES):
    """[(H, W)] of the spectrogram and of every layer's output (valid padding)."""
    H, W = frames(T, win, hop), n_fft // 2 + 1
    out = [(H, W)]
    for (kh, kw), (sh, sw) in zip(kernels, strides):
        H, W = (H - kh) // sh + 1, (W - kw) // sw + 1
        out.append((H, W))
    return out


def spectral_discriminator(P, pre, x, n_fft, hop, win, strides=STRIDES, slope=0.2, layers=False):
    """UnivNetSpectralDiscriminator.forward: x (B, 1, T) -> (B, 1, H', W')."""
    h = spectrogram(x, n_fft, hop, win, P[pre + ".window"]).transpose(-1, -2)
    n = len(strides)
    outs = []
    for i, s in enumerate(strides):
        key = f"{pre}.layers.{i}.0" if i < n - 1 else f"{pre}.layers.{i}"
        h = F.conv2d(h, R._wn(P, key), P.get(key + ".bias"), stride=tuple(s))
        if i < n - 1:
            h = F.leaky_relu(h, slope)
        outs.append(h)
    return outs if layers else h


def discriminator(P, x, fft_sizes, hop_sizes, win_lengths, spectral_discriminator_params=SPEC,
                  periods=(2, 3, 5, 7, 11), period_discriminator_params=None, flat_channel=False, **_):
    """UnivNet.Discriminator.forward: the spectral tensors, then the period lists."""
    b, c, t = x.shape
    if c != 1 and flat_channel:
        x = x.reshape(b * c, 1, t)
    sp = spectral_discriminator_params
    slope = sp.get("nonlinear_activation_params", {}).get("negative_slope", 0.2)
    outs = [spectral_discriminator(P, f"mrsd.discriminators.{i}", x, n, h, w, sp["strides"], slope)
            for i, (n, h, w) in enumerate(zip(fft_sizes, hop_sizes, win_lengths))]
    pp = period_discriminator_params or {}
    plan = R.period_discriminator_plan(**pp)
    pslope = pp.get("nonlinear_activation_params", {}).get("negative_slope", 0.1)
    for i, p in enumerate(periods):
        outs.append(R.period_discriminator(P, f"mpd.discriminators.{i}", x, p, plan, pslope))
    return outs


def redraw(module, seed=SEED):
    """Seeded parameters for a weight-normalised discriminator, in module order:
    v ~ N(0, 1 / fan_in), g = ||v|| * U(0.5, 1.5), bias ~ 0.1 N(0, 1), all
    fp16-representable.  Returns the checksum the golden stores."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            v, g = getattr(m, "weight_v", None), getattr(m, "weight_g", None)
            if v is None:
                continue
            v.copy_(torch.randn(v.shape, generator=gen) / float(v[0].numel()) ** 0.5)
            g.copy_(v.flatten(1).norm(dim=1).view(g.shape) * (0.5 + torch.rand(g.shape, generator=gen)))
            if m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
        for p in module.parameters():
            p.copy_(p.half().float())
    return checksum(module)


def checksum(module):
    return float(sum(float(p.detach().double().abs().sum()) * (i + 1) for i, p in enumerate(module.parameters())))


def cotangent(shape, i, j=0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(7000 + 100 * i + j))


def flat_outputs(outs):
    """{name: tensor} of a discriminator output: out.<i> for a spectral tensor,
    out.<i>.<j> for the layers of a period discriminator."""
    d = {}
    for i, o in enumerate(outs):
        if torch.is_tensor(o):
            d[f"out.{i}"] = o
        else:
            for j, t in enumerate(o):
                d[f"out.{i}.{j}"] = t
    return d


def weighted_sum(outs):
    """sum over outputs of <out, cotangent>: the scalar the goldens differentiate."""
    tot = 0.0
    for name, t in flat_outputs(outs).items():
        idx = [int(s) for s in name.split(".")[1:]]
        tot = tot + (t * cotangent(t.shape, *idx).to(device=t.device, dtype=t.dtype)).sum()
    return tot


def gan_inputs(seed=SEED + 1, B=3, T=T_GOLDEN):
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn(B, 1, T, generator=g), 0.5 * torch.randn(B, 1, T, generator=g)


def gan_terms(D, y_hat, y):
    """The recipe's GAN terms (no averaging, include_final_outputs=False) on a
    discriminator callable: generator adversarial + feature matching on D(y_hat)
    against D(y), and the discriminator's real / fake losses."""
    p_ = D(y_hat)
    with torch.no_grad():
        p = D(y)
    adv = R.generator_adv_loss(p_, average_by_discriminators=False)
    fm = R.feat_match_loss(p_, p, average_by_layers=False, average_by_discriminators=False,
                           include_final_outputs=False)
    real, fake = R.discriminator_adv_loss(D(y_hat.detach()), D(y), average_by_discriminators=False)
    return adv, fm, real, fake


def load_disc_golden(golden):
    """univnet_disc.npz with the parameter-gradient files it is split into."""
    g = golden("univnet_disc")
    g.update(golden("univnet_disc_g01"))
    g.update(golden("univnet_disc_g2"))
    return g


def to_np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())
