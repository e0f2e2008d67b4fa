"""Generate the HiFi-GAN vocoder goldens by importing the reference (build container only).

Run:  python tests/golden/make_goldens_vocoder.py  [--ref /root/reference]

Imports the reference ``models/vocoder/HiFiGAN.py`` the way make_goldens.py
imports the rest (read-only, never copied, never shipped; the same torchaudio
stub, because that file also imports the discriminators) and records on the CPU:

* ``vocoder_v1.npz``  StreamGenerator at reduced width in the MultiGroupConv1d
  form (groups 3, one kernel size 11): state dict, a (2, 64, 7) input with its
  one-shot forward output, seven 1-frame ``decode`` chunks of sample 0 with
  every final ``pad_buffer``, and the parameter count of the full-width
  AudioDec v1 vocoder (sel.configs.VOCODER_V1).
* ``vocoder_v0.npz``  the same in the MultiReceptiveField form (kernel sizes
  3, 7, 11, groups 1), plus the output after ``remove_weight_norm()``.
* ``audiodec_baseline.npz``  the comparison system of testing_denoise.py:97-101:
  reduced-width PQC autoencoder (encoder -> projector -> quantizer) chained with
  the v1 vocoder above (its weights are read from vocoder_v1.npz by the tests,
  not stored twice) on 3600 samples of real speech.

The parameters are redrawn after construction: weight_v ~ N(0, 1/fan_in),
weight_g = ||v|| * U(0.5, 1.5), bias ~ N(0, 0.1) -- as constructed (normal_(0,
0.01)) the output is a near-constant against which a norm-wise comparison sees
nothing -- and rounded to fp16-representable values BEFORE the reference runs,
so the state dict is stored exactly in half the bytes (committed files stay
below 1 MiB).  The script asserts on the reference output that its standard
deviation over time is at least 0.3 x its RMS and that fewer than 1 % of the
samples exceed 0.99 in magnitude.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as MG  # noqa: E402

SCALES = dict(upsample_scales=[5, 5, 4, 3], upsample_kernel_sizes=[10, 10, 8, 6])
V1 = dict(in_channels=64, channels=64, resblock_kernel_sizes=[11], resblock_dilations=[[1, 3, 5]], groups=3, **SCALES)
V0 = dict(in_channels=64, channels=32, resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3,
          groups=1, **SCALES)
GP = dict(encode_channels=4, decode_channels=4, code_dim=64, codebook_num=2, codebook_size=64)
LIMIT = 1 << 20   # bytes per committed fixture


def redraw(G, gen):
    with torch.no_grad():
        for m in G.modules():
            v, g = getattr(m, "weight_v", None), getattr(m, "weight_g", None)
            if v is None:
                continue
            if isinstance(m, torch.nn.ConvTranspose1d):
                fan_in = v.shape[0] * v.shape[2] // m.stride[0]
            else:
                fan_in = v.shape[1] * v.shape[2]
            v.copy_(torch.randn(v.shape, generator=gen) / fan_in ** 0.5)
            norm = v.norm(2, dim=(1, 2), keepdim=True)
            g.copy_(norm * (0.5 + torch.rand(g.shape, generator=gen)))
            if m.bias is not None:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
        for p in G.parameters():
            p.copy_(p.half().float())


def check_output(y, tag):
    y = y.double()
    rms = float(y.pow(2).mean().sqrt())
    std = float(y.std(dim=-1).mean())
    hot = float((y.abs() > 0.99).double().mean())
    print(f"{tag}: std over time {std:.3f}, rms {rms:.3f}, |y| > 0.99: {100 * hot:.2f} %")
    assert std >= 0.3 * rms and hot < 0.01, (tag, std, rms, hot)


def sd16(G):
    """state dict with the (fp16-representable) float parameters stored as fp16"""
    d = {}
    for k, v in G.state_dict().items():
        a = MG._np(v)
        if a.dtype == np.float32 and not k.endswith("pad_buffer"):
            assert np.array_equal(a.astype(np.float16).astype(np.float32), a), k
            a = a.astype(np.float16)
        d["sd." + k] = a
    return d


def save(out, name, d):
    path = os.path.join(out, name)
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print(f"{name}: {size} bytes")
    assert size < LIMIT, (name, size)


def make_vocoder(H, params, tag, seed, out, extra=None):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    G = H.StreamGenerator(**params)
    G.eval()
    redraw(G, gen)
    d = sd16(G)
    x = torch.randn(2, params["in_channels"], 7, generator=gen)
    d["x"] = MG._np(x)
    with torch.no_grad():
        y = G(x)
        check_output(y, tag)
        d["y"] = MG._np(y)
        G.reset_buffer()
        for c in range(7):
            d[f"y.{c}"] = MG._np(G.decode(x[:1, :, c:c + 1].transpose(2, 1).contiguous()))
        d.update({"buf." + k: MG._np(v) for k, v in G.state_dict().items() if k.endswith("pad_buffer")})
        ys = torch.cat([torch.from_numpy(d[f"y.{c}"]) for c in range(7)], -1)
        # the streamed chunks equal the one-shot output once the transposed convs'
        # replicate-versus-zero start has left the receptive field
        d["stream_vs_oneshot_from_600"] = np.float64(
            float((ys[..., 600:] - y[:1, :, 600:]).norm() / y[:1, :, 600:].norm()))
        print(f"{tag}: stream vs one-shot from sample 600: {float(d['stream_vs_oneshot_from_600']):.2e}")
        G.reset_buffer()
    if extra is not None:
        d.update(extra)
    return G, x, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    MG._install_stubs(a.ref)
    MG._install_trainer_stubs()
    import models.vocoder.HiFiGAN as H
    assert os.path.abspath(H.__file__).startswith(os.path.abspath(a.ref)), H.__file__
    # this package's settings file, by path (the reference's packages own the import names)
    configs = MG._load("sel_configs", os.path.join(MG.REPO, "dl-speech-enhancement_amd", "sel", "configs.py"))

    full = H.StreamGenerator(**configs.VOCODER_V1)
    count = {"full_width_param_count": np.int64(sum(p.numel() for p in full.parameters()))}
    del full
    G1, _, d1 = make_vocoder(H, V1, "v1", 93, a.out, count)
    save(a.out, "vocoder_v1.npz", d1)

    G0, x0, d0 = make_vocoder(H, V0, "v0", 94, a.out)
    with torch.no_grad():
        G0.remove_weight_norm()
        d0["y_no_weight_norm"] = MG._np(G0(x0))
    save(a.out, "vocoder_v0.npz", d0)

    # the AudioDec baseline chain (testing_denoise.py:97-101)
    import models.autoencoder.AudioDec as AD
    clean, _ = MG._audio(a.ref)
    torch.manual_seed(93)
    E = AD.Generator(**GP)
    E.eval()
    d = MG._sd(E)
    x = torch.from_numpy(clean[0][:3600]).float().view(1, 1, -1)
    d["x"] = MG._np(x)
    with torch.no_grad():
        z = E.projector(E.encoder(x))
        zq, _, _ = E.quantizer(z)
        _, idx = E.quantizer.inference(z)
        y = G1(zq)
    d.update({"z": MG._np(z), "zq": MG._np(zq), "idx": MG._np(idx), "y": MG._np(y)})
    save(a.out, "audiodec_baseline.npz", d)


if __name__ == "__main__":
    main()
