"""Generate the UnivNet discriminator goldens by importing the reference (build container only).

Run:  python tests/golden/make_goldens_univnet.py  [--ref /root/reference]

Imports the reference read-only (never copied, never shipped), reusing
make_goldens.py's stubs.  torchaudio is absent in the build container, so the
``torchaudio.functional.spectrogram`` stub is replaced by the restatement of
tests/univnet_ref.py (zero pad win // 2, torch.stft(center=True, reflect), abs):
parity with torchaudio itself is not pinned by these goldens.  Records on the CPU:

* ``univnet_disc.npz`` (+ ``univnet_disc_g01.npz`` / ``univnet_disc_g2.npz``: the
  parameter gradients of the three spectral sub-discriminators, split off to
  keep each fixture under 1 MiB)
  the reference ``UnivNet.Discriminator`` at the recipe's spectral settings
  (channels 32, the three resolutions) with the reduced period discriminators of
  discriminator.npz, parameters redrawn by seed (univnet_ref.redraw; a checksum
  is stored, not the tensors), x = randn(3, 1, 1800) from the first seed whose
  gradients are stable under fp32 rounding (_stable): 1800 samples is the
  smallest round length at which the 2048 / 240 resolution still has an output
  (13 frames -> 1 x 117; the others give 9 x 53 and 29 x 21).  The reference runs
  in FP64; every output, grad_x for sum <out, r> (seeded r: univnet_ref.cotangent)
  and every parameter gradient are stored as fp32, with e32.<name> = ||fp32 run -
  fp64 run|| / ||fp64 run||, the reference's own fp32 noise.  Also the default-
  argument ``state_dict`` key list and shapes, and geo.<T>.<i>: the output (H', W')
  of spectral sub-discriminator i for T in {1800, 9600} samples.
* ``univnet_gan_terms.npz``  for a seeded pair (y_hat, y): the reference's
  generator adversarial, feature-matching and discriminator real / fake losses
  with the recipe's settings (no averaging, include_final_outputs=False) and the
  gradient of (adversarial + feature matching) w.r.t. y_hat, FP64 stored as fp32.
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_goldens as MG  # noqa: E402
import make_goldens_vocoder as MV  # noqa: E402
import univnet_ref as U  # noqa: E402

# the tests' fp32 bounds; the reference's own fp32 noise must stay within a third
TOL_OUT, TOL_GRAD = 1e-5, 1e-4


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _spectrogram(waveform, pad, window, n_fft, hop_length, win_length, power, normalized):
    assert power == 1.0 and not normalized and pad == win_length // 2
    return U.spectrogram(waveform, n_fft, hop_length, win_length, window)


def _build(UN):
    torch.manual_seed(U.SEED)
    D = UN.Discriminator(**copy.deepcopy(U.D_PARAMS))
    chk = U.redraw(D)
    return D, chk


def _clone(UN, D, dt):
    """A fresh module with D's parameters (weight-normalised modules do not deepcopy)."""
    M = UN.Discriminator(**copy.deepcopy(U.D_PARAMS))
    M.load_state_dict(D.state_dict(), strict=True)
    return M.to(dt)


EPS32 = 2.0 ** -23
N_PERTURB = 8
SEEDS = 64


def _ulp_perturbed(x, j):
    """x with every sample moved by one fp32 ulp up or down (seeded signs)."""
    sgn = torch.randint(0, 2, x.shape, generator=torch.Generator().manual_seed(900 + j)).float() * 2 - 1
    return x * (1 + EPS32 * sgn)


def _stable(run, inputs, tol):
    """LeakyReLU' and the L1 sign are discontinuous: where a pre-activation (or a
    feature difference) of the fixture lies within fp32 rounding of zero, two
    correct fp32 implementations land on different sides and their gradients
    differ by ~1e-3 (one unit of ~1e6), far above the tests' 1e-4.  As
    make_goldens_autoencoder_train.py rejects seeds with a near-tie at the
    codebooks, a fixture is accepted only if the REFERENCE's fp32 results stay
    within a third of the tests' bounds of its fp64 results, both on the inputs
    as drawn and on N_PERTURB copies moved by one fp32 ulp per sample
    (independent samples of fp32-level rounding).  run(inputs, dtype) -> {name:
    tensor}; returns (fp64 results, fp32 results, worst error / bound)."""
    r64 = run(inputs, torch.float64)
    r32 = run(inputs, torch.float32)
    worst = max(_rel(r32[k].reshape(-1), v.reshape(-1)) / tol(k) for k, v in r64.items())
    for j in range(N_PERTURB):
        if worst > 1.0 / 3:
            break
        rp = run([_ulp_perturbed(t, j) for t in inputs], torch.float32)
        worst = max(worst, max(_rel(rp[k].reshape(-1), v.reshape(-1)) / tol(k) for k, v in r64.items()))
    return r64, r32, worst


def make_disc(UN):
    D, chk = _build(UN)
    sd0 = UN.Discriminator().state_dict()
    # the golden parameters load into the restatement's key set
    P = {k: v.double() for k, v in D.state_dict().items()}

    def run(inputs, dt):
        M = _clone(UN, D, dt)
        xi = inputs[0].detach().to(dt).clone().requires_grad_(True)
        outs = M(xi)
        assert torch.is_tensor(outs[0]) and isinstance(outs[3], list)
        U.weighted_sum(outs).backward()
        r = {k: v.detach() for k, v in U.flat_outputs(outs).items()}
        r["grad_x"] = xi.grad
        r.update({"g." + k: p.grad for k, p in M.named_parameters()})
        return r

    tol = lambda k: TOL_OUT if k.startswith("out.") else TOL_GRAD  # noqa: E731
    for seed in range(U.SEED + 7, U.SEED + 7 + SEEDS):
        x = torch.randn(3, 1, U.T_GOLDEN, generator=torch.Generator().manual_seed(seed))
        r64, r32, worst = _stable(run, [x], tol)
        print(f"univnet_disc: input seed {seed}: worst fp32 error {worst:.2f} x the bound (accepted below 1/3)")
        if worst <= 1.0 / 3:
            break
    else:
        raise AssertionError("no fp32-stable input found")
    d = {"chk": np.float64(chk), "x": MG._np(x), "seed": np.int64(seed)}
    d["keys"] = np.array(list(sd0.keys()))
    d["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd0.values()])
    ours = U.flat_outputs(U.discriminator(P, x.double(), **U.D_PARAMS))
    for k, v in ours.items():
        assert _rel(v, r64[k]) < 1e-12, (k, _rel(v, r64[k]))
    shapes = [tuple(r64[f"out.{i}"].shape) for i in range(3)]
    assert shapes == [(3, 1, 9, 53), (3, 1, 1, 117), (3, 1, 29, 21)], shapes
    assert bool(torch.isfinite(r64["grad_x"]).all())
    for n, h, w in zip(U.D_PARAMS["fft_sizes"], U.D_PARAMS["hop_sizes"], U.D_PARAMS["win_lengths"]):
        s = U.spectrogram(x.double(), n, h, w, torch.hann_window(w, dtype=torch.float64)).detach()
        assert float(s[..., 0].abs().max()) == 0.0, (n, float(s[..., 0].abs().max()))   # frame 0 is exactly zero
    # output shape of every spectral sub-discriminator at the golden and the recipe length
    with torch.no_grad():
        for T in (U.T_GOLDEN, 9600):
            for i, f in enumerate(D.mrsd.discriminators):
                d[f"geo.{T}.{i}"] = np.array(f(torch.zeros(1, 1, T)).shape[2:], dtype=np.int64)
    for k, v in r64.items():
        assert float(v.abs().max()) > 0, k
        d[k] = MG._np(v.float())
        e = _rel(r32[k], v)
        d["e32." + k] = np.float64(e)
        assert e <= tol(k) / 3, (k, e)
    print(f"univnet_disc: {sum(p.numel() for p in D.parameters())} parameters, worst e32 "
          f"{max(float(v) for k, v in d.items() if k.startswith('e32.')):.1e}")
    return d


def make_gan_terms(ref, UN):
    adv = MG._load("ref_adversarial_loss", os.path.join(ref, "losses", "adversarial_loss.py"))
    fm = MG._load("ref_feat_match_loss", os.path.join(ref, "losses", "feat_match_loss.py"))
    D, chk = _build(UN)

    def run(inputs, dt):
        M = _clone(UN, D, dt)
        yh = inputs[0].detach().to(dt).clone().requires_grad_(True)
        yt = inputs[1].detach().to(dt)
        p_ = M(yh)
        with torch.no_grad():
            p = M(yt)
        la = adv.GeneratorAdversarialLoss(average_by_discriminators=False)(p_)
        lf = fm.FeatureMatchLoss(average_by_discriminators=False, average_by_layers=False,
                                 include_final_outputs=False)(p_, p)
        (la + lf).backward()
        real, fake = adv.DiscriminatorAdversarialLoss(average_by_discriminators=False)(M(yh.detach()), M(yt))
        return {"loss.gen_adv": la.detach(), "loss.feat_match": lf.detach(), "loss.dis_real": real.detach(),
                "loss.dis_fake": fake.detach(), "grad": yh.grad}

    tol = lambda k: TOL_GRAD if k == "grad" else TOL_OUT  # noqa: E731
    for seed in range(U.SEED + 1, U.SEED + 1 + SEEDS):
        y_hat, y = U.gan_inputs(seed)
        r64, r32, worst = _stable(run, [y_hat, y], tol)
        print(f"univnet_gan_terms: input seed {seed}: worst fp32 error {worst:.2f} x the bound (accepted below 1/3)")
        if worst <= 1.0 / 3:
            break
    else:
        raise AssertionError("no fp32-stable input found")
    d = {"chk": np.float64(chk), "y_hat": MG._np(y_hat), "y": MG._np(y), "seed": np.int64(seed)}
    P = {k: v.double() for k, v in D.state_dict().items()}
    ours = U.gan_terms(lambda v: U.discriminator(P, v, **U.D_PARAMS), y_hat.double(), y.double())
    for a, k in zip(ours, ("loss.gen_adv", "loss.feat_match", "loss.dis_real", "loss.dis_fake")):
        assert abs(float(a) - float(r64[k])) <= 1e-12 * abs(float(r64[k])), k
    for k, v in r64.items():
        d[k] = MG._np(v.float())
        e = _rel(r32[k].reshape(-1), v.reshape(-1))
        d["e32." + k] = np.float64(e)
        assert e <= tol(k) / 3, (k, e)
        print(f"univnet_gan_terms: {k} e32 {e:.1e}")
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    MG._install_stubs(a.ref)
    MG._install_trainer_stubs()
    sys.modules["torchaudio"].functional.spectrogram = _spectrogram
    import models.vocoder.UnivNet as UN
    assert os.path.abspath(UN.__file__).startswith(os.path.abspath(a.ref)), UN.__file__
    d = make_disc(UN)
    g01, g2 = ("g.mrsd.discriminators.0.", "g.mrsd.discriminators.1."), "g.mrsd.discriminators.2."
    MV.save(a.out, "univnet_disc.npz", {k: v for k, v in d.items() if not k.startswith(g01 + (g2,))})
    MV.save(a.out, "univnet_disc_g01.npz", {k: v for k, v in d.items() if k.startswith(g01)})
    MV.save(a.out, "univnet_disc_g2.npz", {k: v for k, v in d.items() if k.startswith(g2)})
    MV.save(a.out, "univnet_gan_terms.npz", make_gan_terms(a.ref, UN))


if __name__ == "__main__":
    main()
