#!/usr/bin/env python3
"""Per-layer timing of the UnivNet spectral discriminator's 2-D conv kernels
against torch.nn.functional.conv2d (bf16, channels_last) on the same tensors,
and the full discriminator forward + backward with and without side streams.

  python tools/univ_probe.py [--out profiles/univ_probe.md] [--reps 20]

Sizes: the recipe's (B = 16 x 9600 samples) and the C5 clip length (16 x 48000).
Each of the 18 layer instances (3 resolutions x 6 layers) runs our forward,
data-gradient and weight-gradient launches and torch's forward / input-gradient /
weight-gradient, alternating in one process; HIP events around `reps` back-to-back
launches after a warm-up, median of 3 windows.  Algorithmic bytes = the
activations read and written once + the weights; flops = 2 * outputs * taps *
Cin.  Share of peak = max(bytes / 6.29 TB/s measured copy rate, flops / 2517
TFLOP/s bf16 matrix peak) / time.  Needs the GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dl-speech-enhancement_amd")):
    sys.path.insert(0, p)

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # torch's side: no exhaustive algorithm search per shape

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM, PEAK = 6.29e12, 2516.8e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out)


def layer_rows(T, B, reps, dev):
    from models.vocoder.UnivNet import Discriminator
    from sel import sconvops as SC
    from sel import configs
    D = Discriminator(**configs.get("symADuniv_vctk_48000_hop300")["discriminator_params"]).to(dev)
    dt = torch.bfloat16
    rows = []
    for f in D.mrsd.discriminators:
        geo = f.geometry(T)
        params = f._params()
        for li, sp in enumerate(f.plan()):
            H, W = geo[li]
            Ho, Wo = geo[li + 1]
            v, g, b = params[3 * li:3 * li + 3]
            w = SC.effective_weight(v, g)
            x = torch.randn(B, H, W, sp.cin, device=dev).to(SC._in_dtype(sp, dt))
            gy = torch.randn(B, Ho, Wo, sp.cout, device=dev).to(SC._out_dtype(sp, dt))
            wf, wa = SC._pack_fwd(sp, w, dt), SC._pack_adj(sp, w, dt)
            bias = b.detach().float().contiguous()
            aux = x if sp.cin != 1 else None
            ours = [lambda: SC.conv_fwd(sp, x, wf, bias, f.slope, dt),
                    lambda: SC.conv_bwd_data(sp, gy, wa, aux, x.shape, f.slope, dt),
                    lambda: SC.conv_wgrad(sp, gy, x, f.slope, dt)]
            # torch on the same tensors: NCHW views of the channels-last rows, bf16
            xt = x.to(dt).permute(0, 3, 1, 2)
            gt = gy.to(dt).permute(0, 3, 1, 2)
            wt = w.to(dt).contiguous(memory_format=torch.channels_last)
            bt = bias.to(dt)
            st = (sp.sh, sp.sw)
            theirs = [lambda: F.conv2d(xt, wt, bt, stride=st),
                      lambda: torch.ops.aten.convolution_backward(gt, xt, wt, None, st, (0, 0), (1, 1), False, (0, 0), 1,
                                                                  (True, False, False)),
                      lambda: torch.ops.aten.convolution_backward(gt, xt, wt, [sp.cout], st, (0, 0), (1, 1), False,
                                                                  (0, 0), 1, (False, True, True))]
            t = []
            for a, c in zip(ours, theirs):   # alternating: ours, torch, ours, torch, ...
                t += [timed(a, reps), timed(c, reps)]
            nb = x.numel() * x.element_size() + gy.numel() * gy.element_size() + w.numel() * 2
            fl = 2.0 * gy.numel() * sp.kh * sp.kw * sp.cin
            floor_us = max(nb / HBM, fl / PEAK) * 1e6
            bound = "HBM" if nb / HBM >= fl / PEAK else "MFMA"
            rows.append((f.fft_size, li, f"{sp.cin}->{sp.cout} k{sp.kh}x{sp.kw} s{sp.sw}", f"{H}x{W}", t, nb, fl,
                         floor_us, bound))
            print(f"T={T} n_fft={f.fft_size} layer {li}: " + " ".join(f"{v:.1f}" for v in t), flush=True)
    return rows, D


def full_d(D, T, B, reps, dev):
    from sel.convops import precision
    x = torch.randn(B, 1, T, device=dev)

    def step():
        for p in D.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        with precision(torch.bfloat16):
            outs = D(xi)
            tot = sum((o.float() ** 2).mean() if torch.is_tensor(o) else (o[-1].float() ** 2).mean() for o in outs)
        tot.backward()

    res = {}
    for n in ("8", "0", "8", "0"):       # alternating
        os.environ["SEL_D_STREAMS"] = n
        res.setdefault(n, []).append(timed(step, max(3, reps // 4)) / 1e3)
    os.environ.pop("SEL_D_STREAMS", None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "univ_probe.md"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("univ_probe: no GPU visible (this tool measures; it has no fallback)")
    dev = torch.device("cuda:0")
    lines = ["# UnivNet spectral discriminator: per-layer launches (bf16, MI355X)", "",
             f"HIP events around {a.reps} back-to-back launches, median of 3 windows, ours and torch alternating "
             "in one process.  `floor` = max(algorithmic bytes / 6.29 TB/s, flops / 2517 TFLOP/s); "
             "`share` = floor / our forward time.", ""]
    for name, T in (("recipe, 16 x 9600", 9600), ("C5 length, 16 x 48000", 48000)):
        rows, D = layer_rows(T, 16, a.reps, dev)
        lines += [f"## {name}", "",
                  "| n_fft | layer | shape | input HxW | fwd us | torch fwd | dgrad us | torch dgrad | wgrad us | "
                  "torch wgrad | floor us (bound) | fwd share | fwd TB/s |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for n_fft, li, shape, hw, t, nb, fl, floor_us, bound in rows:
            lines.append(f"| {n_fft} | {li} | {shape} | {hw} | {t[0]:.1f} | {t[1]:.1f} | {t[2]:.1f} | {t[3]:.1f} | "
                         f"{t[4]:.1f} | {t[5]:.1f} | {floor_us:.1f} ({bound}) | {floor_us / t[0]:.2f} | "
                         f"{nb / t[0] / 1e6:.2f} |")
        res = full_d(D, T, 16, a.reps, dev)
        lines += ["", f"Full discriminator (MRSD + MPD) forward + backward, bf16, B = 16: side streams "
                  f"{' / '.join(f'{v:.2f}' for v in res['8'])} ms, SEL_D_STREAMS=0 "
                  f"{' / '.join(f'{v:.2f}' for v in res['0'])} ms.", ""]
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:      # rewritten after each size: a partial run keeps what it measured
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
