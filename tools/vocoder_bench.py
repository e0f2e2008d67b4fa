"""HiFi-GAN vocoder generator timing (not the flagship bench.py).  GPU only.

* one-shot forward: sel.configs.VOCODER_V1 (48 kHz, hop 300), bf16, B = 16 x
  160 latent frames (1 s of audio per clip);
* streaming: StreamGenerator.decode at B = 1, one frame (300 samples) per hop,
  the only runtime the reference's report publishes;
* per stage: time between device events at the stage boundaries, algorithmic
  flops and HBM bytes from the launches' shapes (sel.hfgops metadata), and the
  resulting share of the HBM or the dense-bf16 roof (whichever bounds the stage
  at its arithmetic intensity);
* A/B in the same call, alternated: the default dispatch against the two-launch
  residual layers (sel_tune key 71 = 1), and per (C/G, K) the fused residual
  layer (key 71 = 2) against two launches.

* --train: generator forward + backward of VOCODER_V1 in bf16 at B = 16 x 32
  latent frames (the recipes' batch_length 9600) through the training path
  (Generator.enable_training): (forward + backward) against the training
  forward alone, alternated in the same call, and per kernel instance the
  time, algorithmic bytes / flops from the launches' metadata and the share
  of its roof.  Writes profiles/vocoder_train_bench.json.

All timing is by device events after warm-up, over windows of at least 0.5 s
(whole model) / 0.2 s (single layers).  Writes JSON (default
profiles/vocoder_bench.json).

  python tools/vocoder_bench.py [--out PATH] [--batch 16] [--frames 160]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dl-speech-enhancement_amd"))

import torch  # noqa: E402

from sel import _lib as L  # noqa: E402
from sel import configs  # noqa: E402
from sel import convops as CO  # noqa: E402
from sel import hfgops as HF  # noqa: E402

HBM_PEAK = 8.0e12      # B/s, MI355X spec
BF16_PEAK = 2.5e15     # flop/s dense, MI355X spec
KEY = HF.TUNE_RESLAYER


def redraw(G, gen):
    """weights of unit-scale layers (as constructed the output is a near-constant)"""
    with torch.no_grad():
        for m in G.modules():
            v, g = getattr(m, "weight_v", None), getattr(m, "weight_g", None)
            if v is None:
                continue
            fan_in = v.shape[0] * 2 if isinstance(m, torch.nn.ConvTranspose1d) else v.shape[1] * v.shape[2]
            v.copy_(torch.randn(v.shape, generator=gen) / fan_in ** 0.5)
            g.copy_(v.norm(2, dim=(1, 2), keepdim=True) * (0.5 + torch.rand(g.shape, generator=gen)))


def staged_forward(G, xc, mark):
    """Generator.forward piece by piece, mark(name) at every stage boundary"""
    x = HF.causal(xc, G.input_conv)
    mark("input_conv")
    up = HF.slope_of(G.activation_upsamples)
    for i in range(G.num_upsamples):
        x = HF.upsample(x, G.upsamples[i], up)
        x = G._block(i, x, False)
        mark(f"stage{i}_C{G.upsamples[i].deconv.out_channels}")
    x = HF.causal(x, G.output_conv, HF.slope_of(G.activation_output1), tanh=True, out_dtype=torch.float32)
    mark("output_conv")
    return x


def event_loop(fn, min_seconds, max_iters=100000):
    """mean ms per call of fn over a window of at least min_seconds (device events)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = int(min(max_iters, max(3, min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3) + 1)))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def ab(fns, min_seconds, rounds=3):
    """alternate the variants round by round; per variant the mean of its rounds' means"""
    acc = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            acc[k].append(event_loop(fn, min_seconds / rounds)[0])
    return {k: sum(v) / len(v) for k, v in acc.items()}, {k: [round(t, 4) for t in v] for k, v in acc.items()}


def with_key(value, fn):
    def run():
        prev = L.lib().sel_tune(KEY, value)
        try:
            return fn()
        finally:
            L.lib().sel_tune(KEY, prev)
    return run


def stage_table(G, xc):
    # pass 1: launch metadata (bytes, flops) per stage through the kernel timer
    timer = L.KernelTimer({"sel_hfg_conv_fwd", "sel_hfg_reslayer_fwd"})
    cuts = []
    L.TIMER = timer
    try:
        staged_forward(G, xc, lambda name: cuts.append((name, len(timer.records))))
    finally:
        L.TIMER = None
    torch.cuda.synchronize()
    # pass 2: clean timing with events at the stage boundaries only
    reps, sums = 10, {}
    for _ in range(3):
        staged_forward(G, xc, lambda name: None)
    for _ in range(reps):
        evs = [("start", torch.cuda.Event(enable_timing=True))]
        evs[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append((name, e))
        staged_forward(G, xc, mark)
        torch.cuda.synchronize()
        for (_, a), (name, b) in zip(evs, evs[1:]):
            sums[name] = sums.get(name, 0.0) + a.elapsed_time(b)
    table, lo = [], 0
    for name, hi in cuts:
        recs = timer.records[lo:hi]
        lo = hi
        nbytes, flops = sum(r[2] for r in recs), sum(r[3] for r in recs)
        ms = sums[name] / reps
        ridge = BF16_PEAK / HBM_PEAK
        bound = "bf16" if flops / max(nbytes, 1) > ridge else "hbm"
        t_roof = max(flops / BF16_PEAK, nbytes / HBM_PEAK) * 1e3
        kernels = sorted({r[1] for r in recs})
        table.append(dict(stage=name, launches=len(recs), ms=round(ms, 4), gflop=round(flops / 1e9, 3),
                          mbytes=round(nbytes / 1e6, 3), bound=bound, roof_ms=round(t_roof, 4),
                          share_of_roof=round(t_roof / ms, 4), kernels=kernels))
    return table


def layer_ab(dev, B, gen):
    """fused residual layer (key 71 = 2) against two launches (key 71 = 1), per (C/G, K)"""
    from layers.conv_layer import CausalConv1d
    rows = []
    for Cg, T in ((32, 48000), (64, 16000)):
        for K in (3, 7, 11):
            for dil in (1, 5):
                l1 = CausalConv1d(Cg, Cg, K, dilation=dil).to(dev)
                l2 = CausalConv1d(Cg, Cg, K, dilation=1).to(dev)
                x = torch.randn(B, T, Cg, generator=gen).to(dev).to(torch.bfloat16)

                def two():
                    return HF.causal(HF.causal(x, l1, 0.1), l2, 0.1, res=x)
                mean, runs = ab({"fused": with_key(2, lambda: HF.reslayer(x, l1, l2, 0.1)),
                                 "two_launch": with_key(1, two)}, 0.4, rounds=2)
                rows.append(dict(Cg=Cg, K=K, dil=dil, rows=B * T, fused_ms=round(mean["fused"], 4),
                                 two_launch_ms=round(mean["two_launch"], 4), runs=runs))
                print(rows[-1], flush=True)
    return rows


TRAIN_CALLS = {"sel_hfg_conv_fwd", "sel_hfg_conv_bwd_data", "sel_hfg_conv_wgrad", "sel_pack_weight",
               "sel_unpack_wgrad"}


def train_bench(a):
    """generator forward + backward through the training path, bf16"""
    from models.vocoder.HiFiGAN import Generator
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    G = Generator(**configs.VOCODER_V1)
    redraw(G, gen)
    G = G.to(dev).train().enable_training()
    batch, frames = a.batch, a.frames if a.frames != 160 else 32
    x = torch.randn(batch, 64, frames, generator=gen).to(dev)
    r = torch.randn(batch, 1, 300 * frames, generator=gen).to(dev)
    res = dict(run=dict(tool="tools/vocoder_bench.py --train", date=time.strftime("%Y-%m-%d"),
                        device=torch.cuda.get_device_name(0), config="VOCODER_V1", dtype="bf16", batch=batch,
                        frames=frames, samples_per_clip=300 * frames))

    def fwd():
        return G(x)

    def fwd_bwd():
        G.zero_grad(set_to_none=True)
        G(x).backward(r)

    with CO.precision(torch.bfloat16):
        mean, runs = ab({"forward_backward": fwd_bwd, "training_forward": fwd}, 1.5)
        with torch.no_grad():
            inf = event_loop(with_key(1, lambda: G(x)), 0.5)[0]
        res["step_ms"] = dict(forward_backward=round(mean["forward_backward"], 4),
                              training_forward=round(mean["training_forward"], 4),
                              ratio=round(mean["forward_backward"] / mean["training_forward"], 3),
                              no_grad_forward_two_launch=round(inf, 4), runs=runs)
        print("step", res["step_ms"], flush=True)
        # per kernel instance: one timed pass through the kernel timer (events around every call)
        fwd_bwd()
        timer = L.KernelTimer(TRAIN_CALLS)
        L.TIMER = timer
        try:
            fwd_bwd()
        finally:
            L.TIMER = None
        rows = []
        ridge = BF16_PEAK / HBM_PEAK
        for tag, (n, ms, nbytes, flops) in timer.summary().items():
            t_roof = max(flops / BF16_PEAK, nbytes / HBM_PEAK) * 1e3
            rows.append(dict(kernel=tag, launches=n, ms=round(ms, 4), gflop=round(flops / 1e9, 3),
                             mbytes=round(nbytes / 1e6, 3), bound="bf16" if flops / max(nbytes, 1) > ridge else "hbm",
                             roof_ms=round(t_roof, 4), share_of_roof=round(t_roof / ms, 4) if ms > 0 else None))
        rows.sort(key=lambda row: -row["ms"])
        res["kernels"] = rows
        res["kernel_ms_total"] = round(sum(row["ms"] for row in rows), 4)
        for row in rows:
            print(row, flush=True)
    out = a.out if a.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "vocoder_train_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


DEFAULT_OUT = os.path.join(REPO, "profiles", "vocoder_bench.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--train", action="store_true", help="training mode: generator forward + backward (frames default 32)")
    a = ap.parse_args()
    if a.train:
        return train_bench(a)
    from models.vocoder.HiFiGAN import StreamGenerator
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    G = StreamGenerator(**configs.VOCODER_V1)
    redraw(G, gen)
    G = G.to(dev).eval().requires_grad_(False)
    res = dict(run=dict(tool="tools/vocoder_bench.py", date=time.strftime("%Y-%m-%d"),
                        device=torch.cuda.get_device_name(0), config="VOCODER_V1", dtype="bf16", batch=a.batch,
                        frames=a.frames, samples_per_clip=300 * a.frames))
    x = torch.randn(a.batch, 64, a.frames, generator=gen).to(dev)
    with torch.no_grad(), CO.precision(torch.bfloat16):
        xc = HF.enter(x)
        mean, runs = ab({"default": with_key(0, lambda: G(x)), "two_launch": with_key(1, lambda: G(x))}, 1.0)
        res["forward_ms"] = dict(default=round(mean["default"], 4), two_launch=round(mean["two_launch"], 4), runs=runs)
        print("forward", res["forward_ms"], flush=True)
        res["stages_default"] = stage_table(G, xc)
        for row in res["stages_default"]:
            print(row, flush=True)
        flops = sum(r["gflop"] for r in res["stages_default"])
        res["forward_tflops"] = round(flops / mean["default"], 2)
        # streaming: one frame per hop at B = 1
        G.reset_buffer()
        frame = torch.randn(1, 1, 64, generator=gen).to(dev)
        hop_ms, n = event_loop(lambda: G.decode(frame), 0.5)
        res["stream_hop_ms"] = dict(bf16=round(hop_ms, 4), hops=n, realtime_budget_ms=6.25)
    with torch.no_grad():
        G.reset_buffer()
        hop_ms, n = event_loop(lambda: G.decode(frame), 0.5)
        res["stream_hop_ms"]["fp32"] = round(hop_ms, 4)
        print("stream", res["stream_hop_ms"], flush=True)
        if not a.skip_layers:
            res["reslayer_ab"] = layer_ab(dev, a.batch, gen)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
