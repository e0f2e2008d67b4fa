"""Time sel_bss_sdr beside the same formula in plain torch on the
same GPU: fp64 torch.fft.rfft / irfft for the correlations and
torch.linalg.solve on the explicit Toeplitz matrix, which is what a user
without torchmetrics would otherwise run.  Device events around each call,
medians over --reps calls after --warm calls, the inputs rotated over four
seeded sets; both paths alternate inside one process.

The split between the correlation and the solve comes from a kernel trace,
taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/bss_sdr_bench.py --calls-only
    python tools/bss_sdr_bench.py --kernel-trace DIR --out profiles/bss_sdr_bench

usage: python tools/bss_sdr_bench.py [--kernel-trace DIR] [--out PREFIX]   (GPU)"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dl-speech-enhancement_amd")]

import torch  # noqa: E402

from sel import _lib as L  # noqa: E402

SHAPES = [(1, 96000), (16, 96000), (16, 480000)]
TAPS = 512
SETS = 4
TRACE_WARM, TRACE_CALLS = 2, 10
KERNELS = ("k_bss_corr", "k_bss_solve", "k_bss_mean")


def inputs(B, T, dev):
    """SETS seeded (pred, target) pairs: FIR-coloured noise, and white noise added at 10 dB."""
    out = []
    for s in range(SETS):
        g = torch.Generator(device="cpu").manual_seed(100 + s)
        e = torch.randn(B, T + 2, generator=g, dtype=torch.float64)
        t = (e[:, 2:] + 0.9 * e[:, 1:-1] + 0.4 * e[:, :-2]).float()
        n = torch.randn(B, T, generator=g)
        p = t + n * (t.norm(dim=-1, keepdim=True) / n.norm(dim=-1, keepdim=True)) * 10 ** (-10 / 20)
        out.append((p.to(dev).contiguous(), t.to(dev).contiguous()))
    return out


class Hip:
    def __init__(self, B, T, dev):
        self.B, self.T = B, T
        self.ws = L.workspace(L.lib().sel_bss_sdr_workspace(B, T, TAPS), dev)
        self.vals = torch.empty(B, dtype=torch.float32, device=dev)
        self.mean = torch.empty((), dtype=torch.float32, device=dev)

    def __call__(self, p, t):
        L.call("sel_bss_sdr", L.ptr(p), L.ptr(t), self.B, self.T, TAPS, 0, 0.0, L.ptr(self.vals), L.ptr(self.mean),
               None, L.ptr(self.ws), self.ws.numel(), L.stream())
        return self.vals


def torch_sdr(p, t):
    """torchmetrics 1.2.0 signal_distortion_ratio (direct solve) restated in plain torch, fp64."""
    p, t = p.double(), t.double()
    t = t / t.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    p = p / p.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    n_fft = 2 ** math.ceil(math.log2(2 * p.shape[-1] - 1))
    tf = torch.fft.rfft(t, n_fft)
    r = torch.fft.irfft(tf.real ** 2 + tf.imag ** 2, n_fft)[..., :TAPS]
    b = torch.fft.irfft(tf.conj() * torch.fft.rfft(p, n_fft), n_fft)[..., :TAPS]
    i = torch.arange(TAPS, device=p.device)
    R = r[..., (i[:, None] - i[None, :]).abs()]
    sol = torch.linalg.solve(R, b)
    coh = (b * sol).sum(-1)
    return (10 * torch.log10(coh / (1 - coh))).float()


def time_calls(fns, sets, warm, reps):
    """{name: [ms]}: the paths alternate call by call, each on the next input set."""
    for k in range(warm):
        for f in fns.values():
            f(*sets[k % SETS])
    torch.cuda.synchronize()
    out = {n: [] for n in fns}
    for k in range(reps):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(*sets[k % SETS])
            e1.record()
            torch.cuda.synchronize()
            out[n].append(e0.elapsed_time(e1))
    return out


def read_trace(d):
    """{shape index: {kernel: median us}} from the kernel trace of a --calls-only run."""
    path = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = len(KERNELS)
    per_shape = (TRACE_WARM + TRACE_CALLS) * per_call
    assert len(rows) == per_shape * len(SHAPES), (len(rows), per_shape)
    out = {}
    for si in range(len(SHAPES)):
        mine = rows[si * per_shape + TRACE_WARM * per_call:(si + 1) * per_shape]
        out[si] = {}
        for k in KERNELS:
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine if k in r["Kernel_Name"]]
            assert len(us) == TRACE_CALLS, (k, len(us))
            out[si][k] = statistics.median(us)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls-only", action="store_true", help="only launch (for a kernel trace)")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 kernel trace of --calls-only")
    ap.add_argument("--out", default=None, help="write PREFIX.json and PREFIX.md")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bss_sdr_bench: needs the GPU")
    dev = torch.device("cuda")
    if a.calls_only:
        for B, T in SHAPES:
            sets, hip = inputs(B, T, dev), Hip(B, T, dev)
            for k in range(TRACE_WARM + TRACE_CALLS):
                hip(*sets[k % SETS])
            torch.cuda.synchronize()
        return
    split = read_trace(a.kernel_trace) if a.kernel_trace else None
    res = []
    for si, (B, T) in enumerate(SHAPES):
        sets, hip = inputs(B, T, dev), Hip(B, T, dev)
        diff = max((hip(p, t).double() - torch_sdr(p, t).double()).abs().max().item() for p, t in sets)
        ms = time_calls({"hip": hip, "torch": torch_sdr}, sets, a.warm, a.reps)
        r = dict(B=B, T=T, filter_length=TAPS, reps=a.reps,
                 hip_ms_median=statistics.median(ms["hip"]), hip_ms_min=min(ms["hip"]),
                 torch_ms_median=statistics.median(ms["torch"]), torch_ms_min=min(ms["torch"]),
                 max_abs_db_hip_minus_torch=diff)
        r["torch_over_hip"] = r["torch_ms_median"] / r["hip_ms_median"]
        if split:
            r["kernel_us_median"] = split[si]
        res.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=res), f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# sel_bss_sdr beside the torch fp64 formula (tools/bss_sdr_bench.py)\n\n")
            f.write(f"{torch.cuda.get_device_name(0)}; filter_length {TAPS}; device events, medians of {a.reps} calls "
                    f"after {a.warm}, inputs rotated over {SETS} sets, the two paths alternating.\n\n")
            f.write("| B | T | HIP ms (median / min) | torch fp64 ms (median / min) | torch / HIP | "
                    "correlation us | solve us | mean us | max dB difference |\n" + "|---" * 9 + "|\n")
            for r in res:
                k = r.get("kernel_us_median", {})
                f.write(f"| {r['B']} | {r['T']} | {r['hip_ms_median']:.3f} / {r['hip_ms_min']:.3f} | "
                        f"{r['torch_ms_median']:.3f} / {r['torch_ms_min']:.3f} | {r['torch_over_hip']:.1f} | "
                        + " | ".join(f"{k[n]:.1f}" if n in k else "not measured" for n in KERNELS)
                        + f" | {r['max_abs_db_hip_minus_torch']:.1e} |\n")
            f.write("\nKernel columns: medians of the kernel trace of a separate `--calls-only` run.\n")


if __name__ == "__main__":
    main()
