"""Training-mode ResidualVQ forward timing (not the flagship bench.py).  GPU only.

One training-mode ``ResidualVQ.forward`` -- assignment plus EMA codebook update
-- at S = 8, K = 1024, D = 64 (config symAD_vctk_48000_hop300) for N = 512 rows
(the recipe: 16 x 9600 samples) and N = 5120 (the flagship's row count):

* ``fused``  the product path: the all-stage assignment kernel, then one
  sel_rvq_ema_update for all stages (csrc/vq_ema.hip);
* ``torch``  the path it replaced, restated here: a Python loop over the
  stages, per stage a 1-stage assignment kernel, then bincount / index_add_ /
  the elementwise EMA sequence, an mse_loss and the straight-through output.

The two are alternated in one call, timed by device events after warm-up over
windows of at least 0.5 s per variant.  Both start from the same codebooks and
see the same rows on every call (the codebooks drift with the calls, for both
alike).  Writes JSON (default profiles/vq_train_bench.json).

  python tools/vq_train_bench.py [--out PATH]

``--sync`` measures the data-parallel codebook update instead (csrc/vq_ema_sync.hip,
``ResidualVQ.enable_ema_sync``), in one process and without a process group:

* ``fused``  as above;
* ``sync1``  statistics + apply with one segment (what each rank of a process
  group runs on its own rows, without the gather);
* ``sync8``  statistics in 8 segments + apply of the 8 blocks (what the apply
  costs on the gathered blocks of 8 ranks; the statistics of one rank's 1/8).

Same alternation, events and windows; also records the bytes a step gathers,
W x S x (D + 1) x K x 4.  Writes profiles/vq_sync_bench.json by default.

``--trace VARIANT --rows N`` runs 3 + 10 calls of one variant and nothing else:
for a kernel trace from outside (launches per call = kernel calls / 13).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dl-speech-enhancement_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from layers.vq_module import ResidualVQ  # noqa: E402
from sel.vqops import ResidualVQFn  # noqa: E402

S, K, D = 8, 1024, 64
ROWS = (512, 5120)


def torch_layer(layer, input):
    """one VectorQuantize training forward as it was before the fused update"""
    flatten = input.reshape(-1, layer.dim)
    out, _, ppl, idx = ResidualVQFn.apply(flatten.detach(), layer.embed.unsqueeze(0), layer.commitment)
    with torch.no_grad():
        ind, fl = idx[0], flatten.detach().float()
        onehot_sum = torch.bincount(ind, minlength=layer.n_embed).to(fl.dtype)
        layer.cluster_size.mul_(layer.decay).add_(onehot_sum, alpha=1 - layer.decay)
        embed_sum = torch.zeros_like(layer.embed_avg).index_add_(1, ind, fl.t())
        layer.embed_avg.mul_(layer.decay).add_(embed_sum, alpha=1 - layer.decay)
        n = layer.cluster_size.sum()
        cs = (layer.cluster_size + layer.eps) / (n + layer.n_embed * layer.eps) * n
        layer.embed.copy_(layer.embed_avg / cs.unsqueeze(0))
    q = out.view_as(input)
    loss = F.mse_loss(q.detach(), input) * layer.commitment
    return input + (q - input).detach(), loss, ppl[0]


def torch_forward(rvq, x):
    out, residual, losses, ppls = 0.0, x, [], []
    for layer in rvq.layers:
        q, l_, p_ = torch_layer(layer, residual)
        residual = residual - q
        out = out + q
        losses.append(l_)
        ppls.append(p_)
    return out, torch.stack(losses), torch.stack(ppls)


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


SYNC_SEGMENTS = {"sync1": 1, "sync8": 8}


def variants(n, dev, sync=False):
    gen = torch.Generator().manual_seed(n)
    torch.manual_seed(0)
    base = ResidualVQ(num_quantizers=S, dim=D, codebook_size=K)
    x = (1.5 * torch.randn(n, D, generator=gen)).to(dev)
    mods = {}
    for name in ("fused",) + (tuple(SYNC_SEGMENTS) if sync else ("torch",)):
        m = ResidualVQ(num_quantizers=S, dim=D, codebook_size=K)
        m.load_state_dict(base.state_dict())
        if name in SYNC_SEGMENTS:
            m.enable_ema_sync(segments=SYNC_SEGMENTS[name])
        mods[name] = m.to(dev).train()
    if sync:
        return {name: (lambda m=m: m(x)) for name, m in mods.items()}
    return {"fused": lambda: mods["fused"](x), "torch": lambda: torch_forward(mods["torch"], x)}


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sync", action="store_true", help="fused against statistics + apply (1 and 8 segments)")
    ap.add_argument("--trace", choices=("fused", "torch") + tuple(SYNC_SEGMENTS))
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()
    a.sync = a.sync or a.trace in SYNC_SEGMENTS
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "vq_sync_bench.json" if a.sync else "vq_train_bench.json")
    dev = torch.device("cuda:0")
    if a.trace:
        fn = no_grad(variants(a.rows, dev, a.sync)[a.trace])
        for _ in range(13):
            fn()
        torch.cuda.synchronize()
        print(f"traced 13 calls of {a.trace} at N = {a.rows}")
        return
    res = dict(run=dict(tool="tools/vq_train_bench.py", date=time.strftime("%Y-%m-%d"),
                        device=torch.cuda.get_device_name(0), stages=S, codes=K, dim=D,
                        window_seconds=a.seconds), rows={})
    if a.sync:
        res["run"]["gathered_bytes_per_step"] = {f"W={w}": w * S * (D + 1) * K * 4 for w in (1, 2, 8)}
    for n in ROWS:
        fns = {k: no_grad(f) for k, f in variants(n, dev, a.sync).items()}
        acc = {k: [] for k in fns}
        for _ in range(3):                       # alternated, round by round
            for k, fn in fns.items():
                acc[k].append(event_loop(fn, a.seconds)[0])
        mean = {k: sum(v) / len(v) for k, v in acc.items()}
        if a.sync:
            row = {f"{k}_ms": round(v, 4) for k, v in mean.items()}
            row.update({f"{k}_over_fused": round(mean[k] / mean["fused"], 3) for k in SYNC_SEGMENTS})
        else:
            row = dict(fused_ms=round(mean["fused"], 4), torch_ms=round(mean["torch"], 4),
                       speedup=round(mean["torch"] / mean["fused"], 2))
        res["rows"][str(n)] = dict(row, runs={k: [round(t, 4) for t in v] for k, v in acc.items()})
        print(n, res["rows"][str(n)], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
