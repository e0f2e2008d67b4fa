#!/usr/bin/env python3
"""Per-hop latency of the streaming codec: module path vs StreamSession.

For every (dtype, B, chunk) the three paths run ALTERNATING in one process on
the same full-width generator and the same input chunk:

  module  StreamGenerator.encode -> quantize / lookup -> decode (*.inference)
  eager   sel.streaming.StreamSession(graph=False)
  replay  sel.streaming.StreamSession(graph=True)

Each hop times the transmitter half (encode + quantize) and the receiver half
(lookup + decode) twice over: host wall time from the call to a stream
synchronise (what a caller waits for) and HIP-event time on the stream.  After
the warm-up hops it reports median and 5th / 95th percentile over --hops hops and
the real-time factor chunk duration / median latency at --rate Hz.  The
acceptance line compares replay with module at B = 1, chunk 300.

  python tools/stream_bench.py --out profiles/stream_bench
writes <out>.json (every figure) and <out>.md (the table of DESIGN §13).

  python tools/stream_bench.py --decoder v1 v0
measures the receiver half (lookup + decode) with the full-width HiFi-GAN
vocoder decoders instead -- module path (StreamGenerator.decode), eager
sel.streaming.VocoderSession, graph replay, same protocol -- and writes
profiles/stream_bench_vocoder.{json,md} (the table of DESIGN §14); its
acceptance line compares replay with module at B = 1, one frame.

  python tools/stream_bench.py --pool
measures what N independent streams cost per tick (default N = 16, chunk 300;
the transmitter half and the v1 vocoder receiver half), four paths alternating
in one process, same protocol:

  solo      N batch=1 graph sessions stepped one after the other
  lockstep  one batch=N graph session (streams that cannot start or stop alone)
  pool      sel.streaming.StreamPool / VocoderPool, N of N slots active
  pool_k    the same pool with --active (default 4) of N slots active

and writes profiles/stream_pool_bench.{json,md} (the table of DESIGN §15); its
acceptance line compares pool with solo.

  python tools/stream_bench.py --pool --attribution
splits the pool's extra time over the lockstep session (all N slots active)
into its parts, same protocol: the two graphs replayed alone, the same graphs
captured without their commit / copy_slots launch, and the full calls (input
fill + replay, and for the pool the staging of the slot list); writes
profiles/stream_pool_attribution.{json,md} (the second table of DESIGN §15.3).

  python tools/stream_bench.py --codes
measures what the code indices inside the hop graphs save (enable_codes), same
protocol, the paths alternating in one process on separate objects:

  (a)  encode replay + quantize          against  (b)  transmit
  (a') lookup + decode replay            against  (b') receive

at B = 1 and B = --streams in a session and on a pool with all --streams slots
active, chunk 300, with the AudioDec decoder and the v1 vocoder on the receiver,
and writes profiles/stream_codes_bench.{json,md} (the table of DESIGN §16).
Acceptance: at B = 1 the transmitter's (b) must be faster than (a) by more than
the wider 5-95 % band; every other row must be no slower by the same band.

  python tools/stream_bench.py --wire
measures what the packets of the wire format cost inside the hop
(enable_codes(wire=True)), same protocol and objects as --codes, the old path
being an enable_codes() object of the same kind:

  transmit  against  transmit_packets      receive  against  receive_packets

plus, recorded only, the transmitter's hop with the result brought to the host
(transmit + idx.cpu() against transmit_packets + .cpu()), and writes
profiles/stream_wire_bench.{json,md} (the table of DESIGN §17).  Acceptance:
every *_packets row no slower than the row beside it by the wider 5-95 % band.

  python tools/stream_bench.py --datagrams
measures datagrams (wire version 2, enable_codes(datagrams=True)), same protocol,
the old path being an enable_codes(wire=True) object of the same kind:

  transmit_packets  against  transmit_datagrams at s = S, and at s = 4, 2, 1
  receive_packets   against  receive_datagrams with nothing lost, and with every stream lost

and writes profiles/stream_dgram_bench.{json,md} (the table of DESIGN §20).
Acceptance: the two s = S comparisons no slower by the wider 5-95 % band; the
s < S rows are what a smaller stage budget saves.
"""
import argparse
import functools
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dl-speech-enhancement_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _timed(fn, stream):
    """(result, host ms to a stream sync, event ms)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    out = fn()
    e1.record(stream)
    stream.synchronize()
    t1 = time.perf_counter()
    return out, (t1 - t0) * 1e3, e0.elapsed_time(e1)


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(med=float(np.median(v)), p5=float(np.percentile(v, 5)), p95=float(np.percentile(v, 95)))


# ---- what the --pool / --codes / --wire / --datagrams measurements share ------------------------
def _models(dev, vocoder=False):
    """The full-width AudioDec generator (seed 93) and, on request, the v1 vocoder."""
    from models.autoencoder.AudioDec import StreamGenerator as Encoder
    torch.manual_seed(93)
    E = Encoder().to(dev).eval()
    E.quantizer.initial()
    if not vocoder:
        return E, None
    from models.vocoder.HiFiGAN import StreamGenerator as Vocoder
    from sel import configs
    return E, Vocoder(**configs.VOCODER_V1).to(dev).eval()


def _maker(G, kind, N, chunk, dtype, lookup=None):
    """-> make(codes=None): a graph object of generator G (AudioDec or vocoder), `kind`
    = "session" (batch N) or "pool" (capacity N), with `lookup` as its
    lookup_generator and, given a dict, enable_codes(**codes)."""
    from sel import streaming as ST
    vocoder = not hasattr(G, "quantizer")
    cls = {("session", False): ST.StreamSession, ("pool", False): ST.StreamPool,
           ("session", True): ST.VocoderSession, ("pool", True): ST.VocoderPool}[kind, vocoder]

    def make(codes=None):
        o = cls(G, N, chunk // 300 if vocoder else chunk, graph=True, dtype=dtype)
        if lookup is not None:
            o.lookup_generator = lookup
        if codes is not None:
            o.enable_codes(**codes)
        return o
    return make


def _open_all(objs, N):
    """Every slot of every pool among objs, in the same order -> the leading arguments of a tick"""
    lists = [[o.open() for _ in range(N)] for o in objs if hasattr(o, "table")]
    assert all(sl == lists[0] for sl in lists)
    return (lists[0],) if lists else ()


def _measure(paths, hops, warmup, dev):
    """{name: fn}, the paths running alternating hop by hop -> {name: {"host": stats, "gpu": stats}}"""
    stream = torch.cuda.current_stream(dev)
    rec = {p: dict(host=[], gpu=[]) for p in paths}
    for hop in range(warmup + hops):
        for p, fn in paths.items():
            _, h, g = _timed(fn, stream)
            if hop >= warmup:
                rec[p]["host"].append(h)
                rec[p]["gpu"].append(g)
    return {p: {k: _stats(v) for k, v in r.items()} for p, r in rec.items()}


def _pairs(paths, hops, warmup, dev):
    """{half: (old fn, new fn)} -> {half: {"old" / "new": {"host": stats, "gpu": stats}}}"""
    res = _measure({(h, p): fn for h, fns in paths.items() for p, fn in zip(("old", "new"), fns)}, hops, warmup, dev)
    return {h: {p: res[h, p] for p in ("old", "new")} for h in paths}


def _head(dtype, N, chunk, hops, **first):
    return dict(**first, dtype=str(dtype).replace("torch.", ""), streams=N, chunk=chunk, hops=hops)


def _sweep(a, configs, run):
    """run(dtype, *config) for every --dtypes entry and config, each result printed as it comes"""
    results = []
    for dt in a.dtypes:
        for cfg in configs:
            results.append(run(getattr(torch, dt), *cfg))
            print(json.dumps(results[-1]), flush=True)
    return results


def _kinds(a):
    return (("session", 1), ("session", a.streams), ("pool", a.streams))


def _cell(s):
    return f"{s['med']:.3f} ({s['p5']:.3f}-{s['p95']:.3f})"


def _object(r):
    return f"{r['kind']} B={r['streams']}" if r["kind"] == "session" else f"pool {r['streams']} of {r['streams']}"


def _verdict(o, n, faster=False, names=("old", "new")):
    """Host stats of two paths -> the acceptance arithmetic: the first minus the
    second against the wider 5-95 % band; `faster`: must win by more than the
    band, else: must be no slower by more than it."""
    gain = o["med"] - n["med"]
    spread = max(o["p95"] - o["p5"], n["p95"] - n["p5"])
    met = gain > spread if faster else gain >= -spread
    return (f"{names[0]} {o['med']:.3f} ms - {names[1]} {n['med']:.3f} ms = {gain:.3f} ms vs 5-95% band "
            f"{spread:.3f} ms: {'MET' if met else 'NOT MET'}")


def _write(out, default, results, lines, verdicts=None):
    """<out>.json (every figure) and <out>.md (the table, then the verdict lines)"""
    out = out or os.path.join(REPO, "profiles", default)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out + ".json", "w") as f:
        json.dump(results, f, indent=1)
    with open(out + ".md", "w") as f:
        f.write("\n".join(lines + ([""] + verdicts if verdicts is not None else [])) + "\n")
    print("\n".join(lines + (verdicts or [])))


def run_config(dtype, B, chunk, hops, warmup, rate, dev):
    from models.autoencoder.AudioDec import StreamGenerator
    from sel import convops as CO
    from sel.streaming import StreamSession
    torch.manual_seed(93)
    G = StreamGenerator().to(dev).eval()
    G.quantizer.initial()
    L = chunk // 300
    sessions = {"eager": StreamSession(G, B, chunk, graph=False, dtype=dtype),
                "replay": StreamSession(G, B, chunk, graph=True, dtype=dtype)}
    x = 0.1 * torch.randn(B, 1, chunk, generator=torch.Generator().manual_seed(1)).to(dev)
    stream = torch.cuda.current_stream(dev)

    def tx(path):
        if path == "module":
            with CO.precision(dtype):
                return G.quantize(G.encode(x))
        S = sessions[path]
        return S.quantize(S.encode(x))

    def rx(path, idx):
        if path == "module":
            with CO.precision(dtype):
                return G.decode(G.lookup(idx).view(B, L, -1))
        S = sessions[path]
        return S.decode(S.lookup(idx))

    rec = {p: dict(tx_host=[], tx_gpu=[], rx_host=[], rx_gpu=[]) for p in ("module", "eager", "replay")}
    for hop in range(warmup + hops):
        for path in rec:
            idx, h, g = _timed(lambda: tx(path), stream)
            if hop >= warmup:
                rec[path]["tx_host"].append(h)
                rec[path]["tx_gpu"].append(g)
            _, h, g = _timed(lambda: rx(path, idx), stream)
            if hop >= warmup:
                rec[path]["rx_host"].append(h)
                rec[path]["rx_gpu"].append(g)
    dur_ms = chunk / rate * 1e3
    out = {}
    for path, r in rec.items():
        out[path] = {k: _stats(v) for k, v in r.items()}
        for k in r:
            out[path][k]["rtf"] = dur_ms / out[path][k]["med"]
    return dict(dtype=str(dtype).replace("torch.", ""), B=B, chunk=chunk, hops=hops, chunk_ms=dur_ms, paths=out)


def run_vocoder_config(decoder, dtype, B, chunk, hops, warmup, rate, dev):
    """The receiver half (lookup + decode) with a full-width HiFi-GAN vocoder
    decoder (sel.configs.VOCODER_V*): module path, eager VocoderSession and graph
    replay alternating, as run_config.  The codes come from the full-width
    AudioDec encoder once, outside the timed region."""
    from models.autoencoder.AudioDec import StreamGenerator as Encoder
    from models.vocoder.HiFiGAN import StreamGenerator as Vocoder
    from sel import configs
    from sel import convops as CO
    from sel.streaming import VocoderSession
    torch.manual_seed(93)
    E = Encoder().to(dev).eval()
    E.quantizer.initial()
    V = Vocoder(**getattr(configs, "VOCODER_" + decoder.upper())).to(dev).eval()
    L = chunk // 300
    x = 0.1 * torch.randn(B, 1, chunk, generator=torch.Generator().manual_seed(1)).to(dev)
    idx = E.quantize(E.encode(x))
    sessions = {"eager": VocoderSession(V, B, L, graph=False, dtype=dtype),
                "replay": VocoderSession(V, B, L, graph=True, dtype=dtype)}
    for S in sessions.values():
        S.lookup_generator = E
    stream = torch.cuda.current_stream(dev)

    def rx(path):
        if path == "module":
            with CO.precision(dtype):
                return V.decode(E.lookup(idx).view(B, L, -1))
        S = sessions[path]
        return S.decode(S.lookup(idx))

    rec = {p: dict(rx_host=[], rx_gpu=[]) for p in ("module", "eager", "replay")}
    for hop in range(warmup + hops):
        for path in rec:
            _, h, g = _timed(lambda: rx(path), stream)
            if hop >= warmup:
                rec[path]["rx_host"].append(h)
                rec[path]["rx_gpu"].append(g)
    dur_ms = chunk / rate * 1e3
    out = {}
    for path, r in rec.items():
        out[path] = {k: _stats(v) for k, v in r.items()}
        for k in r:
            out[path][k]["rtf"] = dur_ms / out[path][k]["med"]
    return dict(decoder=decoder, dtype=str(dtype).replace("torch.", ""), B=B, chunk=chunk, frames=L, hops=hops,
                chunk_ms=dur_ms, paths=out)


class _no_state_copy:
    """Inside the block a session's or a pool's launch list ends before its
    commit / copy_slots launch, so a graph captured there lacks that node.  For
    measurement only: such an object never advances its state."""

    def __enter__(self):
        from sel import streamops as SO
        self.keep = SO.commit, SO.copy_slots
        SO.commit = lambda pairs: None
        SO.copy_slots = lambda pairs, src_slots, dst_slots, n: None

    def __exit__(self, *exc):
        from sel import streamops as SO
        SO.commit, SO.copy_slots = self.keep


def _graph_half(obj, half):
    """The fixed-buffer launch list (sel.streaming._Half) of a session or pool:
    its run() replays the graph without filling the input or staging a list."""
    return obj._enc if half == "tx" else obj._dec


def run_pool_config(half, dtype, N, active, chunk, hops, warmup, dev):
    """One tick of N independent streams, `half` = "tx" (AudioDec encode +
    quantize) or "rx_v1" (lookup + v1 vocoder decode), at full width."""
    E, V = _models(dev, vocoder=half != "tx")
    x = 0.1 * torch.randn(N, 1, chunk, generator=torch.Generator().manual_seed(1)).to(dev)
    G = E if half == "tx" else V
    solo = [_maker(G, "session", 1, chunk, dtype, E)() for _ in range(N)]
    lock, pool = _maker(G, "session", N, chunk, dtype, E)(), _maker(G, "pool", N, chunk, dtype, E)()
    all_slots, = _open_all([pool], N)
    some_slots = all_slots[::N // active][:active]
    if half == "tx":
        xs, x_some = [x[i:i + 1].contiguous() for i in range(N)], x[some_slots].contiguous()
        paths = {"solo": lambda: [S.quantize(S.encode(xi)) for S, xi in zip(solo, xs)],
                 "lockstep": lambda: lock.quantize(lock.encode(x)),
                 "pool": lambda: pool.quantize(pool.encode(all_slots, x)),
                 "pool_k": lambda: pool.quantize(pool.encode(some_slots, x_some))}
    else:
        idx = E.quantize(E.encode(x))                   # (codebooks, N, frames)
        idxs, idx_some = [idx[:, i].contiguous() for i in range(N)], idx[:, some_slots].contiguous()
        paths = {"solo": lambda: [S.decode(S.lookup(i)) for S, i in zip(solo, idxs)],
                 "lockstep": lambda: lock.decode(lock.lookup(idx)),
                 "pool": lambda: pool.decode(all_slots, pool.lookup(idx)),
                 "pool_k": lambda: pool.decode(some_slots, pool.lookup(idx_some))}
    return dict(half=half, dtype=str(dtype).replace("torch.", ""), streams=N, active=active, chunk=chunk, hops=hops,
                paths=_measure(paths, hops, warmup, dev))


def run_attribution_config(half, dtype, N, chunk, hops, warmup, dev):
    """Where the pool's time over the lockstep session goes at N of N active
    (`half` as run_pool_config).  The inputs are fixed, so the replays alone
    compute the same hop every time."""
    E, V = _models(dev, vocoder=half != "tx")
    if half == "tx":
        inp = 0.1 * torch.randn(N, 1, chunk, generator=torch.Generator().manual_seed(1)).to(dev)
    else:
        inp = torch.randn(N, chunk // 300, 64, generator=torch.Generator().manual_seed(2)).to(dev)

    def build():
        return [_maker(E if half == "tx" else V, kind, N, chunk, dtype)() for kind in ("session", "pool")]

    def full(obj, *slots):
        return obj.encode(*slots, inp) if half == "tx" else obj.decode(*slots, inp)

    lock, pool = build()
    with _no_state_copy():
        lock0, pool0 = build()
    slots, = _open_all([pool, pool0], N)
    for p in (pool, pool0):
        full(p, slots)                  # leaves the full list staged for the bare replays
    hl, hl0, hp, hp0 = (_graph_half(o, half) for o in (lock, lock0, pool, pool0))
    paths = {"lock_replay_no_commit": hl0.run, "lock_replay": hl.run, "pool_replay_no_copy": hp0.run,
             "pool_replay": hp.run, "lock_full": lambda: full(lock), "pool_full": lambda: full(pool, slots)}
    return dict(_head(dtype, N, chunk, hops, half=half), paths=_measure(paths, hops, warmup, dev))


def main_attribution(a, dev):
    results = _sweep(a, (("tx",), ("rx_v1",)),
                     lambda dt, half: run_attribution_config(half, dt, a.streams, 300, a.hops, a.warmup, dev))
    label = {"lock_replay": "lockstep replay", "lock_replay_no_commit": "... without its commit launch",
             "pool_replay_no_copy": "pool replay without its copy launch", "pool_replay": "pool replay",
             "pool_full": "pool full call (staging, input fill, replay)", "lock_full": "lockstep full call"}
    lines = ["| step (host ms med) | " + " | ".join(f"{r['half']} {r['dtype']}" for r in results) + " |",
             "|---|" + "---|" * len(results)]
    for path, lab in label.items():
        lines.append(f"| {lab} | " + " | ".join(f"{r['paths'][path]['host']['med']:.3f}" for r in results) + " |")
    for r in results:
        m = {k: v["host"]["med"] for k, v in r["paths"].items()}
        # staging: what the pool's call adds to its replay beyond the input fill the lockstep call has too
        parts = dict(indirection=m["pool_replay_no_copy"] - m["lock_replay_no_commit"],
                     staging=(m["pool_full"] - m["pool_replay"]) - (m["lock_full"] - m["lock_replay"]),
                     copy=m["pool_replay"] - m["pool_replay_no_copy"],
                     commit=m["lock_replay"] - m["lock_replay_no_commit"])
        r["parts_host_ms"] = parts
        lines.append(f"{r['half']} {r['dtype']}: indirection {parts['indirection']:.3f} ms, staging "
                     f"{parts['staging']:.3f} ms, copy launch {parts['copy']:.3f} ms (commit {parts['commit']:.3f} ms)")
    _write(a.out, "stream_pool_attribution", results, lines)


def main_pool(a, dev):
    results = _sweep(a, (("tx",), ("rx_v1",)),
                     lambda dt, half: run_pool_config(half, dt, a.streams, a.active, 300, a.hops, a.warmup, dev))
    label = {"solo": "(a) {n} solo batch=1 sessions", "lockstep": "(b) lockstep batch={n} session",
             "pool": "(c) pool, {n} of {n} active", "pool_k": "(d) pool, {k} of {n} active"}
    lines = ["| half | dtype | path | host ms med (p5-p95) | GPU ms med (p5-p95) |", "|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for path, lab in label.items():
            lines.append(f"| {r['half']} | {r['dtype']} | {lab.format(n=r['streams'], k=r['active'])} | "
                         f"{_cell(r['paths'][path]['host'])} | {_cell(r['paths'][path]['gpu'])} |")
        pa = {k: v["host"] for k, v in r["paths"].items()}
        verdicts.append(f"acceptance {r['half']} {r['dtype']}: "
                        f"{_verdict(pa['solo'], pa['pool'], True, ('solo', 'pool'))}; (c)/(b) = "
                        f"{pa['pool']['med'] / pa['lockstep']['med']:.3f}, (d)/(c) = "
                        f"{pa['pool_k']['med'] / pa['pool']['med']:.3f}, (a)/(c) = "
                        f"{pa['solo']['med'] / pa['pool']['med']:.2f}")
    _write(a.out, "stream_pool_bench", results, lines, verdicts)


def _codec_objects(kind, dtype, N, chunk, dev, old, new, copies=1):
    """The models and inputs of --codes / --wire: per receiver ("ae": the AudioDec
    decoder, "v1": the vocoder) `copies` pairs of objects of `kind` with
    enable_codes(**old) (None: not enabled) and enable_codes(**new), all pools'
    slots open -> (objects by receiver, the leading arguments of a tick, x, idx
    as the objects' quantize returns it)"""
    E, V = _models(dev, vocoder=True)
    x = 0.1 * torch.randn(N, 1, chunk, generator=torch.Generator().manual_seed(1)).to(dev)
    idx = E.quantize(E.encode(x))
    objs = {name: [_maker(G, kind, N, chunk, dtype, E)(codes) for codes in (old, new) * copies]
            for name, G in (("ae", E), ("v1", V))}
    idx = idx.view(idx.shape[0], N, chunk // 300)
    return objs, _open_all(objs["ae"] + objs["v1"], N), x, idx.squeeze(1) if kind == "session" and N == 1 else idx


def run_codes_config(kind, dtype, N, chunk, hops, warmup, dev):
    """(a) / (b) of the transmitter and (a') / (b') of the receiver with the
    AudioDec decoder and with the v1 vocoder, `kind` = "session" (batch N) or
    "pool" (N of N slots active), at full width.  The old and the new path run
    on separate objects fed the same input, so each advances its own state."""
    objs, sl, x, idx = _codec_objects(kind, dtype, N, chunk, dev, None, {})
    (ae_old, ae_new), (v1_old, v1_new) = objs["ae"], objs["v1"]
    paths = {"tx": (lambda: ae_old.quantize(ae_old.encode(*sl, x)), lambda: ae_new.transmit(*sl, x)),
             "rx": (lambda: ae_old.decode(*sl, ae_old.lookup(idx)), lambda: ae_new.receive(*sl, idx)),
             "rx_v1": (lambda: v1_old.decode(*sl, v1_old.lookup(idx)), lambda: v1_new.receive(*sl, idx))}
    return dict(_head(dtype, N, chunk, hops, kind=kind), halves=_pairs(paths, hops, warmup, dev))


def _pair_table(results, label, faster=lambda r, half: False, recorded=()):
    """The table and the verdict lines of --codes / --wire: per object and half the old row, the new row"""
    lines = ["| dtype | object | half | path | host ms med (p5-p95) | GPU ms med (p5-p95) |",
             "|---|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for half, d in r["halves"].items():
            for p in ("old", "new"):
                lines.append(f"| {r['dtype']} | {_object(r)} | {half} | {label[half, p]} | {_cell(d[p]['host'])} | "
                             f"{_cell(d[p]['gpu'])} |")
            if half not in recorded:
                win = faster(r, half)                    # must win; the rest: no slower
                verdicts.append(f"acceptance {r['dtype']} {_object(r)} {half} ({'faster' if win else 'no slower'}): "
                                f"{_verdict(d['old']['host'], d['new']['host'], win)}")
    return lines, verdicts


def main_codes(a, dev):
    results = _sweep(a, _kinds(a), lambda dt, kind, N: run_codes_config(kind, dt, N, 300, a.hops, a.warmup, dev))
    label = {("tx", "old"): "(a) encode replay + quantize", ("tx", "new"): "(b) transmit",
             ("rx", "old"): "(a') lookup + decode replay", ("rx", "new"): "(b') receive",
             ("rx_v1", "old"): "(a') lookup + v1 decode replay", ("rx_v1", "new"): "(b') v1 receive"}
    lines, verdicts = _pair_table(results, label, lambda r, half: half == "tx" and r["kind"] == "session"
                                  and r["streams"] == 1)
    _write(a.out, "stream_codes_bench", results, lines, verdicts)


def run_wire_config(kind, dtype, N, chunk, hops, warmup, dev):
    """transmit / transmit_packets and receive / receive_packets (AudioDec decoder
    and v1 vocoder), `kind` = "session" (batch N) or "pool" (N of N slots
    active), at full width, old and new on separate objects as run_codes_config;
    tx_host is the transmitter's hop with its result copied to the host."""
    objs, sl, x, idx = _codec_objects(kind, dtype, N, chunk, dev, dict(wire=False), dict(wire=True), copies=2)
    ae_old, ae_new, ae_old_h, ae_new_h = objs["ae"]
    v1_old, v1_new = objs["v1"][:2]
    packets = ae_new.wire.pack(idx.cpu()).to(dev)
    paths = {"tx": (lambda: ae_old.transmit(*sl, x), lambda: ae_new.transmit_packets(*sl, x)),
             "rx": (lambda: ae_old.receive(*sl, idx), lambda: ae_new.receive_packets(*sl, packets)),
             "rx_v1": (lambda: v1_old.receive(*sl, idx), lambda: v1_new.receive_packets(*sl, packets)),
             "tx_host": (lambda: ae_old_h.transmit(*sl, x).cpu(), lambda: ae_new_h.transmit_packets(*sl, x).cpu())}
    w = ae_new.wire
    return dict(_head(dtype, N, chunk, hops, kind=kind),
                wire=dict(version=w.version, bits=w.bits, frame_bytes=w.frame_bytes, packet_bytes=w.packet_bytes,
                          index_bytes=8 * w.codebooks * w.frames),
                halves=_pairs(paths, hops, warmup, dev))


def main_wire(a, dev):
    results = _sweep(a, _kinds(a), lambda dt, kind, N: run_wire_config(kind, dt, N, 300, a.hops, a.warmup, dev))
    label = {("tx", "old"): "transmit", ("tx", "new"): "transmit_packets",
             ("rx", "old"): "receive", ("rx", "new"): "receive_packets",
             ("rx_v1", "old"): "v1 receive", ("rx_v1", "new"): "v1 receive_packets",
             ("tx_host", "old"): "transmit + idx.cpu() (recorded only)",
             ("tx_host", "new"): "transmit_packets + .cpu() (recorded only)"}
    lines, verdicts = _pair_table(results, label, recorded=("tx_host",))
    w = results[0]["wire"]
    verdicts.append(f"wire v{w['version']}: {w['bits']} bits per field, {w['frame_bytes']} bytes per frame against "
                    f"{w['index_bytes']} bytes of int64 indices")
    _write(a.out, "stream_wire_bench", results, lines, verdicts)


def run_dgram_config(kind, dtype, N, chunk, hops, warmup, dev):
    """transmit_packets (the old path: an enable_codes(wire=True) object) against
    transmit_datagrams at every stage budget in BUDGETS, receive_packets against
    receive_datagrams with nothing lost, and a tick with every stream lost;
    `kind` = "session" (batch N) or "pool" (N of N slots active), full width,
    separate objects, the paths alternating hop by hop."""
    E, _ = _models(dev)
    x = 0.1 * torch.randn(N, 1, chunk, generator=torch.Generator().manual_seed(1)).to(dev)
    make = _maker(E, kind, N, chunk, dtype)
    S = len(E.quantizer.codebook.layers)
    budgets = [S] + [b for b in (4, 2, 1) if b < S]
    tx_old, rx_old = make(dict(wire=True)), make(dict(wire=True))
    rx_new, rx_lost = make(dict(datagrams=True)), make(dict(datagrams=True))
    tx_new = {b: make(dict(datagrams=True)) for b in budgets}
    sl = _open_all([tx_old, rx_old, rx_new, rx_lost] + list(tx_new.values()), N)
    packets = tx_old.transmit_packets(*sl, x).clone()
    dgrams = tx_new[S].transmit_datagrams(*sl, x).clone()
    gone = [1] * N
    paths = {"tx": lambda: tx_old.transmit_packets(*sl, x), "rx": lambda: rx_old.receive_packets(*sl, packets),
             "rx_dgram": lambda: rx_new.receive_datagrams(*sl, dgrams),
             "rx_all_lost": lambda: rx_lost.receive_datagrams(*sl, dgrams, gone)}
    for b in budgets:
        paths[f"tx_dgram_s{b}"] = functools.partial(lambda o, b: o.transmit_datagrams(*sl, x, b), tx_new[b], b)
    f = rx_new.datagram
    return dict(_head(dtype, N, chunk, hops, kind=kind), budgets=budgets,
                datagram=dict(version=f.version, bits=f.bits, stride=f.stride,
                              bytes={b: f.datagram_bytes(b) for b in budgets},
                              kbit_per_s={b: f.bitrate(48000, chunk, b) / 1e3 for b in budgets}),
                paths=_measure(paths, hops, warmup, dev))


def main_dgram(a, dev):
    results = _sweep(a, _kinds(a), lambda dt, kind, N: run_dgram_config(kind, dt, N, 300, a.hops, a.warmup, dev))
    S = results[0]["budgets"][0]
    order = ["tx"] + [f"tx_dgram_s{b}" for b in results[0]["budgets"]] + ["rx", "rx_dgram", "rx_all_lost"]
    label = {"tx": "transmit_packets", "rx": "receive_packets", "rx_dgram": "receive_datagrams, none lost",
             "rx_all_lost": "receive_datagrams, all lost"}
    label.update({f"tx_dgram_s{b}": f"transmit_datagrams s = {b}" for b in results[0]["budgets"]})
    lines = ["| dtype | object | path | host ms med (p5-p95) | GPU ms med (p5-p95) |", "|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for p in order:
            lines.append(f"| {r['dtype']} | {_object(r)} | {label[p]} | {_cell(r['paths'][p]['host'])} | "
                         f"{_cell(r['paths'][p]['gpu'])} |")
        for old, new in (("tx", f"tx_dgram_s{S}"), ("rx", "rx_dgram")):
            verdicts.append(f"acceptance {r['dtype']} {_object(r)} {label[new]} against {label[old]} (no slower): "
                            f"{_verdict(r['paths'][old]['host'], r['paths'][new]['host'])}")
    d = results[0]["datagram"]
    verdicts.append(f"datagram v{d['version']}: {d['bits']} bits per field, bytes per hop by budget {d['bytes']}, "
                    f"kbit/s at chunk 300 with the header {d['kbit_per_s']}")
    _write(a.out, "stream_dgram_bench", results, lines, verdicts)


def _rtf_row(first, path, h, g):
    return (f"| {first} | {path} | {_cell(h)} | {h['rtf']:.1f} | {_cell(g)} | {g['rtf']:.1f} |")


def main_vocoder(a, dev):
    results = []
    for dec in a.decoder:
        results += _sweep(a, [(B, chunk) for B in a.batches for chunk in a.chunks], lambda dt, B, chunk:
                          run_vocoder_config(dec, dt, B, chunk, a.hops, a.warmup, a.rate, dev))
    lines = ["| decoder | dtype | B | frames | path | host ms med (p5-p95) | RTF host | GPU ms med (p5-p95) | RTF GPU |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for path in ("module", "eager", "replay"):
            lines.append(_rtf_row(f"{r['decoder']} | {r['dtype']} | {r['B']} | {r['frames']}", path,
                                  r["paths"][path]["rx_host"], r["paths"][path]["rx_gpu"]))
        if r["B"] == 1 and r["frames"] == 1:
            verdicts.append(f"acceptance {r['decoder']} {r['dtype']} B=1 frames=1 rx: " +
                            _verdict(r["paths"]["module"]["rx_host"], r["paths"]["replay"]["rx_host"], True,
                                     ("module", "replay")))
    _write(a.out, "stream_bench_vocoder", results, lines, verdicts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--chunks", type=int, nargs="+", default=[300, 1200])
    ap.add_argument("--dtypes", nargs="+", default=["bfloat16", "float32"])
    ap.add_argument("--decoder", nargs="+", choices=["audiodec", "v0", "v1", "v2"], default=["audiodec"],
                    help="the receiver's decoder: the AudioDec generator (both halves, the default), or one or more "
                         "HiFi-GAN vocoders at full width (receiver half only; profiles/stream_bench_vocoder)")
    ap.add_argument("--pool", action="store_true",
                    help="independent streams: solo sessions, the lockstep session and the stream pool "
                         "(profiles/stream_pool_bench)")
    ap.add_argument("--streams", type=int, default=16, help="--pool: streams / pool capacity")
    ap.add_argument("--active", type=int, default=4, help="--pool: active slots of the partly filled tick")
    ap.add_argument("--attribution", action="store_true",
                    help="with --pool: where the pool's time over the lockstep session goes "
                         "(profiles/stream_pool_attribution)")
    ap.add_argument("--codes", action="store_true",
                    help="quantize / lookup inside the hop graphs: encode + quantize against transmit, lookup + "
                         "decode against receive (profiles/stream_codes_bench)")
    ap.add_argument("--wire", action="store_true",
                    help="the packets of the wire format inside the hop graphs: transmit against transmit_packets, "
                         "receive against receive_packets (profiles/stream_wire_bench)")
    ap.add_argument("--datagrams", action="store_true",
                    help="datagrams inside the hop graphs: transmit_packets against transmit_datagrams at stage "
                         "budgets S, 4, 2, 1, receive_packets against receive_datagrams, and a tick with every "
                         "stream lost (profiles/stream_dgram_bench)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_bench: needs the GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    if a.attribution and not a.pool:
        sys.exit("stream_bench: --attribution goes with --pool")
    if a.codes:
        return main_codes(a, dev)
    if a.wire:
        return main_wire(a, dev)
    if a.datagrams:
        return main_dgram(a, dev)
    if a.pool:
        return main_attribution(a, dev) if a.attribution else main_pool(a, dev)
    if a.decoder != ["audiodec"]:
        if "audiodec" in a.decoder:
            sys.exit("stream_bench: --decoder audiodec cannot be combined with a vocoder")
        return main_vocoder(a, dev)
    results = _sweep(a, [(B, chunk) for B in a.batches for chunk in a.chunks],
                     lambda dt, B, chunk: run_config(dt, B, chunk, a.hops, a.warmup, a.rate, dev))
    lines = ["| dtype | B | chunk | half | path | host ms med (p5-p95) | RTF host | GPU ms med (p5-p95) | RTF GPU |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for half in ("tx", "rx"):
            for path in ("module", "eager", "replay"):
                lines.append(_rtf_row(f"{r['dtype']} | {r['B']} | {r['chunk']} | {half}", path,
                                      r["paths"][path][half + "_host"], r["paths"][path][half + "_gpu"]))
            if r["B"] == 1 and r["chunk"] == 300:
                verdicts.append(f"acceptance {r['dtype']} B=1 chunk=300 {half}: " +
                                _verdict(r["paths"]["module"][half + "_host"], r["paths"]["replay"][half + "_host"],
                                         True, ("module", "replay")))
    _write(a.out, "stream_bench", results, lines, verdicts)


if __name__ == "__main__":
    main()
