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
"""
import argparse
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


def main_vocoder(a, dev):
    results = []
    for dec in a.decoder:
        for dt in a.dtypes:
            for B in a.batches:
                for chunk in a.chunks:
                    r = run_vocoder_config(dec, getattr(torch, dt), B, chunk, a.hops, a.warmup, a.rate, dev)
                    results.append(r)
                    print(json.dumps(r), flush=True)
    lines = ["| decoder | dtype | B | frames | path | host ms med (p5-p95) | RTF host | GPU ms med (p5-p95) | RTF GPU |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for path in ("module", "eager", "replay"):
            h, g = r["paths"][path]["rx_host"], r["paths"][path]["rx_gpu"]
            lines.append(f"| {r['decoder']} | {r['dtype']} | {r['B']} | {r['frames']} | {path} | "
                         f"{h['med']:.3f} ({h['p5']:.3f}-{h['p95']:.3f}) | {h['rtf']:.1f} | "
                         f"{g['med']:.3f} ({g['p5']:.3f}-{g['p95']:.3f}) | {g['rtf']:.1f} |")
        if r["B"] == 1 and r["frames"] == 1:
            m, s = r["paths"]["module"]["rx_host"], r["paths"]["replay"]["rx_host"]
            gain = m["med"] - s["med"]
            spread = max(m["p95"] - m["p5"], s["p95"] - s["p5"])
            verdicts.append(f"acceptance {r['decoder']} {r['dtype']} B=1 frames=1 rx: module {m['med']:.3f} ms - replay "
                            f"{s['med']:.3f} ms = {gain:.3f} ms vs 5-95% band {spread:.3f} ms: "
                            f"{'MET' if gain > spread else 'NOT MET'}")
    out = a.out or os.path.join(REPO, "profiles", "stream_bench_vocoder")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out + ".json", "w") as f:
        json.dump(results, f, indent=1)
    with open(out + ".md", "w") as f:
        f.write("\n".join(lines + [""] + verdicts) + "\n")
    print("\n".join(lines + verdicts))


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_bench: needs the GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    if a.decoder != ["audiodec"]:
        if "audiodec" in a.decoder:
            sys.exit("stream_bench: --decoder audiodec cannot be combined with a vocoder")
        return main_vocoder(a, dev)
    a.out = a.out or os.path.join(REPO, "profiles", "stream_bench")
    results = []
    for dt in a.dtypes:
        for B in a.batches:
            for chunk in a.chunks:
                r = run_config(getattr(torch, dt), B, chunk, a.hops, a.warmup, a.rate, dev)
                results.append(r)
                print(json.dumps(r), flush=True)
    lines = ["| dtype | B | chunk | half | path | host ms med (p5-p95) | RTF host | GPU ms med (p5-p95) | RTF GPU |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in results:
        for half in ("tx", "rx"):
            for path in ("module", "eager", "replay"):
                h, g = r["paths"][path][half + "_host"], r["paths"][path][half + "_gpu"]
                lines.append(f"| {r['dtype']} | {r['B']} | {r['chunk']} | {half} | {path} | "
                             f"{h['med']:.3f} ({h['p5']:.3f}-{h['p95']:.3f}) | {h['rtf']:.1f} | "
                             f"{g['med']:.3f} ({g['p5']:.3f}-{g['p95']:.3f}) | {g['rtf']:.1f} |")
            if r["B"] == 1 and r["chunk"] == 300:
                m, s = r["paths"]["module"][half + "_host"], r["paths"]["replay"][half + "_host"]
                gain = m["med"] - s["med"]
                spread = max(m["p95"] - m["p5"], s["p95"] - s["p5"])
                verdicts.append(f"acceptance {r['dtype']} B=1 chunk=300 {half}: module {m['med']:.3f} ms - replay "
                                f"{s['med']:.3f} ms = {gain:.3f} ms vs 5-95% band {spread:.3f} ms: "
                                f"{'MET' if gain > spread else 'NOT MET'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(results, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("\n".join(lines + [""] + verdicts) + "\n")
    print("\n".join(lines + verdicts))


if __name__ == "__main__":
    main()
