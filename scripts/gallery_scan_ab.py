"""Interleaved A/B of the gallery's scan modes (fh_gallery_set_scan): FP32 vs F16_RERANK on the same rows, one process, the two
modes alternated point by point.  Rows: random unit vectors x 512 (1 M and 1.25 M = one rank's shard of a 10 M gallery over 8),
queries random unit vectors, Q = 64 / 256, k = 1 / 16.  Per point: warm-up, then HIP-event timing of back-to-back calls for
>= --seconds per mode and round; reports median / min / max ms per call and the certified share of the f16 calls.
Prints one JSON line per point and, with --md, a markdown table."""
import argparse
import json
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402


def unit(n, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, dim), device="cuda", generator=g)
    return x / x.norm(dim=1, keepdim=True)


def time_calls(g, q, k, sc, ix, seconds):
    Q = q.shape[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    total = 0.0
    while total < seconds * 1e3 or len(per) < 5:
        e0.record()
        for _ in range(10):
            g.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), torch.cuda.current_stream().cuda_stream)
        e1.record(); e1.synchronize()
        ms = e0.elapsed_time(e1)
        per.append(ms / 10); total += ms
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1310720])
    ap.add_argument("--q", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []
    for G in a.rows:
        rows = unit(G, 512, G)
        g32, g16 = fa.Gallery(512), fa.Gallery(512, scan="f16")
        for g in (g32, g16):
            g.upload(rows.data_ptr(), G, True, 0)
        for Q in a.q:
            q = unit(Q, 512, G + Q)
            for k in a.k:
                sc = torch.zeros((Q, k), device="cuda"); ix = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
                res = {"fp32": [], "f16": []}
                for g in (g32, g16):                          # warm-up (buffers sized, clocks up)
                    time_calls(g, q, k, sc, ix, 0.1)
                g16.scan_stats()
                for _ in range(a.rounds):                     # alternated
                    res["fp32"] += time_calls(g32, q, k, sc, ix, a.seconds)
                    res["f16"] += time_calls(g16, q, k, sc, ix, a.seconds)
                c, f = g16.scan_stats()
                d = {"rows": G, "Q": Q, "k": k}
                for m, v in res.items():
                    d[m] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}
                d["certified_pct"] = round(100.0 * c / max(c + f, 1), 2)
                d["speedup"] = round(d["fp32"]["median_ms"] / d["f16"]["median_ms"], 3)
                print(json.dumps(d), flush=True)
                lines.append(d)
        del g32, g16, rows
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, "w") as fo:
            fo.write("| rows | Q | k | FP32 median (min-max) ms | F16_RERANK median (min-max) ms | speed-up | certified |\n|---|---|---|---|---|---|---|\n")
            for d in lines:
                f32, f16 = d["fp32"], d["f16"]
                fo.write(f"| {d['rows']} | {d['Q']} | {d['k']} | {f32['median_ms']:.3f} ({f32['min_ms']:.3f}-{f32['max_ms']:.3f}) | "
                         f"{f16['median_ms']:.3f} ({f16['min_ms']:.3f}-{f16['max_ms']:.3f}) | {d['speedup']:.2f}x | {d['certified_pct']}% |\n")


if __name__ == "__main__":
    main()
