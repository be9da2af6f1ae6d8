"""Clustering a gallery on the device (fh_gallery_cluster_dev) measured on clustered rows: --rows x 512, --templates templates per identity
(centre + 0.02 noise, shuffled: the generator of gallery_fuse_ab.py), thr 0.8, one process.
  (a) the call at min_pts 1 (init + link pass + flatten) and at min_pts 4 (+ the degree pass), HIP events around each call after a warm-up
      call; with 8 templates per identity every row is core at min_pts 4, so the two calls run the SAME link pass and their difference is
      the degree pass alone; the link pass's atomics = the min_pts 1 call against that degree pass.  Executed FLOP of one pair pass =
      live (A tile, B tile) pairs x 128 x 64 x dim x 2.
  (b) the yardstick (--yardstick): the untouched fp32 scan asked the same question the only way it can — all rows as queries through
      topk_dev, 256 per call, k = 16 — one sweep, HIP events around the whole loop.  This leg uses only calls that existed before
      fh_gallery_cluster_dev, so `--yardstick --no-cluster` runs on an older checkout unchanged.
One JSON line per point; --md FILE writes the table."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[65536, 262144])
ap.add_argument("--templates", type=int, default=8)
ap.add_argument("--thr", type=float, default=0.8)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--yardstick", action="store_true")
ap.add_argument("--no-cluster", action="store_true")
ap.add_argument("--md", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402

DIM = 512


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "samples": len(v)}


def timed(call, n):
    call(); torch.cuda.synchronize()                           # warm-up: buffers sized, code loaded
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def pair_pass_flop(G):
    tiles_n, row_tiles = (G + 63) // 64, (G + 127) // 128
    pairs = sum(min(row_tiles, (bt * 64 + 62) // 128 + 1) for bt in range(tiles_n))
    return pairs * 128 * 64 * DIM * 2


def main():
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for G in a.rows:
        gen = torch.Generator(device="cuda").manual_seed(11)
        T = a.templates
        m = G // T
        centres = unit(torch.randn((m, DIM), device="cuda", generator=gen))
        rows = unit(centres.repeat_interleave(T, 0) + 0.02 * torch.randn((m * T, DIM), device="cuda", generator=gen))
        rows = rows[torch.randperm(m * T, device="cuda", generator=gen)].contiguous()
        G = m * T
        g = fa.Gallery(DIM)
        g.upload(rows.data_ptr(), G, True, 0)
        d = {"what": "cluster", "rows": G, "dim": DIM, "templates": T, "thr": a.thr}
        if not a.no_cluster:
            labels = torch.zeros(G, dtype=torch.int32, device="cuda"); info = torch.zeros(4, dtype=torch.int32, device="cuda")
            t1 = timed(lambda: g.cluster_dev(a.thr, 1, "none", labels.data_ptr(), info.data_ptr(), st), a.calls)
            i1 = info.cpu().tolist()
            t4 = timed(lambda: g.cluster_dev(a.thr, 4, "none", labels.data_ptr(), info.data_ptr(), st), a.calls)
            i4 = info.cpu().tolist()
            flop = pair_pass_flop(G)
            link, both = statistics.median(t1), statistics.median(t4)
            d.update({"call_min_pts_1": stats(t1), "call_min_pts_4": stats(t4), "info_min_pts_1": i1, "info_min_pts_4": i4,
                      "degree_pass_ms": round(both - link, 3), "link_pass_and_small_kernels_ms": round(link, 3),
                      "pair_pass_flop": flop, "degree_pass_TFLOPs": round(flop / max(both - link, 1e-6) / 1e9, 1),
                      "link_pass_TFLOPs": round(flop / link / 1e9, 1), "link_over_degree": round(link / max(both - link, 1e-6), 3)})
        if a.yardstick:
            k, Q = 16, 256
            sc = torch.zeros((Q, k), device="cuda"); ix = torch.zeros((Q, k), dtype=torch.int32, device="cuda")

            def sweep():
                for q0 in range(0, G, Q):
                    g.topk_dev(rows.data_ptr() + q0 * DIM * 4, min(Q, G - q0), k, sc.data_ptr(), ix.data_ptr(), st)

            g.topk_dev(rows.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); sweep(); e1.record(); e1.synchronize()
            d["topk_sweep_ms"] = round(e0.elapsed_time(e1), 3)
            d["topk_sweep_calls"] = (G + Q - 1) // Q
            if "call_min_pts_1" in d:
                d["sweep_over_call_min_pts_1"] = round(d["topk_sweep_ms"] / d["call_min_pts_1"]["median_ms"], 3)
                d["sweep_over_call_min_pts_4"] = round(d["topk_sweep_ms"] / d["call_min_pts_4"]["median_ms"], 3)
        print(json.dumps(d), flush=True)
        out.append(d)
    if a.md:
        with open(a.md, "w") as fo:
            fo.write("| rows | call, min_pts 1 ms | call, min_pts 4 ms | degree pass ms (TFLOP/s) | link pass + small kernels ms (TFLOP/s) | link / degree | "
                     "top-k sweep ms | sweep / call (min_pts 1, 4) | clusters, core, border, noise (min_pts 4) |\n|---|---|---|---|---|---|---|---|---|\n")
            for d in out:
                c1, c4 = d.get("call_min_pts_1"), d.get("call_min_pts_4")
                fo.write(f"| {d['rows']} | " + (f"{c1['median_ms']:.2f} ({c1['min_ms']:.2f}-{c1['max_ms']:.2f}) | {c4['median_ms']:.2f} ({c4['min_ms']:.2f}-{c4['max_ms']:.2f}) | "
                                                f"{d['degree_pass_ms']:.2f} ({d['degree_pass_TFLOPs']}) | {d['link_pass_and_small_kernels_ms']:.2f} ({d['link_pass_TFLOPs']}) | "
                                                f"{d['link_over_degree']} | " if c1 else "not measured | not measured | not measured | not measured | not measured | ")
                         + (f"{d['topk_sweep_ms']:.1f} | " if "topk_sweep_ms" in d else "not measured | ")
                         + (f"{d['sweep_over_call_min_pts_1']}, {d['sweep_over_call_min_pts_4']} | " if "sweep_over_call_min_pts_1" in d else "not measured | ")
                         + (f"{d['info_min_pts_4']} |\n" if c1 else "not measured |\n"))


if __name__ == "__main__":
    main()
