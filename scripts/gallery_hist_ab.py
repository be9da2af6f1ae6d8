"""Genuine / impostor pair histograms of a gallery on the device (fh_gallery_pair_hist_dev) measured on clustered rows: --rows x 512,
--templates templates per identity (centre + 0.02 noise, shuffled: the generator of gallery_cluster_ab.py), one process, HIP events
around each call after a warm-up call, median of --calls.
  (a) the yardstick: the clustering link pass, fh_gallery_cluster_dev at min_pts 1 (init + link pass + flatten) — the same multiply work
      with another epilogue.  `--link-only` uses only calls that existed before fh_gallery_pair_hist_dev, so it runs on an older
      checkout unchanged.
  (b) the histogram call, once per arrangement: --copies privatised copies the workgroups flush into (0 = the library's default; 1 = a
      flush straight into one array) x --tiles A tiles per workgroup run (0 = the automatic choice).  Every arrangement must return the
      same histogram (integer, order-independent) and the two sum invariants are checked.
  (c) what a user would do without the call (--torch): fp32 torch.matmul in row blocks + ceil / clamp / bincount on the device, upper
      triangle only.  Its scores are NOT the scan's bits, so its counts near a threshold are not the counts the scan produces.
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
ap.add_argument("--copies", type=int, nargs="+", default=[0])
ap.add_argument("--tiles", type=int, nargs="+", default=[0])
ap.add_argument("--link-only", action="store_true")
ap.add_argument("--torch", action="store_true")
ap.add_argument("--torch-block", type=int, default=2048)
ap.add_argument("--md", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402

DIM, BINS = 512, 2048


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


def torch_hist(rows, ids, block):
    G = rows.shape[0]
    hist = torch.zeros(2 * BINS, dtype=torch.int64, device="cuda")
    for r0 in range(0, G, block):
        r1 = min(G, r0 + block)
        s = (rows[r0:r1] @ rows[r0:].T + 1.0) / 2.0             # columns from r0 on: the upper triangle's block row
        b = (torch.ceil(s * float(BINS)) - 1.0).clamp_(0, BINS - 1).to(torch.int64)
        b += (ids[r0:r1, None] != ids[None, r0:]).to(torch.int64) * BINS
        keep = torch.arange(r0, r1, device="cuda")[:, None] < torch.arange(r0, G, device="cuda")[None, :]
        hist += torch.bincount(b[keep], minlength=2 * BINS)
    return hist


def main():
    torch.cuda.set_device(0)
    L = fa.lib()
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for G in a.rows:
        gen = torch.Generator(device="cuda").manual_seed(11)
        T = a.templates
        m = G // T
        centres = unit(torch.randn((m, DIM), device="cuda", generator=gen))
        rows = unit(centres.repeat_interleave(T, 0) + 0.02 * torch.randn((m * T, DIM), device="cuda", generator=gen))
        perm = torch.randperm(m * T, device="cuda", generator=gen)
        rows = rows[perm].contiguous()
        ids = (torch.arange(m, device="cuda", dtype=torch.int32).repeat_interleave(T) * 3 + 1)[perm].contiguous()
        G = m * T
        g = fa.Gallery(DIM)
        g.upload(rows.data_ptr(), G, True, 0, ids_ptr=ids.data_ptr())
        d = {"what": "pair_hist", "rows": G, "dim": DIM, "templates": T}
        labels = torch.zeros(G, dtype=torch.int32, device="cuda"); info = torch.zeros(4, dtype=torch.int32, device="cuda")
        tl = timed(lambda: g.cluster_dev(a.thr, 1, "none", labels.data_ptr(), info.data_ptr(), st), a.calls)
        d["link_call"] = stats(tl)
        link = statistics.median(tl)
        if not a.link_only:
            hist = torch.zeros(2 * BINS + 2, dtype=torch.int64, device="cuda")
            first = None
            d["hist_calls"] = []
            for tiles in a.tiles:
                for copies in a.copies:
                    L.fh_debug_cluster_tiles(tiles); L.fh_debug_hist_copies(copies)
                    try:
                        th = timed(lambda: g.pair_hist_dev(hist.data_ptr(), hist.data_ptr() + 2 * BINS * 8, st), a.calls)
                    finally:
                        L.fh_debug_cluster_tiles(0); L.fh_debug_hist_copies(0)
                    h = hist.cpu()
                    first = h if first is None else first
                    assert torch.equal(h, first), "arrangements disagree"
                    assert int(h.sum()) == G * (G - 1) // 2 and int(h[:BINS].sum()) + int(h[2 * BINS]) == m * T * (T - 1) // 2
                    e = {"tiles": tiles, "copies": copies, **stats(th), "over_link": round(statistics.median(th) / link, 4)}
                    d["hist_calls"].append(e)
            d["bins_used"] = [int((first[:BINS] > 0).sum()), int((first[BINS:2 * BINS] > 0).sum())]
            if a.torch:
                tt = timed(lambda: torch_hist(rows, ids, a.torch_block), min(a.calls, 3))
                d["torch_matmul_bincount"] = {**stats(tt), "over_link": round(statistics.median(tt) / link, 3)}
                ref = torch_hist(rows, ids, a.torch_block).cpu()
                d["torch_bins_that_differ_from_the_scan_bits"] = int((ref != first[:2 * BINS]).sum())
        print(json.dumps(d), flush=True)
        out.append(d)
    if a.md:
        with open(a.md, "w") as fo:
            fo.write("| rows | link call ms | tiles | copies | histogram call ms (min-max) | / link call |\n|---|---|---|---|---|---|\n")
            for d in out:
                lc = d["link_call"]
                for e in d.get("hist_calls", []):
                    fo.write(f"| {d['rows']} | {lc['median_ms']:.2f} ({lc['min_ms']:.2f}-{lc['max_ms']:.2f}) | {e['tiles'] or 'auto'} | "
                             f"{e['copies'] or 'default'} | {e['median_ms']:.2f} ({e['min_ms']:.2f}-{e['max_ms']:.2f}) | {e['over_link']} |\n")
                if "torch_matmul_bincount" in d:
                    t = d["torch_matmul_bincount"]
                    fo.write(f"| {d['rows']} | {lc['median_ms']:.2f} | - | torch.matmul + bincount | {t['median_ms']:.2f} ({t['min_ms']:.2f}-{t['max_ms']:.2f}) | "
                             f"{t['over_link']} |\n")


if __name__ == "__main__":
    main()
