"""Interleaved A/B of the identity scan (fh_gallery_topk_ids_dev) against the row-level fp32 scan (fh_gallery_topk_dev) of the same
build on the same rows, one process, the two alternated round by round.  Gallery 1 M x 512, k = 16, Q = 64 / 256; case "a": one
template per identity (random unit rows), case "b": 8 clustered templates per identity (centre + noise, shuffled), queries near
centres.  Per point: warm-up, then HIP events around blocks of 10 back-to-back calls, >= --calls calls per side; prints one JSON line
per point (median / min / max ms per call) and, with --md, a markdown table.
--rows-only times the row-level scan alone (it needs no identity entry point, so it also runs from a checkout of an earlier commit:
--pkg-root DIR imports the package from DIR instead of this tree).  --profile N: N calls of each kind and nothing else, for a
kernel-trace run."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--q", type=int, nargs="+", default=[64, 256])
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--cases", nargs="+", default=["a", "b"])
ap.add_argument("--calls", type=int, default=600)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows-only", action="store_true")
ap.add_argument("--profile", type=int, default=0)
ap.add_argument("--pkg-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--md", default="")
a = ap.parse_args()
sys.path.insert(0, a.pkg_root)

import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402

DIM = 512


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def make_case(case, G, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if case == "a":
        rows = unit(torch.randn((G, DIM), device="cuda", generator=gen))
        ids = (torch.randperm(G, device="cuda", generator=gen) * 3 + 1).to(torch.int32)
        centres = unit(torch.randn((4096, DIM), device="cuda", generator=gen))          # queries: random unit vectors
    else:
        T = 8
        centres = unit(torch.randn((G // T, DIM), device="cuda", generator=gen))
        rows = unit(centres.repeat_interleave(T, 0) + 0.02 * torch.randn((G, DIM), device="cuda", generator=gen))
        ids = (torch.arange(G // T, device="cuda") * 5 + 2).repeat_interleave(T).to(torch.int32)
        o = torch.randperm(G, device="cuda", generator=gen)
        rows, ids = rows[o].contiguous(), ids[o].contiguous()
    return rows, ids, centres, gen


def block_times(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range((calls + 9) // 10):
        e0.record()
        for _ in range(10):
            call()
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) / 10)
    return per


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "blocks_of_10": len(v)}


def main():
    torch.cuda.set_device(0)
    G, k = a.rows, a.k
    out = []
    for case in a.cases:
        rows, ids, centres, gen = make_case(case, G, 7 + ord(case))
        g_rows = fa.Gallery(DIM)
        g_rows.upload(rows.data_ptr(), G, True, 0)
        g_ids = None
        if not a.rows_only:
            g_ids = fa.Gallery(DIM)
            g_ids.upload(rows.data_ptr(), G, True, 0, ids_ptr=ids.data_ptr())
        for Q in a.q:
            pick = torch.randint(0, centres.shape[0], (Q,), device="cuda", generator=gen)
            q = unit(centres[pick] + (0.02 if case == "b" else 0.0) * torch.randn((Q, DIM), device="cuda", generator=gen)).contiguous()
            sc = torch.zeros((Q, k), device="cuda"); ix = torch.zeros((Q, k), dtype=torch.int32, device="cuda"); rw = torch.zeros_like(ix)
            st = torch.cuda.current_stream().cuda_stream
            sides = {"row_scan": lambda: g_rows.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st)}
            if g_ids is not None:
                sides["id_scan"] = lambda: g_ids.topk_ids_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), rw.data_ptr(), st)
            if a.profile:
                for call in sides.values():
                    for _ in range(a.profile):
                        call()
                torch.cuda.synchronize()
                continue
            res = {name: [] for name in sides}
            for call in sides.values():                        # warm-up: buffers sized, clocks up
                block_times(call, 20)
            for _ in range(a.rounds):                          # alternated
                for name, call in sides.items():
                    res[name] += block_times(call, (a.calls + a.rounds - 1) // a.rounds)
            d = {"case": case, "rows": G, "Q": Q, "k": k}
            for name, v in res.items():
                d[name] = stats(v)
            if "id_scan" in d:
                d["ids_over_rows"] = round(d["id_scan"]["median_ms"] / d["row_scan"]["median_ms"], 4)
            print(json.dumps(d), flush=True)
            out.append(d)
        del g_rows, g_ids, rows, ids
        torch.cuda.empty_cache()
    if a.md and out:
        with open(a.md, "w") as fo:
            fo.write("| case | Q | k | row scan median (min-max) ms | identity scan median (min-max) ms | identity / row |\n|---|---|---|---|---|---|\n")
            for d in out:
                r = d["row_scan"]; i = d.get("id_scan")
                fo.write(f"| {d['case']} | {d['Q']} | {d['k']} | {r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f}) | "
                         + (f"{i['median_ms']:.3f} ({i['min_ms']:.3f}-{i['max_ms']:.3f}) | {d['ids_over_rows']:.3f} |\n" if i else "- | - |\n"))


if __name__ == "__main__":
    main()
