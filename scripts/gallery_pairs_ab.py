"""The pair audit of a gallery on the device (fh_gallery_pairs_dev) measured on clustered rows: --rows x 512, --templates templates per
identity (centre + 0.02 noise, shuffled: the generator of gallery_hist_ab.py), one process, HIP events around each call after a warm-up
call, --rounds rounds that visit every arrangement once each (so a drift of the clock hits all of them alike), median and min-max.
  (a) the audit at cap 16 and 1024, impostor pairs above the zero-false-accept threshold of fh_roc_from_hist minus 0.15 (few pairs: two
      identities are merged from one centre first, so the list is not empty) and above a loose threshold (count >> cap), genuine pairs
      not above; against fh_gallery_pair_hist_dev on the same gallery in the same rounds.  The count-only form (all three lists NULL)
      is the count pass + the cut alone, so "call - count only" is the collect pass + the select kernel.
  (b) the same question through fh_gallery_range_dev with all rows as queries, 256 per call: --range-calls calls are timed and the whole
      is their mean times ceil(rows / 256) (every call scans the whole gallery, so the calls cost the same but for their lists).
  (c) `--old-only` times only fh_gallery_cluster_dev and fh_gallery_pair_hist_dev — calls that existed before the audit — so it runs on
      an older checkout unchanged.
One JSON line per point; --md FILE writes the tables."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[65536, 262144])
ap.add_argument("--templates", type=int, default=8)
ap.add_argument("--thr", type=float, default=0.8)
ap.add_argument("--loose", type=float, default=0.6)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--range-calls", type=int, default=8)
ap.add_argument("--old-only", action="store_true")
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


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); call(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def rounds(calls, n):
    """calls: name -> callable; one warm-up of each, then n rounds over all of them in turn"""
    for c in calls.values():
        c()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(n):
        for k, c in calls.items():
            out[k].append(once(c))
    return out


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
        perm = torch.randperm(m * T, device="cuda", generator=gen)
        rows = rows[perm].contiguous()
        ids = torch.arange(m, device="cuda", dtype=torch.int32).repeat_interleave(T) * 3 + 1
        ids[T // 2:T] = 2                                         # one person enrolled under two ids: centre 0's templates split
        ids = ids[perm].contiguous()
        G = m * T
        g = fa.Gallery(DIM)
        g.upload(rows.data_ptr(), G, True, 0, ids_ptr=ids.data_ptr())
        d = {"what": "pairs", "rows": G, "dim": DIM, "templates": T}
        labels = torch.zeros(G, dtype=torch.int32, device="cuda"); cinfo = torch.zeros(4, dtype=torch.int32, device="cuda")
        hist = torch.zeros(2 * BINS + 2, dtype=torch.int64, device="cuda")
        calls = {"cluster_call": lambda: g.cluster_dev(a.thr, 1, "none", labels.data_ptr(), cinfo.data_ptr(), st),
                 "hist_call": lambda: g.pair_hist_dev(hist.data_ptr(), hist.data_ptr() + 2 * BINS * 8, st)}
        arrangements = []
        if not a.old_only:
            h, _ = g.pair_hist()
            op, _ = fa.roc_from_hist(h, 0.0)
            tight = op["threshold"] - 0.15
            d["roc_threshold"] = op["threshold"]
            info = torch.zeros(4, dtype=torch.int64, device="cuda")
            s = torch.zeros(1024, dtype=torch.float32, device="cuda")
            r = torch.zeros(2048, dtype=torch.int32, device="cuda"); di = torch.zeros(2048, dtype=torch.int32, device="cuda")
            for cls, side, thr, what in (("impostor", "above", tight, "impostor above roc - 0.15"), ("impostor", "above", a.loose, f"impostor above {a.loose}"),
                                         ("genuine", "not_above", tight, "genuine not above roc - 0.15")):
                for cap in (16, 1024):
                    name = f"{what}, cap {cap}"
                    arrangements.append((name, cls, side, thr, cap))
                    calls[name] = (lambda cls=cls, side=side, thr=thr, cap=cap:
                                   g.pairs_dev(cls, side, thr, cap, info.data_ptr(), s.data_ptr(), r.data_ptr(), di.data_ptr(), st))
                calls[f"{what}, count only"] = (lambda cls=cls, side=side, thr=thr: g.pairs_dev(cls, side, thr, 16, info.data_ptr(), None, None, None, st))
        t = rounds(calls, a.rounds)
        d["cluster_call"], d["hist_call"] = stats(t["cluster_call"]), stats(t["hist_call"])
        hm = statistics.median(t["hist_call"])
        d["pairs_calls"] = []
        for name, cls, side, thr, cap in arrangements:
            g.pairs_dev(cls, side, thr, cap, info.data_ptr(), s.data_ptr(), r.data_ptr(), di.data_ptr(), st)
            torch.cuda.synchronize()
            got = [int(x) for x in info.cpu().numpy().view("uint64")]
            co = statistics.median(t[name.rsplit(",", 1)[0] + ", count only"])
            med = statistics.median(t[name])
            d["pairs_calls"].append({"what": name, "threshold": round(float(thr), 6), "cap": cap, "info": got, **stats(t[name]),
                                     "over_hist": round(med / hm, 3), "count_only_ms": round(co, 3), "collect_select_ms": round(med - co, 3)})
        if not a.old_only:
            # (b) all rows as queries through the range search, 256 per call; the impostor filter would still be the host's work
            counts = torch.zeros(256, dtype=torch.int64, device="cuda")
            rs = torch.zeros((256, 16), dtype=torch.float32, device="cuda"); ri = torch.zeros((256, 16), dtype=torch.int32, device="cuda")
            rd = torch.zeros((256, 16), dtype=torch.int32, device="cuda")
            ncalls = (G + 255) // 256
            step = max(ncalls // a.range_calls, 1)
            tr = []
            for k in range(0, ncalls, step):
                q0 = min(k * 256, G - 256)
                call = lambda: g.range_dev(rows.data_ptr() + q0 * DIM * 4, 256, tight, 16, counts.data_ptr(), rs.data_ptr(), ri.data_ptr(), rd.data_ptr(), None, st)   # noqa: E731
                if not tr:
                    call(); torch.cuda.synchronize()
                tr.append(once(call))
            d["range_all_rows"] = {"calls": ncalls, "timed": len(tr), "per_call": stats(tr), "total_ms": round(statistics.mean(tr) * ncalls, 1),
                                   "over_hist": round(statistics.mean(tr) * ncalls / hm, 2)}
        print(json.dumps(d), flush=True)
        out.append(d)
    if a.md:
        with open(a.md, "w") as fo:
            fo.write("| rows | cluster call ms (min-max) | histogram call ms (min-max) |\n|---|---|---|\n")
            for d in out:
                c, h = d["cluster_call"], d["hist_call"]
                fo.write(f"| {d['rows']} | {c['median_ms']:.2f} ({c['min_ms']:.2f}-{c['max_ms']:.2f}) | {h['median_ms']:.2f} ({h['min_ms']:.2f}-{h['max_ms']:.2f}) |\n")
            if not a.old_only:
                fo.write("\n| rows | audit | count | returned | call ms (min-max) | / histogram call | count pass + cut ms | collect + select ms |\n|---|---|---|---|---|---|---|---|\n")
                for d in out:
                    for e in d["pairs_calls"]:
                        fo.write(f"| {d['rows']} | {e['what']} (thr {e['threshold']}) | {e['info'][0]} | {e['info'][2]} | {e['median_ms']:.2f} "
                                 f"({e['min_ms']:.2f}-{e['max_ms']:.2f}) | {e['over_hist']} | {e['count_only_ms']:.2f} | {e['collect_select_ms']:.2f} |\n")
                fo.write("\n| rows | range calls of 256 queries | timed | per call ms (min-max) | all calls ms | / histogram call |\n|---|---|---|---|---|---|\n")
                for d in out:
                    e = d["range_all_rows"]
                    p = e["per_call"]
                    fo.write(f"| {d['rows']} | {e['calls']} | {e['timed']} | {p['median_ms']:.2f} ({p['min_ms']:.2f}-{p['max_ms']:.2f}) | {e['total_ms']} | {e['over_hist']} |\n")


if __name__ == "__main__":
    main()
