"""Interleaved A/B of the threshold (range) search, one process, the sides alternated round by round.  Gallery 1 M x 512, Q = 64 / 256,
random unit rows and queries; the threshold is read off the top-k answer so that a query has a handful of hits (the median over the
queries of the midpoint between their 5th and 6th best score).  Legs:
  (a) fh_gallery_topk_dev(k = 16) of this build against the same call of the PARENT commit's library (--parent-lib PATH: its
      libfacehip.so, built from a checkout of the parent and loaded beside this one through ctypes) — the top-k path must not have
      moved.  The margin is the parent's own run-to-run spread: the range of its per-round medians over --rounds rounds.
  (b) fh_gallery_range_dev with all three lists (cap = --cap) against this build's fh_gallery_topk_dev(k = 16) in the same rounds:
      the expectation is range <= top-k + the top-k call's own spread (same K loop, no seed pass, no merges, a few MB of bitmap).
  (c) the count-only form (all list pointers NULL), in the same rounds.
  (d) ONE leg at threshold 0.5 with cap 1024 — about half the gallery is a hit of every query: what a misuse costs (--misuse-calls).
Per side: warm-up, then HIP events around blocks of 10 back-to-back calls, >= --calls calls; one JSON line per (Q, side) with the
median / min / max ms per call and the per-round medians.  --md FILE: the table replaces the text between the `measurements` markers
of FILE (default profiles/gallery_range.md; created if missing).  Before timing, the range lists are compared bit for bit with the
entries of the top-k answer above the threshold, and the counts of the two forms with each other."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--q", type=int, nargs="+", default=[64, 256])
ap.add_argument("--cap", type=int, default=64)
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--misuse-calls", type=int, default=3)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gallery_range.md"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd import _lib  # noqa: E402

DIM, K = 512, 16
BEGIN, END = "<!-- measurements:begin -->", "<!-- measurements:end -->"


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def block_times(call, calls, block=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range((calls + block - 1) // block):
        e0.record()
        for _ in range(block):
            call()
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) / block)
    return per


class ParentLib:
    """fh_gallery_topk_dev of another build of the library (only the entry points every build has)."""

    def __init__(self, path, rows_ptr, G):
        L = C.CDLL(path)
        L.fh_gallery_create.restype = C.c_void_p
        L.fh_gallery_create.argtypes = [C.c_int]
        L.fh_gallery_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_longlong]
        L.fh_gallery_topk_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fh_init.argtypes = [C.c_int]
        assert L.fh_init(0) >= 0
        self.L, self.h = L, L.fh_gallery_create(DIM)
        assert self.h and L.fh_gallery_upload(self.h, rows_ptr, G, 1, 0) >= 0

    def topk(self, q, Q, k, sc, ix, st):
        assert self.L.fh_gallery_topk_dev(self.h, q, Q, k, sc, ix, st) == Q


def main():
    torch.cuda.set_device(0)
    _lib.check(fa.lib().fh_init(0), "fh_init")
    G, cap = a.rows, a.cap
    gen = torch.Generator(device="cuda").manual_seed(2026)
    rows = unit(torch.randn((G, DIM), device="cuda", generator=gen))
    g = fa.Gallery(DIM)
    g.upload(rows.data_ptr(), G, True, 0)
    parent = ParentLib(a.parent_lib, rows.data_ptr(), G) if a.parent_lib else None
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for Q in a.q:
        q = unit(torch.randn((Q, DIM), device="cuda", generator=gen)).contiguous()
        sc = torch.zeros((Q, K), device="cuda"); ix = torch.zeros((Q, K), dtype=torch.int32, device="cuda")
        P = (q.data_ptr(), Q, K, sc.data_ptr(), ix.data_ptr(), st)
        topk = lambda: g.topk_dev(*P)                                                                  # noqa: E731
        topk()
        torch.cuda.synchronize()
        thr = float(((sc[:, 4] + sc[:, 5]) / 2).median())
        cnt = torch.zeros(Q, dtype=torch.int64, device="cuda"); cnt2 = torch.zeros_like(cnt)
        rs = torch.zeros((Q, 1024), device="cuda"); ri = torch.zeros((Q, 1024), dtype=torch.int32, device="cuda")
        rng_lists = lambda t, c: (lambda: g.range_dev(q.data_ptr(), Q, t, c, cnt.data_ptr(), rs.data_ptr(), ri.data_ptr(), None, None, st))   # noqa: E731
        count_only = lambda: g.range_dev(q.data_ptr(), Q, thr, cap, cnt2.data_ptr(), None, None, None, None, st)      # noqa: E731
        # the answers first: the lists are the top-k entries above the threshold, the two forms count alike
        rng_lists(thr, K)(); count_only()
        torch.cuda.synchronize()
        keep = sc > thr
        assert torch.equal(cnt, cnt2) and torch.equal(torch.clamp(cnt, max=K), keep.sum(1))
        assert torch.equal(torch.where(keep, sc, torch.full_like(sc, -1.0)).view(torch.int32), rs.view(-1)[:Q * K].view(Q, K).view(torch.int32))
        assert torch.equal(torch.where(keep, ix, torch.full_like(ix, -1)), ri.view(-1)[:Q * K].view(Q, K))
        hits = cnt.cpu().numpy()

        def timed(sides, calls, block=10):
            res = {name: ([], []) for name, _ in sides}
            for _, call in sides:                               # warm-up: buffers sized, clocks up
                block_times(call, 2 * block, block)
            for _ in range(a.rounds):
                for name, call in sides:
                    v = block_times(call, (calls + a.rounds - 1) // a.rounds, block)
                    res[name][0].extend(v); res[name][1].append(statistics.median(v))
            return res

        def report(leg, name, v, extra=None):
            allv, rounds = v
            d = {"leg": leg, "side": name, "rows": G, "Q": Q, "median_ms": round(statistics.median(allv), 4), "min_ms": round(min(allv), 4),
                 "max_ms": round(max(allv), 4), "round_medians_ms": [round(x, 4) for x in rounds],
                 "round_spread_ms": round(max(rounds) - min(rounds), 4)}
            d.update(extra or {})
            print(json.dumps(d), flush=True)
            out.append(d)

        sides = [("this: topk_dev k=16", topk), (f"this: range_dev, lists, cap {cap}", rng_lists(thr, cap)), ("this: range_dev, counts only", count_only)]
        if parent:
            sides.insert(0, ("parent: topk_dev k=16", lambda: parent.topk(*P)))
        res = timed(sides, a.calls)
        info = {"threshold": round(thr, 6), "hits_per_query_median": float(statistics.median(hits.tolist())), "hits_per_query_max": int(hits.max())}
        for name, _ in sides:
            report("a" if "topk_dev" in name else "b" if "lists" in name else "c", name, res[name], None if "topk" in name else info)
        mis = rng_lists(0.5, 1024)
        mis()
        torch.cuda.synchronize()
        hits = cnt.cpu().numpy()
        res = timed([("this: range_dev, threshold 0.5, cap 1024", mis)], a.misuse_calls * a.rounds, 1)
        report("d", "this: range_dev, threshold 0.5, cap 1024", res["this: range_dev, threshold 0.5, cap 1024"],
               {"threshold": 0.5, "hits_per_query_median": float(statistics.median(hits.tolist())), "hits_per_query_max": int(hits.max())})
    if a.md:
        lines = [BEGIN, "", f"Gallery {G} x {DIM}; {a.calls} calls per side in blocks of 10 (leg d: {a.misuse_calls * a.rounds} single calls), "
                 f"{a.rounds} alternated rounds; ms per call: median (min - max); spread = range of the per-round medians.", "",
                 "| leg | side | Q | median (min - max) ms | spread ms | threshold | hits per query: median / max |", "|---|---|---|---|---|---|---|"]
        for d in out:
            h = f"{d['hits_per_query_median']:.0f} / {d['hits_per_query_max']}" if "threshold" in d else "-"
            t = f"{d['threshold']:.4f}" if "threshold" in d else "-"
            lines.append(f"| {d['leg']} | {d['side']} | {d['Q']} | {d['median_ms']:.3f} ({d['min_ms']:.3f} - {d['max_ms']:.3f}) | "
                         f"{d['round_spread_ms']:.3f} | {t} | {h} |")
        lines += ["", END]
        block = "\n".join(lines)
        text = open(a.md).read() if os.path.exists(a.md) else "# Threshold (range) search\n\n" + BEGIN + "\n" + END + "\n"
        if BEGIN in text and END in text:
            text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):]
        else:
            text = text.rstrip("\n") + "\n\n" + block + "\n"
        with open(a.md, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
