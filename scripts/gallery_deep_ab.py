"""Interleaved A/B of the deep top-k (fh_gallery_topk_deep_dev), one process, the sides alternated round by round.  Gallery 1 M x 512,
Q = 64 / 256, k = 16 / 64 / 128 / 1024, random unit rows and queries.  Per (Q, k), all in the same rounds:
  (a) the deep call (scores + indices) against this build's fh_gallery_topk_dev(k = 16);
  (b) against fh_gallery_range_dev(cap = k) given the IDEAL threshold — nextafter below the k-th score the deep call returned, the
      smallest over the queries: the competitor that knows the answer in advance;
  (c) against torch.matmul + torch.topk on the same tensors — what a caller does today; its scores are not the scan's bits;
  (d) fh_gallery_topk_dev(k = 16) and that fh_gallery_range_dev call of this build against the PARENT commit's library (--parent-lib
      PATH: its libfacehip.so, loaded beside this one through ctypes): they must agree within the run-to-run spread reported here (the
      range of a side's per-round medians).
Per side: warm-up, then HIP events around blocks of 5 back-to-back calls, >= --calls calls; one JSON line per (Q, k, side) with the
median / min / max ms per call and the per-round medians.  --md FILE: the table replaces the text between the `measurements` markers
of FILE (default profiles/gallery_deep.md; created if missing).  Before timing, the deep lists are compared bit for bit with the range
call's lists at the ideal threshold, with the parent's, and (k = 16) with fh_gallery_topk_dev's.
--profile-only: no timing — --calls deep calls per (Q, k) and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--q", type=int, nargs="+", default=[64, 256])
ap.add_argument("--k", type=int, nargs="+", default=[16, 64, 128, 1024])
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--profile-only", action="store_true")
ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gallery_deep.md"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd import _lib  # noqa: E402

DIM, BLOCK = 512, 5
BEGIN, END = "<!-- measurements:begin -->", "<!-- measurements:end -->"


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def block_times(call, calls, block=BLOCK):
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
    """fh_gallery_topk_dev and fh_gallery_range_dev of another build of the library (only the entry points every build has)."""

    def __init__(self, path, rows_ptr, G):
        L = C.CDLL(path)
        L.fh_gallery_create.restype = C.c_void_p
        L.fh_gallery_create.argtypes = [C.c_int]
        L.fh_gallery_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_longlong]
        L.fh_gallery_topk_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fh_gallery_range_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 5
        L.fh_init.argtypes = [C.c_int]
        assert L.fh_init(0) >= 0
        self.L, self.h = L, L.fh_gallery_create(DIM)
        assert self.h and L.fh_gallery_upload(self.h, rows_ptr, G, 1, 0) >= 0

    def topk(self, q, Q, k, sc, ix, st):
        assert self.L.fh_gallery_topk_dev(self.h, q, Q, k, sc, ix, st) == Q

    def range(self, q, Q, thr, cap, cnt, sc, ix, st):
        assert self.L.fh_gallery_range_dev(self.h, q, None, Q, thr, cap, cnt, sc, ix, None, st) == Q


def main():
    torch.cuda.set_device(0)
    _lib.check(fa.lib().fh_init(0), "fh_init")
    G = a.rows
    gen = torch.Generator(device="cuda").manual_seed(2027)
    rows = unit(torch.randn((G, DIM), device="cuda", generator=gen))
    g = fa.Gallery(DIM)
    g.upload(rows.data_ptr(), G, True, 0)
    st = torch.cuda.current_stream().cuda_stream
    if a.profile_only:
        for Q in a.q:
            q = unit(torch.randn((Q, DIM), device="cuda", generator=gen)).contiguous()
            for k in a.k:
                ds = torch.zeros((Q, k), device="cuda"); di = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
                for _ in range(a.calls):
                    g.topk_deep_dev(q.data_ptr(), Q, k, ds.data_ptr(), di.data_ptr(), None, None, st)
                torch.cuda.synchronize()
        return
    parent = ParentLib(a.parent_lib, rows.data_ptr(), G) if a.parent_lib else None
    out = []
    for Q in a.q:
        q = unit(torch.randn((Q, DIM), device="cuda", generator=gen)).contiguous()
        ts = torch.zeros((Q, 16), device="cuda"); ti = torch.zeros((Q, 16), dtype=torch.int32, device="cuda")
        T = (q.data_ptr(), Q, 16, ts.data_ptr(), ti.data_ptr(), st)
        for k in a.k:
            ds = torch.zeros((Q, k), device="cuda"); di = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
            rs = torch.zeros((Q, k), device="cuda"); ri = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
            ps = torch.zeros((Q, k), device="cuda"); pi = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
            cnt = torch.zeros(Q, dtype=torch.int64, device="cuda"); pcnt = torch.zeros_like(cnt)
            deep = lambda: g.topk_deep_dev(q.data_ptr(), Q, k, ds.data_ptr(), di.data_ptr(), None, None, st)          # noqa: E731
            topk = lambda: g.topk_dev(*T)                                                                              # noqa: E731
            deep(); topk()
            torch.cuda.synchronize()
            thr = float(np.nextafter(np.float32(ds[:, k - 1].min().item()), np.float32(-np.inf)))
            rng = lambda: g.range_dev(q.data_ptr(), Q, thr, k, cnt.data_ptr(), rs.data_ptr(), ri.data_ptr(), None, None, st)      # noqa: E731
            mm = lambda: torch.topk(torch.matmul(q, rows.t()), k, dim=1)                                               # noqa: E731
            # the answers first, by bits
            rng()
            torch.cuda.synchronize()
            assert (cnt >= k).all() and torch.equal(ds.view(torch.int32), rs.view(torch.int32)) and torch.equal(di, ri), "deep != range"
            if k == 16:
                assert torch.equal(ds.view(torch.int32), ts.view(torch.int32)) and torch.equal(di, ti), "deep != topk_dev"
            tv, tix = mm()
            agree = float((tix.to(torch.int32) == di).float().mean())       # (not bits: another summation order; ties may swap)
            sides = [("this: topk_dev k=16", topk), (f"this: topk_deep_dev k={k}", deep), (f"this: range_dev, ideal threshold, cap {k}", rng),
                     (f"torch.matmul + torch.topk k={k}", mm)]
            if parent:
                prng = lambda: parent.range(q.data_ptr(), Q, thr, k, pcnt.data_ptr(), ps.data_ptr(), pi.data_ptr(), st)   # noqa: E731
                prng()
                torch.cuda.synchronize()
                assert torch.equal(pcnt, cnt) and torch.equal(ps.view(torch.int32), ds.view(torch.int32)) and torch.equal(pi, di), "parent != deep"
                sides = [("parent: topk_dev k=16", lambda: parent.topk(*T)), (f"parent: range_dev, ideal threshold, cap {k}", prng)] + sides
            res = {name: ([], []) for name, _ in sides}
            for _, call in sides:                               # warm-up: buffers sized, clocks up
                block_times(call, 2 * BLOCK)
            for _ in range(a.rounds):
                for name, call in sides:
                    v = block_times(call, (a.calls + a.rounds - 1) // a.rounds)
                    res[name][0].extend(v); res[name][1].append(statistics.median(v))
            hits = cnt.cpu().numpy()
            for name, _ in sides:
                allv, rounds = res[name]
                d = {"side": name, "rows": G, "Q": Q, "k": k, "median_ms": round(statistics.median(allv), 4), "min_ms": round(min(allv), 4),
                     "max_ms": round(max(allv), 4), "round_medians_ms": [round(x, 4) for x in rounds],
                     "round_spread_ms": round(max(rounds) - min(rounds), 4)}
                if "range_dev" in name:
                    d.update({"threshold": round(thr, 6), "hits_per_query_median": float(statistics.median(hits.tolist())), "hits_per_query_max": int(hits.max())})
                if "torch" in name:
                    d["index_agreement_with_deep"] = round(agree, 6)
                print(json.dumps(d), flush=True)
                out.append(d)
    if a.md:
        lines = [BEGIN, "", f"Gallery {G} x {DIM}; {a.calls} calls per side in blocks of {BLOCK}, {a.rounds} alternated rounds; ms per call: median "
                 "(min - max); spread = range of the per-round medians.", "",
                 "| Q | k | side | median (min - max) ms | spread ms | range hits per query: median / max |", "|---|---|---|---|---|---|"]
        for d in out:
            h = f"{d['hits_per_query_median']:.0f} / {d['hits_per_query_max']}" if "threshold" in d else "-"
            lines.append(f"| {d['Q']} | {d['k']} | {d['side']} | {d['median_ms']:.3f} ({d['min_ms']:.3f} - {d['max_ms']:.3f}) | "
                         f"{d['round_spread_ms']:.3f} | {h} |")
        lines += ["", END]
        block = "\n".join(lines)
        text = open(a.md).read() if os.path.exists(a.md) else "# Deep top-k\n\n" + BEGIN + "\n" + END + "\n"
        if BEGIN in text and END in text:
            text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):]
        else:
            text = text.rstrip("\n") + "\n\n" + block + "\n"
        with open(a.md, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
