"""Interleaved A/B of the tagged (watchlist) scans, one process, the sides alternated round by round.  Gallery 1 M x 512, k = 16,
Q = 64 / 256, random unit rows and queries.  Legs:
  (a) fh_gallery_topk_dev of this build against the same call of the PARENT commit's library (--parent-lib PATH: its libfacehip.so,
      built from a checkout of the parent and loaded beside this one through ctypes) — the untagged path must not have moved.  The
      margin is the parent's own run-to-run spread: the range of its per-round medians over --rounds rounds, printed beside it.
  (b) tagged, all-ones tags and all-ones masks, against (a): the cost of the predicate.
  (c) scattered tags (bit = row % 8), a mask selecting one bit: one row in eight admitted, every tile holds every bit.
  (d) the same tags grouped in runs of whole tiles — by default eight contiguous blocks, one per bit, as enrolments grouped by tenant
      or site are (--run N: runs of N tiles, the bits repeating) — and the same mask: tile skip on, tile skip off (fh_debug_tag_skip),
      and beside them fh_gallery_topk_dev on the compacted one-eighth gallery — the time a perfect skip would approach; tiles
      skipped / visited.  (A workgroup walks the tiles strided by the number of parts, a multiple of 64 on a 256-CU device: runs whose
      period divides that stride land whole groups on the same workgroups again and skip without saving time.)
Per side: warm-up, then HIP events around blocks of 10 back-to-back calls, >= --calls calls; one JSON line per (Q, side) with the
median / min / max ms per call and the per-round medians.  --md FILE: the table replaces the text between the `measurements` markers
of FILE (default profiles/gallery_tags.md; created if missing).  Before timing, the tagged answers of (c) and (d) are compared bit for
bit with the untagged scan of the compacted gallery (indices mapped back)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--q", type=int, nargs="+", default=[64, 256])
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--run", type=int, default=0, help="tiles per run of one tag bit in leg (d); 0 = eight contiguous blocks")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gallery_tags.md"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd import _lib  # noqa: E402

DIM, BIT = 512, 2
BEGIN, END = "<!-- measurements:begin -->", "<!-- measurements:end -->"


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


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
    G, k = a.rows, a.k
    gen = torch.Generator(device="cuda").manual_seed(2025)
    rows = unit(torch.randn((G, DIM), device="cuda", generator=gen))
    pos = torch.arange(G, device="cuda")
    scattered = (1 << (pos % 8)).to(torch.int32)
    run = a.run or ((G + 127) // 128 + 7) // 8
    grouped = (1 << ((pos // (128 * run)) % 8)).to(torch.int32)
    g = fa.Gallery(DIM)
    g.upload(rows.data_ptr(), G, True, 0)
    parent = ParentLib(a.parent_lib, rows.data_ptr(), G) if a.parent_lib else None
    compact, keep = {}, {}
    for name, tags in (("scattered", scattered), ("grouped", grouped)):
        keep[name] = torch.nonzero(tags & (1 << BIT)).flatten()
        sub = rows[keep[name]].contiguous()
        compact[name] = fa.Gallery(DIM)
        compact[name].upload(sub.data_ptr(), sub.shape[0], True, 0)
        del sub
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for Q in a.q:
        q = unit(torch.randn((Q, DIM), device="cuda", generator=gen)).contiguous()
        ones = torch.full((Q,), -1, dtype=torch.int32, device="cuda")
        one_bit = torch.full((Q,), 1 << BIT, dtype=torch.int32, device="cuda")
        sc = torch.zeros((Q, k), device="cuda"); ix = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
        sc2, ix2 = torch.zeros_like(sc), torch.zeros_like(ix)
        P = (q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st)
        untagged = lambda: g.topk_dev(*P)                                                            # noqa: E731
        tagged = lambda m: (lambda: g.topk_tagged_dev(q.data_ptr(), m.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st))   # noqa: E731

        def timed(sides, before=None):
            """[(name, call)] alternated round by round -> {name: all block times, per-round medians}."""
            if before:
                before()
            res = {name: ([], []) for name, _ in sides}
            for _, call in sides:                               # warm-up: buffers sized, clocks up
                block_times(call, 20)
            for _ in range(a.rounds):
                for name, call in sides:
                    v = block_times(call, (a.calls + a.rounds - 1) // a.rounds)
                    res[name][0].extend(v); res[name][1].append(statistics.median(v))
            return res

        def report(leg, name, v, extra=None):
            allv, rounds = v
            d = {"leg": leg, "side": name, "rows": G, "Q": Q, "k": k, "median_ms": round(statistics.median(allv), 4),
                 "min_ms": round(min(allv), 4), "max_ms": round(max(allv), 4),
                 "round_medians_ms": [round(x, 4) for x in rounds], "round_spread_ms": round(max(rounds) - min(rounds), 4)}
            d.update(extra or {})
            print(json.dumps(d), flush=True)
            out.append(d)

        def check(name):
            """the tagged answer on the full gallery = the untagged answer on the compacted one, bit for bit"""
            g.topk_tagged_dev(q.data_ptr(), one_bit.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), st)
            compact[name].topk_dev(q.data_ptr(), Q, k, sc2.data_ptr(), ix2.data_ptr(), st)
            torch.cuda.synchronize()
            assert torch.equal(sc.view(torch.int32), sc2.view(torch.int32)) and torch.equal(ix, keep[name][ix2.long()].to(torch.int32)), name

        # (a) + (b): tags never set = all ones
        sides = [("this: topk_dev", untagged), ("this: tagged, all ones", tagged(ones))]
        if parent:
            sides.insert(0, ("parent: topk_dev", lambda: parent.topk(*P)))
        res = timed(sides)
        for name, _ in sides:
            report("a" if "topk_dev" in name else "b", name, res[name])
        # (c) scattered
        g.set_tags(scattered)
        check("scattered")
        g.tag_stats()
        res = timed([("scattered, one bit in eight", tagged(one_bit))])
        scanned, skipped = g.tag_stats()
        report("c", "scattered, one bit in eight", res["scattered, one bit in eight"], {"tiles_scanned": scanned, "tiles_skipped": skipped})
        # (d) grouped: skip on / off / the compacted gallery
        g.set_tags(grouped)
        check("grouped")
        cg = compact["grouped"]
        g.tag_stats()
        res = timed([("grouped, skip on", tagged(one_bit)),
                     ("compacted 1/8 gallery: topk_dev", lambda: cg.topk_dev(*P))])
        scanned, skipped = g.tag_stats()
        report("d", "grouped, skip on", res["grouped, skip on"], {"tiles_scanned": scanned, "tiles_skipped": skipped, "tiles_per_run": run})
        report("d", "compacted 1/8 gallery: topk_dev", res["compacted 1/8 gallery: topk_dev"])
        try:
            fa.lib().fh_debug_tag_skip(0)
            res = timed([("grouped, skip off", tagged(one_bit))])
            scanned, skipped = g.tag_stats()
            report("d", "grouped, skip off", res["grouped, skip off"], {"tiles_scanned": scanned, "tiles_skipped": skipped})
        finally:
            fa.lib().fh_debug_tag_skip(1)
        g.upload(rows.data_ptr(), G, True, 0)                   # tags back to "never set" for the next Q
    if a.md:
        lines = [BEGIN, "", f"Gallery {G} x {DIM}, k = {k}; {a.calls} calls per side in blocks of 10, {a.rounds} alternated rounds; "
                 "ms per call: median (min - max); spread = range of the per-round medians.", "",
                 "| leg | side | Q | median (min - max) ms | spread ms | tiles multiplied / skipped |", "|---|---|---|---|---|---|"]
        for d in out:
            tiles = f"{d['tiles_scanned']} / {d['tiles_skipped']}" if "tiles_scanned" in d else "-"
            lines.append(f"| {d['leg']} | {d['side']} | {d['Q']} | {d['median_ms']:.3f} ({d['min_ms']:.3f} - {d['max_ms']:.3f}) | "
                         f"{d['round_spread_ms']:.3f} | {tiles} |")
        lines += ["", END]
        block = "\n".join(lines)
        text = open(a.md).read() if os.path.exists(a.md) else "# Tagged gallery scans\n\n" + BEGIN + "\n" + END + "\n"
        if BEGIN in text and END in text:
            text = text[:text.index(BEGIN)] + block + text[text.index(END) + len(END):]
        else:
            text = text.rstrip("\n") + "\n\n" + block + "\n"
        with open(a.md, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
