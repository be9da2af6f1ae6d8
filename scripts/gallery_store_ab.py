"""Wall time of the gallery's synchronous maintenance calls on a handle with every per-row column live (labelled, tagged, F16_RERANK):
1 M x 512 rows uploaded with ids (one identity per 8 rows) and tagged, then 16 enrolments of 65 536 device rows with ids — the
capacity doubles at the first, the others append in place —, 16 set_tags of 65 536 rows from a device list, and remove_ids of every
tenth identity (twice: ids % 10 == 0, then ids % 10 == 1).  These calls allocate, copy and synchronise, so the figure is wall time
around the call (the device idle before it), not a HIP-event time.

One process measures ONE library: the in-tree build, or the one FACEHIP_LIB names (the parent commit's, for an A / B of fresh
processes alternating parent / this / parent / this).  Prints one JSON line: per call kind the median / min / max ms and every sample.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--enrolls", type=int, default=16)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--label", default=os.environ.get("FACEHIP_LIB", "") and "parent" or "this")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd import _lib  # noqa: E402

DIM = 512


def unit(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, DIM), device="cuda", generator=g)
    return x / x.norm(dim=1, keepdim=True)


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "samples_ms": [round(x, 3) for x in ms]}


L = _lib.lib()
_lib.check(L.fh_init(0), "fh_init")
total = a.rows + a.enrolls * a.batch
ids = torch.arange(total, dtype=torch.int32, device="cuda") // 8
g = fa.Gallery(DIM, scan="f16")
rows = unit(a.rows, 1)
g.upload(rows.data_ptr(), a.rows, True, 0, ids_ptr=ids.data_ptr())
g.set_tags(torch.full((a.rows,), 1, dtype=torch.int32, device="cuda"))
del rows

more, tags = unit(a.batch, 2), torch.full((a.batch,), 2, dtype=torch.int32, device="cuda")
enroll, set_tags = [], []
for i in range(a.enrolls):
    at = a.rows + i * a.batch
    ms, first = timed(lambda: L.fh_gallery_enroll_ids(g._h, more.data_ptr(), ids[at:].data_ptr(), a.batch, 1))
    assert first == at, (first, _lib.last_error())
    enroll.append(ms)
for i in range(a.enrolls):
    ms, n = timed(lambda: g.set_tags(tags, first=a.rows + i * a.batch))
    assert n == a.batch
    set_tags.append(ms)
assert len(g) == total
remove = []
for r in (0, 1):
    gone = np.arange(r, total // 8, 10, dtype=np.int32)
    ms, n = timed(lambda: g.remove_ids(gone))
    assert n == 8 * len(gone), (n, len(gone))
    remove.append(ms)
assert g.scan == "f16" and len(g) == total - 8 * (len(np.arange(0, total // 8, 10)) + len(np.arange(1, total // 8, 10)))
print(json.dumps({"script": "gallery_store_ab", "lib": a.label, "rows": a.rows, "enrolls": a.enrolls, "batch": a.batch,
                  "enroll_first_ms": round(enroll[0], 3), "enroll_in_place": stats(enroll[1:]), "set_tags": stats(set_tags),
                  "remove_ids": stats(remove)}), flush=True)
