"""Interleaved A/B of tiled detection (fh_det_detect_tiled_dev) on one MI355X, one process, det_500m's seeded stand-in, tile 640 with
overlap 128, frames resident in HBM.  Two cases: 16 synthetic 1080x1920 frames and 4 synthetic 2160x3840 frames.  Three legs per case,
HIP events around every block of steps, the legs alternated round by round after a warm-up:

  tiled          fh_det_detect_tiled_dev on the frames
  ragged_views   fh_det_detect_ragged_dev on the SAME views listed as plain frames: the same letterbox and network work, a plain decode
                 and one NMS per view (this leg also runs on code without tiled detection)
  ragged_frames  fh_det_detect_ragged_dev on the frames alone (what a caller had before: one down-scaled view per frame)

The quantity to judge is tiled / ragged_views: what the view-aware decode and the per-frame merge cost on top of the network.
Writes --md (default profiles/tiled_ab.md; the section "where the time is" there comes from separate --profile runs under a kernel
trace) and prints one JSON line per case.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=30, help="timed steps per leg (at least)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--block", type=int, default=3, help="steps per HIP-event sample")
ap.add_argument("--tile", type=int, default=640)
ap.add_argument("--overlap", type=int, default=128)
ap.add_argument("--border", type=int, default=2)
ap.add_argument("--cases", nargs="+", default=["1080x1920", "2160x3840"])
ap.add_argument("--profile", type=int, default=0, help="N tiled steps, then N ragged-on-the-views steps, of --cases and nothing else "
                "(for a separate `rocprofv3 --kernel-trace --stats` run: the two legs use the two instantiations of the decode kernel; "
                "their NMS launches differ in grid size, one workgroup per frame against one per view)")
ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tiled_ab.md"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402

THR, NMS, MAX_PF = 0.5, 0.4, 64
CASES = (("1080x1920", 16, 1080, 1920), ("2160x3840", 4, 2160, 3840))


def samples(step, steps, block):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range((steps + block - 1) // block):
        e0.record()
        for _ in range(block):
            step()
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) / block)
    return per


def stats(v):
    q = statistics.quantiles(v, n=10) if len(v) >= 10 else [min(v)] * 8 + [max(v)]
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4), "samples": len(v)}


def ab(legs):
    res = {k: [] for k in legs}
    for step in legs.values():
        samples(step, a.warmup, a.block)
    for _ in range(a.rounds):
        for name, step in legs.items():
            res[name] += samples(step, (a.steps + a.rounds - 1) // a.rounds, a.block)
    return {k: stats(v) for k, v in res.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tiled_ab.py measures on a GPU; none found")
    torch.cuda.set_device(0)
    fa._lib.check(fa.lib().fh_init(0), "fh_init")
    det = fa.FaceDetector()
    if not det.loadModel(models.cached("det_500m_seed100.onnx", models.make_det_500m)):
        raise SystemExit("model load failed: " + fa._lib.last_error())
    stream = torch.cuda.current_stream().cuda_stream
    tiling = fa.Tiling(a.tile, a.overlap, a.border)
    out = []
    for name, n, rows, cols in CASES:
        if name not in a.cases:
            continue
        rng = np.random.default_rng(rows)
        data = torch.from_numpy(rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)).cuda()
        views = fa.tile_plan(rows, cols, a.tile, a.overlap, a.border)
        step = cols * 3
        frames = [(data.data_ptr() + i * rows * step, rows, cols, step) for i in range(n)]
        listed = [(p + y * step + 3 * x, h, w, step) for p, _, _, _ in frames for x, y, w, h, _ in views]
        fr_arr, vw_arr = fa.frame_array(frames), fa.frame_array(listed)
        V = len(listed)
        rec = torch.zeros((V, MAX_PF, 15), device="cuda"); cnt = torch.zeros(V, dtype=torch.int32, device="cuda")

        def tiled():
            det.detect_tiled_dev(fr_arr, tiling, rec.data_ptr(), MAX_PF, cnt.data_ptr(), THR, NMS, stream)

        def ragged_views():
            det.detect_ragged_dev(vw_arr, rec.data_ptr(), MAX_PF, cnt.data_ptr(), THR, NMS, stream)

        def ragged_frames():
            det.detect_ragged_dev(fr_arr, rec.data_ptr(), MAX_PF, cnt.data_ptr(), THR, NMS, stream)

        if a.profile:
            for leg in (tiled, ragged_views):
                for _ in range(a.profile):
                    leg()
                torch.cuda.synchronize()
            print(json.dumps({"case": name, "profile_steps": a.profile, "views": V}), flush=True)
            continue
        st = ab({"tiled": tiled, "ragged_views": ragged_views, "ragged_frames": ragged_frames})
        tiled(); torch.cuda.synchronize()
        faces = int(cnt[:n].sum().item())
        d = {"case": name, "frames": n, "views_per_frame": len(views), "views": V, "faces_tiled": faces, **st,
             "tiled_over_ragged_views": round(st["tiled"]["median_ms"] / st["ragged_views"]["median_ms"], 4),
             "tiled_over_ragged_frames": round(st["tiled"]["median_ms"] / st["ragged_frames"]["median_ms"], 2)}
        print(json.dumps(d), flush=True)
        out.append(d)
        del data
    if a.md and out:
        write_md(out)


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['min_ms']:.3f}-{s['max_ms']:.3f}; p10-p90 {s['p10_ms']:.3f}-{s['p90_ms']:.3f}; {s['samples']} samples)"


def write_md(out):
    L = ["# Tiled detection: interleaved A/B", "",
         f"`scripts/tiled_ab.py` on one MI355X, one process: det_500m (seeded stand-in), tile {a.tile}, overlap {a.overlap}, border {a.border}, "
         f"thresholds {THR} / {NMS}, frames resident in HBM; {a.warmup} warm-up steps per leg, then the legs alternated for {a.rounds} rounds, "
         f">= {a.steps} timed steps per leg, HIP events around blocks of {a.block} steps (ms per step: median, min-max, p10-p90 over the block "
         "samples).", ""]
    for d in out:
        L += [f"## {d['frames']} frames of {d['case']}: {d['views_per_frame']} views per frame, {d['views']} views per call", "",
              "| leg | ms per step |", "|---|---|",
              f"| `fh_det_detect_tiled_dev` on the frames | {fmt(d['tiled'])} |",
              f"| `fh_det_detect_ragged_dev` on the same views listed as plain frames | {fmt(d['ragged_views'])} |",
              f"| `fh_det_detect_ragged_dev` on the frames alone | {fmt(d['ragged_frames'])} |", "",
              f"tiled / ragged-on-the-same-views (medians): **{d['tiled_over_ragged_views']:.3f}**; tiled / ragged-on-the-frames: "
              f"{d['tiled_over_ragged_frames']:.1f}x for {d['views_per_frame']}x the views.", ""]
    os.makedirs(os.path.dirname(a.md), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
