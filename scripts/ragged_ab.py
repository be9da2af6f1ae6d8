"""Interleaved A/B of the mixed-size pipeline (fh_pipeline_run_ragged_dev) on one MI355X, one process, full-size seeded models
(det_500m + w600k_r50), 128 frames per step, HIP events around every block of steps, the legs alternated round by round after a warm-up.

  (a) same-size frames: 128 x 640x640 through fh_pipeline_run_ragged_dev against fh_pipeline_run_dev (unchanged code: the uniform path).
      Expectation: the ragged step exceeds the uniform one by about the time of letterbox_ragged_kernel, which comes from a SEPARATE
      `rocprofv3 --kernel-trace --stats` run of `--profile N` (pass its *_kernel_stats.csv with --kernel-stats).
  (b) mixed sizes: 128 seeded frames with sizes drawn from {480x640, 720x1280, 1080x1920, 3000x4000, 250x250}, resident in HBM, through
      fh_pipeline_run_ragged_dev, against a loop of fh_det_detect + fh_rec_extract over the same images on the host (one image per
      call: the only way before).  Faces/s of both and the ratio: a record, not a gate.

Writes --md (default profiles/ragged_ab.md) and prints one JSON line per leg pair.  Needs a GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=128)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--steps", type=int, default=100, help="timed steps per leg (at least)")
ap.add_argument("--loop-steps", type=int, default=0, help="timed steps of the host-loop leg of (b); 0 = --steps")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--block", type=int, default=5, help="steps per HIP-event sample")
ap.add_argument("--cases", nargs="+", default=["a", "b"])
ap.add_argument("--profile", type=int, default=0, help="N ragged steps of case (a) and nothing else (for a kernel-trace run)")
ap.add_argument("--kernel-stats", default="", help="glob of the *_kernel_stats.csv of that rocprofv3 run")
ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ragged_ab.md"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402

THR, NMS, F = 0.5, 0.4, 1
SIZES = ((480, 640), (720, 1280), (1080, 1920), (3000, 4000), (250, 250))


def samples(step, steps, block):
    """ms per step of ceil(steps / block) blocks of `block` back-to-back steps (every step ends in the pipeline's own hand-off; the
    block ends in an event synchronise), and the faces of the last step."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per, faces = [], 0
    for _ in range((steps + block - 1) // block):
        e0.record()
        for _ in range(block):
            faces = step()
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) / block)
    return per, faces


def stats(v):
    q = statistics.quantiles(v, n=10) if len(v) >= 10 else [min(v)] * 9
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4), "samples": len(v)}


def ab(legs, warmup, steps, rounds, block):
    """legs: name -> (step, timed steps).  Warm every leg up, then alternate them round by round."""
    res, faces = {k: [] for k in legs}, {}
    for name, (step, _) in legs.items():
        samples(step, warmup, block)
    for _ in range(rounds):
        for name, (step, n) in legs.items():
            per, faces[name] = samples(step, (n + rounds - 1) // rounds, block)
            res[name] += per
    return {k: stats(v) for k, v in res.items()}, faces


def letterbox_us(pattern):
    files = sorted(glob.glob(pattern, recursive=True), key=os.path.getmtime) if pattern else []
    if not files:
        return None
    for row in csv.DictReader(open(files[-1])):
        if "letterbox_ragged_kernel" in row["Name"]:
            return {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                    "max_us": float(row["MaxNs"]) / 1e3}
    return None


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ragged_ab.py measures on a GPU; none found")
    torch.cuda.set_device(0)
    fa._lib.check(fa.lib().fh_init(0), "fh_init")
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    if not det.loadModel(models.cached("det_500m_seed100.onnx", models.make_det_500m)) or \
            not rec.loadModel(models.cached("w600k_r50_seed200.onnx", models.make_w600k_r50)):
        raise SystemExit("model load failed: " + fa._lib.last_error())
    B = a.frames
    stream = torch.cuda.current_stream().cuda_stream
    faces = torch.zeros((B * F, 15), device="cuda"); frame_of = torch.zeros(B * F, dtype=torch.int32, device="cuda")
    emb = torch.zeros((B * F, 512), device="cuda")
    out = {}

    if "a" in a.cases or a.profile:
        rng = np.random.default_rng(0)
        data = torch.from_numpy(rng.integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)).cuda()
        descs = fa.frame_array([(data.data_ptr() + i * 640 * 640 * 3, 640, 640) for i in range(B)])

        def ragged():
            return fa.pipeline_run_ragged_dev(det, rec, descs, F, faces.data_ptr(), frame_of.data_ptr(), emb.data_ptr(), THR, NMS, stream)

        def uniform():
            return fa.pipeline_run_dev(det, rec, data.data_ptr(), B, 640, 640, F, faces.data_ptr(), frame_of.data_ptr(), emb.data_ptr(), THR, NMS, stream)

        if a.profile:
            for _ in range(a.profile):
                ragged()
            torch.cuda.synchronize()
            print(json.dumps({"profile_steps": a.profile}))
            return
        st, fc = ab({"uniform": (uniform, a.steps), "ragged": (ragged, a.steps)}, a.warmup, a.steps, a.rounds, a.block)
        out["a"] = {"frames": B, "size": "640x640", "faces_per_step": fc, **st,
                    "excess_ms": round(st["ragged"]["median_ms"] - st["uniform"]["median_ms"], 4),
                    "uniform_spread_ms": round(st["uniform"]["p90_ms"] - st["uniform"]["p10_ms"], 4),
                    "letterbox_kernel": letterbox_us(a.kernel_stats)}
        print(json.dumps({"case": "a", **out["a"]}), flush=True)
        del data

    if "b" in a.cases:
        rng = np.random.default_rng(1)
        pick = rng.integers(0, len(SIZES), B)
        imgs = [rng.integers(0, 256, (SIZES[k][0], SIZES[k][1], 3), dtype=np.uint8) for k in pick]
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        descs = fa.frame_array([(d.data_ptr(), im.shape[0], im.shape[1]) for d, im in zip(dev, imgs)])

        def ragged():
            return fa.pipeline_run_ragged_dev(det, rec, descs, F, faces.data_ptr(), frame_of.data_ptr(), emb.data_ptr(), THR, NMS, stream)

        def host_loop():                                         # detect + extractFeature per image, as src/main.cpp:88-104
            n = 0
            for im in imgs:
                r = det.detect_records(im, THR, NMS, max_faces=F)
                for f in r[:F]:
                    n += int(rec.extractFeature(im, f).size > 0)
            return n

        loop_steps = a.loop_steps or a.steps
        st, fc = ab({"host_loop": (host_loop, loop_steps), "ragged": (ragged, a.steps)}, a.warmup, a.steps, a.rounds, a.block)
        fps = {k: fc[k] / (st[k]["median_ms"] * 1e-3) for k in st}
        out["b"] = {"frames": B, "sizes": {f"{r}x{c}": int((pick == i).sum()) for i, (r, c) in enumerate(SIZES)},
                    "mbytes": round(sum(im.nbytes for im in imgs) / 1e6, 1), "faces_per_step": fc, **st,
                    "faces_per_s": {k: round(v, 1) for k, v in fps.items()}, "ratio": round(fps["ragged"] / fps["host_loop"], 2)}
        print(json.dumps({"case": "b", **out["b"]}), flush=True)

    if a.md and out:
        write_md(out)


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['min_ms']:.3f}-{s['max_ms']:.3f}; p10-p90 {s['p10_ms']:.3f}-{s['p90_ms']:.3f}; {s['samples']} samples)"


def write_md(out):
    L = ["# Mixed-size pipeline: interleaved A/B", "",
         f"`scripts/ragged_ab.py` on one MI355X, one process: det_500m + w600k_r50 (seeded), {a.frames} frames per step, one face per frame, "
         f"thresholds {THR} / {NMS}; {a.warmup} warm-up steps per leg, then the legs alternated for {a.rounds} rounds, >= {a.steps} timed steps per "
         f"leg, HIP events around blocks of {a.block} steps (ms per step: median, min-max, p10-p90 over the block samples).", ""]
    if "a" in out:
        d = out["a"]; k = d["letterbox_kernel"]
        L += ["## (a) 128 same-size frames (640x640): ragged entry point against the uniform one", "",
              "| leg | ms per step | faces per step |", "|---|---|---|",
              f"| `fh_pipeline_run_dev` (uniform, unchanged code) | {fmt(d['uniform'])} | {d['faces_per_step']['uniform']} |",
              f"| `fh_pipeline_run_ragged_dev` | {fmt(d['ragged'])} | {d['faces_per_step']['ragged']} |", "",
              f"Excess of the ragged step (medians): **{d['excess_ms']:.3f} ms**; spread of the uniform leg (p90 - p10): {d['uniform_spread_ms']:.3f} ms."]
        if k:
            L += [f"`letterbox_ragged_kernel` in a separate `rocprofv3 --kernel-trace --stats` run of `--profile`: {k['avg_us']:.1f} us per launch "
                  f"(min {k['min_us']:.1f}, max {k['max_us']:.1f}, {k['calls']} launches).",
                  ("The excess is within the kernel's time plus the uniform leg's spread." if d["excess_ms"] <= k["avg_us"] / 1e3 + d["uniform_spread_ms"]
                   else "The excess is LARGER than the kernel's time plus the uniform leg's spread: see the note below.")]
        else:
            L += ["`letterbox_ragged_kernel`'s own time: not measured (no kernel-stats file given)."]
        L += [""]
    if "b" in out:
        d = out["b"]
        L += ["## (b) 128 mixed-size frames", "",
              "Sizes (frames): " + ", ".join(f"{k}: {v}" for k, v in d["sizes"].items()) + f"; {d['mbytes']} MB of pixels.", "",
              "| leg | ms per step | faces per step | faces/s |", "|---|---|---|---|",
              f"| loop of `fh_det_detect` + `fh_rec_extract` (host images, one per call) | {fmt(d['host_loop'])} | {d['faces_per_step']['host_loop']} | {d['faces_per_s']['host_loop']:.0f} |",
              f"| `fh_pipeline_run_ragged_dev` (frames resident in HBM) | {fmt(d['ragged'])} | {d['faces_per_step']['ragged']} | {d['faces_per_s']['ragged']:.0f} |", "",
              f"Ratio: **{d['ratio']:.2f}x**.  A record, not a gate; the host loop pays the upload of every image, the ragged leg reads them from HBM.", ""]
    os.makedirs(os.path.dirname(a.md), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("\n".join(L))


if __name__ == "__main__":
    main()
