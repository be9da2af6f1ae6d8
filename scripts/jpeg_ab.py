"""A/B of the file front end on one MI355X: 128 copies of tests/golden/images/c1_640x640.jpg through
  (baseline) a per-file fh_image_decode loop followed by fh_pipeline_run_images — the only way in before the JPEG split, unchanged code;
  (files)    fh_pipeline_run_files: fh_jpeg_entropy on host threads, one copy, two reconstruction launches, the ragged pipeline.
Every leg runs in a FRESH process (this script calls itself with --leg), the legs alternated over --rounds rounds; full-size seeded models
(det_500m + w600k_r50), one face per frame.  Also taken, each in its own leg: the host entropy stage alone at 1 and 16 threads (no GPU
work) and the two reconstruction kernels alone on coefficients resident in HBM (HIP events around fh_jpeg_reconstruct_batch_dev), against
the traffic floor of 1.23 MB of coefficients read + 1.23 MB of pixels written per image.  Nothing here is a gate.

Writes --md (default profiles/jpeg_dev.md) and prints one JSON line per leg run.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--files", type=int, default=128)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5, help="timed steps per leg run")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--leg", default="", help="internal: run one leg in this process and print its JSON line")
ap.add_argument("--bench-line", default="", help="the JSON line of a bench.py run of this tree, to quote")
ap.add_argument("--parent-bench-line", default="", help="the JSON line of a bench.py run of the parent commit, to quote")
ap.add_argument("--bench-note", default="", help="a sentence to put under the two bench.py lines")
ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "jpeg_dev.md"))
a = ap.parse_args()
sys.path.insert(0, ROOT)

IMAGE = os.path.join(ROOT, "tests", "golden", "images", "c1_640x640.jpg")
LEGS = ("entropy_t1", "entropy_t16", "kernels", "baseline", "files_t16", "files_t1")
THR, NMS, F = 0.5, 0.4, 1
FLOOR_BYTES = 2 * 640 * 640 * 3                                  # per 640 x 640 4:2:0 image: coefficients read + pixels written


def wall(step, warmup, steps):
    for _ in range(warmup):
        step()
    per = []
    for _ in range(steps):
        t = time.perf_counter()
        step()
        per.append((time.perf_counter() - t) * 1e3)
    return per


def leg_entropy(threads):
    import numpy as np
    import facerecognizeonnx_amd as fa
    from facerecognizeonnx_amd import _lib
    L = fa.lib()
    data = open(IMAGE, "rb").read()
    buf = C.create_string_buffer(data, len(data))
    hd = _lib.FhJpegDesc()
    assert L.fh_jpeg_header(C.addressof(buf), len(data), C.byref(hd)) == 0
    n = int(hd.coef_count)
    coef = [np.zeros(n, np.int16) for _ in range(threads)]

    def worker(t, count):
        d = _lib.FhJpegDesc()
        for _ in range(count):
            assert L.fh_jpeg_entropy(C.addressof(buf), len(data), C.byref(d), coef[t].ctypes.data, n) == 0

    def step():                                                  # a.files decodes over `threads` threads (ctypes releases the GIL)
        share = [a.files // threads + (t < a.files % threads) for t in range(threads)]
        ts = [threading.Thread(target=worker, args=(t, share[t])) for t in range(threads)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    per = wall(step, 1, a.steps)
    return {"ms_per_image": [p / a.files for p in per], "cpus": os.cpu_count(), "affinity": len(os.sched_getaffinity(0))}


def gpu_setup(models_too):
    import torch
    import facerecognizeonnx_amd as fa
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_ab.py measures on a GPU; none found")
    torch.cuda.set_device(0)
    fa._lib.check(fa.lib().fh_init(0), "fh_init")
    if not models_too:
        return fa, torch, None, None
    from facerecognizeonnx_amd.synth import models
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    if not det.loadModel(models.cached("det_500m_seed100.onnx", models.make_det_500m)) or \
            not rec.loadModel(models.cached("w600k_r50_seed200.onnx", models.make_w600k_r50)):
        raise SystemExit("model load failed: " + fa._lib.last_error())
    return fa, torch, det, rec


def leg_kernels():
    import numpy as np
    fa, torch, _, _ = gpu_setup(False)
    from facerecognizeonnx_amd import _lib
    L = fa.lib()
    data = open(IMAGE, "rb").read()
    buf = C.create_string_buffer(data, len(data))
    d = _lib.FhJpegDesc()
    assert L.fh_jpeg_header(C.addressof(buf), len(data), C.byref(d)) == 0
    n = int(d.coef_count)
    coef = np.zeros(n, np.int16)
    assert L.fh_jpeg_entropy(C.addressof(buf), len(data), C.byref(d), coef.ctypes.data, n) == 0
    B = a.files
    d_coef = torch.from_numpy(np.tile(coef, B)).cuda()
    out = torch.zeros((B, d.rows, d.cols, 3), dtype=torch.uint8, device="cuda")
    descs = (_lib.FhJpegDesc * B)(*([d] * B))
    base = (np.arange(B, dtype=np.int64) * n)
    frames = fa.frame_array([(out.data_ptr() + i * d.rows * d.cols * 3, d.rows, d.cols) for i in range(B)])
    dec = fa.JpegDecoder()
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        assert L.fh_jpeg_reconstruct_batch_dev(dec.handle, descs, B, d_coef.data_ptr(), base.ctypes.data, frames, stream) == B

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    per = []
    for _ in range(max(a.steps, 10)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1))
    ref = fa.imread(IMAGE)
    same = bool(np.array_equal(out[B - 1].cpu().numpy(), ref))
    return {"ms_per_batch": per, "equals_imread": same, "floor_bytes": FLOOR_BYTES * B,
            "note": "HIP events around the call: the 70 KB descriptor-table copy and both kernels"}


def leg_pipeline(which, threads):
    fa, torch, det, rec = gpu_setup(True)
    import numpy as np
    data = open(IMAGE, "rb").read()
    files = [data] * a.files
    faces = [0]
    if which == "baseline":
        from facerecognizeonnx_amd import _lib
        L = fa.lib()
        buf = C.create_string_buffer(data, len(data))

        def step():
            imgs = []
            for _ in range(a.files):                             # fh_image_decode per file, as fh_imread's callers do
                p, r, c = C.c_void_p(), C.c_int(), C.c_int()
                assert L.fh_image_decode(C.addressof(buf), len(data), C.byref(p), C.byref(r), C.byref(c)) == 0
                imgs.append((p, r.value, c.value))
            arr = fa.frame_array([(p.value, r, c) for p, r, c in imgs])
            faces[0] = fa._lib.check(L.fh_pipeline_run_images(det.handle, rec.handle, arr, a.files, THR, NMS, F, None, None, None, 0), "run_images")
            for p, _, _ in imgs:
                L.fh_image_free(p)
    else:
        dec = fa.JpegDecoder()
        blobs, keep = fa.api._blobs(files)

        def step():
            faces[0] = fa._lib.check(fa.lib().fh_pipeline_run_files(det.handle, rec.handle, dec.handle, blobs, a.files, threads, THR, NMS, F,
                                                                    None, None, None, 0, None), "run_files")
    per = wall(step, a.warmup, a.steps)
    return {"ms_per_call": per, "faces": faces[0]}


def run_leg(name):
    if name.startswith("entropy_t"):
        return leg_entropy(int(name[9:]))
    if name == "kernels":
        return leg_kernels()
    if name == "baseline":
        return leg_pipeline("baseline", 0)
    return leg_pipeline("files", int(name[7:]))


def med(v):
    return statistics.median(v)


def main():
    if a.leg:
        print(json.dumps({"leg": a.leg, **run_leg(a.leg)}), flush=True)
        return
    res = {k: [] for k in LEGS}
    for rnd in range(a.rounds):
        for leg in LEGS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--files", str(a.files), "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"leg {leg} failed in round {rnd}")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps({"round": rnd, **line}), flush=True)
            res[leg].append(line)
    write_md(res)


def span(runs, key, scale=1.0):
    v = [x * scale for r in runs for x in r[key]]
    per_run = [med([x * scale for x in r[key]]) for r in runs]
    return f"{med(v):.3f} (per-process medians {min(per_run):.3f}-{max(per_run):.3f}; samples {min(v):.3f}-{max(v):.3f}, {len(v)} of them)"


def write_md(res):
    B = a.files
    k = res["kernels"]
    kms = med([x for r in k for x in r["ms_per_batch"]])
    floor = k[0]["floor_bytes"]
    tbs = floor / (kms * 1e-3) / 1e12
    base = med([x for r in res["baseline"] for x in r["ms_per_call"]])
    f16 = med([x for r in res["files_t16"] for x in r["ms_per_call"]])
    e = res["entropy_t1"][0]

    def bench(line):
        if not line:
            return "not measured"
        j = json.loads(line)
        return f"{j['value']:.0f} {j['unit']} ({j['ms_per_step']:.3f} ms per step, {j['steps']} steps)"

    L = ["# JPEG: host entropy decode, device reconstruction", "",
         f"`scripts/jpeg_ab.py` on one MI355X: {B} copies of `tests/golden/images/c1_640x640.jpg` (640 x 640, 4:2:0), det_500m + w600k_r50 (seeded), "
         f"one face per frame.  Every leg in a fresh process, the legs alternated over {a.rounds} rounds, {a.steps} timed steps per process after "
         f"{a.warmup} warm-up steps; figures are medians over all samples.  The host of the GPU gives a process {e['affinity']} CPUs "
         f"(`os.cpu_count()` = {e['cpus']}).  Nothing here is a gate.", "",
         "## Host entropy stage alone (`fh_jpeg_entropy`, no GPU work)", "",
         "| threads | ms per image (wall time of the batch / images) |", "|---|---|",
         f"| 1 | {span(res['entropy_t1'], 'ms_per_image')} |",
         f"| 16 | {span(res['entropy_t16'], 'ms_per_image')} |", "",
         "## Reconstruction kernels alone (`fh_jpeg_reconstruct_batch_dev`, coefficients resident in HBM)", "",
         f"| batch | ms per batch | bytes/s against the traffic floor |", "|---|---|---|",
         f"| {B} images | {span(k, 'ms_per_batch')} | floor {floor / 1e6:.1f} MB (coefficients read + pixels written) -> **{tbs:.2f} TB/s**, "
         f"{tbs / 8.0:.2f} of the 8 TB/s spec |", "",
         f"HIP events around the call, so the figure includes the descriptor-table copy; the plane round trip between the two kernels "
         f"(about {B * 1.2:.0f} MB written and read again) is traffic the floor does not count.  Pixels equal `fh_imread`'s: "
         f"{all(r['equals_imread'] for r in k)}.  What bounds the two kernels (per-kernel times from a separate `rocprofv3 --kernel-trace` run "
         f"of `--leg kernels`): docs/kernels.md §3.3f.", "",
         "## The blocking call end to end", "",
         "| leg | ms per call | faces |", "|---|---|---|",
         f"| baseline: `fh_image_decode` per file, then `fh_pipeline_run_images` | {span(res['baseline'], 'ms_per_call')} | {res['baseline'][0]['faces']} |",
         f"| `fh_pipeline_run_files`, threads = 16 | {span(res['files_t16'], 'ms_per_call')} | {res['files_t16'][0]['faces']} |",
         f"| `fh_pipeline_run_files`, threads = 1 | {span(res['files_t1'], 'ms_per_call')} | {res['files_t1'][0]['faces']} |", "",
         f"Ratio baseline / files (threads = 16): **{base / f16:.2f}x**.", "",
         "## `bench.py` headline (no existing path changes)", "",
         f"- this tree: {bench(a.bench_line)}", f"- parent commit: {bench(a.parent_bench_line)}", ""] + ([a.bench_note, ""] if a.bench_note else [])
    os.makedirs(os.path.dirname(a.md), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("\n".join(L))


if __name__ == "__main__":
    main()
