"""Measurement of the JPEG encoder on one MI355X, quality 90, 4:2:0, two workloads: 128 frames of 640 x 640 (the decoded
tests/golden/images/c1_640x640.jpg) and 1024 chips of 112 x 112 (windows of that picture at seeded positions).  Legs, each in a FRESH
process (this script calls itself with --leg), alternated over --rounds rounds:
  pillow      a per-image Pillow `save` loop on one core of the same host: the CPU baseline
  huff_t1/16  the host Huffman stage alone: fh_jpeg_write per image on 1 / 16 threads, coefficients already in host memory (no GPU work)
  kernels     the two forward kernels alone on frames resident in HBM (events around fh_jpeg_forward_batch_dev), against their traffic
              floor: pixels read once, sample planes written and read once, coefficients written once
  encode_t1/16  fh_jpeg_encode_batch end to end (kernels, one device-to-host copy, Huffman coding on 1 / 16 threads), blocking
  coder       the device Huffman coder alone on coefficients resident in HBM (events around fh_jpeg_code_batch_dev, its two stream
              synchronisations included)
  encode_gpu  fh_jpeg_encode_batch_gpu end to end (kernels, the device coder, one device-to-host copy of the files' bytes), blocking
--legs picks a subset (with --md: profiles/jpeg_huff.md was written with --legs huff_t16,kernels,encode_t16,encode_t1,coder,encode_gpu).
Nothing here is a gate.  Writes --md (default profiles/jpeg_enc.md) and prints one JSON line per leg run.  Needs a GPU; no fallback."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=5, help="timed steps per leg run")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--leg", default="", help="internal: run one leg in this process and print its JSON line")
ap.add_argument("--load", default="frames640", help="internal: the workload of --leg")
ap.add_argument("--legs", default="", help="comma-separated subset of the legs (default: all)")
ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "jpeg_enc.md"))
a = ap.parse_args()
sys.path.insert(0, ROOT)

IMAGE = os.path.join(ROOT, "tests", "golden", "images", "c1_640x640.jpg")
LOADS = {"frames640": (128, 640), "chips112": (1024, 112)}
LEGS = ("pillow", "huff_t1", "huff_t16", "kernels", "encode_t16", "encode_t1", "coder", "encode_gpu")
QUALITY, SUB = 90, 2


def pictures(load):
    import numpy as np
    import facerecognizeonnx_amd as fa
    n, side = LOADS[load]
    img = fa.imread(IMAGE)
    if side == 640:
        return [img] * n
    rng = np.random.default_rng(3)
    return [np.ascontiguousarray(img[y: y + side, x: x + side]) for y, x in rng.integers(0, 640 - side, (n, 2))]


def wall(step, warmup, steps):
    for _ in range(warmup):
        step()
    per = []
    for _ in range(steps):
        t = time.perf_counter()
        step()
        per.append((time.perf_counter() - t) * 1e3)
    return per


def floor_bytes(side):
    return side * side * 3 + 2 * (side * side * 3 // 2) + (side * side * 3 // 2) * 2      # 4:2:0, sides that are multiples of 16


def leg_pillow(load):
    from PIL import Image
    pics = [Image.fromarray(p[:, :, ::-1].copy(), "RGB") for p in pictures(load)]
    sizes = []

    def step():
        sizes.clear()
        for p in pics:
            buf = io.BytesIO()
            p.save(buf, "JPEG", quality=QUALITY, subsampling=SUB, optimize=False)
            sizes.append(buf.tell())
    return {"ms": wall(step, 1, max(a.steps // 2, 2)), "bytes": sum(sizes)}


def leg_huff(load, threads):
    import numpy as np
    import facerecognizeonnx_amd as fa
    from facerecognizeonnx_amd import _lib
    L = fa.lib()
    pics = pictures(load)
    n, side = LOADS[load]
    d = _lib.FhJpegDesc()
    assert L.fh_jpeg_enc_desc(side, side, 0, SUB, QUALITY, C.byref(d)) == 0
    count, bound = int(d.coef_count), int(L.fh_jpeg_write_bound(C.byref(d)))
    coefs = np.zeros((n, count), np.int16)
    for i, p in enumerate(pics):
        assert L.fh_jpeg_forward(C.byref(d), p.ctypes.data, side * 3, coefs[i].ctypes.data, count) == 0
    outs = [np.zeros(bound, np.uint8) for _ in range(threads)]
    sizes = np.zeros(n, np.int64)

    def work(t):
        w = C.c_size_t(0)
        for i in range(t, n, threads):
            L.fh_jpeg_write(C.byref(d), coefs[i].ctypes.data, outs[t].ctypes.data, bound, C.byref(w))
            sizes[i] = w.value

    def step():
        ts = [threading.Thread(target=work, args=(t,)) for t in range(1, threads)]
        for t in ts:
            t.start()
        work(0)
        for t in ts:
            t.join()
    return {"ms": wall(step, a.warmup, a.steps), "bytes": int(sizes.sum())}


def device_frames(load):
    import numpy as np
    import torch
    pics = pictures(load)
    n, side = LOADS[load]
    buf = torch.from_numpy(np.stack(pics)).cuda()
    one = side * side * 3
    return buf, [(buf.data_ptr() + i * one, side, side) for i in range(n)]


def leg_kernels(load):
    import numpy as np
    import torch
    import facerecognizeonnx_amd as fa
    from facerecognizeonnx_amd import _lib
    L = fa.lib()
    L.fh_init(0)
    n, side = LOADS[load]
    keep, frames = device_frames(load)
    fr = fa.frame_array(frames)
    d = _lib.FhJpegDesc()
    assert L.fh_jpeg_enc_desc(side, side, 0, SUB, QUALITY, C.byref(d)) == 0
    count = int(d.coef_count)
    descs = (_lib.FhJpegDesc * n)(*([d] * n))
    base = np.arange(n, dtype=np.int64) * count
    d_coef = torch.zeros(n * count, dtype=torch.int16, device="cuda")
    enc = fa.JpegEncoder()
    s = torch.cuda.current_stream().cuda_stream
    per = []
    for k in range(a.warmup + 2 * a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert L.fh_jpeg_forward_batch_dev(enc.handle, descs, n, fr, d_coef.data_ptr(), base.ctypes.data, s) == n
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            per.append(e0.elapsed_time(e1))
    host = np.zeros(count, np.int16)                                           # the first and the last image against the host path
    same = True
    for i in (0, n - 1):
        first = np.ascontiguousarray(keep[i].cpu().numpy())                    # (held in a name: ctypes takes a bare address)
        assert L.fh_jpeg_forward(C.byref(d), first.ctypes.data, side * 3, host.ctypes.data, count) == 0
        same = same and bool(np.array_equal(d_coef[i * count: (i + 1) * count].cpu().numpy(), host))
    del keep
    return {"ms": per, "equal_host": same, "floor_bytes": n * floor_bytes(side)}


def leg_encode(load, threads, coder="host"):
    import torch
    import facerecognizeonnx_amd as fa
    fa.lib().fh_init(0)
    keep, frames = device_frames(load)
    enc = fa.JpegEncoder()
    torch.cuda.synchronize()
    sizes = []

    def step():
        sizes[:] = [len(f) for f in enc.encode_dev(frames, QUALITY, SUB, threads, coder=coder)]
    out = {"ms": wall(step, a.warmup, a.steps), "bytes": sum(sizes)}
    if coder == "device":
        n, side = LOADS[load]
        out["coef_bytes"] = n * side * side * 3                                # 4:2:0: 1.5 int16 per pixel
        out["equal_host"] = enc.encode_dev(frames, QUALITY, SUB, 16) == enc.encode_dev(frames, QUALITY, SUB, coder="device")
    del keep
    return out


def leg_coder(load):
    import numpy as np
    import torch
    import facerecognizeonnx_amd as fa
    from facerecognizeonnx_amd import _lib
    L = fa.lib()
    L.fh_init(0)
    n, side = LOADS[load]
    keep, frames = device_frames(load)
    d = _lib.FhJpegDesc()
    assert L.fh_jpeg_enc_desc(side, side, 0, SUB, QUALITY, C.byref(d)) == 0
    count = int(d.coef_count)
    descs = (_lib.FhJpegDesc * n)(*([d] * n))
    base = np.arange(n, dtype=np.int64) * count
    d_coef = torch.zeros(n * count, dtype=torch.int16, device="cuda")
    enc = fa.JpegEncoder()
    s = torch.cuda.current_stream().cuda_stream
    assert L.fh_jpeg_forward_batch_dev(enc.handle, descs, n, fa.frame_array(frames), d_coef.data_ptr(), base.ctypes.data, s) == n
    torch.cuda.synchronize()
    blobs, status = (_lib.FhBlob * n)(), np.zeros(n, np.int32)
    per = []
    for k in range(a.warmup + 2 * a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert L.fh_jpeg_code_batch_dev(enc.handle, descs, n, d_coef.data_ptr(), base.ctypes.data, blobs, status.ctypes.data, s) == n
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            per.append(e0.elapsed_time(e1))
    del keep
    return {"ms": per, "bytes": sum(b.n for b in blobs), "coef_bytes": n * count * 2}


def run_leg(leg, load):
    if leg == "pillow":
        r = leg_pillow(load)
    elif leg.startswith("huff_t"):
        r = leg_huff(load, int(leg[6:]))
    elif leg == "kernels":
        r = leg_kernels(load)
    elif leg == "coder":
        r = leg_coder(load)
    elif leg == "encode_gpu":
        r = leg_encode(load, 0, coder="device")
    else:
        r = leg_encode(load, int(leg[8:]))
    r.update(leg=leg, load=load)
    print(json.dumps(r), flush=True)


def fmt(runs):
    """median over all samples (per-process medians lo-hi; samples lo-hi, count)"""
    allv = [v for r in runs for v in r["ms"]]
    meds = [statistics.median(r["ms"]) for r in runs]
    return statistics.median(allv), f"{statistics.median(allv):.3f} (per-process medians {min(meds):.3f}-{max(meds):.3f}; samples {min(allv):.3f}-{max(allv):.3f}, {len(allv)} of them)"


def main():
    if a.leg:
        return run_leg(a.leg, a.load)
    res = {}
    legs = [leg for leg in LEGS if not a.legs or leg in a.legs.split(",")]
    for rnd in range(a.rounds):
        for load in LOADS:
            for leg in legs:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--load", load, "--steps", str(a.steps), "--warmup",
                                    str(a.warmup)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not line:
                    print(f"leg {leg} {load} failed ({p.returncode}): {p.stderr[-800:]}", flush=True)
                    if p.returncode in (124, 134, 137, 139, -6, -9, -11):
                        return 1                                               # a fault or a hang: start nothing more
                    continue
                print(line[-1], flush=True)
                res.setdefault((load, leg), []).append(json.loads(line[-1]))
    title = "Huffman coding on host threads" if "encode_gpu" not in legs else "Huffman coding on host threads or on the device"
    md = [f"# JPEG out: forward DCT on the device, {title}", "",
          f"`scripts/jpeg_enc_ab.py` on one MI355X, quality {QUALITY}, 4:2:0.  Every leg in a fresh process, the legs alternated over {a.rounds} "
          f"rounds, {a.steps} timed steps per process after {a.warmup} warm-up steps; figures are medians over all samples, in ms per BATCH.  "
          f"`os.cpu_count()` = {os.cpu_count()}; the library never uses more than 16 threads.  Nothing here is a gate.", ""]
    for load, (n, side) in LOADS.items():
        md += [f"## {n} x {side} x {side}", "", "| leg | ms per batch | per image | note |", "|---|---|---|---|"]
        names = {"pillow": "Pillow `save` per image, one core (CPU baseline)", "huff_t1": "`fh_jpeg_write` alone, 1 thread", "huff_t16": "`fh_jpeg_write` alone, 16 threads",
                 "kernels": "the two kernels (`fh_jpeg_forward_batch_dev`)", "encode_t16": "`fh_jpeg_encode_batch`, threads = 16", "encode_t1": "`fh_jpeg_encode_batch`, threads = 1",
                 "coder": "the device coder alone (`fh_jpeg_code_batch_dev`)", "encode_gpu": "`fh_jpeg_encode_batch_gpu`"}
        med = {}
        for leg in legs:
            runs = res.get((load, leg))
            if not runs:
                md.append(f"| {names[leg]} | not measured | | |")
                continue
            med[leg], text = fmt(runs)
            note = ""
            if leg == "kernels":
                fb = runs[0]["floor_bytes"]
                note = (f"floor {fb / 1e6:.1f} MB (pixels read, planes written + read, coefficients written) -> **{fb / med[leg] / 1e9:.2f} TB/s**; "
                        f"coefficients equal the host's: {all(r['equal_host'] for r in runs)}")
            elif "bytes" in runs[0]:
                note = f"{runs[0]['bytes'] / n / 1e3:.1f} kB per file"
                if leg == "coder":
                    note += f"; {runs[0]['coef_bytes'] / 1e6:.1f} MB of coefficients read twice; 2 stream synchronisations per call"
                if leg == "encode_gpu":
                    note += (f"; {runs[0]['bytes'] / 1e6:.1f} MB copied to the host against {runs[0]['coef_bytes'] / 1e6:.1f} MB of coefficients; "
                             f"3 stream synchronisations per call; files equal the host coder's: {all(r['equal_host'] for r in runs)}")
            md.append(f"| {names[leg]} | {text} | {med[leg] / n * 1e3:.1f} us | {note} |")
        if "pillow" in med and "encode_t16" in med:
            md += ["", f"Pillow loop / `fh_jpeg_encode_batch` (16 threads): **{med['pillow'] / med['encode_t16']:.1f}x**; "
                       f"(1 thread): {med['pillow'] / med['encode_t1']:.2f}x." if "encode_t1" in med else ""]
        if "encode_gpu" in med and "encode_t16" in med:
            t16 = [v for r in res[(load, "encode_t16")] for v in r["ms"]]
            md += ["", f"`fh_jpeg_encode_batch` (16 threads) / `fh_jpeg_encode_batch_gpu`, same rounds: **{med['encode_t16'] / med['encode_gpu']:.1f}x** "
                       f"({med['encode_t16']:.3f} ms against {med['encode_gpu']:.3f} ms; the 16-thread leg's own samples span {min(t16):.3f}-{max(t16):.3f} ms)."]
        md.append("")
    md += ["The kernels' figure is taken with events around the call, so it includes the descriptor-table copy.  `jpeg_dev.hip` is unchanged (the "
           "encoder keeps a private copy of `find_entry`), so `fh_jpeg_decode_batch` was not re-timed.", ""]
    with open(a.md, "w") as f:
        f.write("\n".join(md))
    print("wrote", a.md)
    return 0


if __name__ == "__main__":
    sys.exit(main())
