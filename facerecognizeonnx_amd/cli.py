"""Text-mode counterpart of the reference's demo executable (reference src/main.cpp:264-319):

    python -m facerecognizeonnx_amd.cli detect  <image>            [--det det.onnx] [--tile N --overlap M [--border B]] [--chips DIR [--rec rec.onnx] [--coder device]]
    python -m facerecognizeonnx_amd.cli compare <image1> <image2>  [--det det.onnx] [--rec rec.onnx] [--device-jpeg]
    python -m facerecognizeonnx_amd.cli simple  <image1> <image2>  [--rec rec.onnx]

Same flows as testDetection / testRecognition / testRecognitionSimple (main.cpp:39-199) — detect, take
faces[0] of each image, extractFeature, compareFaces, threshold 0.6 — but boxes / scores / similarity
are printed instead of drawn (no GUI, no webcam).  Images are read by the library's own cv::imread replacement
(fh_imread: JPEG / PNG / BMP / PPM -> BGR u8) or from `.npy` arrays of shape [rows, cols, 3] (BGR u8).
`detect --tile N` runs the tiled detection of large frames (whole frame + overlapping N x N tiles, one merged NMS; facehip.h).
`detect --chips DIR` also writes every detected face's aligned crop as DIR/<image>_<k>.jpg: the recogniser's alignment
(fh_rec_align_dev, so the recogniser model is loaded too) and the JPEG encoder's forward path run on the GPU, the Huffman coding on host
threads (fh_jpeg_encode_batch); with `--coder device` the Huffman coding runs on the GPU as well (fh_jpeg_encode_batch_gpu), the same bytes.
`compare --device-jpeg` reads both files through fh_pipeline_run_files: JPEGs are entropy-decoded on host threads and reconstructed on the
GPU (the same pixels), then detected and embedded in one call; without the flag nothing changes.
Model paths default to the reference's (models/det_500m.onnx, models/w600k_r50.onnx, main.cpp:269-270).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import api
from .api import FaceDetector, FaceRecognizer


def imread(path: str):
    if path.endswith(".npy"):
        return np.ascontiguousarray(np.load(path), np.uint8)
    return api.imread(path)


def compare_files(det, rec, a) -> int:
    """compare (main.cpp:67-134) with the files decoded, detected and embedded by one fh_pipeline_run_files call: faces[0] of each."""
    if len(a.images) < 2:
        print("need two images", file=sys.stderr)
        return -1
    faces, frame_of, emb, status = api.pipeline_files(det, rec, a.images[:2], faces_per_frame=1, scoreThreshold=a.score, nmsThreshold=a.nms)
    for p, st in zip(a.images, status):
        if st < 0:
            print(f"Cannot read image: {p}", file=sys.stderr)                   # main.cpp:43-46
            return -1
    n1, n2 = int(np.count_nonzero(frame_of == 0)), int(np.count_nonzero(frame_of == 1))
    print(f"Image 1: {n1} faces, Image 2: {n2} faces (the first of each)")
    if not n1 or not n2:
        print("No face detected in one of the images")
        return -1
    e1, e2 = emb[int(np.flatnonzero(frame_of == 0)[0])], emb[int(np.flatnonzero(frame_of == 1)[0])]
    print(f"Feature dimension: {e1.size}")
    sim = rec.compareFaces(e1, e2)
    print(f"Similarity: {sim:.6f}")
    print("Same person" if sim > 0.6 else "Different person")                  # main.cpp:118
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="facerecognizeonnx_amd.cli")
    ap.add_argument("mode", choices=["detect", "compare", "simple"])
    ap.add_argument("images", nargs="+")
    ap.add_argument("--det", default="models/det_500m.onnx")
    ap.add_argument("--rec", default="models/w600k_r50.onnx")
    ap.add_argument("--score", type=float, default=0.5)
    ap.add_argument("--nms", type=float, default=0.4)
    ap.add_argument("--tile", type=int, default=0, help="detect: tile side in pixels (0 = plain detection)")
    ap.add_argument("--overlap", type=int, default=0, help="detect --tile: overlap of neighbouring tiles in pixels")
    ap.add_argument("--border", type=int, default=2, help="detect --tile: drop boxes within this many pixels of an interior tile edge (< 0: off)")
    ap.add_argument("--chips", default=None, metavar="DIR", help="detect: write every face's aligned crop as DIR/<image>_<k>.jpg")
    ap.add_argument("--chip-quality", type=int, default=95, help="detect --chips: JPEG quality")
    ap.add_argument("--coder", choices=["host", "device"], default="host", help="detect --chips: where the Huffman coding runs")
    ap.add_argument("--device-jpeg", action="store_true", help="compare: decode the files through fh_pipeline_run_files (JPEG reconstruction on the GPU)")
    a = ap.parse_args(argv)
    det, rec = FaceDetector(), FaceRecognizer()
    if a.mode != "simple" and not det.loadModel(a.det):
        print("Failed to load face detector model", file=sys.stderr)           # main.cpp:274-278
        return -1
    if a.chips is not None and a.mode != "detect":
        print("--chips applies to detect", file=sys.stderr)
        return -1
    if (a.mode != "detect" or a.chips is not None) and not rec.loadModel(a.rec):
        print("Failed to load face recognizer model", file=sys.stderr)         # main.cpp:280-284
        return -1
    if a.device_jpeg:
        if a.mode != "compare" or any(p.endswith(".npy") for p in a.images):
            print("--device-jpeg applies to compare on image files", file=sys.stderr)
            return -1
        return compare_files(det, rec, a)
    imgs = [imread(p) for p in a.images]
    for p, im in zip(a.images, imgs):
        if im is None:
            print(f"Cannot read image: {p}", file=sys.stderr)                   # main.cpp:43-46
            return -1
    if a.mode == "detect":                                                     # main.cpp:39-65
        if a.tile > 0:
            recs = det.detect_tiled_records(imgs[0], api.Tiling(a.tile, a.overlap, a.border), a.score, a.nms)
            faces = [api.FaceBox.from_record(r) for r in recs]
        else:
            faces = det.detect(imgs[0], a.score, a.nms)
        print(f"Detected {len(faces)} faces")
        for i, f in enumerate(faces):
            print(f"Face {i}: box={f.box} score={f.score:.4f} landmarks={np.round(f.landmarks, 1).tolist()}")
        if a.chips is not None and faces:
            os.makedirs(a.chips, exist_ok=True)
            files, _ = api.face_chips(rec, imgs[0], np.concatenate([f.to_record() for f in faces]), quality=a.chip_quality,
                                      coder=a.coder)
            stem = os.path.splitext(os.path.basename(a.images[0]))[0]
            for k, data in enumerate(files):
                if data is None:
                    continue
                path = os.path.join(a.chips, f"{stem}_{k}.jpg")
                with open(path, "wb") as fp:
                    fp.write(data)
                print(f"Chip {k}: {path} ({len(data)} bytes)")
        return 0
    if len(imgs) < 2:
        print("need two images", file=sys.stderr)
        return -1
    if a.mode == "compare":                                                    # main.cpp:67-134
        f1s, f2s = det.detect(imgs[0], a.score, a.nms), det.detect(imgs[1], a.score, a.nms)
        print(f"Image 1: {len(f1s)} faces, Image 2: {len(f2s)} faces")
        if not f1s or not f2s:
            print("No face detected in one of the images")
            return -1
        e1, e2 = rec.extractFeature(imgs[0], f1s[0]), rec.extractFeature(imgs[1], f2s[0])
    else:                                                                      # main.cpp:136-199
        e1, e2 = rec.extractFeatureSimple(imgs[0]), rec.extractFeatureSimple(imgs[1])
    if e1.size == 0 or e2.size == 0:
        print("Feature extraction failed")
        return -1
    print(f"Feature dimension: {e1.size}")
    sim = rec.compareFaces(e1, e2)
    print(f"Similarity: {sim:.6f}")
    print("Same person" if sim > 0.6 else "Different person")                  # main.cpp:118
    return 0


if __name__ == "__main__":
    sys.exit(main())
