"""Shared helpers for the test-suite (model builders, seeded inputs)."""
from __future__ import annotations

import os

import numpy as np

from facerecognizeonnx_amd.synth import models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tiny_iresnet(d, fold_bn=True, seed=1):
    return models.make_iresnet(os.path.join(d, f"r_tiny_{int(fold_bn)}_{seed}.onnx"), (1, 2, 1, 1), (8, 16, 32, 64),
                               112, 512, seed=seed, fold_bn=fold_bn)


def tiny_mbf(d, fold_bn=True, seed=3):
    """MobileFaceNet with 16 base channels: every op kind of the full w600k_mbf graph (grouped 3x3, depthwise + PReLU, GDC, MatMul)."""
    return models.make_mobilefacenet(os.path.join(d, f"m_tiny_{int(fold_bn)}_{seed}.onnx"), (1, 2, 2, 1), 16, 112, 128, seed=seed,
                                     fold_bn=fold_bn)


def tiny_scrfd(d, hw=None, seed=2, cls_bias=-2.0):
    return models.make_scrfd(os.path.join(d, f"s_tiny_{hw}_{seed}.onnx"), (1, 2, 1, 2), (8, 8, 16, 24, 32, 48), 8, 16,
                             seed=seed, cls_bias=cls_bias, static_hw=hw)


def frames_u8(n, rows, cols, seed=0, smooth=False):
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    out = np.empty((n, rows, cols, 3), np.uint8)
    for i in range(n):
        img = np.zeros((rows, cols, 3), np.float32)
        for c in range(3):
            img[..., c] = 128 + 60 * np.sin(xx * rng.uniform(.02, .2) + rng.uniform(0, 6)) * np.cos(yy * rng.uniform(.02, .2))
        for _ in range(6):
            cx, cy, r = rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(4, min(rows, cols) / 4)
            img += rng.uniform(-80, 80, 3) * np.exp(-(((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r)))[..., None]
        out[i] = np.clip(img + rng.normal(0, 3, img.shape), 0, 255).astype(np.uint8)
    return out


TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366],
                     [41.5493, 92.3655], [70.7299, 92.2041]], np.float32)


def random_landmarks(n, rows, cols, seed=3, jitter=1.0):
    """Template x random similarity (scale U(1,4), rot U(-30,30) deg, shift inside the frame) + N(0,jitter) px."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 5, 2), np.float32)
    for i in range(n):
        s = rng.uniform(1, 4); th = np.deg2rad(rng.uniform(-30, 30))
        R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        t = np.array([rng.uniform(0, max(1, cols - 112 * s)), rng.uniform(0, max(1, rows - 112 * s))])
        out[i] = (TEMPLATE @ R.T + t + rng.normal(0, jitter, (5, 2))).astype(np.float32)
    return out


def write_ppm(path, bgr):
    """Binary PPM (P6, RGB order) of a BGR u8 image."""
    h, w, _ = bgr.shape
    with open(path, "wb") as f:
        f.write(f"P6\n{w} {h}\n255\n".encode())
        f.write(np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())


def write_bmp(path, bgr):
    """24-bit bottom-up BMP of a BGR u8 image."""
    import struct
    h, w, _ = bgr.shape
    stride = (w * 3 + 3) & ~3
    rows = b"".join(bgr[y].tobytes() + b"\0" * (stride - w * 3) for y in range(h - 1, -1, -1))
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", 54 + len(rows), 0, 0, 54))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(rows), 2835, 2835, 0, 0))
        f.write(rows)


def match_records(got, ref, box_tol=1, lm_tol=1e-2, score_tol=1e-4):
    """Pair EVERY record of `ref` (oracle) with one of `got` (GPU): score within `score_tol`, box within `box_tol` px (a 1e-6 network
    difference may flip an int truncation, face_detector.cpp:255-265), landmarks within `lm_tol` px.  Returns the index lists
    (unmatched ref, unmatched got)."""
    used = np.zeros(len(got), bool)
    missing = []
    for i, r in enumerate(ref):
        near = np.where(~used & (np.abs(got["score"] - r["score"]) < score_tol))[0]
        ok = [j for j in near if max(abs(int(got[j][k]) - int(r[k])) for k in ("x", "y", "w", "h")) <= box_tol and
              np.abs(got[j]["lm"] - r["lm"]).max() < lm_tol]
        if ok:
            used[ok[0]] = True
        else:
            missing.append(i)
    return missing, [int(j) for j in np.where(~used)[0]]


def _iou_int(a, b):
    """FaceDetector::iou (face_detector.cpp:340-354): integer intersection, int denominator."""
    x1 = max(int(a["x"]), int(b["x"])); y1 = max(int(a["y"]), int(b["y"]))
    x2 = min(int(a["x"]) + int(a["w"]), int(b["x"]) + int(b["w"])); y2 = min(int(a["y"]) + int(a["h"]), int(b["y"]) + int(b["h"]))
    inter = max(0, x2 - x1) * max(0, y2 - y1)
    den = int(a["w"]) * int(a["h"]) + int(b["w"]) * int(b["h"]) - inter
    return inter / den if den else float("nan")


def assert_records_equivalent(got, ref, score_thr, nms_thr, box_tol=1, lm_tol=1e-2, max_unexplained=0):
    """All records, not a prefix: every oracle record has a GPU counterpart and vice versa.  A record may be unmatched only where a
    ~1e-6 difference of the network outputs can legitimately change the decision: its score lies within 1e-4 of the score threshold
    (strict `>`, face_detector.cpp:253), or its integer IoU with a better-scored record of EITHER list lies within 0.02 of the NMS
    threshold (a +-1 px truncation flip moves the IoU of a small box across the strict `>` of face_detector.cpp:369-371)."""
    missing, surplus = match_records(got, ref, box_tol, lm_tol)
    unexplained = []
    both = list(got) + list(ref)
    for side, idx, arr in (("ref", missing, ref), ("gpu", surplus, got)):
        for i in idx:
            r = arr[i]
            if abs(float(r["score"]) - score_thr) < 1e-4:
                continue
            ious = [_iou_int(r, o) for o in both if float(o["score"]) >= float(r["score"]) - 1e-4]
            if any(abs(v - nms_thr) < 0.02 for v in ious if v == v):
                continue
            unexplained.append((side, i, float(r["score"]), [int(r[k]) for k in ("x", "y", "w", "h")]))
    assert len(unexplained) <= max_unexplained, (len(got), len(ref), unexplained[:8])
    return len(missing), len(surplus)


def dwpw_graph(path, H, W, Cc, Cout, ds, stem_stride=1):
    """input [1,3,H,W] -> Conv3x3(3 -> Cc) stride `stem_stride` +ReLU -> depthwise 3x3 stride `ds` +ReLU -> pointwise 1x1 (Cc -> Cout)+ReLU
    -> [H'W', Cout]"""
    from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder
    rng = np.random.default_rng(H * 100 + Cc)
    b = OnnxBuilder("dwpw")
    x = b.add_input("input", [1, 3, H, W])
    def conv(x, w, bias, relu=True, **kw):
        y = b.node("Conv", [x, b.init(b.uid("w"), w.astype(np.float32)), b.init(b.uid("b"), bias.astype(np.float32))], **kw)
        return b.node("Relu", [y]) if relu else y
    y = conv(x, rng.standard_normal((Cc, 3, 3, 3)) / 5, rng.standard_normal(Cc) / 10, kernel_shape=[3, 3], pads=[1, 1, 1, 1],
             strides=[stem_stride, stem_stride])
    y = conv(y, rng.standard_normal((Cc, 1, 3, 3)) / 3, rng.standard_normal(Cc) / 10, kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[ds, ds], group=Cc)
    y = conv(y, rng.standard_normal((Cout, Cc, 1, 1)) / np.sqrt(Cc), rng.standard_normal(Cout) / 10, kernel_shape=[1, 1], strides=[1, 1])
    y = b.node("Transpose", [y], perm=[0, 2, 3, 1])
    b.node("Reshape", [y, b.init("shape", np.array([-1, Cout], np.int64))], outputs=["out"])
    b.add_output("out", ["A", Cout])
    return b.save(path)


def dw_graph(path, H, W, CH, stride, act, seed):
    """input [1,3,H,W] -> Conv3x3(3 -> CH)+ReLU -> depthwise 3x3 stride `stride` (+act) -> depthwise 3x3 stride 1 (+act) -> [H'W', CH]"""
    from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder
    rng = np.random.default_rng(seed)
    b = OnnxBuilder("dw")
    x = b.add_input("input.1", [1, 3, H, W])

    def conv(x, cin, cout, stride, tag, group=1):
        w = (rng.standard_normal((cout, cin // group, 3, 3)) * (0.6 / np.sqrt(9 * cin // group))).astype(np.float32)
        bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        return b.node("Conv", [x, b.init(f"{tag}.w", w), b.init(f"{tag}.b", bias)], kernel_shape=[3, 3], strides=[stride, stride],
                      pads=[1, 1, 1, 1], dilations=[1, 1], group=group)

    def activation(x, tag):
        if act == "relu":
            return b.node("Relu", [x])
        if act == "prelu":
            return b.node("PRelu", [x, b.init(f"{tag}.slope", (0.25 * rng.uniform(0.5, 1.5, (CH, 1, 1))).astype(np.float32))])
        return x

    x = b.node("Relu", [conv(x, 3, CH, 1, "stem")])
    x = activation(conv(x, CH, CH, stride, "dw1", group=CH), "a1")
    x = activation(conv(x, CH, CH, 1, "dw2", group=CH), "a2")
    x = b.node("Transpose", [x], perm=[0, 2, 3, 1])
    b.node("Reshape", [x, b.init("shape", np.array([-1, CH], np.int64))], outputs=["out"])
    b.add_output("out", ["A", CH])
    return b.save(path)


def halo_graph(path, H, W, Cin, Cout, res):
    """input [1,3,H,W] -> stem Conv3x3(3 -> Cin)+ReLU -> [3x3 (Cin -> Cout) (-> ReLU), or + a 1x1 projection of the stem map] -> [HW, Cout]"""
    from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder
    rng = np.random.default_rng(H * 100 + Cin + Cout)
    b = OnnxBuilder("halo")
    x = b.add_input("input", [1, 3, H, W])
    def conv(x, cout, cin, k, relu):
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
        y = b.node("Conv", [x, b.init(b.uid("w"), w), b.init(b.uid("b"), (rng.standard_normal(cout) / 10).astype(np.float32))],
                   kernel_shape=[k, k], pads=[k // 2] * 4, strides=[1, 1])
        return b.node("Relu", [y]) if relu else y
    y0 = conv(x, Cin, 3, 3, True)
    if res:                                                  # the residual must have Cout channels: a 1x1 projection of the stem map
        side = conv(y0, Cout, Cin, 1, False)
        y = b.node("Add", [conv(y0, Cout, Cin, 3, False), side])
    else:
        y = conv(y0, Cout, Cin, 3, True)
    y = b.node("Transpose", [y], perm=[0, 2, 3, 1])
    b.node("Reshape", [y, b.init("shape", np.array([-1, Cout], np.int64))], outputs=["out"])
    b.add_output("out", ["A", Cout])
    return b.save(path)


def stem_graph(path, H, W, C, stride, act, bn, seed):
    """input [1,3,H,W] -> y = Conv3x3(3 -> C) stride `stride` (+ReLU | +PReLU | nothing) -> depthwise 3x3 of y, or (bn) of
    BatchNormalization(y) with y added back, so that the stem's plain map, its affine second output, s2 / t2 and the slope are all live
    -> [H'W', C]"""
    from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder
    rng = np.random.default_rng(seed)
    b = OnnxBuilder("stem")
    x = b.add_input("input.1", [1, 3, H, W])
    y = b.node("Conv", [x, b.init("stem.w", (rng.standard_normal((C, 3, 3, 3)) / 5).astype(np.float32)),
                        b.init("stem.b", (rng.standard_normal(C) / 10).astype(np.float32))],
               kernel_shape=[3, 3], strides=[stride, stride], pads=[1, 1, 1, 1], dilations=[1, 1], group=1)
    if act == "relu":
        y = b.node("Relu", [y])
    elif act == "prelu":
        y = b.node("PRelu", [y, b.init("stem.slope", (0.25 * rng.uniform(0.5, 1.5, (C, 1, 1))).astype(np.float32))])
    z = y
    if bn:
        z = b.node("BatchNormalization", [y, b.init("bn.weight", rng.uniform(0.5, 1.5, C).astype(np.float32)),
                                          b.init("bn.bias", (rng.standard_normal(C) / 10).astype(np.float32)),
                                          b.init("bn.running_mean", (rng.standard_normal(C) / 10).astype(np.float32)),
                                          b.init("bn.running_var", rng.uniform(0.5, 1.5, C).astype(np.float32))], epsilon=1e-5, momentum=0.9)
    z = b.node("Conv", [z, b.init("dw.w", (rng.standard_normal((C, 1, 3, 3)) / 3).astype(np.float32)),
                        b.init("dw.b", (rng.standard_normal(C) / 10).astype(np.float32))],
               kernel_shape=[3, 3], strides=[1, 1], pads=[1, 1, 1, 1], dilations=[1, 1], group=C)
    if bn:
        z = b.node("Add", [z, y])
    z = b.node("Transpose", [z], perm=[0, 2, 3, 1])
    b.node("Reshape", [z, b.init("shape", np.array([-1, C], np.int64))], outputs=["out"])
    b.add_output("out", ["A", C])
    return b.save(path)
