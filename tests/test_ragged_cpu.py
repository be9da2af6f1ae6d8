"""Host side of the mixed-size frame batches (include/facehip.h: fh_frame, fh_letterbox_plan, fh_*_ragged_dev,
fh_pipeline_run_images): the letterbox plan against numpy float32 arithmetic and the oracle's preprocess, the argument errors of every
new entry point (no GPU is touched: every call below fails on its arguments first), the bindings and the descriptor's size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("fh_letterbox_plan", "fh_det_letterbox_ragged_dev", "fh_det_run_network_ragged_dev", "fh_det_detect_ragged_dev",
               "fh_rec_align_ragged_dev", "fh_rec_embed_faces_ragged_dev", "fh_pipeline_run_ragged_dev", "fh_pipeline_run_images")
HAND_PICKED = ((128, 128), (256, 256), (1, 1), (1, 2000), (2000, 1), (640, 639), (639, 640))


def _plan(rows, cols, in_w, in_h):
    nw, nh, sc = C.c_int(-7), C.c_int(-7), C.c_float(-7.0)
    live = fa.lib().fh_letterbox_plan(rows, cols, in_w, in_h, C.byref(nw), C.byref(nh), C.byref(sc))
    return live, nw.value, nh.value, np.float32(sc.value)


def _numpy_plan(rows, cols, in_w, in_h):
    """face_detector.cpp:101-106 in numpy float32: every operation rounds to float, as the C++ does."""
    sw = np.float32(in_w) / np.float32(cols)
    sh = np.float32(in_h) / np.float32(rows)
    sc = min(sw, sh)
    return int(np.float32(cols) * sc), int(np.float32(rows) * sc), np.float32(sc)


@pytest.mark.parametrize("inp", [128, 640])
def test_letterbox_plan_equals_float32_arithmetic_and_the_oracle(inp):
    rng = np.random.default_rng(1000 + inp)
    shapes = [tuple(int(v) for v in rng.integers(1, 4001, 2)) for _ in range(300)] + list(HAND_PICKED)
    dead = 0
    for rows, cols in shapes:
        live, nw, nh, sc = _plan(rows, cols, inp, inp)
        enw, enh, esc = _numpy_plan(rows, cols, inp, inp)
        elive = enw > 0 and enh > 0
        assert live == int(elive), (rows, cols)
        # the oracle's preprocess (its own C restatement of :94-113) on an image of that size: same liveness, same scale bits
        ref, oscale = oracle.det_preprocess(np.zeros((rows, cols, 3), np.uint8), inp, inp)
        assert (ref is not None) == elive, (rows, cols)
        if elive:
            assert (nw, nh) == (enw, enh), (rows, cols, nw, nh, enw, enh)
            assert sc.tobytes() == esc.tobytes() == np.float32(oscale).tobytes(), (rows, cols, sc, esc, oscale)
            assert 0 < nw <= inp and 0 < nh <= inp
        else:
            dead += 1
            assert (nw, nh) == (0, 0) and sc.tobytes() == np.float32(0).tobytes(), (rows, cols)
    assert _plan(1, 2000, inp, inp)[0] == 0 and _plan(2000, 1, inp, inp)[0] == 0 and dead >= 2      # new_h == 0 / new_w == 0
    assert _plan(inp, inp, inp, inp) == (1, inp, inp, np.float32(1))                                 # the copy branch's plan
    assert _plan(2 * inp, 2 * inp, inp, inp) == (1, inp, inp, np.float32(0.5))                       # the exact-2x branch's plan


def test_letterbox_plan_of_empty_frames_and_null_outputs():
    for rows, cols in ((0, 0), (0, 10), (10, 0), (-1, 5), (5, -3)):
        assert _plan(rows, cols, 640, 640) == (0, 0, 0, np.float32(0)), (rows, cols)
    L = fa.lib()
    assert L.fh_letterbox_plan(100, 180, 128, 128, None, None, None) == 1 and L.fh_letterbox_plan(0, 0, 128, 128, None, None, None) == 0
    # the Python mirror
    assert fa.letterbox_plan(100, 180, 128, 128) == (True,) + _numpy_plan(100, 180, 128, 128)[:2] + (float(_numpy_plan(100, 180, 128, 128)[2]),)
    assert fa.letterbox_plan(1, 2000, 128, 128) == (False, 0, 0, 0.0)


def test_fh_frame_is_24_bytes():
    assert C.sizeof(_lib.FhFrame) == 24
    assert (_lib.FhFrame.bgr.offset, _lib.FhFrame.rows.offset, _lib.FhFrame.cols.offset, _lib.FhFrame.step.offset) == (0, 8, 12, 16)
    arr = fa.frame_array([(4096, 10, 20), None, (8192, 3, 5, 17), (0, 4, 4)])
    assert [(f.bgr, f.rows, f.cols, f.step) for f in arr] == [(4096, 10, 20, 60), (None, 0, 0, 0), (8192, 3, 5, 17), (None, 4, 4, 12)]
    assert fa.frame_array(arr) is arr


def test_every_new_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "facehip.h")).read()
    declared = set(re.findall(r"FH_API\s+[\w\s\*]+?\b(fh_\w+)\s*\(", hdr))          # the means test_host_cpu.py uses
    L = fa.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(L, name), name
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    assert re.search(r"typedef struct fh_frame \{ const uint8_t\* bgr; int32_t rows, cols, step; \} fh_frame;", hdr)


def test_ragged_entry_points_reject_bad_arguments_before_touching_a_device():
    L = fa.lib()
    one = C.c_void_p(16)                                       # a non-null token: every call below must fail on its arguments first
    ok1 = fa.frame_array([(4096, 8, 8)])
    short = fa.frame_array([(4096, 8, 8), (4096, 8, 8, 23)])   # step < cols * 3 on a live frame
    empty_short = fa.frame_array([(0, 8, 8, 1)])               # ... is no error on an EMPTY frame (checked where no GPU is needed: below)
    calls = {
        "fh_det_letterbox_ragged_dev": lambda h, fr, n: L.fh_det_letterbox_ragged_dev(h, fr, n, one, None),
        "fh_det_run_network_ragged_dev": lambda h, fr, n: L.fh_det_run_network_ragged_dev(h, fr, n, None),
        "fh_det_detect_ragged_dev": lambda h, fr, n: L.fh_det_detect_ragged_dev(h, fr, n, 0.5, 0.4, one, 4, one, None),
        "fh_rec_align_ragged_dev": lambda h, fr, n: L.fh_rec_align_ragged_dev(h, fr, n, one, None, 1, one, one, None),
        "fh_rec_embed_faces_ragged_dev": lambda h, fr, n: L.fh_rec_embed_faces_ragged_dev(h, fr, n, one, None, 1, one, None, None),
        "fh_pipeline_run_ragged_dev": lambda h, fr, n: L.fh_pipeline_run_ragged_dev(h, h, fr, n, 0.5, 0.4, 1, one, one, one, None),
        "fh_pipeline_run_images": lambda h, fr, n: L.fh_pipeline_run_images(h, h, fr, n, 0.5, 0.4, 1, one, one, one, 4),
    }
    assert set(calls) | {"fh_letterbox_plan"} == set(NEW_SYMBOLS)
    for name, call in calls.items():
        for what, args in (("null handle", (None, ok1, 1)), ("n = 0", (one, ok1, 0)), ("n = 4097", (one, ok1, 4097)),
                           ("null descriptors", (one, None, 1)), ("short step", (one, short, 2))):
            assert L.fh_det_num_anchors(None) == -1            # (leaves ITS message, so a stale one cannot pass below)
            assert call(*args) == -1, (name, what)             # FH_ERR_ARG
            msg = _lib.last_error()
            assert msg.startswith(name + ":") and len(msg) > len(name) + 2, (name, what, msg)
    # the pipeline entry points need BOTH handles
    assert L.fh_pipeline_run_ragged_dev(one, None, ok1, 1, 0.5, 0.4, 1, one, one, one, None) == -1
    assert L.fh_pipeline_run_images(None, one, ok1, 1, 0.5, 0.4, 1, one, one, one, 4) == -1
    # sizes of their own
    assert L.fh_det_detect_ragged_dev(one, ok1, 1, 0.5, 0.4, one, 0, one, None) == -1                 # max_per_frame
    assert L.fh_pipeline_run_ragged_dev(one, one, ok1, 1, 0.5, 0.4, 0, one, one, one, None) == -1     # faces_per_frame
    assert L.fh_pipeline_run_images(one, one, ok1, 1, 0.5, 0.4, 1, one, one, one, -1) == -1           # cap
    assert L.fh_rec_align_ragged_dev(one, ok1, 1, one, None, 2, one, one, None) == -1                 # identity mapping: n <= n_frames
    assert L.fh_det_letterbox_ragged_dev(one, ok1, 1, C.c_void_p(18), None) == -1 and "aligned" in _lib.last_error()
    # a batch of only empty images is no error and needs no device: zero faces (face_detector.cpp:148-156)
    assert L.fh_pipeline_run_images(one, one, empty_short, 1, 0.5, 0.4, 1, one, one, one, 4) == 0
    assert L.fh_pipeline_run_images(one, one, fa.frame_array([None, None, (0, 0, 0)]), 3, 0.5, 0.4, 2, None, None, None, 0) == 0
