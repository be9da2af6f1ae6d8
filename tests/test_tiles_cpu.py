"""The tile plan of tiled detection on the host (include/facehip.h: fh_tile_plan; csrc/tile_plan.h), no GPU: against the numpy model
(tests/tile_model.py), its properties, its argument errors, and the plan function under AddressSanitizer + UndefinedBehaviorSanitizer
as a stand-alone program (tests/native/tile_plan_sanitize.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import tile_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILINGS = [(128, 128, 32), (64, 96, 16), (128, 128, 0)]          # (tile_w, tile_h, overlap)


def _sizes(tile, overlap):
    """1..300 on a fixed grid, plus the values around each multiple of the stride and around the tile size."""
    s = set(range(1, 301, 7)) | {1, 2, 299, 300}
    for k in range(0, 300 // (tile - overlap) + 2):
        for base in (k * (tile - overlap), tile + k * (tile - overlap)):
            s |= {base - 1, base, base + 1}
    return sorted(v for v in s if 1 <= v <= 300)


def _plan(rows, cols, tw, th, ov, border=2):
    return fa.tile_plan(rows, cols, (tw, th), ov, border)


@pytest.mark.parametrize("tw,th,ov", TILINGS)
def test_plan_equals_the_model(tw, th, ov):
    n = 0
    for rows in _sizes(th, ov):
        for cols in _sizes(tw, ov):
            assert _plan(rows, cols, tw, th, ov) == tile_model.plan(rows, cols, tw, th, ov), (rows, cols)
            n += 1
    assert n > 2000


@pytest.mark.parametrize("tw,th,ov", TILINGS)
def test_plan_properties(tw, th, ov):
    for rows in _sizes(th, ov)[::3]:
        for cols in _sizes(tw, ov)[::3]:
            views = _plan(rows, cols, tw, th, ov)
            assert views[0] == (0, 0, cols, rows, 0)
            fits = cols <= tw and rows <= th
            assert (len(views) == 1) == fits, (rows, cols)                        # a frame that fits has exactly one view
            if fits:
                continue
            cover = np.zeros((rows, cols), bool)
            for x, y, w, h, edges in views[1:]:
                assert 0 <= x and 0 <= y and x + w <= cols and y + h <= rows and w == min(tw, cols) and h == min(th, rows)
                assert edges == ((x > 0) | (y > 0) << 1 | (x + w < cols) << 2 | (y + h < rows) << 3)
                cover[y:y + h, x:x + w] = True
            assert cover.all(), (rows, cols)
            xs = sorted({v[0] for v in views[1:]}); ys = sorted({v[1] for v in views[1:]})
            assert len(views) == 1 + len(xs) * len(ys)
            assert [(v[0], v[1]) for v in views[1:]] == [(x, y) for y in ys for x in xs]      # row-major
            assert all(a + min(tw, cols) - b >= ov and b > a for a, b in zip(xs, xs[1:]))   # neighbours overlap by at least `overlap`
            assert all(a + min(th, rows) - b >= ov and b > a for a, b in zip(ys, ys[1:]))


def test_named_frames():
    assert len(_plan(128, 128, 128, 128, 32)) == 1 and len(_plan(100, 90, 128, 128, 32)) == 1
    assert _plan(129, 128, 128, 128, 32) == [(0, 0, 128, 129, 0), (0, 0, 128, 128, 8), (0, 1, 128, 128, 2)]     # tiles one pixel apart
    assert len(_plan(300, 200, 128, 128, 32)) == 7 and len(_plan(128, 400, 128, 128, 32)) == 5
    v = _plan(64, 500, 128, 128, 32)
    assert all(t[3] == 64 and not t[4] & 10 for t in v[1:])                     # tiles 64 high: no interior top / bottom edge
    assert len(_plan(1, 2000, 128, 128, 32)) == 22
    assert _plan(0, 100, 128, 128, 32) == [] and _plan(100, -1, 128, 128, 32) == []           # an empty image has no views


def test_argument_errors_and_cap():
    L = fa.lib()

    def raw(rows, cols, t, views=None, cap=0):
        return L.fh_tile_plan(rows, cols, C.byref(t) if t is not None else None, views, cap)

    for tw, th, ov in ((15, 128, 0), (128, 15, 0), (128, 128, -1), (128, 64, 64), (64, 128, 64), (16, 16, 16)):
        assert raw(300, 300, fa.Tiling((tw, th), ov, 2)) == -1, (tw, th, ov)      # FH_ERR_ARG
        assert "tiling" in _lib.last_error()
    assert raw(300, 300, None) == -1
    assert raw(300, 300, fa.Tiling((16, 16), 15, -5)) > 1                        # the smallest legal tile; border < 0 is legal
    t = fa.Tiling(128, 32, 2)
    n = raw(300, 200, t)                                                         # views == NULL only counts
    assert n == 7
    views = (_lib.FhView * (n + 1))()
    views[n].x = 12345
    assert raw(300, 200, t, views, n - 1) == -1 and views[0].w == 0              # cap too small: rejected, nothing written
    assert raw(300, 200, t, views, n) == n and views[n].x == 12345 and views[n - 1].w == 128
    assert raw(300, 200, t, views, 0) == -1 and raw(300, 200, t, views, -4) == -1


def test_tiling_helper_defaults():
    t = fa.Tiling(640, 128)
    assert (t.tile_w, t.tile_h, t.overlap, t.border) == (640, 640, 128, 2)
    t = fa.Tiling((320, 640), 64, -1)
    assert (t.tile_w, t.tile_h, t.overlap, t.border) == (320, 640, 64, -1)


@pytest.mark.timeout(300)
def test_tile_plan_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "tile_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "native", "tile_plan_sanitize.cpp")]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]
