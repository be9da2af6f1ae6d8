"""The host half of the JPEG split (include/facehip.h "JPEG in two halves", csrc/image_io.cpp): fh_jpeg_header / fh_jpeg_entropy /
fh_jpeg_reconstruct / fh_jpeg_desc_check.  fh_jpeg_entropy + fh_jpeg_reconstruct must give the committed (Pillow) pixels of every JPEG
fixture, write nothing outside coef[0 .. coef_count) and the pixel rows, and the validator must refuse every malformed field before any
reconstruction — host or device — indexes with it.  No GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import jpeg_split as js

EXPECTED = np.load(os.path.join(js.HERE, "golden", "images_expected.npz"))
with open(os.path.join(js.HERE, "golden", "images_sha256.json")) as _f:
    SHA256 = json.load(_f)
FH_ERR_ARG = -1


def test_descriptor_layout():
    assert C.sizeof(_lib.FhJpegComp) == 160 and C.sizeof(_lib.FhJpegDesc) == 528 and C.sizeof(_lib.FhBlob) == 16
    assert _lib.FhJpegDesc.coef_count.offset == 40 and _lib.FhJpegDesc.comp.offset == 48
    assert _lib.FhJpegComp.coef_off.offset == 24 and _lib.FhJpegComp.quant.offset == 32


@pytest.mark.parametrize("name", js.JPEGS)
def test_entropy_then_reconstruct_equals_the_fixture(name):
    data = js.read(name)
    rc, d, coef = js.entropy(data, guard=64)
    assert rc == 0, _lib.last_error()
    assert fa.lib().fh_jpeg_desc_check(C.byref(d)) == 0, _lib.last_error()
    n = int(d.coef_count)
    assert np.all(coef[n:].view(np.uint16) == 0x5A5A)                       # the guard band behind coef_count
    got = js.picture(d, coef[:n])
    if name in EXPECTED.files:
        exp = EXPECTED[name]
        assert got.shape == exp.shape and np.array_equal(got, exp)
    else:                                                                     # (the 640 x 640 photograph is pinned by its digest)
        assert hashlib.sha256(got.tobytes()).hexdigest() == SHA256[name]
    # the header alone: same sizes, same block grids, same coef_count
    h = js.header(data)
    assert h is not None
    for k in ("width", "height", "rows", "cols", "ncomp", "hmax", "vmax", "orientation", "coef_count", "color"):
        assert getattr(h, k) == getattr(d, k), k
    for i in range(d.ncomp):
        for k in ("h", "v", "wblocks", "hblocks", "dw", "dh", "coef_off"):
            assert getattr(h.comp[i], k) == getattr(d.comp[i], k), (i, k)
        assert any(d.comp[i].quant) and d.comp[i].coef_off % 64 == 0
    assert sum(d.comp[i].wblocks * d.comp[i].hblocks * 64 for i in range(d.ncomp)) == n


def test_the_fixtures_cover_the_paths():
    seen = set()
    for name in js.JPEGS:
        d = js.header(js.read(name))
        seen.add((d.ncomp, d.hmax, d.vmax, d.orientation, d.comp[d.ncomp - 1].dw <= 2))
    assert {o for _, _, _, o, _ in seen} == set(range(1, 9))
    # (the other sampling ratios — 4:1:1, h1v2, 4 x 4 — have no fixture: test_hand_made_descriptors_reconstruct, tests/test_gpu_jpeg.py)
    assert {(1, 1, 1), (3, 2, 2), (3, 2, 1), (3, 1, 1)} <= {(n, h, v) for n, h, v, _, _ in seen}
    assert {small for _, _, _, _, small in seen} == {False, True}


def test_cap_one_short_is_an_error_and_writes_nothing_behind_cap():
    data = js.read("j420_q75_odd.jpg")
    n = int(js.header(data).coef_count)
    rc, _, coef = js.entropy(data, cap=n - 1, guard=8)
    assert rc != 0 and "too small" in _lib.last_error()
    assert np.all(coef.view(np.uint16) == 0x5A5A)                            # refused before the first write
    rc, _, coef = js.entropy(data, cap=n, guard=8)
    assert rc == 0 and np.all(coef[n:].view(np.uint16) == 0x5A5A)


def test_entropy_zero_fills_what_the_scans_leave():
    data = js.read("j420_q75_odd.jpg")
    rc, d, coef = js.entropy(data[: len(data) // 2], fill=0x7777)            # entropy data cut: the rest decodes as zeros
    assert rc == 0 and d.rows == EXPECTED["j420_q75_odd.jpg"].shape[0]
    assert not np.any(coef.view(np.uint16) == 0x7777) and np.count_nonzero(coef) > 0 and coef[-64:].tolist() == [0] * 64
    assert js.header(data[:20]) is None and js.entropy(data[:20])[0] != 0    # header cut short
    assert js.header(b"not a jpeg") is None and "SOI" in _lib.last_error()


def test_step_padding_is_left_alone():
    data = js.read("jexif6.jpg")
    rc, d, coef = js.entropy(data)
    assert rc == 0
    rc, out = js.reconstruct(d, coef, pad=7)
    assert rc == 0, _lib.last_error()
    assert np.all(out[:, d.cols * 3:] == 0xA5)
    assert np.array_equal(out[:, : d.cols * 3].reshape(d.rows, d.cols, 3), EXPECTED["jexif6.jpg"])
    d1 = js.clone(d)
    assert fa.lib().fh_jpeg_reconstruct(C.byref(d1), coef.ctypes.data, out.ctypes.data, d.cols * 3 - 1) == FH_ERR_ARG


def _set(path, value):
    def f(d):
        o = d
        for p in path[:-1]:
            o = o.comp[p] if isinstance(p, int) else getattr(o, p)
        setattr(o, path[-1], value)
    return f


MALFORMED = {
    "ncomp 2": _set(("ncomp",), 2),
    "ncomp 0": _set(("ncomp",), 0),
    "sampling factor 5": _set((1, "h"), 5),
    "sampling factor 0": _set((2, "v"), 0),
    "hmax % h": _set((1, "h"), 3),                                            # hmax = 4 in the base descriptor
    "vmax % v": _set((1, "v"), 3),
    "hmax not the largest": _set(("hmax",), 2),
    "wblocks": _set((0, "wblocks"), 7),
    "hblocks": _set((2, "hblocks"), 2),
    "dw": _set((1, "dw"), 40),
    "dh": _set((1, "dh"), 1),
    "coef_off overlap": _set((2, "coef_off"), 0),
    "coef_off past coef_count": _set((2, "coef_off"), 1 << 40),
    "coef_off negative": _set((0, "coef_off"), -64),
    "coef_count short": _set(("coef_count",), 100),
    "orientation 0": _set(("orientation",), 0),
    "orientation 9": _set(("orientation",), 9),
    "rows": _set(("rows",), 41),
    "cols swapped": lambda d: (setattr(d, "rows", d.cols), setattr(d, "cols", d.height)),
    "width 0": _set(("width",), 0),
    "color 3": _set(("color",), 3),
    "color 0 with three components": _set(("color",), 0),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_desc_check_rejects(what):
    base = js.make_desc(40, 24, [(4, 4), (1, 1), (1, 1)], color=1, orientation=6, quant=3)
    assert fa.lib().fh_jpeg_desc_check(C.byref(base)) == 0, _lib.last_error()
    bad = js.clone(base)
    MALFORMED[what](bad)
    assert fa.lib().fh_jpeg_desc_check(C.byref(bad)) == FH_ERR_ARG, what
    coef = np.zeros(int(base.coef_count), np.int16)
    out = np.full((bad.rows if 0 < bad.rows < 4096 else 64) * 4096, 0xA5, np.uint8)
    assert fa.lib().fh_jpeg_reconstruct(C.byref(bad), coef.ctypes.data, out.ctypes.data, 4096) == FH_ERR_ARG
    assert np.all(out == 0xA5)                                                # refused before any work
    assert fa.lib().fh_jpeg_desc_check(None) == FH_ERR_ARG


def test_hand_made_descriptors_reconstruct():
    """Descriptors nobody parsed: every chroma ratio, grey / YCbCr / RGB; the all-zero coefficient plane is mid-grey (128) everywhere,
    a DC-only luma block a flat one."""
    for hv in [(1, 1), (2, 1), (1, 2), (2, 2), (4, 1), (1, 4), (4, 2), (2, 4), (4, 4)]:
        d = js.make_desc(17, 9, [hv, (1, 1), (1, 1)], color=1, orientation=5)
        coef = np.zeros(int(d.coef_count), np.int16)
        assert np.all(js.picture(d, coef) == 128), hv
    d = js.make_desc(9, 17, [(1, 1)], color=0, quant=2)
    coef = np.zeros(int(d.coef_count), np.int16)
    coef[0::64] = 4 * 10                                                      # DC 40 * quant 2 / 8 = +10 on every block
    assert np.all(js.picture(d, coef) == 138)


def test_split_path_against_pillow_live():
    """The 60-image sweep of tests/test_image_io.py through fh_jpeg_entropy + fh_jpeg_reconstruct."""
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(7)
    for i in range(60):
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 2:
            arr = (arr // 8 + np.linspace(0, 200, w, dtype=np.uint8)[None, :, None]).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(arr, "RGB").save(buf, "JPEG", quality=int(rng.integers(5, 101)), subsampling=int(rng.integers(0, 3)),
                                         progressive=bool(i % 3 == 0), optimize=bool(i % 5 == 0))
        exp = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[:, :, ::-1]
        rc, d, coef = js.entropy(buf.getvalue(), guard=16)
        assert rc == 0, _lib.last_error()
        assert np.all(coef[int(d.coef_count):].view(np.uint16) == 0x5A5A)
        assert np.array_equal(js.picture(d, coef[: int(d.coef_count)]), exp), (i, h, w)


def test_new_symbols_are_declared_and_bound():
    L = fa.lib()
    for name in ("fh_jpeg_header", "fh_jpeg_entropy", "fh_jpeg_reconstruct", "fh_jpeg_desc_check", "fh_jpegdec_create", "fh_jpegdec_destroy",
                 "fh_jpeg_reconstruct_batch_dev", "fh_jpeg_decode_batch", "fh_pipeline_run_files"):
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    one = C.c_void_p(16)                                                      # argument errors come before any device is touched
    assert L.fh_jpeg_reconstruct_batch_dev(None, one, 1, one, one, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_reconstruct_batch_dev(one, one, 0, one, one, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_reconstruct_batch_dev(one, one, 4097, one, one, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_decode_batch(one, None, 1, 0, one, None, None) == FH_ERR_ARG
    assert L.fh_jpeg_decode_batch(one, one, 0, 0, one, None, None) == FH_ERR_ARG
    assert L.fh_pipeline_run_files(one, one, None, one, 1, 0, 0.5, 0.4, 1, None, None, None, 0, None) == FH_ERR_ARG
    assert L.fh_pipeline_run_files(one, one, one, one, 1, 0, 0.5, 0.4, 0, None, None, None, 0, None) == FH_ERR_ARG
