"""The host half of the JPEG encoder (include/facehip.h "JPEG out", csrc/image_io.cpp): fh_jpeg_quant_tables / fh_jpeg_enc_desc /
fh_jpeg_enc_check / fh_jpeg_forward / fh_jpeg_write / fh_imwrite_jpeg.  The forward path must give, coefficient for coefficient, what
libjpeg-turbo stored for the same pixels (files written by Pillow: tests/golden/jpeg_enc, tests/golden/make_jpeg_enc.py) and what the
numpy model of the rule gives (tests/jpeg_enc_model.py); the writer must be read back to the same descriptor and coefficients by
fh_jpeg_entropy.  Identical, no tolerance.  No GPU."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import jpeg_enc_model as m
from tests import jpeg_split as js

FH_ERR_ARG = -1
CASES = m.cases()
DESC_FIELDS = ("width", "height", "rows", "cols", "ncomp", "hmax", "vmax", "orientation", "coef_count", "color")
COMP_FIELDS = ("h", "v", "wblocks", "hblocks", "dw", "dh", "coef_off")


def _fixture(case) -> bytes:
    with open(os.path.join(m.FIXTURES, m.case_name(*case)), "rb") as f:
        return f.read()


def _same_desc(a, b, quant=True):
    for k in DESC_FIELDS:
        assert getattr(a, k) == getattr(b, k), k
    for i in range(a.ncomp):
        for k in COMP_FIELDS:
            assert getattr(a.comp[i], k) == getattr(b.comp[i], k), (i, k)
        if quant:
            assert list(a.comp[i].quant) == list(b.comp[i].quant), i


def test_abi_layout_and_symbols():
    assert C.sizeof(_lib.FhJpegDesc) == 528 and C.sizeof(_lib.FhBlob) == 16 and C.sizeof(_lib.FhFrame) == 24
    L = fa.lib()
    for name in ("fh_jpeg_quant_tables", "fh_jpeg_enc_desc", "fh_jpeg_enc_check", "fh_jpeg_forward", "fh_jpeg_write", "fh_jpeg_write_bound",
                 "fh_imwrite_jpeg", "fh_jpegenc_create", "fh_jpegenc_destroy", "fh_jpeg_forward_batch_dev", "fh_jpeg_encode_batch"):
        assert name in _lib.PROTOTYPES and hasattr(L, name), name
    one = C.c_void_p(16)                                                      # argument errors come before any device is touched
    assert L.fh_jpeg_forward_batch_dev(None, one, 1, one, one, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_forward_batch_dev(one, one, 0, one, one, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_forward_batch_dev(one, one, 4097, one, one, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_encode_batch(one, None, 1, 90, 2, 0, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_encode_batch(one, one, 0, 90, 2, 0, one, None) == FH_ERR_ARG
    assert L.fh_jpeg_encode_batch(one, one, 1, 90, 3, 0, one, None) == FH_ERR_ARG


def _tables(quality):
    luma, chroma = np.zeros(64, np.uint16), np.zeros(64, np.uint16)
    assert fa.lib().fh_jpeg_quant_tables(quality, luma.ctypes.data, chroma.ctypes.data) == 0
    return luma, chroma


def test_quant_tables_equal_the_files_and_the_model():
    for q in list(range(-3, 105)):
        luma, chroma = _tables(q)
        ml, mc = m.quant_tables(q)
        assert np.array_equal(luma, ml) and np.array_equal(chroma, mc), q
        assert luma.min() >= 1 and luma.max() <= 255 and chroma.min() >= 1 and chroma.max() <= 255
    for case in CASES:
        rc, d, _ = js.entropy(_fixture(case))
        assert rc == 0, _lib.last_error()
        luma, chroma = _tables(case[4])
        assert list(d.comp[0].quant) == luma.tolist(), case
        if d.ncomp == 3:
            assert list(d.comp[1].quant) == chroma.tolist() and list(d.comp[2].quant) == chroma.tolist(), case


def test_quant_tables_against_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    arr = np.zeros((8, 8, 3), np.uint8)
    for q in range(1, 101):
        buf = io.BytesIO()
        Image.fromarray(arr, "RGB").save(buf, "JPEG", quality=q, optimize=False)
        tabs = Image.open(io.BytesIO(buf.getvalue())).quantization
        luma, chroma = _tables(q)
        # Pillow hands the tables out in the file's (zigzag) order or in natural order, depending on its version: accept exactly those two
        for got, exp in ((tabs[0], luma), (tabs[1], chroma)):
            got = np.asarray(list(got))
            assert np.array_equal(got, exp) or np.array_equal(got, exp[m.ZIGZAG]), q


@pytest.mark.parametrize("case", CASES, ids=lambda c: m.case_name(*c)[:-4])
def test_desc_and_forward_equal_pillow_and_the_model(case):
    kind, w, h, layout, q = case
    data = _fixture(case)
    rc, pd, pcoef = js.entropy(data)
    assert rc == 0, _lib.last_error()
    d = m.enc_desc(w, h, layout, q)
    assert fa.lib().fh_jpeg_enc_check(C.byref(d)) == 0, _lib.last_error()
    _same_desc(d, pd)                                                          # fh_jpeg_entropy's = fh_jpeg_header's fields + the tables
    _same_desc(d, js.header(data), quant=False)
    comps, hmax, vmax, count = m.geometry(w, h, layout)
    assert count == d.coef_count and all(c.coef_off % 64 == 0 for c in d.comp)
    bgr = m.picture(kind, w, h, grey=layout == "grey")
    rc, coef = m.c_forward(d, bgr, pad=5, guard=64)
    assert rc == 0, _lib.last_error()
    n = int(d.coef_count)
    assert np.all(coef[n:].view(np.uint16) == 0x5A5A)
    assert np.array_equal(coef[:n], pcoef[:n])                                 # libjpeg-turbo's
    assert np.array_equal(coef[:n], m.forward(bgr, layout, q))                 # the rule's


def test_the_fixtures_keep_the_edge_cases():
    names = {m.case_name(*c) for c in CASES}
    assert names == {f for f in os.listdir(m.FIXTURES) if f.endswith(".jpg")}
    for (w, h) in m.KEY_SIZES:
        for layout in m.LAYOUTS:
            assert {q for (_, cw, ch, cl, q) in CASES if (cw, ch, cl) == (w, h, layout)} == set(m.QUALITIES)
    assert {(c[1], c[2]) for c in CASES} == set(m.SIZES) and {c[0] for c in CASES} == {"noise", "ramp"}
    # the dummy-block rule has work to do: some fixture pads right, some below, some both
    pads = set()
    for (_, w, h, layout, _) in CASES:
        for (ch, cv, wb, hb, dw, dh, _) in m.geometry(w, h, layout)[0]:
            pads.add((wb > -(-dw // 8), hb > -(-dh // 8)))
    assert pads == {(False, False), (True, False), (False, True), (True, True)}


def test_forward_against_pillow_live():
    """The whole cross product of sizes, layouts, qualities and both pictures, plus 640 x 640, against the Pillow at hand."""
    Image = pytest.importorskip("PIL.Image")
    from tests.golden import make_jpeg_enc as gen
    todo = m.cases(committed=False) + [("noise", 640, 640, "420", 90), ("ramp", 120, 72, "422", 75), ("noise", 50, 50, "420", 30)]
    for case in todo:
        kind, w, h, layout, q = case
        rc, pd, pcoef = js.entropy(gen.pillow_bytes(*case))
        assert rc == 0, _lib.last_error()
        d = m.enc_desc(w, h, layout, q)
        _same_desc(d, pd)
        rc, coef = m.c_forward(d, m.picture(kind, w, h, grey=layout == "grey"))
        assert rc == 0 and np.array_equal(coef, pcoef[: int(d.coef_count)]), case


def _closure(d, coef):
    """fh_jpeg_write, then fh_jpeg_entropy of the bytes: the same descriptor, the same coefficients."""
    rc, n, out = m.c_write(d, coef, guard=32)
    assert rc == 0, _lib.last_error()
    assert 0 < n <= int(fa.lib().fh_jpeg_write_bound(C.byref(d))) and np.all(out[-32:] == 0xA5)
    data = out[:n].tobytes()
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    rc, rd, rcoef = js.entropy(data, guard=8)
    assert rc == 0, _lib.last_error()
    _same_desc(d, rd)
    assert np.array_equal(rcoef[: int(d.coef_count)], np.asarray(coef)[: int(d.coef_count)])
    return data


@pytest.mark.parametrize("case", [c for c in CASES if (c[1], c[2]) in m.KEY_SIZES or c[1] >= 100 or c[1] <= 2], ids=lambda c: m.case_name(*c)[:-4])
def test_write_then_entropy_is_the_identity(case):
    kind, w, h, layout, q = case
    d = m.enc_desc(w, h, layout, q)
    rc, coef = m.c_forward(d, m.picture(kind, w, h, grey=layout == "grey"))
    assert rc == 0
    data = _closure(d, coef)
    # the Huffman tables are the Annex K ones libjpeg writes without `optimize`: the same DHT segments as Pillow's file, byte for byte
    def dht(b):
        out, i = [], 2
        while i + 4 <= len(b) and b[i] == 0xFF and b[i + 1] != 0xDA:
            ln = (b[i + 2] << 8) | b[i + 3]
            if b[i + 1] == 0xC4:
                out.append(bytes(b[i: i + 2 + ln]))
            i += 2 + ln
        return b"".join(out)
    assert dht(data) == dht(_fixture(case)) and len(dht(data)) > 0
    Image = pytest.importorskip("PIL.Image")                                  # a foreign decoder reads the file to the same pixels
    rc, rd, rcoef = js.entropy(data)
    exp = js.picture(rd, rcoef[: int(rd.coef_count)])
    got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_write_closure_on_extreme_coefficients(layout):
    d = m.enc_desc(40, 24, layout, 75)
    n = int(d.coef_count)
    rng = np.random.default_rng(5)
    zero = np.zeros(n, np.int16)
    _closure(d, zero)                                                          # an all-zero picture
    dc = zero.copy()
    for i in range(d.ncomp):                                                   # DC +-1023 / -1024 alternating in the component's raster (differences up to 2047)
        c = d.comp[i]
        v = np.where(np.arange(c.wblocks * c.hblocks) % 2 == 0, 1023, -1024)
        if c.h == 2:                                                           # in scan order the blocks of an MCU follow each other: alternate there
            v = np.where((np.arange(c.wblocks * c.hblocks) % c.wblocks) % 2 == 0, 1023, -1024)
        dc[int(c.coef_off): int(c.coef_off) + v.size * 64: 64] = v
    _closure(d, dc)
    ac = zero.copy()
    ac[:] = np.where(rng.integers(0, 2, n) == 0, 1023, -1023)
    ac[0::64] = 0
    _closure(d, ac)
    for gap in (15, 16, 17, 31, 32, 33, 62):                                   # runs of zeros around the ZRL symbol
        runs = zero.copy()
        blk = np.zeros(64, np.int16)
        blk[m.ZIGZAG[np.arange(gap + 1, 64, gap + 1)]] = -3                    # `gap` zeros in front of every value (62: three ZRLs, then
        runs[:] = np.tile(blk, n // 64)                                        # the last coefficient and no EOB)
        _closure(d, runs)
    mixed = rng.integers(-1023, 1024, n).astype(np.int16) * (rng.integers(0, 4, n) == 0)
    mixed[0::64] = rng.integers(-500, 500, n // 64)
    _closure(d, mixed.astype(np.int16))


def test_write_refuses_what_baseline_cannot_code():
    d = m.enc_desc(16, 16, "444", 90)
    n = int(d.coef_count)
    for at, value in ((0, 2048), (0, -2048), (64 * 5 + 9, 1024), (64 * 7 + 63, -1024), (int(d.comp[2].coef_off), 2048)):
        coef = np.zeros(n, np.int16)
        coef[at] = value
        rc, written, _ = m.c_write(d, coef)
        assert rc == FH_ERR_ARG and written == 0 and "baseline" in _lib.last_error(), (at, value)
    coef = np.zeros(n, np.int16)
    coef[0], coef[64] = 1023, -1024                                            # a difference of -2047 is still coded
    assert m.c_write(d, coef)[0] == 0


def test_cap_one_short_writes_nothing_behind_cap_and_reports_the_size():
    bgr = m.picture("noise", 33, 16, False)
    d, coef, data = m.encode_host(bgr, "420", 90)
    need = len(data)
    for cap in (0, 1, 100, need - 1):
        rc, written, out = m.c_write(d, coef, cap=cap, guard=64)
        assert rc == FH_ERR_ARG and written == need and "too small" in _lib.last_error(), cap
        assert np.all(out[cap:] == 0xA5), cap
        assert out[:cap].tobytes() == data[:cap]
    rc, written, out = m.c_write(d, coef, cap=need, guard=64)
    assert rc == 0 and written == need and out[:need].tobytes() == data and np.all(out[need:] == 0xA5)
    rc, c2 = m.c_forward(d, bgr, guard=16, cap=int(d.coef_count) - 1)            # fh_jpeg_forward: refused before the first write
    assert rc == FH_ERR_ARG and "too small" in _lib.last_error() and np.all(c2.view(np.uint16) == 0x5A5A)


def _set(path, value):
    def f(d):
        o = d
        for p in path[:-1]:
            o = o.comp[p] if isinstance(p, int) else getattr(o, p)
        setattr(o, path[-1], value)
    return f


def _quant(i, k, v):
    def f(d):
        d.comp[i].quant[k] = v
    return f


def _factors(hv, w=40, h=24):
    def f(d):
        new = js.make_desc(w, h, [hv, (1, 1), (1, 1)], color=1, quant=3)
        C.memmove(C.byref(d), C.byref(new), C.sizeof(d))
    return f


REFUSED = {
    "orientation 6": lambda d: (setattr(d, "orientation", 6), setattr(d, "rows", d.width), setattr(d, "cols", d.height)),
    "orientation 0": _set(("orientation",), 0),
    "color 2 (RGB)": _set(("color",), 2),
    "color 3": _set(("color",), 3),
    "luma 4 x 1 (4:1:1)": _factors((4, 1)),
    "luma 1 x 2": _factors((1, 2)),
    "luma 2 x 4": _factors((2, 4)),
    "chroma 2 x 1": lambda d: C.memmove(C.byref(d), C.byref(js.make_desc(40, 24, [(2, 1), (2, 1), (1, 1)], color=1, quant=3)), C.sizeof(d)),
    "grey 2 x 2": lambda d: C.memmove(C.byref(d), C.byref(js.make_desc(40, 24, [(2, 2)], color=0, quant=3)), C.sizeof(d)),
    "quantiser 0": _quant(0, 17, 0),
    "quantiser 256": _quant(2, 63, 256),
    "quantiser 65535": _quant(1, 0, 65535),
    "width 65536": lambda d: C.memmove(C.byref(d), C.byref(js.make_desc(65536, 8, [(1, 1)], color=0, quant=3)), C.sizeof(d)),
    # ... and everything fh_jpeg_desc_check refuses
    "ncomp 2": _set(("ncomp",), 2),
    "wblocks": _set((0, "wblocks"), 7),
    "dh": _set((1, "dh"), 1),
    "coef_off overlap": _set((2, "coef_off"), 0),
    "coef_count short": _set(("coef_count",), 100),
    "rows": _set(("rows",), 41),
    "width 0": _set(("width",), 0),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_enc_check_rejects(what):
    L = fa.lib()
    base = m.enc_desc(40, 24, "420", 75)
    assert L.fh_jpeg_enc_check(C.byref(base)) == 0, _lib.last_error()
    bad = js.clone(base)
    REFUSED[what](bad)
    assert L.fh_jpeg_enc_check(C.byref(bad)) == FH_ERR_ARG, what
    bgr = np.zeros((1 << 12, 1 << 12), np.uint8)                              # (room for whatever rows / cols the bad descriptor names)
    coef = np.full(1 << 16, 0x5A5A, np.uint16).view(np.int16)
    assert L.fh_jpeg_forward(C.byref(bad), bgr.ctypes.data, 1 << 12, coef.ctypes.data, coef.size) == FH_ERR_ARG
    assert np.all(coef.view(np.uint16) == 0x5A5A)                             # refused before any work
    out = np.full(1 << 16, 0xA5, np.uint8)
    written = C.c_size_t(7)
    assert L.fh_jpeg_write(C.byref(bad), np.zeros(1 << 16, np.int16).ctypes.data, out.ctypes.data, out.size, C.byref(written)) == FH_ERR_ARG
    assert np.all(out == 0xA5) and written.value == 0 and L.fh_jpeg_write_bound(C.byref(bad)) == 0
    assert L.fh_jpeg_enc_check(None) == FH_ERR_ARG


def test_enc_desc_arguments():
    L = fa.lib()
    d = _lib.FhJpegDesc()
    for args in ((0, 8, 0, 0, 90), (8, 0, 0, 0, 90), (65536, 8, 0, 0, 90), (8, 65536, 1, 0, 90), (8, 8, 0, 3, 90), (8, 8, 0, -1, 90)):
        assert L.fh_jpeg_enc_desc(*args, C.byref(d)) == FH_ERR_ARG, args
    assert L.fh_jpeg_enc_desc(8, 8, 0, 2, 90, None) == FH_ERR_ARG
    assert L.fh_jpeg_enc_desc(65535, 1, 1, 7, 90, C.byref(d)) == 0 and d.ncomp == 1 and d.comp[0].wblocks == 8192   # grey ignores subsampling
    assert L.fh_jpeg_enc_check(C.byref(d)) == 0


@pytest.mark.parametrize("layout,sub", [("444", 0), ("422", 1), ("420", 2)])
def test_imwrite_then_imread_equals_forward_plus_reconstruct(tmp_path, layout, sub):
    bgr = m.picture("ramp", 37, 21, False)
    wide = np.full((21, 37 * 3 + 9), 0xEE, np.uint8)                          # a pitch with slack
    wide[:, : 37 * 3] = bgr.reshape(21, -1)
    path = str(tmp_path / "out.jpg")
    assert fa.lib().fh_imwrite_jpeg(path.encode(), wide.ctypes.data, 21, 37, wide.shape[1], 85, sub) == 0, _lib.last_error()
    d, coef, data = m.encode_host(bgr, layout, 85)
    with open(path, "rb") as f:
        assert f.read() == data
    got = fa.imread(path)
    assert got is not None and np.array_equal(got, js.picture(d, coef))
    assert np.abs(got.astype(int) - bgr.astype(int)).mean() < 6                # and it is the picture that went in
    assert fa.lib().fh_imwrite_jpeg(str(tmp_path / "no" / "dir.jpg").encode(), wide.ctypes.data, 21, 37, wide.shape[1], 85, sub) < 0
    assert fa.lib().fh_imwrite_jpeg(path.encode(), wide.ctypes.data, 21, 37, 37 * 3 - 1, 85, sub) == FH_ERR_ARG
    assert fa.lib().fh_imwrite_jpeg(path.encode(), wide.ctypes.data, 0, 37, 111, 85, sub) == FH_ERR_ARG


def test_grey_descriptor_takes_luma_from_bgr():
    bgr = m.picture("noise", 17, 23, False)
    d = m.enc_desc(17, 23, "grey", 90)
    rc, coef = m.c_forward(d, bgr)
    assert rc == 0
    b, g, r = (bgr[:, :, k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    assert np.array_equal(coef, m.forward(np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8), "grey", 90))


def test_cv_imwrite_of_the_shim_header(tmp_path):
    """cv::imwrite in shim/cv_compat.h (a build without OpenCV): OpenCV's defaults (quality 95, 4:2:0), its parameter list, its refusals."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    pkg = os.path.dirname(os.path.abspath(fa.__file__))
    exe = str(tmp_path / "cv_imwrite_demo")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(js.HERE, "native", "cv_imwrite_demo.cpp"), "-I", os.path.join(pkg, "shim"),
           "-L", pkg, "-lfacehip", f"-Wl,-rpath,{pkg}"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-2000:]
    y, x = np.mgrid[0:21, 0:37 * 3]
    bgr = ((x * 7 + y * 13 + (x % 3) * 40) & 255).astype(np.uint8).reshape(21, 37, 3)
    for name, layout, q in (("default.jpg", "420", 95), ("q80_444.JPG", "444", 80)):
        with open(str(tmp_path / name), "rb") as f:
            assert f.read() == m.encode_host(bgr, layout, q)[2], name
    assert sorted(p.name for p in tmp_path.iterdir() if p.suffix.lower() in (".jpg", ".png")) == ["default.jpg", "q80_444.JPG"]
