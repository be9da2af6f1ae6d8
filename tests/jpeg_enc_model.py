"""The forward path of the JPEG encoder as a numpy model (include/facehip.h "JPEG out"): libjpeg's rule — jccolor.c, jcsample.c without
smoothing, jfdctint.c "islow", jcdctmgr.c's quantiser, jccoefct.c's dummy blocks — written down independently of csrc/image_io.cpp, plus
the seeded test pictures and the ctypes helpers the encoder tests share (tests/test_jpeg_enc_cpu.py, tests/test_gpu_jpeg_enc.py,
tests/golden/make_jpeg_enc.py)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "jpeg_enc")

SIZES = [(1, 1), (2, 2), (8, 8), (17, 23), (33, 16), (9, 40), (40, 9), (24, 8), (31, 31), (100, 75), (112, 112)]   # (width, height)
KEY_SIZES = [(8, 8), (40, 9), (100, 75), (17, 23)]                       # the ones that separate the edge rules: every layout, every quality
LAYOUTS = ["grey", "444", "422", "420"]
QUALITIES = [30, 75, 90, 100]
SUBSAMPLING = {"grey": 0, "444": 0, "422": 1, "420": 2}

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                      95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99] + [99] * 36,
                       np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


# ------------------------------------------------------------------------------------------ the cases
def cases(committed=True):
    """(kind, width, height, layout, quality): the committed fixtures, or the whole cross product (for a live Pillow)."""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for li, layout in enumerate(LAYOUTS):
            for qi, q in enumerate(QUALITIES):
                if committed and (w, h) not in KEY_SIZES and qi != (si + li) % 4:
                    continue
                kinds = ["noise", "ramp"] if not committed else ["noise" if (si + li + qi) % 2 == 0 else "ramp"]
                out += [(k, w, h, layout, q) for k in kinds]
    return out


def case_name(kind, w, h, layout, q):
    return f"{kind}_{w}x{h}_{layout}_q{q}.jpg"


def picture(kind, w, h, grey=False):
    """The seeded BGR u8 picture of a case: integer hash noise or a smooth two-way ramp; pure uint32 arithmetic, the same everywhere.
    grey: B = G = R."""
    i = np.arange(h * w * 3, dtype=np.uint32).reshape(h, w, 3)
    if kind == "noise":
        x = i * np.uint32(2654435761) + np.uint32(w * 7919 + h * 104729 + 12345)
        x ^= x >> np.uint32(15)
        x = x * np.uint32(0x2C1B3C6D)
        x ^= x >> np.uint32(12)
        a = (x >> np.uint32(11)).astype(np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 255 // max(w + h - 2, 1))], axis=2).astype(np.uint8)
    if grey:
        a = np.repeat(a[:, :, 1:2], 3, axis=2)
    return np.ascontiguousarray(a)


# ------------------------------------------------------------------------------------------ the rule
def quant_tables(quality):
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * scale + 50) // 100, 1, 255).astype(np.uint16) for b in (BASE_LUMA, BASE_CHROMA))


def geometry(width, height, layout):
    """[(h, v, wblocks, hblocks, dw, dh, coef_off)] per component, hmax, vmax, coef_count."""
    if layout == "grey":
        factors = [(1, 1)]
    else:
        factors = [{"444": (1, 1), "422": (2, 1), "420": (2, 2)}[layout], (1, 1), (1, 1)]
    hmax, vmax = factors[0]
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    comps, off = [], 0
    for h, v in factors:
        comps.append((h, v, mcux * h, mcuy * v, -(-width * h // hmax), -(-height * v // vmax), off))
        off += mcux * h * mcuy * v * 64
    return comps, hmax, vmax, off


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint.c's 1-D transform on d[0..7] (arrays); first: the row pass."""
    n = 11 if first else 15
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return o


def forward(bgr, layout, quality=None, quant=None):
    """BGR u8 [rows][cols][3] -> the int16 coefficients of every component, dummy blocks included, natural order."""
    bgr = np.asarray(bgr)
    height, width = bgr.shape[:2]
    comps, hmax, vmax, count = geometry(width, height, layout)
    if quant is None:
        luma, chroma = quant_tables(quality)
        quant = [luma, chroma, chroma]
    b, g, r = (bgr[:, :, k].astype(np.int64) for k in range(3))
    planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
              (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
              (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    out = np.zeros(count, np.int16)
    for ci, (h, v, wblocks, hblocks, dw, dh, off) in enumerate(comps):
        hx, vx = hmax // h, vmax // v
        bw, bh = -(-dw // 8), -(-dh // 8)
        p = planes[ci]
        p = np.pad(p, ((0, -(-height // vmax) * vmax - height), (0, 8 * bw * hx - width)), mode="edge")   # rows to a multiple of vmax ONLY
        if hx == 2 and vx == 2:
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif hx == 2:
            p = (p[:, 0::2] + p[:, 1::2] + (np.arange(p.shape[1] // 2) & 1)) >> 1
        p = p[: bh * 8]
        p = np.pad(p, ((0, bh * 8 - p.shape[0]), (0, 0)), mode="edge")                                # then the last DOWN-SAMPLED row
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
        rows = np.stack(_fdct_1d([blocks[..., k] for k in range(8)], True), axis=-1)
        cols = np.stack(_fdct_1d([rows[..., k, :] for k in range(8)], False), axis=-2)
        qv = 8 * np.asarray(quant[ci], np.int64).reshape(8, 8)
        q = np.sign(cols) * ((np.abs(cols) + (qv >> 1)) // qv)
        grid = np.zeros((hblocks, wblocks, 64), np.int64)
        grid[:bh, :bw] = q.reshape(bh, bw, 64)
        for bx in range(bw, wblocks):
            grid[:bh, bx, 0] = grid[:bh, bx - 1, 0]
        for by in range(bh, hblocks):
            for bx in range(wblocks):
                grid[by, bx, 0] = grid[by - 1, bx // h * h + h - 1, 0]
        out[off: off + grid.size] = grid.reshape(-1)
    return out


# ------------------------------------------------------------------------------------------ the C ABI through ctypes
def _fa():
    import facerecognizeonnx_amd as fa
    from facerecognizeonnx_amd import _lib
    return fa.lib(), _lib


def enc_desc(width, height, layout, quality):
    L, _lib = _fa()
    d = _lib.FhJpegDesc()
    rc = L.fh_jpeg_enc_desc(width, height, int(layout == "grey"), SUBSAMPLING[layout], quality, C.byref(d))
    assert rc == 0, _lib.last_error()
    return d


def c_forward(desc, bgr, pad=0, guard=0, fill=0x5A5A, cap=None):
    """fh_jpeg_forward at pitch cols * 3 + pad: (rc, int16 array of coef_count + guard elements pre-filled with `fill`)."""
    L, _ = _fa()
    rows, cols = bgr.shape[:2]
    buf = np.full((rows, cols * 3 + pad), 0xEE, np.uint8)
    buf[:, : cols * 3] = bgr.reshape(rows, cols * 3)
    n = int(desc.coef_count)
    coef = np.full(max(n + guard, 1), fill, np.uint16).view(np.int16)
    rc = L.fh_jpeg_forward(C.byref(desc), buf.ctypes.data, cols * 3 + pad, coef.ctypes.data, n if cap is None else cap)
    return rc, coef


def c_write(desc, coef, cap=None, guard=0):
    """fh_jpeg_write into a buffer of `cap` (default: the bound) + guard bytes pre-filled with 0xA5: (rc, written, buffer)."""
    L, _ = _fa()
    cap = int(L.fh_jpeg_write_bound(C.byref(desc))) if cap is None else cap
    out = np.full(max(cap + guard, 1), 0xA5, np.uint8)
    written = C.c_size_t(12345)
    rc = L.fh_jpeg_write(C.byref(desc), np.ascontiguousarray(coef).ctypes.data, out.ctypes.data, cap, C.byref(written))
    return rc, int(written.value), out


def encode_host(bgr, layout, quality):
    """fh_jpeg_enc_desc + fh_jpeg_forward + fh_jpeg_write: (desc, coefficients, the file's bytes)."""
    _, _lib = _fa()
    d = enc_desc(bgr.shape[1], bgr.shape[0], layout, quality)
    rc, coef = c_forward(d, bgr)
    assert rc == 0, _lib.last_error()
    rc, n, out = c_write(d, coef)
    assert rc == 0, _lib.last_error()
    return d, coef, out[:n].tobytes()
