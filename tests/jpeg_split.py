"""Helpers of the JPEG split tests (tests/test_jpeg_split_cpu.py, tests/test_gpu_jpeg.py): the host half of the C ABI through ctypes
(fh_jpeg_header / fh_jpeg_entropy / fh_jpeg_reconstruct / fh_jpeg_desc_check) and hand-made descriptors."""
import ctypes as C
import os

import numpy as np

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGES = os.path.join(HERE, "golden", "images")
JPEGS = sorted(f for f in os.listdir(IMAGES) if f.endswith(".jpg"))


def read(name: str) -> bytes:
    with open(os.path.join(IMAGES, name), "rb") as f:
        return f.read()


def _buf(data: bytes):
    return (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data or b"\0")


def header(data: bytes):
    """fh_jpeg_header -> FhJpegDesc, or None."""
    d = _lib.FhJpegDesc()
    rc = fa.lib().fh_jpeg_header(C.cast(_buf(data), C.c_void_p), len(data), C.byref(d))
    return d if rc == 0 else None


def entropy(data: bytes, cap=None, guard: int = 0, fill: int = 0x5A5A):
    """fh_jpeg_entropy into an int16 array of `cap` (default: the header's coef_count) + `guard` elements pre-filled with `fill`:
    (rc, desc, array)."""
    h = header(data)
    count = int(h.coef_count) if h is not None else 0
    cap = count if cap is None else cap
    coef = np.full(max(cap + guard, 1), fill, np.uint16).view(np.int16)
    d = _lib.FhJpegDesc()
    rc = fa.lib().fh_jpeg_entropy(C.cast(_buf(data), C.c_void_p), len(data), C.byref(d), coef.ctypes.data, cap)
    return rc, d, coef


def reconstruct(desc, coef: np.ndarray, pad: int = 0, fill: int = 0xA5):
    """fh_jpeg_reconstruct at pitch cols * 3 + pad into a buffer pre-filled with `fill`: (rc, uint8[rows][cols * 3 + pad])."""
    rows, cols = max(desc.rows, 0), max(desc.cols, 0)
    step = cols * 3 + pad
    out = np.full((max(rows, 1), max(step, 1)), fill, np.uint8)
    rc = fa.lib().fh_jpeg_reconstruct(C.byref(desc), np.ascontiguousarray(coef).ctypes.data, out.ctypes.data, step)
    return rc, out


def picture(desc, coef) -> np.ndarray:
    rc, out = reconstruct(desc, coef)
    assert rc == 0, _lib.last_error()
    return out.reshape(desc.rows, desc.cols, 3)


def make_desc(width: int, height: int, factors, color: int, orientation: int = 1, quant=1):
    """A descriptor as the parser would make it for a width x height frame with the components' (h, v) sampling factors `factors`;
    quant = one value for every entry or an array [ncomp][64]."""
    d = _lib.FhJpegDesc()
    d.width, d.height, d.ncomp, d.color, d.orientation = width, height, len(factors), color, orientation
    d.rows, d.cols = (width, height) if orientation >= 5 else (height, width)
    d.hmax, d.vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mcux, mcuy = -(-width // (8 * d.hmax)), -(-height // (8 * d.vmax))
    off = 0
    for i, (h, v) in enumerate(factors):
        c = d.comp[i]
        c.h, c.v, c.wblocks, c.hblocks = h, v, mcux * h, mcuy * v
        c.dw, c.dh = -(-width * h // d.hmax), -(-height * v // d.vmax)
        c.coef_off = off
        off += c.wblocks * c.hblocks * 64
        q = np.broadcast_to(np.asarray(quant, np.uint16) if np.ndim(quant) == 0 else np.asarray(quant, np.uint16)[i], (64,))
        for k in range(64):
            c.quant[k] = int(q[k])
    d.coef_count = off
    return d


def clone(desc):
    d = _lib.FhJpegDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    return d
