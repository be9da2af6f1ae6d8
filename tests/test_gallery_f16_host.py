"""Host-side contract of the gallery's F16_RERANK scan mode (fh_gallery_set_scan / get_scan / scan_stats): symbols, argument
errors, the default mode.  No GPU needed: a fresh gallery handle owns no device memory and the argument checks come first."""
import ctypes as C

import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib

FH_ERR_ARG = -1


def test_scan_mode_symbols_resolve():
    L = fa.lib()
    for name in ("fh_gallery_set_scan", "fh_gallery_get_scan", "fh_gallery_scan_stats"):
        assert hasattr(L, name) and name in _lib.PROTOTYPES


def test_set_scan_rejects_null_handle_and_unknown_mode():
    L = fa.lib()
    assert L.fh_gallery_set_scan(None, 1) == FH_ERR_ARG
    assert L.fh_gallery_set_scan(None, 0) == FH_ERR_ARG
    g = L.fh_gallery_create(512)
    try:
        assert L.fh_gallery_set_scan(g, 2) == FH_ERR_ARG
        assert L.fh_gallery_set_scan(g, -1) == FH_ERR_ARG
        assert b"unknown mode" in L.fh_last_error()
        assert L.fh_gallery_get_scan(g) == 0                       # an unknown mode changes nothing
    finally:
        L.fh_gallery_destroy(g)


def test_fresh_gallery_scans_fp32_and_null_handles_are_errors():
    L = fa.lib()
    g = L.fh_gallery_create(256)
    try:
        assert L.fh_gallery_get_scan(g) == 0
    finally:
        L.fh_gallery_destroy(g)
    assert L.fh_gallery_get_scan(None) == FH_ERR_ARG
    c, f = C.c_longlong(0), C.c_longlong(0)
    assert L.fh_gallery_scan_stats(None, C.byref(c), C.byref(f)) == FH_ERR_ARG


def test_python_gallery_scan_argument():
    g = fa.Gallery(512)
    assert g.scan == "fp32"
    with pytest.raises(ValueError):
        g.set_scan("int8")
    with pytest.raises(ValueError):
        fa.Gallery(512, scan="bf16")
