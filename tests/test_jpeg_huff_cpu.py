"""The host rules of the device Huffman coder (include/facehip.h "JPEG out"): fh_jpeg_write_header is the front of fh_jpeg_write's output
under the same cap contract, fh_jpeg_scan_bits is the bits of every block in scan order, and the PARALLEL decomposition the device runs
(tests/jpeg_huff_model.py: neighbour predictor, prefix sum, pack, pad, stuff, header + stream + EOI) gives fh_jpeg_write's files byte for
byte — on every encoder case and on the crafted coefficient planes.  Plus the two host functions under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (tests/native/jpeg_huff_sanitize.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from facerecognizeonnx_amd import _lib
from tests import jpeg_enc_model as m
from tests import jpeg_huff_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "facerecognizeonnx_amd", "csrc")


@pytest.fixture(scope="module")
def planes():
    """[(name, descriptor, coefficients, fh_jpeg_write's file)]: every encoder case through the host forward path, then the crafted planes."""
    out = []
    for case in m.cases():
        kind, w, h, layout, q = case
        d, coef, data = m.encode_host(m.picture(kind, w, h, grey=layout == "grey"), layout, q)
        out.append((m.case_name(*case), d, coef[: int(d.coef_count)], data))
    for name, d, coef in hm.crafted():
        rc, n, buf = m.c_write(d, coef)
        assert rc == 0, (name, _lib.last_error())
        out.append((name, d, coef, buf[:n].tobytes()))
    return out


def sos_end(data):
    """Where the entropy-coded bytes start: behind the SOS header."""
    at = data.index(b"\xff\xda")
    return at + 2 + int.from_bytes(data[at + 2: at + 4], "big")


def test_header_is_the_front_of_the_file(planes):
    for name, d, coef, data in planes:
        rc, n, buf = hm.c_header(d, guard=8)
        assert rc == 0 and n == sos_end(data), name
        assert buf[:n].tobytes() == data[:n] and np.all(buf[n:] == 0xA5), name


def test_header_cap_contract():
    for layout in m.LAYOUTS:
        d = m.enc_desc(17, 23, layout, 75)
        rc, need, full = hm.c_header(d)
        assert rc == 0 and 0 < need <= 704
        for cap in list(range(0, need, 7)) + [need - 1]:
            rc, n, buf = hm.c_header(d, cap=cap, guard=16)
            assert rc == hm.FH_ERR_ARG and n == need                           # the size whatever cap is
            assert np.array_equal(buf[:cap], full[:cap]) and np.all(buf[cap:] == 0xA5)     # nothing at or behind cap
        rc, n, buf = hm.c_header(d, cap=need, guard=16)
        assert rc == 0 and n == need and np.all(buf[need:] == 0xA5)
    bad = m.enc_desc(17, 23, "420", 75)
    bad.orientation = 3
    rc, n, buf = hm.c_header(bad)
    assert rc == hm.FH_ERR_ARG and n == 0 and np.all(buf == 0xA5)


def test_model_bits_equal_scan_bits(planes):
    for name, d, coef, data in planes:
        rc, bits = hm.c_scan_bits(d, coef, guard=4)
        assert rc == 0, (name, _lib.last_error())
        nb = hm.blocks_of(d)
        assert np.all(bits[nb:] == 0xA5A5A5A5), name
        assert np.array_equal(bits[:nb], hm.scan_bits(d, coef)), name
        stream_bytes = len(data) - sos_end(data) - 2 - data[sos_end(data):-2].count(b"\xff\x00")
        assert (int(bits[:nb].sum()) + 7) // 8 == stream_bytes, name           # the bits add up to the file's entropy-coded bytes


def test_model_files_equal_the_host_writer(planes):
    for name, d, coef, data in planes:
        assert hm.file_bytes(d, coef) == data, name


def test_scan_bits_refuses_what_the_writer_refuses():
    for name, d, coef in hm.uncodable():
        assert m.c_write(d, coef)[0] == hm.FH_ERR_ARG, name
        assert hm.c_scan_bits(d, coef)[0] == hm.FH_ERR_ARG, name
        assert hm.scan_bits(d, coef) is None, name
    d = m.enc_desc(40, 9, "420", 75)
    coef = np.zeros(int(d.coef_count), np.int16)
    rc, bits = hm.c_scan_bits(d, coef, cap=hm.blocks_of(d) - 1, guard=2)
    assert rc == hm.FH_ERR_ARG and np.all(bits == 0xA5A5A5A5)                   # a short output: refused before the first write


def test_crafted_planes_reach_the_rare_paths(planes):
    """What the GPU test relies on, asserted here on the host writer's output as well."""
    by_name = {name: (d, coef, data) for name, d, coef, data in planes}
    d, coef, data = by_name["zero_grey"]
    assert int(hm.c_scan_bits(d, coef)[1][:64].sum()) == 64 * 6
    assert b"\xff\x00\xff\x00" in by_name["ones_grey"][2][sos_end(by_name["ones_grey"][2]):]
    assert by_name["extreme_grey"][2][-4:] == b"\xff\x00\xff\xd9"
    assert int(hm.c_scan_bits(*by_name["extreme_grey"][:2])[1].max()) == 9 + 11 + 63 * 26      # the longest luma block there is
    chroma = hm.c_scan_bits(*by_name["extreme_420"][:2])[1][4:6]                                # (chroma codes +-1023 behind run 0 in 12 bits)
    assert chroma.tolist() == [11 + 11 + 63 * 22] * 2


@pytest.mark.timeout(600)
def test_jpeg_huff_host_rules_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "jpeg_huff_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "native", "jpeg_huff_sanitize.cpp"), os.path.join(CSRC, "image_io.cpp"), "-lz"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
    assert b.returncode == 0, b.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1:max_allocation_size_mb=4096:detect_leaks=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]
