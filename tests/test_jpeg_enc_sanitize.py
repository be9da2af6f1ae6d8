"""AddressSanitizer + UndefinedBehaviorSanitizer over the host half of the JPEG encoder (fh_jpeg_enc_desc -> exactly sized heap buffers ->
fh_jpeg_forward -> fh_jpeg_write at every cap -> fh_jpeg_entropy, csrc/image_io.cpp) as a stand-alone CPU program:
tests/native/jpeg_enc_sanitize.cpp.  Seeded sizes 1..40 in both axes, all layouts, unaligned bases, pitches with slack, pixel extremes,
hostile descriptors: no report, no access outside the buffers, 0 failures."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "facerecognizeonnx_amd", "csrc")


@pytest.mark.timeout(600)
def test_jpeg_encoder_host_half_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "jpeg_enc_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "native", "jpeg_enc_sanitize.cpp"), os.path.join(CSRC, "image_io.cpp"), "-lz"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
    assert b.returncode == 0, b.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1:max_allocation_size_mb=4096:detect_leaks=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]
