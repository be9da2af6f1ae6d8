"""AddressSanitizer + UndefinedBehaviorSanitizer over the host rule of the pair audit behind fh_pairs_from_scores / fh_gallery_pairs_dev
(csrc/pairs_plan.h), as a stand-alone CPU program with exactly sized arrays: tests/native/pairs_plan_sanitize.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_pairs_plan_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "pairs_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "native", "pairs_plan_sanitize.cpp")]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]
