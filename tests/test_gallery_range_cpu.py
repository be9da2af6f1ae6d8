"""fh_range_from_scores (csrc/range_plan.h: the one definition of the threshold search rule; host only, no GPU) against the numpy model
of tests/gallery_range_model.py: counts, score bits and indices, on random scores and on the rule's edges — duplicate scores (order by
index, a cap that cuts between two equal scores keeps the lower index), NaNs, a threshold equal to a score (not a hit) and one float
below it (a hit), tags and a zero mask, cap 1 and 1024, count > cap, empty input — and the ctypes error returns."""
import ctypes as C

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import gallery_range_model as model

FH_ERR_ARG = -1
ALL = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(sc, thr, cap, base=0, tags=None, mask=ALL):
    """The library's answer for one query's scores, held to the model's; returns (count, scores, indices)."""
    sc = np.ascontiguousarray(sc, np.float32)
    h = model.hits(sc[None, :], thr, tags, None if tags is None and mask == ALL else np.array([mask], np.uint32))[0]
    want = model.one_query(sc, h, cap, base)
    got = fa.range_from_scores(sc, thr, cap, base, tags, mask)
    assert got[0] == want[0], (got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2]), (got[1][:8], want[1][:8], got[2][:8], want[2][:8])
    return got


def test_the_constant_is_the_header_s():
    assert fa.RANGE_MAX_CAP == _lib.RANGE_MAX_CAP == 1024


@pytest.mark.parametrize("n", [1, 2, 31, 1000, 5000])
@pytest.mark.parametrize("cap", [1, 8, 1024])
def test_random_scores_match_the_model(n, cap):
    rng = np.random.default_rng(100 * n + cap)
    sc = rng.random(n, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    sc[rng.random(n) < 0.05] = np.nan
    if n > 10:
        sc[rng.integers(0, n, n // 4)] = sc[rng.integers(0, n, n // 4)]      # many equal scores
    seen = set()
    for thr in (0.0, 0.5, 0.9, 0.999, -1.0, 2.0, float("-inf"), float("inf")):
        count, s, i = check(sc, thr, cap, base=rng.integers(0, 10**6))
        seen.add("0" if count == 0 else "+" if count <= cap else ">")
        listed = min(count, cap)
        assert (i[:listed] >= 0).all() and (i[listed:] == -1).all() and (s[listed:] == -1.0).all() and not np.isnan(s).any()
    assert "0" in seen and ("+" in seen or ">" in seen)
    if n == 5000:
        assert ">" in seen                                              # a count above cap 1024 too


def test_equal_scores_rank_by_index_and_a_cap_between_them_keeps_the_lower():
    sc = np.array([0.7, 0.9, 0.9, 0.2, 0.9, 0.7, 0.95], np.float32)
    for cap in (1, 2, 3, 4, 5, 8):
        count, s, i = check(sc, 0.5, cap, base=10)
        assert count == 6 and list(i[:min(cap, 6)]) == [16, 11, 12, 14, 10, 15][:cap]
    count, s, i = check(sc, 0.5, 2, base=10)                            # the cut falls between the equal scores at 11 and 12 | 14
    assert list(i) == [16, 11] and check(sc, 0.5, 3, base=10)[2][2] == 12


def test_a_nan_is_never_a_hit():
    sc = np.array([np.nan, 0.8, np.nan, 0.3, np.inf, -np.inf], np.float32)
    for thr in (0.5, -1.0, float("-inf")):
        count, s, i = check(sc, thr, 8)
        assert 0 not in i and 2 not in i and not np.isnan(s).any()
    assert check(sc, float("-inf"), 8)[0] == 3 and list(check(sc, float("-inf"), 8)[2][:3]) == [4, 1, 3]      # -inf is not above -inf
    assert check(sc, float("inf"), 8)[0] == 0


def test_the_threshold_is_strict():
    rng = np.random.default_rng(3)
    sc = rng.random(500, dtype=np.float32)
    for r in (0, 17, 499):
        thr = sc[r]
        at = check(sc, thr, 1024)
        below = check(sc, np.nextafter(thr, np.float32(-np.inf)), 1024)
        assert r not in at[2] and r in below[2] and below[0] == at[0] + int((sc == thr).sum())


def test_tags_and_masks():
    rng = np.random.default_rng(4)
    n = 2000
    sc = rng.random(n, dtype=np.float32)
    tags = (np.uint32(1) << rng.integers(0, 8, n).astype(np.uint32)).astype(np.uint32)
    tags[rng.random(n) < 0.1] = 0
    tags[rng.random(n) < 0.1] |= np.uint32(1 << 31)
    plain = check(sc, 0.3, 1024)
    for mask in (1, 6, 1 << 31, 0x80000001, ALL, 1 << 20):
        got = check(sc, 0.3, 1024, 5, tags, mask)
        assert got[0] <= plain[0]
    assert check(sc, 0.3, 8, 0, tags, 0)[0] == 0                         # a zero mask admits nothing
    assert check(sc, 0.3, 8, 0, None, 0)[0] == 0                         # ... also on rows without tags
    assert check(sc, 0.3, 8, 0, None, 4)[0] == plain[0]                  # rows without tags carry all ones
    assert check(sc, 0.3, 8, 0, tags, ALL)[0] == int(((sc > np.float32(0.3)) & (tags != 0)).sum()) < plain[0]


def test_empty_input_and_errors():
    count, s, i = fa.range_from_scores(np.empty(0, np.float32), 0.5, 4)
    assert count == 0 and (s == -1.0).all() and (i == -1).all() and len(s) == 4
    L = fa.lib()
    sc = np.array([0.6, 0.7], np.float32)
    out_s, out_i = np.full(4, 7.0, np.float32), np.full(4, -7, np.int32)
    cnt = C.c_longlong(-5)
    a = (C.byref(cnt), out_s.ctypes.data, out_i.ctypes.data)
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 0, None, ALL, 0.5, 0, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 0, None, ALL, 0.5, 1025, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 0, None, ALL, float("nan"), 4, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(None, 2, 0, None, ALL, 0.5, 4, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(sc.ctypes.data, -1, 0, None, ALL, 0.5, 4, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 2**31 - 2, None, ALL, 0.5, 4, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(sc.ctypes.data, 2, -1, None, ALL, 0.5, 4, *a) == FH_ERR_ARG
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 0, None, ALL, 0.5, 4, None, out_s.ctypes.data, out_i.ctypes.data) == FH_ERR_ARG
    assert cnt.value == -5 and (out_s == 7.0).all() and (out_i == -7).all()          # nothing was written
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 2**31 - 3, None, ALL, 0.5, 4, *a) == 2 and list(out_i) == [2**31 - 2, 2**31 - 3, -1, -1]
    assert L.fh_range_from_scores(sc.ctypes.data, 2, 0, None, ALL, 0.65, 4, C.byref(cnt), None, None) == 1 and cnt.value == 1
    with pytest.raises(fa.FaceHipError):
        fa.range_from_scores(sc, float("nan"), 4)
    with pytest.raises(ValueError):
        fa.range_from_scores(sc, 0.5, 4, tags=np.zeros(3, np.uint32))
