"""fh_topk_from_scores (csrc/deep_plan.h: the one definition of the deep top-k; host only, no GPU) against the numpy model of
tests/gallery_deep_model.py — score bits and indices on random scores, ties, NaN and +-inf, tags and masks, n < k, n = 0 — its error
returns, its equality with fh_range_from_scores(-inf, cap = k), and the BLOCK RULE the device call relies on: the top-k of the rows of
the chosen blocks is the top-k of all rows, and no more than k blocks are chosen (the library's blocks, fh_debug_deep_blocks, against the
model's; the top-k over them by the model)."""
import ctypes as C

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import gallery_deep_model as model

FH_ERR_ARG = -1
ALL = 0xFFFFFFFF
KS = (1, 8, 16, 17, 100, 1024)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(sc, k, base=0, tags=None, mask=ALL):
    """The library's answer for one query's scores, held to the model's and to fh_range_from_scores(-inf, cap = k); returns
    (listed, scores, indices)."""
    sc = np.ascontiguousarray(sc, np.float32)
    _, S, R, _ = model.topk_from_scores(sc[None, :], k, base, tags, None if tags is None and mask == ALL else np.array([mask], np.uint32))
    n_el = int(model.eligible(sc, tags, mask).sum())
    got = fa.topk_from_scores(sc, k, base, tags, mask)
    assert got[0] == min(k, n_el), (got[0], k, n_el)
    assert np.array_equal(bits(got[1]), bits(S[0])) and np.array_equal(got[2], R[0]), (got[1][:8], S[0][:8], got[2][:8], R[0][:8])
    assert (got[2][:got[0]] >= 0).all() and (got[2][got[0]:] == -1).all() and (got[1][got[0]:] == -1.0).all() and not np.isnan(got[1]).any()
    rg = fa.range_from_scores(sc, float("-inf"), k, base, tags, mask)
    assert rg[0] == n_el and np.array_equal(bits(rg[1]), bits(got[1])) and np.array_equal(rg[2], got[2])
    return got


def lib_blocks(sc, k, tags=None, mask=ALL):
    sc = np.ascontiguousarray(sc, np.float32)
    out = np.full(k, -7, np.int64)
    t = None if tags is None else np.ascontiguousarray(tags, np.uint32)
    n = fa.lib().fh_debug_deep_blocks(sc.ctypes.data if sc.size else None, sc.size, None if t is None or sc.size == 0 else t.ctypes.data, mask, k,
                                      out.ctypes.data)
    assert 0 <= n <= k and (out[n:] == -7).all()
    return out[:n]


def check_block_rule(sc, k, tags=None, mask=ALL):
    """The property the device relies on, for one query."""
    sc = np.ascontiguousarray(sc, np.float32)
    blocks = model.chosen_blocks(sc, k, tags, mask)
    assert np.array_equal(lib_blocks(sc, k, tags, mask), blocks)
    nb_live = len(np.unique(np.flatnonzero(model.eligible(sc, tags, mask)) // model.BLOCK))
    assert len(blocks) == min(k, nb_live) <= k
    S, R = model.topk_of_blocks(sc, blocks, k, 5, tags, mask)
    _, s, i = check(sc, k, 5, tags, mask)
    assert np.array_equal(bits(S), bits(s)) and np.array_equal(R, i), (k, np.flatnonzero(R != i)[:6])
    return blocks


def test_the_constant_is_the_header_s():
    assert fa.TOPK_DEEP_MAX == _lib.TOPK_DEEP_MAX == 1024


@pytest.mark.parametrize("n", [1, 2, 31, 1000, 5000])
@pytest.mark.parametrize("k", KS)
def test_random_scores_match_the_model(n, k):
    rng = np.random.default_rng(100 * n + k)
    sc = rng.random(n, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    sc[rng.random(n) < 0.05] = np.nan
    sc[rng.random(n) < 0.02] = np.inf
    sc[rng.random(n) < 0.02] = -np.inf
    if n > 10:
        sc[rng.integers(0, n, n // 4)] = sc[rng.integers(0, n, n // 4)]      # many equal scores
    listed, s, i = check(sc, k, base=int(rng.integers(0, 10**6)))
    if n == 5000:
        assert listed == k
    if n < 17 <= k:
        assert listed < k                                                # n < k: a list cut short


def test_equal_scores_rank_by_index_and_a_k_between_them_keeps_the_lower():
    sc = np.array([0.7, 0.9, 0.9, 0.2, 0.9, 0.7, 0.95], np.float32)
    for k in (1, 2, 3, 4, 5, 7, 8):
        listed, s, i = check(sc, k, base=10)
        assert listed == min(k, 7) and list(i[:listed]) == [16, 11, 12, 14, 10, 15, 13][:k]


def test_nan_and_infinities():
    sc = np.array([np.nan, 0.8, np.nan, 0.3, np.inf, -np.inf], np.float32)
    listed, s, i = check(sc, 8)
    assert listed == 3 and list(i[:3]) == [4, 1, 3] and np.isposinf(s[0])          # +inf leads; NaN and -inf are never listed
    assert check(np.array([np.nan, -np.inf], np.float32), 4)[0] == 0


def test_tags_and_masks():
    rng = np.random.default_rng(4)
    n = 2000
    sc = rng.random(n, dtype=np.float32)
    tags = (np.uint32(1) << rng.integers(0, 8, n).astype(np.uint32)).astype(np.uint32)
    tags[rng.random(n) < 0.1] = 0
    tags[rng.random(n) < 0.1] |= np.uint32(1 << 31)
    for mask in (1, 6, 1 << 31, 0x80000001, ALL, 1 << 20):
        for k in (8, 1024):
            check(sc, k, 5, tags, mask)
    assert check(sc, 1024, 0, tags, 1)[0] == int((tags & 1 != 0).sum()) < 1024    # fewer admitted rows than k
    assert check(sc, 8, 0, tags, 0)[0] == 0                              # a zero mask admits nothing
    assert check(sc, 8, 0, None, 0)[0] == 0                              # ... also on rows without tags
    assert check(sc, 8, 0, None, 4)[0] == 8                              # rows without tags carry all ones


def test_empty_input_and_errors():
    listed, s, i = fa.topk_from_scores(np.empty(0, np.float32), 4)
    assert listed == 0 and (s == -1.0).all() and (i == -1).all() and len(s) == 4
    L = fa.lib()
    sc = np.array([0.6, 0.7], np.float32)
    out_s, out_i = np.full(1025, 7.0, np.float32), np.full(1025, -7, np.int32)
    a = (out_s.ctypes.data, out_i.ctypes.data)
    for bad_k in (0, 1025, -1):
        assert L.fh_topk_from_scores(sc.ctypes.data, 2, 0, None, ALL, bad_k, *a) == FH_ERR_ARG
    assert L.fh_topk_from_scores(None, 2, 0, None, ALL, 4, *a) == FH_ERR_ARG
    assert L.fh_topk_from_scores(sc.ctypes.data, -1, 0, None, ALL, 4, *a) == FH_ERR_ARG
    assert L.fh_topk_from_scores(sc.ctypes.data, 2, 2**31 - 2, None, ALL, 4, *a) == FH_ERR_ARG
    assert L.fh_topk_from_scores(sc.ctypes.data, 2, -1, None, ALL, 4, *a) == FH_ERR_ARG
    assert (out_s == 7.0).all() and (out_i == -7).all()                  # nothing was written
    assert L.fh_topk_from_scores(sc.ctypes.data, 2, 2**31 - 3, None, ALL, 4, *a) == 2 and list(out_i[:4]) == [2**31 - 2, 2**31 - 3, -1, -1]
    assert (out_s[4:] == 7.0).all() and (out_i[4:] == -7).all()          # nothing behind [k]
    assert L.fh_topk_from_scores(sc.ctypes.data, 2, 0, None, ALL, 1, None, out_i.ctypes.data) == 1 and out_i[0] == 1     # either list may be null
    assert L.fh_topk_from_scores(sc.ctypes.data, 2, 0, None, ALL, 1, out_s.ctypes.data, None) == 1
    blocks = np.zeros(4, np.int64)
    assert L.fh_debug_deep_blocks(sc.ctypes.data, 2, None, ALL, 0, blocks.ctypes.data) == FH_ERR_ARG
    assert L.fh_debug_deep_blocks(sc.ctypes.data, 2, None, ALL, 4, None) == FH_ERR_ARG
    with pytest.raises(fa.FaceHipError):
        fa.topk_from_scores(sc, 0)
    with pytest.raises(ValueError):
        fa.topk_from_scores(sc, 4, tags=np.zeros(3, np.uint32))


# ------------------------------------------------------------------------------------------ the block rule
@pytest.mark.parametrize("seed", range(6))
def test_block_rule_on_random_scores(seed):
    rng = np.random.default_rng(50 + seed)
    n = int(rng.integers(1, 6000))
    sc = rng.random(n, dtype=np.float32)
    sc[rng.random(n) < 0.05] = np.nan
    sc[rng.random(n) < 0.01] = -np.inf
    sc[rng.random(n) < 0.005] = np.inf
    sc[rng.integers(0, n, n // 3)] = sc[rng.integers(0, n, n // 3)]
    tags = (np.uint32(1) << rng.integers(0, 4, n).astype(np.uint32)).astype(np.uint32)
    tags[rng.random(n) < 0.3] = 0
    for k in KS:
        check_block_rule(sc, k)
        check_block_rule(sc, k, tags, 3)
        check_block_rule(sc, k, tags, 1 << 9)                            # nothing admitted: no block chosen


def test_block_rule_when_all_scores_are_equal():
    sc = np.full(300, 0.75, np.float32)
    for k in (1, 8, 9, 10, 33, 300, 301):
        blocks = check_block_rule(sc, k)
        assert list(blocks) == list(range(min(k, 10)))                  # every block ties: the first k of the 10
        assert list(fa.topk_from_scores(sc, k, 7)[2][:min(k, 300)]) == list(range(7, 7 + min(k, 300)))


def test_block_rule_with_duplicates_at_block_borders():
    rng = np.random.default_rng(9)
    sc = (rng.random(300, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    sc[[31, 32, 33, 95, 96, 127, 128, 255, 256]] = np.float32(0.9)       # the best score, in blocks 0, 1, 2, 3, 4, 7, 8
    for k in (1, 2, 3, 4, 5, 6, 8, 9, 10, 17):
        blocks = check_block_rule(sc, k)
        assert list(blocks[:7]) == [0, 1, 2, 3, 4, 7, 8][:k]
        assert list(fa.topk_from_scores(sc, k)[2][:min(k, 9)]) == [31, 32, 33, 95, 96, 127, 128, 255, 256][:k]


def test_block_rule_when_one_block_holds_the_whole_top():
    rng = np.random.default_rng(10)
    sc = (rng.random(300, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    sc[32:64] = np.float32(0.6) + np.arange(32, dtype=np.float32) * np.float32(0.01)
    for k in (8, 32, 33):
        blocks = check_block_rule(sc, k)
        assert blocks[0] == 1 and len(blocks) == min(k, 10)
        assert set(fa.topk_from_scores(sc, k)[2][:min(k, 32)]) <= set(range(32, 64))
