"""The host rule of the pair audit (fh_pairs_from_scores, csrc/pairs_plan.h) against the numpy model of tests/pairs_model.py.  No GPU.
Counts, score bits, positions and ids must be IDENTICAL: there is no tolerance."""
import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import pairs_model as pm
from tests import roc_model as rm

FH_ERR_ARG = -1


def sym(rng, n, lo=-0.1, hi=1.1, dup=0.0, nan_rows=()):
    """a symmetric float32 matrix of scores; dup: the share of entries copied from another one (equal scores); nan_rows: all-NaN rows"""
    s = rng.uniform(lo, hi, (n, n)).astype(np.float32)
    if n and dup:
        flat = s.reshape(-1)
        k = int(dup * flat.size)
        flat[rng.integers(0, flat.size, k)] = flat[rng.integers(0, flat.size, k)]
    s = np.triu(s, 1)
    s = s + s.T
    for r in nan_rows:
        s[r, :] = np.nan
        s[:, r] = np.nan
    return np.ascontiguousarray(s)


def same(got, want, what):
    gi, gs, gr, gd = got
    wi, ws, wr, wd = want
    assert [gi[k] for k in ("count", "nan", "returned", "complete")] == [int(x) for x in wi], (what, gi, wi)
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), what
    assert np.array_equal(gr, wr), what
    assert np.array_equal(gd, wd), what


def both(S, ids, cls, side, thr, cap, room=None):
    want = pm.pairs(S, ids, cls, side, thr, cap, room)
    got = fa.pairs_from_scores(S, ids, cls, side, thr, cap, room)
    same(got, want, (cls, side, float(thr), cap, room))
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 3, 37, 150])
def test_random_matrices_all_classes_sides_and_caps(n):
    rng = np.random.default_rng(100 + n)
    S = sym(rng, n, dup=0.2, nan_rows=(5, 20) if n > 30 else ())
    ids = rng.integers(0, max(n // 4, 1), n).astype(np.int32) * 31 + 3
    regimes = set()
    for cls in pm.CLASSES:
        total = pm.class_total(n, ids, cls)
        for thr in (0.5, 517 / 2048, 0.93, 1900 / 2048, 0.017, -1.0, 2.0, np.inf, -np.inf):       # on and off bin edges, nothing / all
            thr = np.float32(thr)
            seen = []
            for side in pm.SIDES:
                for cap in (1, 7, 1024):
                    info = both(S, ids, cls, side, thr, cap)[0]
                    regimes.add(("<", "==", ">")[int(np.sign(int(info[0]) - cap)) + 1])
                seen.append(info)
            assert int(seen[0][0]) + int(seen[1][0]) + int(seen[0][1]) == total and seen[0][1] == seen[1][1]
    if n >= 37:
        assert {"<", ">"} <= regimes, regimes                       # (count == cap: test_count_equal_to_cap)
    # without ids only "any" is legal, and the id lists stay empty
    for side in pm.SIDES:
        info, _, _, d = both(S, None, "any", side, np.float32(0.5), 7)
        assert (d == -1).all()


def test_count_equal_to_cap():
    rng = np.random.default_rng(3)
    S = sym(rng, 60)
    ids = rng.integers(0, 12, 60).astype(np.int32)
    s, _, _, _ = pm.selected(S, ids, "impostor", "above", -np.inf)
    assert len(s) > 1024
    for cap in (7, 1024):
        thr = s[cap]                                               # exactly `cap` scores are strictly above the (cap + 1)-th (no ties here)
        assert s[cap - 1] > thr
        info = both(S, ids, "impostor", "above", thr, cap)[0]
        assert int(info[0]) == cap == int(info[2]) and int(info[3]) == 1
        both(S, ids, "impostor", "above", thr, cap + 1 if cap < 1024 else cap - 1)


def test_equal_scores_are_listed_in_pair_order():
    n = 50
    S = np.full((n, n), 0.75, np.float32)
    ids = (np.arange(n) % 5).astype(np.int32)
    for cls in pm.CLASSES:
        for side, thr in (("above", 0.5), ("not_above", 0.75)):
            for cap in (1, 7, 1024):
                info, s, r, _ = both(S, ids, cls, side, np.float32(thr), cap)
                m = int(info[2])
                assert m == min(cap, int(info[0])) and (s[:m] == 0.75).all()
                assert [tuple(x) for x in r[:m]] == sorted(tuple(x) for x in r[:m])
    assert both(S, ids, "any", "above", np.float32(0.75), 7)[0][0] == 0           # strict


def test_the_cut_when_the_boundary_bin_does_not_fit():
    rng = np.random.default_rng(9)
    n = 120
    S = sym(rng, n, lo=0.2, hi=0.9)
    ids = rng.integers(0, 30, n).astype(np.int32)
    S2 = S.copy()
    blk = np.arange(40)
    S2[np.ix_(blk, blk)] = np.float32(0.95)                        # 780 pairs in one bin, the most extreme one for "above"
    hit = {0: 0, 1: 0}
    for M, what in ((S, "spread"), (S2, "one heavy bin")):
        for cls in pm.CLASSES:
            for side in pm.SIDES:
                for cap in (1, 7, 100, 1024):
                    for room in (cap, cap + 1, 2 * cap, 10 * cap):
                        info = both(M, ids, cls, side, np.float32(0.5), cap, room)[0]
                        hit[int(info[3])] += 1
                        if int(info[3]) == 0:
                            assert int(info[2]) < cap and int(info[0]) > int(info[2])
    assert hit[0] > 20 and hit[1] > 20, hit
    # room == cap on the heavy bin: nothing can be returned, the count is still exact
    info, s, r, d = both(S2, ids, "any", "above", np.float32(0.9), 8, 8)
    assert [int(x) for x in info] == [780, 0, 0, 0] and (s == -1).all() and (r == -1).all() and (d == -1).all()
    # a room that holds the boundary bin exactly, and one smaller
    s_all, _, _, _ = pm.selected(S2, ids, "any", "above", 0.5)
    b = rm.bins(s_all)
    cap = 900                                                      # beyond the 780: the boundary bin lies further down
    bstar = b[cap - 1]
    need = int((b >= bstar).sum())
    strict = int((b > bstar).sum())
    assert strict < cap <= need
    assert [int(x) for x in both(S2, ids, "any", "above", np.float32(0.5), cap, max(need, cap))[0][2:]] == [cap, 1]
    if need > cap:
        assert [int(x) for x in both(S2, ids, "any", "above", np.float32(0.5), cap, need - 1)[0][2:]] == [strict, 0]


def test_count_above_at_a_bin_edge_is_the_histogram_suffix_sum():
    rng = np.random.default_rng(21)
    n = 90
    S = sym(rng, n, dup=0.1, nan_rows=(11,))
    iu = np.triu_indices(n, 1)
    S[iu] = np.round(S[iu] * 512) / 512                             # many scores exactly on bin edges
    S = np.ascontiguousarray(np.triu(S, 1) + np.triu(S, 1).T)
    ids = rng.integers(0, 20, n).astype(np.int32)
    hist, nan = rm.pair_hist(S, ids)
    planes = {"genuine": hist[0], "impostor": hist[1], "any": hist[0] + hist[1]}
    nans = {"genuine": int(nan[0]), "impostor": int(nan[1]), "any": int(nan.sum())}
    for cls in pm.CLASSES:
        suffix = np.cumsum(planes[cls][::-1].astype(np.int64))[::-1]
        for b in (1, 2, 100, 512, 1023, 1024, 1025, 1536, 2046, 2047):
            info = both(S, ids, cls, "above", np.float32(b / 2048), 7)[0]
            assert int(info[0]) == int(suffix[b]) and int(info[1]) == nans[cls], (cls, b)


def test_argument_errors_write_nothing():
    L = _lib.lib()
    S = sym(np.random.default_rng(1), 4)
    ids = np.array([1, 1, 2, 2], np.int32)
    info = np.full(4, 77, np.uint64)
    s = np.full(8, 7.0, np.float32)
    r = np.full((8, 2), -7, np.int32)
    d = np.full((8, 2), -7, np.int32)

    def call(scores=S.ctypes.data, n=4, idp=ids.ctypes.data, cls=0, side=0, thr=0.5, cap=8, room=8, infop=info.ctypes.data):
        return L.fh_pairs_from_scores(scores, n, idp, cls, side, thr, cap, room, infop, s.ctypes.data, r.ctypes.data, d.ctypes.data)

    assert call() >= 0                                             # the baseline is a legal call
    info[:] = 77; s[:] = 7.0; r[:] = -7; d[:] = -7
    for kw in (dict(n=-1), dict(scores=None), dict(infop=None), dict(thr=float("nan")), dict(cls=3), dict(cls=-1), dict(side=2), dict(side=-1),
               dict(idp=None, cls=0), dict(idp=None, cls=1), dict(cap=0), dict(cap=_lib.PAIRS_MAX_CAP + 1), dict(room=7), dict(cap=-3)):
        assert call(**kw) == FH_ERR_ARG, kw
        assert _lib.last_error()
    assert (info == 77).all() and (s == 7.0).all() and (r == -7).all() and (d == -7).all()
    with pytest.raises(ValueError):
        fa.pairs_from_scores(S, ids, "other", "above", 0.5)
    with pytest.raises(ValueError):
        fa.pairs_from_scores(S[:3], ids, "any", "above", 0.5)
    # any subset of the lists may be null; n == 0 with null scores is legal
    assert L.fh_pairs_from_scores(S.ctypes.data, 4, ids.ctypes.data, 2, 0, -1.0, 8, 8, info.ctypes.data, None, None, None) == 6
    assert [int(x) for x in info] == [6, 0, 6, 1]
    assert L.fh_pairs_from_scores(None, 0, None, 2, 1, 0.5, 8, 8, info.ctypes.data, s.ctypes.data, None, None) == 0
    assert [int(x) for x in info] == [0, 0, 0, 1] and (s == -1).all()
