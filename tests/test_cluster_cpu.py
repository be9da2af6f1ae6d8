"""The clustering rule on the host (fh_cluster_scores, csrc/cluster_plan.h) against the numpy model of tests/cluster_model.py: seeded
random symmetric matrices, and crafted matrices — a chain, tied and two-sided border rows, NaN, the strict threshold, a garbage lower
triangle — each of which first proves ON THE MODEL that it contains what it claims.  No GPU."""
import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import cluster_model as cm

FH_ERR_ARG = -1


def both(s, thr, min_pts, noise):
    want_l, want_i = cm.cluster(s, thr, min_pts, noise)
    got_l, got_i = fa.cluster_scores(s, thr, min_pts, noise)
    assert got_l.dtype == np.int32 and got_i.dtype == np.int32
    assert np.array_equal(got_l, want_l), (thr, min_pts, noise, np.flatnonzero(got_l != want_l)[:8])
    assert np.array_equal(got_i, want_i), (thr, min_pts, noise, got_i, want_i)
    assert got_i[1:].sum() == len(s)
    return want_l, want_i


def sym(n, fill=0.0):
    return np.full((n, n), fill, np.float32)


def link(s, i, j, v):
    s[i, j] = s[j, i] = np.float32(v)


@pytest.mark.parametrize("min_pts", [1, 2, 3, 5])
@pytest.mark.parametrize("noise", ["none", "self"])
def test_random_symmetric_matrices(min_pts, noise):
    rng = np.random.default_rng(100 * min_pts + len(noise))
    seen = np.zeros(4, np.int64)
    for n in (0, 1, 2, 3, 7, 31, 64, 65, 130, 200):
        for density in (0.5, 2.0, 6.0):                          # expected edges per row
            a = rng.random((n, n), dtype=np.float32)
            s = np.triu(a, 1) + np.triu(a, 1).T
            thr = np.float32(1.0 - min(1.0, density / max(n, 1)))
            _, info = both(s, thr, min_pts, noise)
            seen += info
    # every kind of row was exercised (a non-core row at min_pts 2 has no neighbour at all: border rows need min_pts >= 3)
    assert (seen[:2] > 0).all() and (min_pts < 3 or seen[2] > 0) and (min_pts < 2 or seen[3] > 0)


def test_chain_is_single_linkage_and_its_ends_become_border_rows():
    n = 9
    s = sym(n, 0.1)
    for t in range(n - 1):
        link(s, t, t + 1, 0.9)
    labels, info = both(s, 0.5, 1, "none")
    assert (labels == 0).all() and tuple(info) == (1, n, 0, 0)
    core, border, noise = cm.kinds(s, 0.5, 3)
    assert border[0] and border[-1] and core[1:-1].all() and not noise.any()
    labels, info = both(s, 0.5, 3, "none")
    assert (labels == 1).all() and tuple(info) == (1, n - 2, 2, 0)       # the smallest CORE position


def two_clusters_and_a_border_row():
    """rows 0-2 and 3-5: two triangles (core at min_pts 3); row 6 touches 1 and 4 only (degree 2 + itself: core at 3 — so min_pts is 4
    and the triangles get a fourth member each: rows 7 and 8); row 9 is alone."""
    s = sym(10, 0.0)
    for grp in ((0, 1, 2, 7), (3, 4, 5, 8)):
        for i in grp:
            for j in grp:
                if i < j:
                    link(s, i, j, 0.9)
    return s


def test_border_row_tied_between_two_clusters_takes_the_lower_position():
    s = two_clusters_and_a_border_row()
    link(s, 6, 4, 0.75)
    link(s, 6, 1, 0.75)                                           # the same bits from both clusters
    core, border, noise = cm.kinds(s, 0.5, 4)
    want, info = cm.cluster(s, 0.5, 4, "none")
    assert border[6] and noise[9] and info[0] == 2 and want[1] != want[4]
    labels, _ = both(s, 0.5, 4, "none")
    assert labels[6] == labels[1] == 0
    link(s, 6, 4, np.nextafter(np.float32(0.75), np.float32(1)))  # one ulp better: the other cluster wins
    labels, _ = both(s, 0.5, 4, "self")
    assert labels[6] == labels[4] == 3 and labels[9] == 9


def test_border_row_between_two_clusters_does_not_merge_them():
    s = two_clusters_and_a_border_row()
    link(s, 6, 2, 0.8)
    link(s, 6, 3, 0.7)
    core, border, noise = cm.kinds(s, 0.5, 4)
    assert border[6] and noise[9] and core[[2, 3]].all()
    labels, info = both(s, 0.5, 4, "none")
    assert info[0] == 2 and labels[2] == 0 and labels[3] == 3 and labels[6] == 0 and labels[9] == -1
    # the same graph at min_pts 1: now row 6 is core and DOES merge them
    labels, info = both(s, 0.5, 1, "none")
    assert info[0] == 2 and (labels[:9] == 0).all() and labels[9] == 9


def test_nan_entries_and_a_nan_threshold_give_no_edge():
    s = two_clusters_and_a_border_row()
    link(s, 6, 2, np.nan)
    link(s, 9, 0, np.nan)
    link(s, 6, 3, 0.7)
    for min_pts in (1, 4):
        for noise in ("none", "self"):
            labels, info = both(s, 0.5, min_pts, noise)
            assert labels[9] == (9 if noise == "self" or min_pts == 1 else -1) and labels[6] == 3
    core, border, noise = cm.kinds(s, 0.5, 4)
    assert border[6] and noise[9] and cm.cluster(s, 0.5, 4)[1][0] == 2
    for min_pts in (1, 2):
        labels, info = both(s, np.nan, min_pts, "none")
        assert info[0] == (10 if min_pts == 1 else 0) and info[3] == (0 if min_pts == 1 else 10)


def test_the_threshold_is_strict_to_the_bit():
    s = two_clusters_and_a_border_row()
    v = np.float32(0.7312345)
    link(s, 6, 3, v)
    core, border, noise = cm.kinds(s, np.nextafter(v, np.float32(0)), 4)
    assert border[6] and noise[9] and cm.cluster(s, v, 4)[1][0] == 2
    labels, info = both(s, v, 4, "none")                          # thr == the entry's exact bits: no edge
    assert labels[6] == -1 and info[3] == 2
    labels, info = both(s, np.nextafter(v, np.float32(0)), 4, "none")
    assert labels[6] == 3 and info[2] == 1 and info[3] == 1


def test_the_lower_triangle_and_the_diagonal_are_never_read():
    rng = np.random.default_rng(5)
    s = two_clusters_and_a_border_row()
    link(s, 6, 2, 0.8)
    want = {(m, z): cm.cluster(s, 0.5, m, z) for m in (1, 4) for z in ("none", "self")}
    core, border, noise = cm.kinds(s, 0.5, 4)
    assert border.any() and noise.any() and want[(4, "none")][1][0] == 2
    g = s.copy()
    lo = np.tril_indices(len(s), 0)
    g[lo] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, 0.99, -5.0], np.float32), len(lo[0]))
    for (m, z), (wl, wi) in want.items():
        gl, gi = fa.cluster_scores(g, 0.5, m, z)
        assert np.array_equal(gl, wl) and np.array_equal(gi, wi), (m, z)


def test_argument_errors_leave_the_outputs_untouched():
    L = fa.lib()
    s = two_clusters_and_a_border_row()
    n = len(s)
    labels, info = np.full(n, 77, np.int32), np.full(4, 77, np.int32)
    sp, lp, ip = s.ctypes.data, labels.ctypes.data, info.ctypes.data
    for args in ((sp, -1, 0.5, 1, 0, lp, ip), (sp, n, 0.5, 0, 0, lp, ip), (sp, n, 0.5, -3, 1, lp, ip), (sp, n, 0.5, 1, 2, lp, ip),
                 (sp, n, 0.5, 1, -1, lp, ip), (None, n, 0.5, 1, 0, lp, ip), (sp, n, 0.5, 1, 0, None, ip)):
        assert L.fh_cluster_scores(*args) == FH_ERR_ARG, args[1:5]
        assert _lib.last_error()
        assert (labels == 77).all() and (info == 77).all()
    with pytest.raises(fa.FaceHipError):
        fa.cluster_scores(s, 0.5, 0)
    with pytest.raises(ValueError):
        fa.cluster_scores(s, 0.5, 1, "other")
    # n == 0: 0 clusters, NULL matrix and labels are fine, info is written; info may be NULL
    assert L.fh_cluster_scores(None, 0, 0.5, 1, 0, None, ip) == 0 and (info == 0).all()
    assert L.fh_cluster_scores(sp, n, 0.5, 4, 0, lp, None) == 2 and labels[9] == -1
    one = np.zeros((1, 1), np.float32)
    for min_pts, want in ((1, (1, 1, 0, 0)), (2, (0, 0, 0, 1))):
        l1, i1 = fa.cluster_scores(one, 0.0, min_pts, "self")
        assert tuple(i1) == want and l1[0] == 0
