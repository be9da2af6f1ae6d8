"""Host-side contract of the labelled gallery (fh_gallery_*_ids, fh_topk_merge_ids_dev) and the claims its numpy model
(tests/gallery_ids_model.py) rests on.  No GPU needed: a fresh gallery handle owns no device memory and the argument checks come
before any device work."""
import ctypes as C

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from oracle import oracle
from tests import gallery_ids_model as model

FH_ERR_ARG = -1
NEW = ("fh_gallery_enroll_ids", "fh_gallery_upload_ids", "fh_gallery_topk_ids_dev", "fh_gallery_label_ids_dev", "fh_gallery_remove_ids",
       "fh_gallery_get_ids", "fh_topk_merge_ids_dev")


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_identity_symbols_resolve():
    L = fa.lib()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    assert callable(fa.topk_merge_ids_dev)
    for name in ("topk_ids_dev", "label_ids_dev", "remove_ids", "ids"):
        assert callable(getattr(fa.Gallery, name)), name


def test_null_handles_null_pointers_and_sizes_are_argument_errors():
    L = fa.lib()
    buf = (C.c_float * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: the checks come before it is touched
    g = L.fh_gallery_create(64)
    try:
        assert L.fh_gallery_enroll_ids(None, one, one, 1, 0) == FH_ERR_ARG
        assert L.fh_gallery_enroll_ids(g, None, one, 1, 0) == FH_ERR_ARG
        assert L.fh_gallery_enroll_ids(g, one, None, 1, 0) == FH_ERR_ARG
        assert L.fh_gallery_enroll_ids(g, one, one, 0, 0) == FH_ERR_ARG
        assert L.fh_gallery_upload_ids(None, one, one, 1, 0, 0) == FH_ERR_ARG
        assert L.fh_gallery_upload_ids(g, None, one, 1, 0, 0) == FH_ERR_ARG
        assert L.fh_gallery_upload_ids(g, one, None, 1, 0, 0) == FH_ERR_ARG
        assert L.fh_gallery_upload_ids(g, one, one, -3, 0, 0) == FH_ERR_ARG
        T = L.fh_gallery_topk_ids_dev
        assert T(None, one, 1, 1, one, one, one, None) == FH_ERR_ARG
        assert T(g, None, 1, 1, one, one, one, None) == FH_ERR_ARG
        assert T(g, one, 1, 1, None, one, one, None) == FH_ERR_ARG
        assert T(g, one, 1, 1, one, None, one, None) == FH_ERR_ARG
        for nq, k in ((0, 1), (257, 1), (-1, 4), (1, 0), (1, 17), (256, -1)):
            assert T(g, one, nq, k, one, one, None, None) == FH_ERR_ARG, (nq, k)
            assert "fh_gallery_topk_ids_dev" in _lib.last_error()
        B = L.fh_gallery_label_ids_dev
        assert B(None, one, 1, 0.6, one, one, None) == FH_ERR_ARG
        assert B(g, None, 1, 0.6, one, one, None) == FH_ERR_ARG
        assert B(g, one, 1, 0.6, None, one, None) == FH_ERR_ARG
        assert B(g, one, 1, 0.6, one, None, None) == FH_ERR_ARG
        assert B(g, one, 0, 0.6, one, one, None) == FH_ERR_ARG and B(g, one, 257, 0.6, one, one, None) == FH_ERR_ARG
        assert L.fh_gallery_remove_ids(None, one, 1) == FH_ERR_ARG
        assert L.fh_gallery_remove_ids(g, None, 1) == FH_ERR_ARG
        assert L.fh_gallery_remove_ids(g, one, 0) == FH_ERR_ARG
        assert L.fh_gallery_get_ids(None, 0, 0, one) == FH_ERR_ARG
        assert L.fh_gallery_get_ids(g, -1, 0, one) == FH_ERR_ARG
        assert L.fh_gallery_get_ids(g, 0, 1, None) == FH_ERR_ARG
        assert L.fh_gallery_get_ids(g, 0, 1, one) == FH_ERR_ARG    # beyond the (empty) gallery
        assert L.fh_gallery_size(g) == 0
    finally:
        L.fh_gallery_destroy(g)
    M = L.fh_topk_merge_ids_dev
    for nulls in range(6):
        args = [one] * 6
        args[nulls] = None
        assert M(args[0], args[1], args[2], 2, 3, 4, args[3], args[4], args[5], None) == FH_ERR_ARG
        assert "null argument" in _lib.last_error()
    for nparts, nq, k in ((2, 3, 0), (2, 3, 17), (4097, 1, 16), (65537, 1, 1), (0, 3, 4), (2, 0, 4)):
        assert M(one, one, one, nparts, nq, k, one, one, one, None) == FH_ERR_ARG, (nparts, nq, k)
        assert "fh_topk_merge_ids_dev: bad size" in _lib.last_error()


def test_a_negative_id_in_a_host_list_is_an_argument_error_and_changes_nothing():
    L = fa.lib()
    rows = np.zeros((3, 64), np.float32)
    ids = np.array([4, -1, 9], np.int32)
    g = L.fh_gallery_create(64)
    try:
        assert L.fh_gallery_enroll_ids(g, rows.ctypes.data, ids.ctypes.data, 3, 0) == FH_ERR_ARG
        assert "negative id" in _lib.last_error()
        assert L.fh_gallery_upload_ids(g, rows.ctypes.data, ids.ctypes.data, 3, 0, 0) == FH_ERR_ARG
        assert L.fh_gallery_remove_ids(g, ids.ctypes.data, 3) == FH_ERR_ARG
        assert L.fh_gallery_size(g) == 0
    finally:
        L.fh_gallery_destroy(g)
    pg = fa.Gallery(64)
    with pytest.raises(_lib.FaceHipError, match="negative id"):
        pg.enroll(rows, ids=ids)
    with pytest.raises(_lib.FaceHipError, match="negative id"):
        pg.remove_ids([3, -7])
    assert len(pg) == 0 and pg.remove_ids([]) == 0 and pg.ids().shape == (0,)


def clustered_labelled(rng, dim, n_ids):
    """1 to 40 templates per identity (a centre plus noise), rows shuffled, sparse unsorted ids, and exact duplicate rows across
    identities."""
    per = rng.integers(1, 41, n_ids)
    labels = rng.permutation(10 * n_ids)[:n_ids].astype(np.int32) * 7 + 3
    centres = unit(rng, n_ids, dim)
    rows = np.repeat(centres, per, axis=0) + np.float32(0.05) * rng.standard_normal((per.sum(), dim), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = np.repeat(labels, per)
    o = rng.permutation(len(ids))
    rows, ids = rows[o], ids[o]
    for _ in range(12):                                          # exact copies of a row under another identity
        a, b = rng.integers(0, len(ids), 2)
        rows[b] = rows[a]
    return np.ascontiguousarray(rows, np.float32), ids


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merging_per_part_identity_lists_is_the_identity_list_of_the_whole(seed):
    """The decomposition the scan and the sharded merge rely on: cut the gallery into contiguous parts, take each part's identity
    top-k, merge the lists (keep an identity's best entry) -> the identity top-k of the whole gallery, for every k in 1..16."""
    rng = np.random.default_rng(1000 + seed)
    dim, base = 64, 1000 * seed
    rows, ids = clustered_labelled(rng, dim, 40)
    G = len(ids)
    q = np.concatenate([unit(rng, 3, dim), rows[rng.integers(0, G, 3)]])       # some queries ARE a (possibly duplicated) row
    sc = model.scores(q, rows)
    for k in range(1, 17):
        whole = model.topk_ids_from_scores(sc, ids, k, base)
        for W in (1, 2, int(rng.integers(3, 9)), 37):
            cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, G), W - 1, replace=False)), [G]]) if W > 1 else np.array([0, G])
            parts = [model.topk_ids_from_scores(sc[:, a:b], ids[a:b], k, base + a) for a, b in zip(cuts[:-1], cuts[1:])]
            ps, pd, pr = (np.stack([p[j] for p in parts]) for j in range(3))
            got = model.merge_ids(ps, pd, pr, k)
            for a, b, what in zip(got, whole, ("scores", "ids", "rows")):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), \
                    (what, k, W)
    # the crowding the feature exists for: at k = 16 the row-level answer of a query holds fewer identities than the identity answer
    rs, ri = oracle.gallery_topk_mfma(q, rows, 16, base=base)
    S, D, R = model.topk_ids_from_scores(sc, ids, 16, base)
    assert all(len(set(D[i])) == 16 for i in range(len(q)))
    assert any(len(set(ids[ri[i] - base])) < 16 for i in range(len(q)))


@pytest.mark.parametrize("dim,G", [(64, 1), (64, 300), (192, 1000)])
def test_with_distinct_ids_the_model_is_the_row_level_model(dim, G):
    rng = np.random.default_rng(2000 + dim + G)
    rows, q = unit(rng, G, dim), unit(rng, 5, dim)
    rows[G // 2] = rows[0]                                        # a tie: the lower row first
    if G > 10:
        rows[7, 3] = np.nan
    labels = (rng.permutation(5 * G)[:G] * 11 + 1).astype(np.int32)
    for k in (1, 5, 16):
        for base in (0, 123456):
            S, D, R = model.topk_ids(q, rows, labels, k, base)
            ms, mi = oracle.gallery_topk_mfma(q, rows, k, base=base)
            assert np.array_equal(R, mi) and np.array_equal(S.view(np.uint32), ms.view(np.uint32))
            assert np.array_equal(D, np.where(mi >= 0, labels[np.maximum(mi - base, 0)], -1))
