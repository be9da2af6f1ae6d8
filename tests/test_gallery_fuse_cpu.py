"""Host-side contract of template pooling (fh_gallery_group_ids, fh_gallery_fuse_ids, fh_gallery_get_rows, fh_gallery_self_scores_dev)
and the claims its numpy model (tests/gallery_fuse_model.py) rests on.  No GPU needed: fh_gallery_group_ids is host code, a fresh gallery
handle owns no device memory, and the argument and state checks come before any device work."""
import ctypes as C

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import gallery_fuse_model as fm

FH_ERR_ARG, FH_ERR_STATE = -1, -4
NEW = ("fh_gallery_group_ids", "fh_gallery_fuse_ids", "fh_gallery_get_rows", "fh_gallery_self_scores_dev")


def test_fuse_symbols_resolve():
    L = fa.lib()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    assert callable(fa.group_ids)
    for name in ("fuse", "rows", "self_scores_dev"):
        assert callable(getattr(fa.Gallery, name)), name


def check_grouping(ids):
    ids = np.asarray(ids, np.int32)
    order, starts, uniq = fa.group_ids(ids)
    assert order.dtype == np.int32 and starts.dtype == np.int64 and uniq.dtype == np.int32
    assert np.array_equal(order, np.argsort(ids, kind="stable"))
    want_uniq, counts = np.unique(ids, return_counts=True)
    assert np.array_equal(uniq, want_uniq)
    assert np.array_equal(starts, np.concatenate([[0], np.cumsum(counts)]))
    mo, ms, mu = fm.group(ids)                                   # the model groups the same way
    assert np.array_equal(order, mo) and np.array_equal(starts, ms) and np.array_equal(uniq, mu)
    return order, starts, uniq


def test_group_ids_against_numpy():
    rng = np.random.default_rng(1)
    pool = (rng.permutation(100000)[:300] * 9 + 4).astype(np.int32)
    check_grouping(rng.choice(pool, 5000))                       # sparse, unsorted, repeated
    check_grouping(np.concatenate([rng.choice(pool, 700), [0, 2 ** 31 - 1, 0, 2 ** 31 - 1]]))
    order, starts, uniq = check_grouping(np.full(777, 42))       # all equal
    assert list(starts) == [0, 777] and list(uniq) == [42] and np.array_equal(order, np.arange(777))
    order, starts, uniq = check_grouping(rng.permutation(1000) * 3)          # all distinct
    assert len(uniq) == 1000 and np.array_equal(starts, np.arange(1001))
    order, starts, uniq = fa.group_ids([])                       # n = 0
    assert order.shape == (0,) and uniq.shape == (0,) and list(starts) == [0]
    L = fa.lib()
    assert L.fh_gallery_group_ids(None, 0, None, None, None) == 0


def test_group_ids_output_pointers_are_optional_and_a_negative_id_is_an_argument_error():
    L = fa.lib()
    ids = np.array([7, 3, 7, 1, 3, 7], np.int32)
    n = len(ids)
    assert L.fh_gallery_group_ids(ids.ctypes.data, n, None, None, None) == 3
    order, starts, uniq = np.full(n, -5, np.int32), np.full(n + 1, -5, np.int64), np.full(n, -5, np.int32)
    assert L.fh_gallery_group_ids(ids.ctypes.data, n, order.ctypes.data, None, None) == 3 and list(order) == [3, 1, 4, 0, 2, 5]
    assert L.fh_gallery_group_ids(ids.ctypes.data, n, None, starts.ctypes.data, None) == 3 and list(starts[:4]) == [0, 1, 3, 6]
    assert L.fh_gallery_group_ids(ids.ctypes.data, n, None, None, uniq.ctypes.data) == 3 and list(uniq[:3]) == [1, 3, 7]
    bad = np.array([7, 3, -1, 1], np.int32)
    order[:] = -5; starts[:] = -5; uniq[:] = -5
    assert L.fh_gallery_group_ids(bad.ctypes.data, 4, order.ctypes.data, starts.ctypes.data, uniq.ctypes.data) == FH_ERR_ARG
    assert "negative id" in _lib.last_error()
    assert (order == -5).all() and (starts == -5).all() and (uniq == -5).all()        # an error writes nothing
    assert L.fh_gallery_group_ids(None, 3, None, None, None) == FH_ERR_ARG
    assert L.fh_gallery_group_ids(ids.ctypes.data, -1, None, None, None) == FH_ERR_ARG
    with pytest.raises(_lib.FaceHipError, match="negative id"):
        fa.group_ids([1, 2, -3])


def test_argument_and_state_errors_on_fresh_handles():
    L = fa.lib()
    buf = (C.c_float * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: the checks come before it is touched
    a, b, wide = L.fh_gallery_create(64), L.fh_gallery_create(64), L.fh_gallery_create(128)
    try:
        F = L.fh_gallery_fuse_ids
        assert F(None, b, 0) == FH_ERR_ARG and F(a, None, 0) == FH_ERR_ARG
        assert F(a, a, 0) == FH_ERR_ARG and "different" in _lib.last_error()
        assert F(a, wide, 0) == FH_ERR_ARG and "dims" in _lib.last_error()
        assert F(a, b, 2) == FH_ERR_ARG and F(a, b, -1) == FH_ERR_ARG and "mode" in _lib.last_error()
        assert F(a, b, 0) == 0 and F(a, b, 1) == 0                # an empty source: nothing to do, no device work
        assert L.fh_gallery_size(a) == 0 and L.fh_gallery_size(b) == 0
        R = L.fh_gallery_get_rows
        assert R(None, 0, 0, one) == FH_ERR_ARG
        assert R(a, -1, 0, one) == FH_ERR_ARG and R(a, 0, -1, one) == FH_ERR_ARG
        assert R(a, 0, 1, None) == FH_ERR_ARG
        assert R(a, 0, 1, one) == FH_ERR_ARG and "range" in _lib.last_error()      # beyond the (empty) gallery
        assert R(a, 1, 0, one) == FH_ERR_ARG
        assert R(a, 0, 0, None) == 0
        S = L.fh_gallery_self_scores_dev
        assert S(None, b, one, None) == FH_ERR_ARG and S(a, None, one, None) == FH_ERR_ARG and S(a, b, None, None) == FH_ERR_ARG
        assert S(a, wide, one, None) == FH_ERR_ARG and "dims" in _lib.last_error()
        fresh = L.fh_gallery_create(64)                            # never the result of a fuse
        try:
            assert S(a, fresh, one, None) == FH_ERR_STATE and "fh_gallery_fuse_ids" in _lib.last_error()
        finally:
            L.fh_gallery_destroy(fresh)
        assert S(a, b, one, None) == 0                            # b IS the (empty) result of a fuse; a has no rows to score
    finally:
        for g in (a, b, wide):
            L.fh_gallery_destroy(g)
    g = fa.Gallery(64)
    with pytest.raises(ValueError, match="fuse mode"):
        g.fuse(mode="mean")
    d = g.fuse()
    assert isinstance(d, fa.Gallery) and d.dim == 64 and len(d) == 0 and d.rows().shape == (0, 64) and g.rows().shape == (0, 64)
    assert g.fuse(d, mode="sum") is d


# ------------------------------------------------------------------------------------------ the model's own claims
def test_model_keeps_a_one_template_identity_verbatim():
    rows, ids, _, _ = fm.clustered_case(64, G=600)
    sums, uniq, counts = fm.fuse_sums(rows, ids)
    single = np.flatnonzero(counts == 1)
    assert len(single) >= 2
    u64 = fm.unit64(sums, counts)
    for j in single:
        src = rows[ids == uniq[j]][0]
        assert np.array_equal(sums[j].view(np.uint32), src.view(np.uint32))
        assert np.array_equal(u64[j], src.astype(np.float64))
        assert np.array_equal(fm.unit32(sums, counts)[j].view(np.uint32), src.view(np.uint32))
    many = np.flatnonzero(counts > 1)
    assert np.allclose(np.linalg.norm(u64[many], axis=1), 1.0, atol=1e-12)


def test_chunked_order_differs_in_bits_from_the_plain_order_on_the_skew_case():
    """So the GPU test can tell a kernel that sums 1 300 rows on one wave in one go from one that follows the contract."""
    rows, ids, big = fm.skew_case()
    sums, uniq, counts = fm.fuse_sums(rows, ids)
    plain, uniq2 = fm.plain_sums(rows, ids)
    assert np.array_equal(uniq, uniq2)
    differs = (sums.view(np.uint32) != plain.view(np.uint32)).any(1)
    by_id = dict(zip(uniq.tolist(), differs.tolist()))
    cnt = dict(zip(uniq.tolist(), counts.tolist()))
    assert [cnt[int(b)] for b in big] == [512, 513, 1300]
    assert not by_id[int(big[0])]                                 # 512 rows are ONE chunk: the same order
    assert by_id[int(big[2])]                                     # 1 300 rows: 512 + 512 + 276
    assert not differs[counts <= fm.CHUNK].any()
    assert np.allclose(sums, plain, atol=1e-4)                    # (the two orders differ by rounding only)


@pytest.mark.parametrize("dim", [64, 192, 512])
def test_fp32_normalisation_of_the_models_sums_is_within_the_unit_tolerance(dim):
    """On exactly the inputs the GPU test uses: the tolerance leaves room for an honest float32 implementation."""
    rows, ids, _, _ = fm.clustered_case(dim)
    assert rows.shape == (5000, dim)
    sums, uniq, counts = fm.fuse_sums(rows, ids)
    assert counts.min() == 1 and counts.max() == 40
    ok = fm.within_unit_tolerance(fm.unit32(sums, counts), fm.unit64(sums, counts), dim)
    assert ok.all(), (dim, int((~ok).sum()))
