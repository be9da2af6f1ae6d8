"""Exact genuine / impostor score histograms over a gallery's pairs on the GPU (fh_gallery_pair_hist_dev, the histogram epilogue of
gallery_cluster.hip).  Expected = gallery_ids_model.scores(rows, rows) — the oracle.dot_mfma bits the fp32 scan reports — pushed through
the bin rule of tests/roc_model.py; got = pair_hist_dev into buffers prefilled with a sentinel.  Counts must be IDENTICAL: there is no
tolerance.  Shapes as for the clustering passes (the rows and score matrices are shared with tests/test_gpu_gallery_cluster.py): dim 64
(the odd-chunk tail), 128, 192, 256 and 512 (four and eight chunks, at three sizes); G around the 64-row B tile and the 128-row A tile; runs of several A tiles through the debug hook.  Then
the bin rule's edges on the device with dyadic rows, the call's contract, and histogram -> threshold -> clustering end to end."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa                      # noqa: E402
from facerecognizeonnx_amd import _lib                  # noqa: E402
from tests import gallery_ids_model as model            # noqa: E402
from tests import roc_model as rm                       # noqa: E402
from tests import test_gpu_gallery_cluster as tc        # noqa: E402   (its helpers and its cache of rows / score matrices)

FH_ERR_ARG, FH_ERR_STATE = -1, -4
BINS = rm.BINS
SENT = -7
PAD = 5


def run(g, want_nan=True, stream=0, wait=None):
    """pair_hist_dev into sentinel-filled buffers; the pad behind both outputs must come back untouched.  wait: what the caller does
    after the call before the buffers are read (default: a device-wide synchronise)."""
    hist = torch.full((2 * BINS + PAD,), SENT, dtype=torch.int64, device="cuda")
    nan = torch.full((2 + PAD,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.pair_hist_dev(hist.data_ptr(), nan.data_ptr() if want_nan else None, stream)
    (wait or torch.cuda.synchronize)()
    hist, nan = hist.cpu().numpy(), nan.cpu().numpy()
    assert (hist[2 * BINS:] == SENT).all() and (nan[2:] == SENT).all()
    return hist[:2 * BINS].view(np.uint64).reshape(2, BINS), nan[:2].view(np.uint64) if want_nan else nan[:2]


def ids_for(G, seed, per_id=5):
    """about G / per_id random identities, neither dense nor sorted"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, max(G // per_id, 1), G) * 7919 + 13).astype(np.int32)


def invariants(hist, nan, ids):
    G = len(ids)
    cnt = np.unique(ids, return_counts=True)[1].astype(np.int64)
    assert int(hist[0].sum()) + int(nan[0]) == int((cnt * (cnt - 1) // 2).sum())
    assert int(hist.sum()) + int(nan.sum()) == G * (G - 1) // 2


def check(g, S, ids, what, **kw):
    want_h, want_n = rm.pair_hist(S, ids)
    got_h, got_n = run(g, **kw)
    bad = np.argwhere(got_h != want_h)
    print(f"{what}: G {len(ids)}: genuine {int(want_h[0].sum())} in {int((want_h[0] > 0).sum())} bins, impostor {int(want_h[1].sum())} in "
          f"{int((want_h[1] > 0).sum())} bins, nan {want_n.tolist()}; {len(bad)} bins differ")
    assert len(bad) == 0, (what, bad[:8], got_h[tuple(bad[:8].T)], want_h[tuple(bad[:8].T)])
    if kw.get("want_nan", True):
        assert np.array_equal(got_n, want_n), (what, got_n, want_n)
        invariants(got_h, got_n, ids)
    return want_h, want_n


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dim", [64, 128, 192, 256, 512])
def test_sizes_around_the_tiles(dim):
    used = np.zeros((2, BINS), bool)
    for G in tc.sizes_for(dim):
        rows, S, _ = tc.case(dim, G)
        ids = ids_for(G, 7 * dim + G)
        want_h, _ = check(tc.gallery(rows, ids), S, ids, f"dim {dim}")
        used |= want_h > 0
    assert (used.sum(axis=1) >= 50).all(), used.sum(axis=1)     # both planes spread over many bins


@pytest.mark.timeout(300)
def test_one_identity_and_all_distinct_identities():
    rows, S, _ = tc.case(128, 129)
    for what, ids in (("one id", np.full(129, 4242, np.int32)), ("distinct ids", (np.arange(129, dtype=np.int32)[::-1] * 31 + 5))):
        want_h, _ = check(tc.gallery(rows, ids), S, ids, what)
        assert int(want_h[int(what == "one id")].sum()) == 0 and int(want_h.sum()) == 129 * 128 // 2


@pytest.mark.timeout(300)
@pytest.mark.parametrize("tiles", [3, 4, 9])
def test_runs_of_several_tiles_per_workgroup(tiles):
    rows, S, _ = tc.case(128, 1100)                            # 9 A tiles: runs of 3 + 3 + 3, 4 + 4 + 1, 9
    ids = ids_for(1100, 99)
    g = tc.gallery(rows, ids)
    try:
        assert _lib.lib().fh_debug_cluster_tiles(tiles) == 0
        check(g, S, ids, f"runs of {tiles}")
    finally:
        _lib.lib().fh_debug_cluster_tiles(0)


def dyadic_case():
    """dim 64; two or three non-zero components per row, each a multiple of 1/32 in the first six positions: every product is a multiple
    of 1/1024 and every partial sum is exact in fp32 whatever the order, so a score (dot + 1) / 2 is a multiple of 1/2048 — exactly a
    bin edge — and, the rows not being unit, ranges from well below 0 to well above 1.  Row 150 holds a NaN."""
    rng = np.random.default_rng(5)
    G = 151
    rows = np.zeros((G, 64), np.float32)
    for r in range(G):
        where = rng.choice(6, int(rng.integers(2, 4)), replace=False)
        rows[r, where] = rng.integers(-48, 49, len(where)).astype(np.float32) / np.float32(32)
    rows[0] = 0; rows[0, 0] = 1                                # scores exactly 1 (rows 0 and 2) and exactly 0 (rows 0 and 1, 1 and 2)
    rows[1] = 0; rows[1, 0] = -1
    rows[2] = 0; rows[2, 0] = 1
    rows[3] = 0; rows[3, 0] = 1; rows[3, 1] = 1.0 / 32           # (dot with row 0 is 1: another exact 1 from a non-unit row)
    rows[150, 9] = np.nan
    ids = ids_for(G, 17, per_id=8)
    ids[2] = ids[0]; ids[1] = ids[0] + 1                        # the exact 1 is a genuine pair, an exact 0 an impostor pair
    ids[150] = ids[0]                                           # the NaN row has genuine and impostor partners
    return rows, ids


@pytest.mark.timeout(300)
def test_scores_on_the_bin_edges_and_a_nan_row():
    rows, ids = dyadic_case()
    S = model.scores(rows, rows)
    up = S[np.triu_indices(len(rows), 1)]
    fin = up[~np.isnan(up)].astype(np.float64)
    assert np.array_equal(fin * BINS, np.round(fin * BINS))     # every score sits exactly on an edge
    assert S[0, 2] == 1.0 and S[0, 1] == 0.0 and S[0, 3] == 1.0
    assert (fin < 0).sum() > 50 and (fin > 1).sum() > 50 and ((fin > 0) & (fin < 1)).sum() > 1000
    assert np.isnan(S[150, :150]).all()
    want_h, want_n = check(tc.gallery(rows, ids), S, ids, "dyadic")
    assert want_n[0] > 0 and want_n[1] > 0 and int(want_n.sum()) == 150
    assert want_h[0, BINS - 1] > 0 and want_h[1, 0] > 0
    # the suffix sums of the device's histogram are the counts of the strict test at every edge
    got_h, _ = run(tc.gallery(rows, ids))
    suffix = np.cumsum(got_h.sum(axis=0)[::-1].astype(np.int64))[::-1]
    for b in (1, 2, 512, 1023, 1024, 1025, 2046, 2047):
        assert suffix[b] == int((fin > b / BINS).sum()), b


@pytest.mark.timeout(300)
def test_a_second_call_overwrites_and_nan_may_be_null():
    rows, S, _ = tc.case(192, 300)
    ids = ids_for(300, 3)
    g = tc.gallery(rows, ids)
    want_h, want_n = rm.pair_hist(S, ids)
    hist = torch.full((2 * BINS,), SENT, dtype=torch.int64, device="cuda")
    nan = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
    g.pair_hist_dev(hist.data_ptr(), nan.data_ptr(), 0)
    g.pair_hist_dev(hist.data_ptr(), nan.data_ptr(), 0)         # no wait in between: the scratch is re-cleared on the stream
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy().view(np.uint64).reshape(2, BINS), want_h)
    assert np.array_equal(nan.cpu().numpy().view(np.uint64), want_n)
    got_h, nan_buf = run(g, want_nan=False)
    assert (nan_buf == SENT).all() and np.array_equal(got_h, want_h)
    h2, n2 = g.pair_hist()                                      # the synchronous convenience
    assert h2.dtype == np.uint64 and h2.shape == (2, BINS) and np.array_equal(h2, want_h) and np.array_equal(n2, want_n)
    # a smaller row set on the same handle
    rows2, S2, _ = tc.case(192, 65)
    ids2 = ids_for(65, 4)
    rd, idd = tc.dev(rows2), tc.dev(ids2)
    g.upload(rd.data_ptr(), 65, True, 0, ids_ptr=idd.data_ptr())
    check(g, S2, ids2, "after a smaller upload")


@pytest.mark.timeout(120)
def test_errors_write_nothing_and_an_empty_gallery_writes_zeros():
    L = _lib.lib()
    rows, S, _ = tc.case(128, 65)
    ids = ids_for(65, 5)
    hist = torch.full((2 * BINS,), SENT, dtype=torch.int64, device="cuda")
    nan = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
    hp, npn = hist.data_ptr(), nan.data_ptr()
    g, unlabelled = tc.gallery(rows, ids), tc.gallery(rows)
    assert L.fh_gallery_pair_hist_dev(None, hp, npn, None) == FH_ERR_ARG and _lib.last_error()
    assert L.fh_gallery_pair_hist_dev(g._h, None, npn, None) == FH_ERR_ARG and _lib.last_error()
    assert L.fh_gallery_pair_hist_dev(unlabelled._h, hp, npn, None) == FH_ERR_STATE and _lib.last_error()
    with pytest.raises(_lib.FaceHipError):
        unlabelled.pair_hist()
    torch.cuda.synchronize()
    assert (hist.cpu().numpy() == SENT).all() and (nan.cpu().numpy() == SENT).all()
    assert unlabelled.set_ids(ids) == 65                        # what such a caller does first
    check(unlabelled, S, ids, "after set_ids")
    empty = fa.Gallery(128)
    assert L.fh_gallery_pair_hist_dev(empty._h, hp, npn, None) == 0
    torch.cuda.synchronize()
    assert (hist.cpu().numpy() == 0).all() and (nan.cpu().numpy() == 0).all()
    check(g, S, ids, "after the errors")                        # the handle still works


@pytest.mark.timeout(300)
def test_index_base_scan_mode_removal_and_stream_play_no_part():
    rows, S, _ = tc.case(128, 300)
    ids = ids_for(300, 6)
    want_h, _ = check(tc.gallery(rows, ids), S, ids, "base 0")
    for what, g in (("index base 1000", tc.gallery(rows, ids, base=1000)), ("f16 re-rank", tc.gallery(rows, ids, scan="f16")),
                    ("f16, base", tc.gallery(rows, ids, base=1000, scan="f16"))):
        assert np.array_equal(check(g, S, ids, what)[0], want_h)
    g = tc.gallery(rows, ids)
    gone = int(np.bincount(ids).argmax())                       # the identity with the most templates
    keep = np.flatnonzero(ids != gone)
    assert g.remove_ids([gone]) == 300 - len(keep) > 1
    check(g, S[np.ix_(keep, keep)], ids[keep], "after remove_ids")
    # a non-default stream, then a synchronise of that stream alone.  The stream is the runtime's own, made and destroyed here (the
    # library's handle resolves the runtime it is linked against): nothing is taken from torch's stream pool, whose round-robin the
    # two-stream tests later in the suite would otherwise see shifted.
    L = _lib.lib()
    side = C.c_void_p()
    assert L.hipStreamCreateWithFlags(C.byref(side), 1) == 0 and side.value            # hipStreamNonBlocking
    try:
        check(g, S[np.ix_(keep, keep)], ids[keep], "on a side stream", stream=side.value,
              wait=lambda: L.hipStreamSynchronize(side) == 0 or pytest.fail("hipStreamSynchronize"))
    finally:
        assert L.hipStreamDestroy(side) == 0


@pytest.mark.timeout(300)
def test_histogram_to_threshold_to_clusters():
    rng = np.random.default_rng(7)
    dim, planted, lone = 128, 60, 9
    sizes = rng.integers(4, 13, planted)
    centres = tc.unit(rng.standard_normal((planted, dim), dtype=np.float32))
    x = np.repeat(centres, sizes, axis=0) + np.float32(0.02) * rng.standard_normal((int(sizes.sum()), dim), dtype=np.float32)
    rows = np.concatenate([tc.unit(x), tc.unit(rng.standard_normal((lone, dim), dtype=np.float32))])
    ids = np.concatenate([np.repeat(np.arange(planted), sizes), planted + np.arange(lone)]).astype(np.int32) * 101 + 7
    perm = rng.permutation(len(rows))
    rows, ids = np.ascontiguousarray(rows[perm]), np.ascontiguousarray(ids[perm])
    S = model.scores(rows, rows)
    g = tc.gallery(rows, ids)
    hist, nan = g.pair_hist()
    want_h, want_n = rm.pair_hist(S, ids)
    assert np.array_equal(hist, want_h) and np.array_equal(nan, want_n) and int(nan.sum()) == 0
    op, eer = fa.roc_from_hist(hist, 0.0)
    assert op["bin"] >= 1 and op["false_accepts"] == 0 and op["far"] == 0.0
    iu = np.triu_indices(len(rows), 1)
    genuine = ids[iu[0]] == ids[iu[1]]
    thr = np.float32(op["threshold"])
    assert op["true_accepts"] == int((S[iu][genuine] > thr).sum()) and int((S[iu][~genuine] > thr).sum()) == 0
    assert op["true_accepts"] == op["genuine"] == int(genuine.sum())       # planted this tightly, no genuine pair is lost
    assert eer["false_accepts"] * eer["genuine"] <= (eer["genuine"] - eer["true_accepts"]) * eer["impostor"]
    labels, info = g.cluster(op["threshold"], 1)
    for lab in np.unique(labels):
        assert len(np.unique(ids[labels == lab])) == 1, lab     # no accepted impostor pair: no two identities share a cluster
    assert info[0] == planted + lone
