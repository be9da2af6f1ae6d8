"""Deep top-k on the GPU (gallery_deep.hip behind fh_gallery_topk_deep_dev), BIT FOR BIT — score bits, indices, ids — against the numpy
model of tests/gallery_deep_model.py: the list part of the threshold search's model at threshold -inf with cap = k (oracle.dot_mfma scores,
(score desc, row asc)), and against the project's own calls on the GPU (range_dev at -inf, topk_dev, topk_tagged_dev).

Shapes are the smallest at which this can go wrong: row counts around the 32-row block of the block maxima (1, 31, 32, 33) and the 128-row
tile (127, 128, 129, 300), around "as many blocks as k" (256 and 257 rows with k = 8: 8 and 9 blocks; 32768 and 32769 rows with k = 1024:
1024 and 1025 blocks), 4097, 20001 with 256 queries and 70001 at dim 64 (a workgroup walks two tiles, the last one partial); query counts
around the 64-query tile (1, 63, 64, 65, 256); dims of one chunk (64), two, an odd number (192) and eight (512); k 1, 16, 17, 100, 1024.
Not the full product: every value appears, every dim meets ragged G and ragged Q.  Every case states which regime it holds — full lists
('f') or lists cut short by G < k ('s') — and asserts that on the model first.  Rows, queries and model scores are the shared, read-only
ones of tests/test_gpu_gallery_range.py, computed once per session; the cases that need other rows patch a copy."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_deep_model as model  # noqa: E402
from tests.test_gpu_gallery_range import (BASE, G_BIG, G_MAIN, assert_same, big_scores, data, dev, dev_u32, gallery, random_masks,  # noqa: E402
                                          random_tags)

FH_ERR_ARG, FH_ERR_STATE = -1, -4
ALL = 0xFFFFFFFF
NEG_INF = float("-inf")


def call(g, qd, k, md=None, want="sid", stream=None):
    """One fh_gallery_topk_deep_dev call into sentinel-filled buffers with a guard row behind [Q][k]: returns (None, scores, indices,
    ids) as numpy arrays — the shape of the range model's tuple without its counts — None for a plane that was not asked for ('s', 'i',
    'd' in `want`)."""
    Q = qd.shape[0]
    s = torch.full((Q + 1, k), 7.0, device="cuda")
    i = torch.full((Q + 1, k), -7, dtype=torch.int32, device="cuda")
    d = torch.full((Q + 1, k), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.topk_deep_dev(qd.data_ptr(), Q, k, s.data_ptr() if "s" in want else None, i.data_ptr() if "i" in want else None,
                    d.data_ptr() if "d" in want else None, None if md is None else md.data_ptr(), 0 if stream is None else stream)
    torch.cuda.synchronize()
    s, i, d = s.cpu().numpy(), i.cpu().numpy(), d.cpu().numpy()
    assert (s[Q] == 7.0).all() and (i[Q] == -7).all() and (d[Q] == -7).all(), "the guard row was written"
    for name, a, fill in (("s", s, 7.0), ("i", i, -7), ("d", d, -7)):
        if name not in want:
            assert (a == fill).all(), f"plane {name} was not asked for and was written"
    return None, s[:Q] if "s" in want else None, i[:Q] if "i" in want else None, d[:Q] if "d" in want else None


def assert_regime(n_listed, k, claim, what):
    have = ("f" if (n_listed >= k).any() else "") + ("s" if (n_listed < k).any() else "")
    assert have == claim, (what, have, claim)


# ------------------------------------------------------------------------------------------ shapes vs the model
# (dim, G): [(Q, k, regime)]
SHAPES = {
    (64, 1): [(1, 1, "f"), (63, 16, "s"), (64, 1024, "s")],
    (64, 33): [(65, 17, "f"), (256, 100, "s"), (1, 1024, "s")],
    (64, 129): [(64, 1024, "s"), (65, 1, "f"), (256, 16, "f")],
    (64, 256): [(65, 8, "f"), (1, 8, "f")],                       # 8 blocks, k = 8: every block is chosen
    (64, 257): [(63, 8, "f"), (256, 8, "f")],                     # 9 blocks, k = 8: one is left out
    (64, 4097): [(65, 1024, "f"), (256, 17, "f"), (1, 100, "f"), (63, 1, "f"), (64, 16, "f")],
    (64, 20001): [(256, 1024, "f"), (256, 1, "f"), (256, 100, "f")],
    (128, 31): [(1, 1024, "s"), (63, 1, "f"), (64, 17, "f")],
    (128, 128): [(63, 100, "f"), (64, 16, "f"), (65, 1024, "s"), (256, 1, "f")],
    (128, 300): [(64, 17, "f"), (65, 1024, "s"), (256, 100, "f"), (1, 16, "f"), (63, 1, "f")],
    (128, 20001): [(256, 16, "f"), (256, 1024, "f")],
    (192, 32): [(256, 1, "f"), (1, 17, "f"), (63, 1024, "s"), (64, 100, "s")],
    (192, 127): [(1, 16, "f"), (63, 1024, "s"), (65, 100, "f"), (256, 17, "f")],
    (192, 4097): [(63, 1024, "f"), (64, 1, "f"), (65, 17, "f"), (256, 100, "f")],
    (192, 20001): [(256, 17, "f"), (256, 1024, "f")],
    (512, 1): [(65, 16, "s"), (256, 1024, "s"), (1, 1, "f")],
    (512, 33): [(256, 1024, "s"), (1, 1, "f"), (63, 17, "f"), (64, 100, "s")],
    (512, 129): [(63, 16, "f"), (64, 1024, "s"), (65, 100, "f"), (256, 17, "f")],
    (512, 300): [(63, 100, "f"), (64, 1024, "s"), (65, 1, "f"), (256, 16, "f"), (1, 17, "f")],
    (512, 20001): [(256, 1024, "f"), (256, 100, "f"), (256, 1, "f")],
}


@pytest.mark.parametrize("dim,G", list(SHAPES))
def test_lists_match_the_model(dim, G):
    rows, ids, q, sc = data(dim)
    sc = sc[:, :G]
    g = gallery(rows[:G], ids[:G])
    qd = dev(q)
    for Q, k, claim in SHAPES[(dim, G)]:
        what = f"dim{dim} G{G} Q{Q} k{k}"
        want = model.topk_from_scores(sc[:Q], k, BASE, ids=ids[:G])
        assert_regime(model.listed(sc[:Q]), k, claim, what)
        assert_same(call(g, qd[:Q], k), want, what)


@pytest.mark.parametrize("G", [32768, 32769, G_BIG])
def test_as_many_blocks_as_k_and_a_workgroup_that_walks_two_tiles(G):
    """32768 rows are 1024 blocks, 32769 are 1025: with k = 1024 every block is chosen, or all but one.  70001 rows are 547 row tiles,
    more than the resident workgroups of one query tile; the last tile holds 113 rows."""
    rows, ids, q, _ = data(64)
    sc = big_scores()[:, :G]
    g = gallery(rows[:G], ids[:G])
    qd = dev(q[:64])
    for k in (1024,) if G != G_BIG else (1024, 100, 16):
        want = model.topk_from_scores(sc, k, BASE, ids=ids[:G])
        assert_regime(model.listed(sc), k, "f", f"G{G} k{k}")
        assert_same(call(g, qd, k), want, f"G{G} k{k}")


# ------------------------------------------------------------------------------------------ the block rule's edges
def test_one_block_holds_the_whole_top():
    dim, G, Q = 64, 300, 65
    rows, ids, q, _ = data(dim)
    rows = rows[:G].copy()
    rows[32:64] = q[0]                                                 # block 1 is 32 copies of query 0
    sc = model.scores(q[:Q], rows)
    assert (sc[0, 32:64] == sc[0].max()).all() and (np.delete(sc[0], np.s_[32:64]) < sc[0].max()).all()
    g = gallery(rows)
    qd = dev(q[:Q])
    for k in (8, 32, 33):
        got = call(g, qd, k, want="si")
        assert_same(got, model.topk_from_scores(sc, k, BASE), f"k {k}")
        assert list(got[2][0][:min(k, 32)]) == list(range(BASE + 32, BASE + 32 + min(k, 32)))


def test_all_rows_equal():
    dim, G, Q = 128, 300, 65
    rows, ids, q, _ = data(dim)
    rows = np.repeat(rows[:1], G, axis=0)
    sc = model.scores(q[:Q], rows)
    assert (sc == sc[:, :1]).all()                                     # every score of a query ties
    g = gallery(rows)
    qd = dev(q[:Q])
    for k in (1, 8, 33, 300, 301):
        got = call(g, qd, k, want="si")
        assert_same(got, model.topk_from_scores(sc, k, BASE), f"k {k}")
        n = min(k, G)
        assert (got[2][:, :n] == BASE + np.arange(n)).all() and (got[2][:, n:] == -1).all() and (got[1][:, n:] == -1.0).all()


def test_ties_across_blocks_at_the_cut_keep_the_lower_rows():
    dim, G, Q = 64, 300, 65
    rows, ids, q, _ = data(dim)
    rows = rows[:G].copy()
    rows[[5, 100, 230]] = q[0]                                         # blocks 0, 3 and 7
    rows[[127, 128]] = q[1]                                            # across the border of row tiles 0 and 1
    rows[[31, 32, 33]] = q[2]                                          # across the border of blocks 0 and 1
    sc = model.scores(q[:Q], rows)
    assert sc[0, 5] == sc[0, 100] == sc[0, 230] == sc[0].max() and sc[1, 127] == sc[1, 128] == sc[1].max()
    assert sc[2, 31] == sc[2, 32] == sc[2, 33] == sc[2].max()
    g = gallery(rows)
    qd = dev(q[:Q])
    for k in (1, 2, 3, 4):
        got = call(g, qd, k, want="si")
        assert_same(got, model.topk_from_scores(sc, k, BASE), f"k {k}")
        assert list(got[2][0][:3]) == [BASE + 5, BASE + 100, BASE + 230][:k]
        assert list(got[2][1][:2]) == [BASE + 127, BASE + 128][:k]
        assert list(got[2][2][:3]) == [BASE + 31, BASE + 32, BASE + 33][:k]


def test_a_nan_or_minus_inf_score_is_never_listed_and_plus_inf_leads():
    dim, G, Q = 128, 300, 65
    rows, ids, q, _ = data(dim)
    rows = rows[:G].copy()
    rows[40, 5] = np.nan
    rows[200, 7] = np.inf
    sc = model.scores(q[:Q], rows)
    up, down = np.isposinf(sc[:, 200]), np.isneginf(sc[:, 200])
    assert np.isnan(sc[:, 40]).all() and up.any() and down.any()
    g = gallery(rows)
    qd = dev(q[:Q])
    for k in (1, 17, 1024):
        got = call(g, qd, k, want="si")
        assert_same(got, model.topk_from_scores(sc, k, BASE), f"k {k}")
        assert not (got[2] == BASE + 40).any() and not np.isnan(got[1]).any()
        assert (got[2][up, 0] == BASE + 200).all() and np.isposinf(got[1][up, 0]).all() and not (got[2][down] == BASE + 200).any()
    assert ((got[2] >= 0).sum(1) == np.where(down, G - 2, G - 1)).all()      # k = 1024: every eligible row, and only those


# ------------------------------------------------------------------------------------------ masks
def test_scattered_tags_and_masks_match_the_model():
    dim, G, Q = 64, 4097, 256
    rows, ids, q, sc = data(dim)
    sc = sc[:, :G]
    rng = np.random.default_rng(21)
    tags, masks = random_tags(rng, G), random_masks(rng, Q)
    tags[64:128] &= np.uint32(0x7FFFFFFF)                              # two blocks without a row of bit 31
    masks[:6] = [1, 2, 0, ALL, 1 << 31, 128]                           # 128: a bit no row carries
    admitted = model.listed(sc, tags, masks)
    assert (admitted[masks == 0] == 0).all() and admitted[5] == 0 and 0 < admitted[4] < 1024 < admitted[3]
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q), dev_u32(masks)
    g.tag_stats()
    for k in (8, 1024, 17):
        want = model.topk_from_scores(sc, k, BASE, tags, masks, ids[:G])
        assert_regime(admitted, k, "fs", f"masked k{k}")
        assert_same(call(g, qd, k, md), want, f"masked k{k}")
        assert_same(call(g, qd[:65], k, md[:65]), [None if w is None else w[:65] for w in want], f"masked Q65 k{k}")
    assert_same(call(g, qd, 8), model.topk_from_scores(sc, 8, BASE, ids=ids[:G]), "the unmasked call ignores the tags")
    assert g.tag_stats() == (0, 0)                                    # the tile counters are the tagged top-k scans' alone


def test_masks_on_a_gallery_without_tags():
    dim, G, Q, k = 192, 300, 65, 17
    rows, ids, q, sc = data(dim)
    sc = sc[:Q, :G]
    g = gallery(rows[:G])                                           # tags never set: every row carries all ones
    qd = dev(q[:Q])
    plain = call(g, qd, k, want="si")
    assert_same(call(g, qd, k, dev_u32(np.full(Q, ALL)), want="si"), plain, "all-ones masks")
    masks = random_masks(np.random.default_rng(22), Q)
    masks[:2] = [0, 4]
    got = call(g, qd, k, dev_u32(masks), want="si")
    assert_same(got, model.topk_from_scores(sc, k, BASE, None, masks), "masks without tags")
    assert (got[2][masks == 0] == -1).all() and np.array_equal(got[2][masks != 0], plain[2][masks != 0])
    zero = call(g, qd, k, dev_u32(np.zeros(Q)), want="si")
    assert (zero[1] == -1.0).all() and (zero[2] == -1).all()


# ------------------------------------------------------------------------------------------ against the project's own calls
def range_lists(g, qd, k, md=None):
    Q = qd.shape[0]
    c = torch.zeros(Q, dtype=torch.int64, device="cuda")
    s = torch.full((Q, k), 7.0, device="cuda"); i = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.range_dev(qd.data_ptr(), Q, NEG_INF, k, c.data_ptr(), s.data_ptr(), i.data_ptr(), None, None if md is None else md.data_ptr(), 0)
    torch.cuda.synchronize()
    return None, s.cpu().numpy(), i.cpu().numpy(), None


def test_equal_to_the_range_call_at_minus_inf():
    dim, Q = 512, 256
    rows, ids, q, sc = data(dim)
    g = gallery(rows)
    qd = dev(q)
    for k in (1024, 17):
        assert_same(call(g, qd, k, want="si"), range_lists(g, qd, k), f"against fh_gallery_range_dev, k {k}")


def test_equal_to_the_top_k_calls_up_to_16():
    dim, G, Q = 128, G_MAIN, 256
    rows, ids, q, sc = data(dim)
    rng = np.random.default_rng(23)
    tags, masks = random_tags(rng, G), random_masks(rng, Q)
    g = gallery(rows, tags=tags)
    qd, md = dev(q), dev_u32(masks)
    for k in (1, 8, 16):
        ts = torch.full((Q, k), 7.0, device="cuda"); ti = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
        g.topk_dev(qd.data_ptr(), Q, k, ts.data_ptr(), ti.data_ptr(), 0)
        torch.cuda.synchronize()
        assert_same(call(g, qd, k, want="si"), (None, ts.cpu().numpy(), ti.cpu().numpy(), None), f"against fh_gallery_topk_dev, k {k}")
    ts = torch.full((Q, 16), 7.0, device="cuda"); ti = torch.full((Q, 16), -7, dtype=torch.int32, device="cuda")
    g.topk_tagged_dev(qd.data_ptr(), md.data_ptr(), Q, 16, ts.data_ptr(), ti.data_ptr(), 0)
    torch.cuda.synchronize()
    got = call(g, qd, 16, md, want="si")
    assert (got[2][masks == 0] == -1).all() and (got[2][masks == ALL] >= 0).all()
    assert_same(got, (None, ts.cpu().numpy(), ti.cpu().numpy(), None), "against fh_gallery_topk_tagged_dev")


# ------------------------------------------------------------------------------------------ calling conventions
def test_ids_need_a_labelled_gallery_and_every_plane_may_be_null():
    dim, G, Q, k = 64, 4097, 65, 17
    rows, ids, q, sc = data(dim)
    want = model.topk_from_scores(sc[:Q, :G], k, BASE, ids=ids[:G])
    g, u = gallery(rows[:G], ids[:G]), gallery(rows[:G])
    qd = dev(q[:Q])
    for planes in ("sid", "id", "sd", "si", "s", "i", "d"):           # each pointer NULL in turn
        assert_same(call(g, qd, k, want=planes), want, f"planes {planes!r}")
    assert_same(call(u, qd, k, want="si"), want, "unlabelled, without ids")
    d = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    assert fa.lib().fh_gallery_topk_deep_dev(u._h, qd.data_ptr(), None, Q, k, None, None, d.data_ptr(), None) == FH_ERR_STATE
    assert "labelled" in _lib.last_error()
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == -7).all()


def test_the_same_bytes_in_f16_mode_twice_and_on_a_side_stream():
    dim, G, Q, k = 128, 4097, 65, 100
    rows, ids, q, sc = data(dim)
    want = model.topk_from_scores(sc[:Q, :G], k, BASE)
    g32, g16 = gallery(rows[:G]), gallery(rows[:G], scan="f16")
    qd = dev(q[:Q])
    first = call(g32, qd, k, want="si")
    assert_same(first, want, "fp32 mode")
    assert_same(call(g32, qd, k, want="si"), first, "a second identical call")
    g16.scan_stats()
    assert_same(call(g16, qd, k, want="si"), first, "f16 scan mode")
    assert g16.scan_stats() == (0, 0)                                 # the F16_RERANK counters are left alone
    # a non-default stream: the runtime's own, made and destroyed here (the library's handle resolves the runtime it is linked against).
    # Nothing is taken from torch's stream pool and no pool stream is used for the first time here: the two-stream tests later in
    # the suite get their streams, and with them their hardware queues, as they always did.
    L = _lib.lib()
    side = C.c_void_p()
    assert L.hipStreamCreateWithFlags(C.byref(side), 1) == 0 and side.value            # hipStreamNonBlocking
    try:
        assert_same(call(g32, qd, k, want="si", stream=side.value), first, "on a side stream")      # (call() waits for the device)
    finally:
        assert L.hipStreamDestroy(side) == 0


def test_the_same_bytes_after_enroll_and_remove_ids():
    dim, Q = 192, 256
    rows, ids, q, sc = data(dim)
    g = gallery(rows[:300], ids[:300])
    qd = dev(q)
    assert_same(call(g, qd[:1], 8), model.topk_from_scores(sc[:1, :300], 8, BASE, ids=ids[:300]), "before")
    assert g.enroll(rows[300:4097], ids[300:4097]) == BASE + 300      # more rows, more queries AND a deeper list than the scratch has seen
    assert_same(call(g, qd, 100), model.topk_from_scores(sc[:, :4097], 100, BASE, ids=ids[:4097]), "after enroll")
    gone = np.unique(ids[:4097])[::3]
    keep = ~np.isin(ids[:4097], gone)
    assert g.remove_ids(gone) == int((~keep).sum()) and len(g) == int(keep.sum())
    want = model.topk_from_scores(sc[:, :4097][:, keep], 100, BASE, ids=ids[:4097][keep])
    assert_same(call(g, qd, 100), want, "after remove_ids")


# ------------------------------------------------------------------------------------------ errors, empty gallery
def test_argument_errors_and_an_empty_gallery():
    dim, G, Q, k = 64, 300, 9, 8
    rows, ids, q, _ = data(dim)
    L = fa.lib()
    g = gallery(rows[:G])
    qd = dev(q[:Q])
    s = torch.full((257, 1025), 7.0, device="cuda"); i = torch.full((257, 1025), -7, dtype=torch.int32, device="cuda")
    a = (s.data_ptr(), i.data_ptr(), None, None)
    for bad_k in (0, 1025, -1):
        assert L.fh_gallery_topk_deep_dev(g._h, qd.data_ptr(), None, Q, bad_k, *a) == FH_ERR_ARG and "k" in _lib.last_error()
    assert L.fh_gallery_topk_deep_dev(g._h, qd.data_ptr(), None, 257, k, *a) == FH_ERR_ARG
    assert L.fh_gallery_topk_deep_dev(g._h, qd.data_ptr(), None, -1, k, *a) == FH_ERR_ARG
    assert L.fh_gallery_topk_deep_dev(None, qd.data_ptr(), None, Q, k, *a) == FH_ERR_ARG
    assert L.fh_gallery_topk_deep_dev(g._h, None, None, Q, k, *a) == FH_ERR_ARG
    assert L.fh_gallery_topk_deep_dev(g._h, qd.data_ptr(), None, Q, k, None, None, None, None) == FH_ERR_ARG
    assert L.fh_gallery_topk_deep_dev(g._h, qd.data_ptr(), None, 0, k, *a) == 0
    g96 = fa.Gallery(96)                                              # such a gallery can be created, and takes no rows
    q96 = torch.zeros((Q, 96), device="cuda")
    assert L.fh_gallery_topk_deep_dev(g96._h, q96.data_ptr(), None, Q, k, *a) == FH_ERR_ARG and "64" in _lib.last_error()
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 7.0).all() and (i.cpu().numpy() == -7).all()      # nothing was written
    assert L.fh_gallery_topk_deep_dev(g._h, qd.data_ptr(), None, Q, k, *a) == Q   # the good call returns nq
    e = fa.Gallery(dim)                                               # an empty gallery: empty lists, ids too
    for md in (None, dev_u32(np.full(Q, 1))):
        got = call(e, qd, k, md)
        assert (got[1] == -1.0).all() and (got[2] == -1).all() and (got[3] == -1).all()
    sc_, ix = g.topk_deep(q[:Q], 40)                                  # the synchronous convenience
    assert sc_.shape == (Q, 40) and ix.shape == (Q, 40) and sc_.dtype == np.float32 and ix.dtype == np.int32
    assert_same((None, sc_, ix), call(g, qd, 40, want="si"), "Gallery.topk_deep")
