"""Threshold (range) search on the GPU (gallery_range.hip behind fh_gallery_range_dev), BIT FOR BIT — score bits, indices, ids, counts —
against the numpy model of tests/gallery_range_model.py (oracle.dot_mfma scores, the strict fp32 test, (score desc, row asc)).

Shapes are the smallest at which this can go wrong: row counts around the 32-row word of the hit bitmap (1, 31, 32, 33) and the 128-row
tile (127, 128, 129, 300), 4097, 20001 with 256 queries (more row tiles than workgroups per query tile: a workgroup walks two tiles, the
last one partial) and 70001 at dim 64; query counts around the 64-query tile (1, 63, 64, 65, 256); dims of one chunk (64), two, an odd
number (192) and eight (512); cap 1, 8, 1024.  Not the full product: every value appears, every dim meets ragged G and ragged Q.  Every
case states which regimes it holds — queries with no hit ('0'), with 1..cap hits ('+'), with more than cap ('>') — and asserts that on
the model first.  One set of rows, queries and model scores per dim is computed once and shared, read-only; the cases that need other
rows patch a copy."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_range_model as model  # noqa: E402
from tests.test_gpu_gallery_tags import side_stream_leaving_the_pool_as_it_was  # noqa: E402

FH_ERR_ARG, FH_ERR_STATE = -1, -4
ALL = 0xFFFFFFFF
G_MAIN, G_BIG = 20001, 70001                  # 157 row tiles, the last one of 33 rows; 547 row tiles, the last one of 113 rows
BASE = 1000


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared arrays are read-only)


def dev_u32(a):
    return dev(np.ascontiguousarray(np.asarray(a).astype(np.uint32)).view(np.int32))


@functools.lru_cache(maxsize=None)
def data(dim):
    """Rows in shuffled clusters of 5 templates with noise 0.05 and sparse ids (G_BIG of them at dim 64, G_MAIN otherwise), 256 queries
    (60 near the first 120 rows, 60 near the first 4097, 80 near any row, 56 near nobody) and the model's [256][G_MAIN] scores.  Shared:
    read only."""
    G = G_BIG if dim == 64 else G_MAIN
    rng = np.random.default_rng(2000 + dim)
    T, n_ids = 5, (G + 4) // 5
    centres = unit(rng, n_ids, dim)
    rows = np.repeat(centres, T, axis=0)[:G] + np.float32(0.05) * rng.standard_normal((G, dim), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = np.repeat((rng.permutation(4 * n_ids)[:n_ids] * 13 + 5).astype(np.int32), T)[:G]
    o = rng.permutation(G)
    rows, ids = np.ascontiguousarray(rows[o], np.float32), np.ascontiguousarray(ids[o])
    near = np.concatenate([rows[rng.integers(0, 120, 60)], rows[rng.integers(0, 4097, 60)], rows[rng.integers(0, G, 80)]])
    q = near + np.float32(0.05) * rng.standard_normal(near.shape, dtype=np.float32)
    q = np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), unit(rng, 56, dim)])
    q = np.ascontiguousarray(q[rng.permutation(256)], np.float32)
    sc = model.scores(q, rows[:G_MAIN])
    for a in (rows, ids, q, sc):
        a.setflags(write=False)
    return rows, ids, q, sc


@functools.lru_cache(maxsize=None)
def big_scores():
    rows, _, q, _ = data(64)
    sc = model.scores(q[:64], rows)
    sc.setflags(write=False)
    return sc


def gallery(rows, ids=None, tags=None, base=BASE, scan="fp32"):
    g = fa.Gallery(rows.shape[1], scan=scan)
    rd = dev(rows)
    if ids is None:
        g.upload(rd.data_ptr(), rows.shape[0], True, base)
    else:
        idd = dev(np.asarray(ids, np.int32))
        g.upload(rd.data_ptr(), rows.shape[0], True, base, ids_ptr=idd.data_ptr())
    if tags is not None:
        assert g.set_tags(np.asarray(tags, np.uint32)) == rows.shape[0]
    return g


def call(g, qd, thr, cap, md=None, want="sid", stream=None):
    """One fh_gallery_range_dev call into sentinel-filled buffers with a guard row behind [Q][cap] (and a guard word behind the counts):
    returns (counts, scores, indices, ids) as numpy arrays, None for a plane that was not asked for ('s', 'i', 'd' in `want`)."""
    Q = qd.shape[0]
    c = torch.full((Q + 1,), -99, dtype=torch.int64, device="cuda")
    s = torch.full((Q + 1, cap), 7.0, device="cuda")
    i = torch.full((Q + 1, cap), -7, dtype=torch.int32, device="cuda")
    d = torch.full((Q + 1, cap), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.range_dev(qd.data_ptr(), Q, float(thr), cap, c.data_ptr(), s.data_ptr() if "s" in want else None, i.data_ptr() if "i" in want else None,
                d.data_ptr() if "d" in want else None, None if md is None else md.data_ptr(), 0 if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    c, s, i, d = c.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), d.cpu().numpy()
    assert c[Q] == -99 and (s[Q] == 7.0).all() and (i[Q] == -7).all() and (d[Q] == -7).all(), "the guard row was written"
    for name, a, fill in (("s", s, 7.0), ("i", i, -7), ("d", d, -7)):
        if name not in want:
            assert (a == fill).all(), f"plane {name} was not asked for and was written"
    return c[:Q], s[:Q] if "s" in want else None, i[:Q] if "i" in want else None, d[:Q] if "d" in want else None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    """(counts, scores, indices, ids): scores by their bits, everything else by value; a None on either side is not compared."""
    for j, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            continue
        a, b = bits(a), bits(b)
        assert a.shape == b.shape and np.array_equal(a, b), (what, j, np.argwhere(a != b)[:6], a[a != b][:6], b[a != b][:6])


def assert_regimes(counts, cap, claims, what):
    have = ("0" if (counts == 0).any() else "") + ("+" if ((counts >= 1) & (counts <= cap)).any() else "") + (">" if (counts > cap).any() else "")
    assert have == claims, (what, have, claims)


def random_tags(rng, G):
    """One row in ten carries no bit at all; the others a sparse subset of bits 0..6 and, one in eight, bit 31."""
    t = np.zeros(G, np.uint32)
    for b in range(7):
        t |= (rng.random(G) < 0.3).astype(np.uint32) << np.uint32(b)
    t |= (rng.random(G) < 0.125).astype(np.uint32) << np.uint32(31)
    t[rng.random(G) < 0.1] = 0
    return t


def random_masks(rng, Q):
    pool = np.array([0, ALL, 1, 2, 4, 64, 3, 1 << 31, (1 << 31) | 8, 128, 0x70], np.uint64)      # 128: a bit no row carries
    return rng.choice(pool, Q).astype(np.uint32)


# ------------------------------------------------------------------------------------------ shapes vs the model
# (dim, G): [(Q, cap, threshold, regimes)]
SHAPES = {
    (64, 1): [(1, 1, 0.5, "0"), (63, 8, 0.6, "0+"), (64, 1024, 0.5, "0+"), (65, 1, 0.6, "0+"), (256, 8, 0.55, "0+")],
    (64, 33): [(63, 8, 0.55, "+>"), (64, 1024, 0.7, "0+"), (65, 1, 0.55, "+>"), (256, 8, 0.7, "0+"), (1, 1024, 0.6, "+")],
    (64, 129): [(64, 1024, 0.6, "+"), (65, 1, 0.5, ">"), (256, 8, 0.6, "+>"), (1, 1024, 0.5, "+"), (63, 1, 0.7, "0+")],
    (64, 4097): [(65, 1, 0.7, "0+>"), (256, 8, 0.55, ">"), (1, 1024, 0.7, "+"), (63, 1, 0.55, ">"), (64, 8, 0.5, ">")],
    (64, 20001): [(256, 1024, 0.5, ">"), (256, 8, 0.55, ">"), (256, 1024, 0.6, "+>"), (256, 1, 0.7, ">"), (256, 8, 0.6, ">")],
    (128, 31): [(1, 1024, 0.55, "+"), (63, 1, 0.7, "0+"), (64, 8, 0.55, "0+>"), (65, 1024, 0.7, "0+"), (256, 1, 0.6, "0+>")],
    (128, 128): [(63, 1, 0.6, "0+>"), (64, 8, 0.5, ">"), (65, 1024, 0.6, "0+"), (256, 1, 0.5, ">"), (1, 8, 0.7, "0")],
    (128, 300): [(64, 8, 0.7, "0+"), (65, 1024, 0.55, "+"), (256, 1, 0.7, "0+>"), (1, 8, 0.55, ">"), (63, 1024, 0.5, "+")],
    (128, 20001): [(256, 1024, 0.5, ">"), (256, 8, 0.55, ">"), (256, 1024, 0.6, "+"), (256, 1, 0.7, "0>"), (256, 8, 0.6, ">")],
    (192, 32): [(256, 1, 0.55, "0+>"), (1, 8, 0.7, "0"), (63, 1024, 0.55, "0+"), (64, 1, 0.7, "0+"), (65, 8, 0.6, "0+")],
    (192, 127): [(1, 8, 0.6, "+"), (63, 1024, 0.5, "+"), (64, 1, 0.6, "0+>"), (65, 8, 0.5, ">"), (256, 1024, 0.7, "0+")],
    (192, 4097): [(63, 1024, 0.7, "0+"), (64, 1, 0.55, ">"), (65, 8, 0.7, "0+"), (256, 1024, 0.55, "+"), (1, 1, 0.5, ">")],
    (192, 20001): [(256, 1024, 0.5, ">"), (256, 8, 0.55, ">"), (256, 1024, 0.6, "+"), (256, 1, 0.7, "0>"), (256, 8, 0.6, ">")],
    (512, 1): [(65, 8, 0.55, "0+"), (256, 1024, 0.7, "0"), (1, 1, 0.55, "0"), (63, 8, 0.7, "0"), (64, 1024, 0.6, "0")],
    (512, 33): [(256, 1024, 0.6, "0+"), (1, 1, 0.5, ">"), (63, 8, 0.6, "0+"), (64, 1024, 0.5, "+"), (65, 1, 0.7, "0+")],
    (512, 129): [(1, 1, 0.7, "0"), (63, 8, 0.55, "0+"), (64, 1024, 0.7, "0+"), (65, 1, 0.55, "0+>"), (256, 8, 0.5, ">"), (256, 1024, 0.6, "0+")],
    (512, 300): [(63, 8, 0.5, ">"), (64, 1024, 0.6, "0+"), (65, 1, 0.5, ">"), (256, 8, 0.6, "0+"), (1, 1024, 0.55, "+")],
    (512, 20001): [(256, 1024, 0.5, ">"), (256, 8, 0.55, ">"), (256, 1024, 0.55, "+"), (256, 1024, 0.6, "0+"), (256, 1, 0.7, "0+>"),
                   (256, 8, 0.6, "0+")],
}


@pytest.mark.parametrize("dim,G", list(SHAPES))
def test_counts_and_lists_match_the_model(dim, G):
    rows, ids, q, sc = data(dim)
    sc = sc[:, :G]
    g = gallery(rows[:G], ids[:G])
    qd = dev(q)
    for Q, cap, thr, claims in SHAPES[(dim, G)]:
        what = f"dim{dim} G{G} Q{Q} cap{cap} thr{thr}"
        want = model.range_from_scores(sc[:Q], thr, cap, BASE, ids=ids[:G])
        assert_regimes(want[0], cap, claims, what)
        assert_same(call(g, qd[:Q], thr, cap), want, what)


def test_a_seeded_size_gallery_of_70001_rows():
    """547 row tiles, more than the resident workgroups of one query tile: a workgroup walks two tiles; the last tile holds 113 rows."""
    rows, ids, q, _ = data(64)
    sc = big_scores()
    g = gallery(rows, ids)
    qd = dev(q[:64])
    for cap, thr, claims in ((8, 0.7, ">"), (1024, 0.7, "+"), (1024, 0.6, ">"), (1, 0.5, ">")):
        want = model.range_from_scores(sc, thr, cap, BASE, ids=ids)
        assert_regimes(want[0], cap, claims, f"cap{cap} thr{thr}")
        assert_same(call(g, qd, thr, cap), want, f"G{G_BIG} cap{cap} thr{thr}")


# ------------------------------------------------------------------------------------------ the rule's edges
def test_the_threshold_is_strict_at_a_score():
    dim, G, Q, cap = 128, 4097, 65, 1024
    rows, ids, q, sc = data(dim)
    sc = sc[:Q, :G]
    g = gallery(rows[:G])
    qd = dev(q[:Q])
    for j in (0, 17, 64):
        order = np.argsort(-sc[j].astype(np.float64), kind="stable")
        r = order[4]                                                   # a mid-ranked pair of a crowded top
        thr = sc[j, r]
        assert sc[j, order[3]] > thr > sc[j, order[5]]
        at = call(g, qd, thr, cap, want="si")
        below = call(g, qd, np.nextafter(thr, np.float32(-np.inf)), cap, want="si")
        assert_same(at, model.range_from_scores(sc, thr, cap, BASE), f"query {j} at the score")
        assert_same(below, model.range_from_scores(sc, np.nextafter(thr, np.float32(-np.inf)), cap, BASE), f"query {j} a hair below")
        assert at[0][j] == 4 and BASE + r not in at[2][j] and below[0][j] == 5 and below[2][j, 4] == BASE + r


def test_equal_scores_rank_by_row_and_a_cap_between_them_keeps_the_lower_row():
    dim, G, Q = 64, 300, 65
    rows, ids, q, _ = data(dim)
    rows = rows[:G].copy()
    rows[[31, 32, 33]] = q[0]                                          # across the border of bitmap words 0 and 1
    rows[[127, 128]] = q[1]                                            # across the border of row tiles 0 and 1
    sc = model.scores(q[:Q], rows)
    assert sc[0, 31] == sc[0, 32] == sc[0, 33] == sc[0].max() and sc[1, 127] == sc[1, 128] == sc[1].max()
    g = gallery(rows)
    qd = dev(q[:Q])
    for cap in (1, 2, 8):
        got = call(g, qd, 0.9, cap, want="si")
        assert_same(got, model.range_from_scores(sc, 0.9, cap, BASE), f"cap {cap}")
        assert got[0][0] == 3 and got[0][1] == 2
        assert list(got[2][0][:min(cap, 3)]) == [BASE + 31, BASE + 32, BASE + 33][:cap]
        assert list(got[2][1][:min(cap, 2)]) == [BASE + 127, BASE + 128][:cap]


def test_a_nan_row_is_never_a_hit_and_an_inf_row_is():
    dim, G, Q = 128, 300, 65
    rows, ids, q, _ = data(dim)
    rows = rows[:G].copy()
    rows[40, 5] = np.nan
    rows[200, 7] = np.inf
    sc = model.scores(q[:Q], rows)
    assert np.isnan(sc[:, 40]).all() and np.isposinf(sc[:, 200]).any() and np.isneginf(sc[:, 200]).any()
    g = gallery(rows)
    qd = dev(q[:Q])
    for thr, cap in ((0.55, 8), (-1.0, 1024), (float("-inf"), 1024), (float("inf"), 8)):
        want = model.range_from_scores(sc, thr, cap, BASE)
        got = call(g, qd, thr, cap, want="si")
        assert_same(got, want, f"thr {thr}")
        assert not (got[2] == BASE + 40).any()
    assert (want[0] == 0).all()                                        # nothing is above +inf
    got = call(g, qd, 0.55, 8, want="si")
    up = np.isposinf(sc[:, 200])
    assert (got[2][up, 0] == BASE + 200).all() and np.isposinf(got[1][up, 0]).all() and not (got[2][~up] == BASE + 200).any()


# ------------------------------------------------------------------------------------------ masks
def test_scattered_tags_and_masks_match_the_model():
    dim, G, Q = 64, 4097, 256
    rows, ids, q, sc = data(dim)
    sc = sc[:, :G]
    rng = np.random.default_rng(11)
    tags, masks = random_tags(rng, G), random_masks(rng, Q)
    masks[:4] = [1, 2, 0, ALL]
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q), dev_u32(masks)
    g.tag_stats()
    for cap, thr in ((8, 0.7), (1024, 0.6), (1, 0.55)):
        want = model.range_from_scores(sc, thr, cap, BASE, tags, masks, ids[:G])
        plain = model.range_from_scores(sc, thr, cap, BASE)
        assert (want[0][masks == 0] == 0).all() and (want[0] < plain[0]).sum() > 100 and (want[0] > 0).sum() > 100
        assert_same(call(g, qd, thr, cap, md), want, f"masked cap{cap} thr{thr}")
        assert_same(call(g, qd[:65], thr, cap, md[:65]), [w[:65] for w in want], f"masked Q65 cap{cap} thr{thr}")
    assert_same(call(g, qd, 0.6, 8), model.range_from_scores(sc, 0.6, 8, BASE, ids=ids[:G]), "the unmasked call ignores the tags")
    assert g.tag_stats() == (0, 0)                                    # the tile counters are the tagged top-k scans' alone


def test_masks_on_a_gallery_without_tags():
    dim, G, Q, cap, thr = 192, 300, 65, 8, 0.55
    rows, ids, q, sc = data(dim)
    sc = sc[:Q, :G]
    g = gallery(rows[:G])                                           # tags never set: every row carries all ones
    qd = dev(q[:Q])
    plain = call(g, qd, thr, cap, want="si")
    assert (plain[0] > 0).sum() > 30
    assert_same(call(g, qd, thr, cap, dev_u32(np.full(Q, ALL)), want="si"), plain, "all-ones masks")
    masks = random_masks(np.random.default_rng(12), Q)
    masks[:2] = [0, 4]
    got = call(g, qd, thr, cap, dev_u32(masks), want="si")
    assert_same(got, model.range_from_scores(sc, thr, cap, BASE, None, masks), "masks without tags")
    assert (got[0][masks == 0] == 0).all() and np.array_equal(got[0][masks != 0], plain[0][masks != 0])
    zero = call(g, qd, thr, cap, dev_u32(np.zeros(Q)), want="si")
    assert (zero[0] == 0).all() and (zero[1] == -1.0).all() and (zero[2] == -1).all()


# ------------------------------------------------------------------------------------------ ids, NULL planes, empty slots
def test_ids_need_a_labelled_gallery_and_every_plane_may_be_null():
    dim, G, Q, cap, thr = 64, 4097, 65, 8, 0.7
    rows, ids, q, sc = data(dim)
    sc = sc[:Q, :G]
    want = model.range_from_scores(sc, thr, cap, BASE, ids=ids[:G])
    assert_regimes(want[0], cap, "0+", "ids")
    assert (want[1][want[0] == 0] == -1.0).all() and (want[2][want[0] == 0] == -1).all() and (want[3][want[0] == 0] == -1).all()
    g, u = gallery(rows[:G], ids[:G]), gallery(rows[:G])
    qd = dev(q[:Q])
    for planes in ("sid", "id", "sd", "si", "s", "i", "d", ""):       # each pointer NULL in turn, down to the count-only form
        assert_same(call(g, qd, thr, cap, want=planes), want, f"planes {planes!r}")
    assert_same(call(u, qd, thr, cap, want="si"), want, "unlabelled, without ids")
    c = torch.zeros(Q, dtype=torch.int64, device="cuda"); d = torch.zeros((Q, cap), dtype=torch.int32, device="cuda")
    L = fa.lib()
    assert L.fh_gallery_range_dev(u._h, qd.data_ptr(), None, Q, thr, cap, c.data_ptr(), None, None, d.data_ptr(), None) == FH_ERR_STATE
    assert "labelled" in _lib.last_error()
    torch.cuda.synchronize()


def test_the_top_16_above_the_threshold_are_the_top_k_call_s():
    dim, G, Q, thr = 512, G_MAIN, 256, 0.6
    rows, ids, q, sc = data(dim)
    g = gallery(rows)
    qd = dev(q)
    counts, s, i, _ = call(g, qd, thr, 16, want="si")
    ts = torch.full((Q, 16), 7.0, device="cuda"); ti = torch.full((Q, 16), -7, dtype=torch.int32, device="cuda")
    g.topk_dev(qd.data_ptr(), Q, 16, ts.data_ptr(), ti.data_ptr(), 0)
    torch.cuda.synchronize()
    ts, ti = ts.cpu().numpy(), ti.cpu().numpy()
    keep = (ts > np.float32(thr)) & (ti >= 0)
    assert (counts == 0).any() and (counts > 0).any() and np.array_equal(np.minimum(counts, 16), keep.sum(1))
    assert_same((s, i), (np.where(keep, ts, np.float32(-1.0)), np.where(keep, ti, -1)), "against fh_gallery_topk_dev")


# ------------------------------------------------------------------------------------------ the same bytes
def test_the_same_bytes_in_f16_mode_twice_and_on_a_side_stream():
    dim, G, Q, cap, thr = 128, 4097, 65, 8, 0.6
    rows, ids, q, sc = data(dim)
    want = model.range_from_scores(sc[:Q, :G], thr, cap, BASE)
    g32, g16 = gallery(rows[:G]), gallery(rows[:G], scan="f16")
    qd = dev(q[:Q])
    first = call(g32, qd, thr, cap, want="si")
    assert_same(first, want, "fp32 mode")
    assert_same(call(g32, qd, thr, cap, want="si"), first, "a second identical call")
    g16.scan_stats()
    assert_same(call(g16, qd, thr, cap, want="si"), first, "f16 scan mode")
    assert g16.scan_stats() == (0, 0)                                 # the F16_RERANK counters are left alone
    side = side_stream_leaving_the_pool_as_it_was()
    assert_same(call(g32, qd, thr, cap, want="si", stream=side), first, "on a side stream")


def test_the_same_bytes_after_enroll_and_remove_ids():
    dim, Q, cap, thr = 192, 256, 8, 0.6
    rows, ids, q, sc = data(dim)
    g = gallery(rows[:300], ids[:300])
    qd = dev(q)
    assert_same(call(g, qd[:1], thr, cap), model.range_from_scores(sc[:1, :300], thr, cap, BASE, ids=ids[:300]), "before")
    assert g.enroll(rows[300:4097], ids[300:4097]) == BASE + 300      # more rows AND more queries than the scratch has seen
    want = model.range_from_scores(sc[:, :4097], thr, cap, BASE, ids=ids[:4097])
    assert_regimes(want[0], cap, "+>", "enrolled")
    assert_same(call(g, qd, thr, cap), want, "after enroll")
    gone = np.unique(ids[:4097])[::3]
    keep = ~np.isin(ids[:4097], gone)
    assert g.remove_ids(gone) == int((~keep).sum()) and len(g) == int(keep.sum())
    want = model.range_from_scores(sc[:, :4097][:, keep], thr, cap, BASE, ids=ids[:4097][keep])
    assert (want[0] > 0).sum() > 50
    assert_same(call(g, qd, thr, cap), want, "after remove_ids")


# ------------------------------------------------------------------------------------------ errors, empty gallery
def test_argument_errors_and_an_empty_gallery():
    dim, G, Q, cap = 64, 300, 9, 8
    rows, ids, q, _ = data(dim)
    L = fa.lib()
    g = gallery(rows[:G])
    qd = dev(q[:Q])
    c = torch.full((257,), -99, dtype=torch.int64, device="cuda")
    s = torch.full((Q, 1025), 7.0, device="cuda"); i = torch.full((Q, 1025), -7, dtype=torch.int32, device="cuda")
    a = (c.data_ptr(), s.data_ptr(), i.data_ptr(), None, None)
    for bad_cap in (0, 1025, -1):
        assert L.fh_gallery_range_dev(g._h, qd.data_ptr(), None, Q, 0.5, bad_cap, *a) == FH_ERR_ARG and "cap" in _lib.last_error()
    assert L.fh_gallery_range_dev(g._h, qd.data_ptr(), None, Q, float("nan"), cap, *a) == FH_ERR_ARG and "NaN" in _lib.last_error()
    assert L.fh_gallery_range_dev(g._h, qd.data_ptr(), None, 257, 0.5, cap, *a) == FH_ERR_ARG
    assert L.fh_gallery_range_dev(g._h, qd.data_ptr(), None, -1, 0.5, cap, *a) == FH_ERR_ARG
    assert L.fh_gallery_range_dev(None, qd.data_ptr(), None, Q, 0.5, cap, *a) == FH_ERR_ARG
    assert L.fh_gallery_range_dev(g._h, None, None, Q, 0.5, cap, *a) == FH_ERR_ARG
    assert L.fh_gallery_range_dev(g._h, qd.data_ptr(), None, Q, 0.5, cap, None, s.data_ptr(), i.data_ptr(), None, None) == FH_ERR_ARG
    assert L.fh_gallery_range_dev(g._h, qd.data_ptr(), None, 0, 0.5, cap, *a) == 0
    g96 = fa.Gallery(96)                                              # such a gallery can be created, and takes no rows
    q96 = torch.zeros((Q, 96), device="cuda")
    assert L.fh_gallery_range_dev(g96._h, q96.data_ptr(), None, Q, 0.5, cap, *a) == FH_ERR_ARG and "64" in _lib.last_error()
    torch.cuda.synchronize()
    assert (c.cpu().numpy() == -99).all() and (s.cpu().numpy() == 7.0).all() and (i.cpu().numpy() == -7).all()      # nothing was written
    e = fa.Gallery(dim)                                               # an empty gallery: counts of 0, empty lists, ids too
    for md in (None, dev_u32(np.full(Q, 1))):
        got = call(e, qd, 0.0, cap, md)
        assert (got[0] == 0).all() and (got[1] == -1.0).all() and (got[2] == -1).all() and (got[3] == -1).all()
    counts, sc_, ix = g.range(q[:Q], 0.55, cap=4)                     # the synchronous convenience
    assert counts.shape == (Q,) and sc_.shape == (Q, 4) and ix.shape == (Q, 4) and counts.dtype == np.int64
    assert_same((counts, sc_, ix), call(g, qd, 0.55, 4, want="si"), "Gallery.range")
