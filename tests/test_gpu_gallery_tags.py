"""Watchlists on the GPU (gallery_tags.hip): row tags, per-query masks and the tag-filtered exact 1:N search, BIT FOR BIT (score bits,
indices, ids, rows) against the numpy model of tests/gallery_tags_model.py — the untagged model on each query's admitted rows — and,
at dim 512, against the library's own untagged scans on a compacted copy of the admitted rows.

Shapes are the smallest at which the scan can go wrong: row counts around the 128-row tile (1, 127, 128, 129, 300), one beyond the
4096-row seed prefix (4097, unseeded) and one above the seed threshold with a partial last tile (70001); query counts around the
64-query tile (1, 63, 64, 65) and four tiles (256); k = 1, 5, 16.  Every mask / tag case first asserts on the CPU model that it is not
vacuous.  One set of rows, queries and model scores per dim is computed once and shared (never modified: the cases that need other
rows patch a copy)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_tags_model as model  # noqa: E402

FH_ERR_ARG, FH_ERR_STATE = -1, -4
ALL = model.TAG_ALL
G_SEED = 70001                                # >= 65536 (seed pass); last 128-row tile holds 113 rows
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
    """G_SEED rows in shuffled clusters of 5 templates with sparse ids, 256 queries (200 near a cluster, 56 near nobody) and the
    model's [256][G_SEED] scores.  Shared: read only."""
    rng = np.random.default_rng(1000 + dim)
    T, n_ids = 5, (G_SEED + 4) // 5
    centres = unit(rng, n_ids, dim)
    rows = np.repeat(centres, T, axis=0)[:G_SEED] + np.float32(0.05) * rng.standard_normal((G_SEED, dim), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = np.repeat((rng.permutation(4 * n_ids)[:n_ids] * 13 + 5).astype(np.int32), T)[:G_SEED]
    o = rng.permutation(G_SEED)
    rows, ids = np.ascontiguousarray(rows[o], np.float32), np.ascontiguousarray(ids[o])
    # queries near the clusters of rows in the FIRST 300 positions too, so that the small galleries have crowded tops as well
    near = np.concatenate([rows[rng.integers(0, 120, 60)], rows[rng.integers(0, 4097, 60)], rows[rng.integers(0, G_SEED, 80)]])
    q = near + np.float32(0.05) * rng.standard_normal(near.shape, dtype=np.float32)
    q = np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), unit(rng, 56, dim)])
    q = np.ascontiguousarray(q[rng.permutation(256)], np.float32)
    sc = model.scores(q, rows)
    for a in (rows, ids, q, sc):
        a.setflags(write=False)
    return rows, ids, q, sc


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


def topk_rows(g, qd, k):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda"); ix = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_dev(qd.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ix.cpu().numpy()


def topk_ids(g, qd, k):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda")
    di = torch.full((Q, k), -7, dtype=torch.int32, device="cuda"); ri = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_ids_dev(qd.data_ptr(), Q, k, sc.data_ptr(), di.data_ptr(), ri.data_ptr(), 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), di.cpu().numpy(), ri.cpu().numpy()


def tagged_rows(g, qd, md, k):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda"); ix = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_tagged_dev(qd.data_ptr(), md.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ix.cpu().numpy()


def tagged_ids(g, qd, md, k, want_rows=True):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda")
    di = torch.full((Q, k), -7, dtype=torch.int32, device="cuda"); ri = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_ids_tagged_dev(qd.data_ptr(), md.data_ptr(), Q, k, sc.data_ptr(), di.data_ptr(), ri.data_ptr() if want_rows else None, 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), di.cpu().numpy(), ri.cpu().numpy()


def tagged_label(g, qd, md, thr, ids=False):
    Q = qd.shape[0]
    lab = torch.full((Q,), -5, dtype=torch.int32, device="cuda"); sc = torch.full((Q,), 7.0, device="cuda")
    (g.label_ids_tagged_dev if ids else g.label_tagged_dev)(qd.data_ptr(), md.data_ptr(), Q, float(thr), lab.data_ptr(), sc.data_ptr(), 0)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), sc.cpu().numpy()


def side_stream_leaving_the_pool_as_it_was():
    """A non-default stream for graph capture.  torch hands out the streams of a fixed pool in rotation, and the tests that run later
    in the process get their streams (and with them their hardware queues) by their place in that rotation: so this draws exactly two
    whole rotations — the pool is back where it was — and returns the last stream drawn, which is the one handed out last BEFORE this
    call: no stream is used here that had not been in use already."""
    first = torch.cuda.Stream()
    size = 0
    while True:
        s = torch.cuda.Stream()
        size += 1
        if s.cuda_stream == first.cuda_stream:
            break
    for _ in range(size - 1):
        s = torch.cuda.Stream()
    return s


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    """Tuples of [Q][k] planes: scores by their bits, everything else by value."""
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        a, b = bits(a), bits(b)
        assert a.shape == b.shape and np.array_equal(a, b), (what, j, np.argwhere(a != b)[:6], a[a != b][:6], b[a != b][:6])


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


# ------------------------------------------------------------------------------------------ random tags and masks vs the model
@pytest.mark.parametrize("G", [1, 127, 128, 129, 300, 4097, G_SEED])
@pytest.mark.parametrize("dim", [64, 128])
def test_random_tags_and_masks_match_the_model(dim, G):
    rows, ids, q, sc = data(dim)
    rng = np.random.default_rng(7 * G + dim)
    tags, masks = random_tags(rng, G), random_masks(rng, 256)
    masks[:4] = [1, 2, 0, ALL]
    adm = model.admitted(tags, masks)
    best = np.argmax(sc[:, :G], axis=1)
    assert G < 100 or (~adm[np.arange(256), best]).sum() > 20           # many a query's best row is excluded for it
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q), dev_u32(masks)
    want_r = model.topk_from_scores(sc[:, :G], tags, masks, 16, BASE)
    want_i = model.topk_ids_from_scores(sc[:, :G], ids[:G], tags, masks, 16, BASE)
    assert (want_r[1][2] == -1).all() and (want_i[1][2] == -1).all()     # mask 0
    for Q, k in ((1, 1), (63, 5), (64, 16), (65, 1), (256, 16), (256, 5)):
        assert_same(tagged_rows(g, qd[:Q], md[:Q], k), [w[:Q, :k] for w in want_r], f"rows dim{dim} G{G} Q{Q} k{k}")
        assert_same(tagged_ids(g, qd[:Q], md[:Q], k), [w[:Q, :k] for w in want_i], f"ids dim{dim} G{G} Q{Q} k{k}")
    s, d, _ = tagged_ids(g, qd[:65], md[:65], 5, want_rows=False)         # d_rows = NULL
    assert_same((s, d), [w[:65, :5] for w in want_i[:2]], "ids without rows")


# ------------------------------------------------------------------------------------------ cross-checks against the library itself
@pytest.mark.parametrize("G", [300, G_SEED])
def test_one_shared_mask_answers_as_the_untagged_scan_of_the_compacted_gallery(G):
    """dim 512, no numpy scores: a second gallery holds the admitted rows only, its indices are mapped back."""
    rng = np.random.default_rng(31 + G)
    dim = 512
    rows, q = unit(rng, G, dim), unit(rng, 256, dim)
    rows[G // 2] = rows[G // 3] = rows[5] = q[9]                     # a tie among admitted and excluded copies
    ids = (rng.permutation(G) // 4 * 7 + 3).astype(np.int32)
    tags = random_tags(rng, G)
    tags[[5, G // 2]] = 4; tags[G // 3] = 2
    g = gallery(rows, ids, tags)
    qd = dev(q)
    for mask in (4, 0x80000001):
        keep = np.flatnonzero(tags & np.uint32(mask))
        assert 0 < len(keep) < G
        c = gallery(rows[keep], ids[keep], base=0)
        md = dev_u32(np.full(256, mask))
        back = lambda i: np.where(i >= 0, BASE + keep[np.maximum(i, 0)], -1).astype(np.int32)     # noqa: E731
        for Q, k in ((256, 16), (65, 5), (1, 1)):
            s, i = topk_rows(c, qd[:Q], k)
            assert_same(tagged_rows(g, qd[:Q], md[:Q], k), (s, back(i)), f"rows G{G} mask{mask:x} Q{Q} k{k}")
            s, d, r = topk_ids(c, qd[:Q], k)
            assert_same(tagged_ids(g, qd[:Q], md[:Q], k), (s, d, back(r)), f"ids G{G} mask{mask:x} Q{Q} k{k}")
    got = tagged_rows(g, qd, dev_u32(np.full(256, 4)), 3)[1]
    assert got[9, 0] == BASE + 5 and got[9, 1] == BASE + G // 2 and BASE + G // 3 not in got[9]


@pytest.mark.parametrize("G", [129, G_SEED])
def test_all_ones_answer_as_the_untagged_call_on_the_same_gallery(G):
    rng = np.random.default_rng(41 + G)
    dim = 512
    rows, q = unit(rng, G, dim), unit(rng, 256, dim)
    ids = (rng.permutation(G) // 3 + 10).astype(np.int32)
    qd, md = dev(q), dev_u32(np.full(256, ALL))
    g = gallery(rows, ids)                                         # tags never set
    assert (g.get_tags() == ALL).all() and len(g.get_tags(3, 0)) == 0
    for explicit in (False, True):
        if explicit:
            g.set_tags(np.full(G, ALL, np.uint32))
        for Q, k in ((256, 16), (64, 1), (63, 5)):
            assert_same(tagged_rows(g, qd[:Q], md[:Q], k), topk_rows(g, qd[:Q], k), f"rows G{G} Q{Q} k{k} set{explicit}")
            assert_same(tagged_ids(g, qd[:Q], md[:Q], k), topk_ids(g, qd[:Q], k), f"ids G{G} Q{Q} k{k} set{explicit}")
    one = dev_u32(np.full(256, 0x100))                              # any single bit admits an all-ones row
    assert_same(tagged_rows(g, qd, one, 16), topk_rows(g, qd, 16), "one bit against all-ones tags")


# ------------------------------------------------------------------------------------------ mask and tag cases
def test_the_best_row_of_every_query_is_excluded_for_it():
    """A kernel whose threshold is fed by excluded rows loses admitted rows here; one that filters afterwards lists too few."""
    dim, G, Q, k = 64, 4097, 65, 16
    rows, ids, q, sc = data(dim)
    sc = sc[:Q, :G]
    order = np.argsort(-sc.astype(np.float64), axis=1, kind="stable")
    tags = np.full(G, 1, np.uint32)
    tags[np.unique(order[:, :20])] = 2                              # the 20 best rows of EVERY query: more than k outrank the first admitted one
    masks = np.full(Q, 1, np.uint32)
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q[:Q]), dev_u32(masks)
    plain, got = topk_rows(g, qd, k), tagged_rows(g, qd, md, k)
    assert np.array_equal(plain[1][:, 0], BASE + order[:, 0])        # listed by the untagged call ...
    assert not np.isin(got[1], BASE + np.unique(order[:, :20])).any()   # ... and no excluded row by the tagged one
    assert (got[1] >= 0).all()                                      # full lists of other rows: filtering the untagged 16 gives nothing
    assert not any(set(a) & set(b) for a, b in zip(got[1].tolist(), plain[1].tolist()))
    assert_same(got, model.topk_from_scores(sc, tags, masks, k, BASE), "rows")
    assert_same(tagged_ids(g, qd, md, k), model.topk_ids_from_scores(sc, ids[:G], tags, masks, k, BASE), "ids")


@pytest.mark.parametrize("G", [4097, G_SEED])
def test_two_queries_of_one_tile_carry_different_masks(G):
    """Queries 0 and 1 are the SAME vector: the rows at its top alternate between bit 0 and bit 1, query 0 asks for bit 0 and query 1
    for bit 1 — the same scores, disjoint answers."""
    dim, k = 128, 16
    rows, ids, q, sc = data(dim)
    q2, sc2 = q[:64].copy(), sc[:64, :G].copy()
    q2[1], sc2[1] = q2[0], sc2[0]
    top = np.argsort(-sc2[0].astype(np.float64), kind="stable")[:40]
    tags = np.full(G, 3, np.uint32)
    tags[top[0::2]], tags[top[1::2]] = 1, 2
    masks = np.full(64, 3, np.uint32)
    masks[0], masks[1] = 1, 2
    want = model.topk_from_scores(sc2, tags, masks, k, BASE)
    assert not np.isin(want[1][0], want[1][1]).any() and want[1][0, 0] == BASE + top[0] and want[1][1, 0] == BASE + top[1]
    assert BASE + top[0] not in want[1][1] and BASE + top[1] not in want[1][0]
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q2), dev_u32(masks)
    assert_same(tagged_rows(g, qd, md, k), want, "rows")
    assert_same(tagged_ids(g, qd, md, k), model.topk_ids_from_scores(sc2, ids[:G], tags, masks, k, BASE), "ids")


REGIONS = {                                                          # name: (G, admitted positions)
    "three rows in all": (G_SEED, np.array([17, 4096, 69999])),
    "last partial tile, small": (300, np.arange(256, 300)),
    "last partial tile, seeded": (G_SEED, np.arange(69888, G_SEED)),
    "beyond the seed prefix": (G_SEED, np.arange(5000, G_SEED)),
    "inside the seed prefix": (G_SEED, np.arange(0, 4000)),
    "seed prefix holds fewer than k": (G_SEED, np.concatenate([np.arange(4090, 4096), np.arange(30000, 30100)])),
}


@pytest.mark.parametrize("name", list(REGIONS))
def test_admitted_rows_in_one_region_only(name):
    dim, k = 64, 16
    G, where = REGIONS[name]
    rows, ids, q, sc = data(dim)
    tags = np.full(G, 1, np.uint32)
    tags[where] = 6
    masks = np.full(256, 2, np.uint32)
    masks[100:110] = 1                                               # and a few queries that ask for everything else
    want = model.topk_from_scores(sc[:, :G], tags, masks, k, BASE)
    n_adm = min(len(where), k)
    assert ((want[1][:100] >= 0).sum(1) == n_adm).all() and np.isin(want[1][:100][want[1][:100] >= 0] - BASE, where).all()
    if n_adm < k:
        assert (want[1][0, n_adm:] == -1).all() and (want[0][0, n_adm:] == -1.0).all()      # the tail slots are empty
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q), dev_u32(masks)
    for Q in (256, 65):
        assert_same(tagged_rows(g, qd[:Q], md[:Q], k), [w[:Q] for w in want], f"{name} rows Q{Q}")
    assert_same(tagged_ids(g, qd, md, k), model.topk_ids_from_scores(sc[:, :G], ids[:G], tags, masks, k, BASE), f"{name} ids")
    assert_same(tagged_rows(g, qd[:1], md[:1], 1), [w[:1, :1] for w in want], f"{name} k1")


def test_duplicate_rows_with_different_tags_and_an_admitted_nan_row():
    dim, G, k = 128, G_SEED, 5
    rows, ids, q, sc = data(dim)
    rows, sc = rows.copy(), sc[:65].copy()
    dup, nan_row = [200, 9000, 9001, 69990], 4000
    rows[dup] = q[0]
    rows[nan_row, 5] = np.nan
    sc[:, dup + [nan_row]] = model.scores(q[:65], rows[dup + [nan_row]])
    tags = np.full(G, 1, np.uint32)
    tags[dup] = [1, 2, 6, 2]
    tags[nan_row] = 2
    masks = np.full(65, 2, np.uint32)
    masks[1] = 4
    want = model.topk_from_scores(sc, tags, masks, k, BASE)
    assert list(want[1][0, :3] - BASE) == [9000, 9001, 69990] and want[1][1, 0] == BASE + 9001 and (want[1][1, 1:] == -1).all()
    assert np.isnan(sc[:, nan_row]).all() and not (want[1] == BASE + nan_row).any()
    g = gallery(rows, ids, tags)
    qd, md = dev(q[:65]), dev_u32(masks)
    assert_same(tagged_rows(g, qd, md, k), want, "rows")
    assert_same(tagged_ids(g, qd, md, k), model.topk_ids_from_scores(sc, ids, tags, masks, k, BASE), "ids")


def test_an_unseeded_gallery_with_a_wholly_admitted_first_tile_replays_the_overflow():
    """4097 rows run without a seed: the lists start empty, all 128 rows of the first tile pass (-inf, INT_MAX), a 32-entry queue
    overflows and the four-round replay runs with the tag test in it."""
    dim, G, k = 64, 4097, 16
    rows, ids, q, sc = data(dim)
    sc = sc[:, :G]
    tags = np.full(G, 1, np.uint32)
    tags[128:] = np.where(np.arange(128, G) % 3 == 0, 2, 1)
    masks = np.full(256, 1, np.uint32)
    adm = model.admitted(tags, masks)
    assert ((adm[:, :128] & ~np.isnan(sc[:, :128])).sum(1) > 32).all()
    g = gallery(rows[:G], ids[:G], tags)
    qd, md = dev(q), dev_u32(masks)
    assert_same(tagged_rows(g, qd, md, k), model.topk_from_scores(sc, tags, masks, k, BASE), "rows")
    assert_same(tagged_ids(g, qd, md, k), model.topk_ids_from_scores(sc, ids[:G], tags, masks, k, BASE), "ids")


# ------------------------------------------------------------------------------------------ tile skip
def test_grouped_tags_skip_tiles_and_the_switch_changes_no_bit():
    dim, G, k = 64, G_SEED, 16
    rows, ids, q, sc = data(dim)
    tags = (np.uint32(1) << ((np.arange(G) // (128 * 9)) % 8).astype(np.uint32)).astype(np.uint32)      # runs of nine whole tiles share a bit
    g = gallery(rows, ids, tags)
    qd = dev(q)
    per_tile = np.repeat(np.uint32(1) << np.arange(4, dtype=np.uint32), 64)            # U differs per query tile
    for what, masks in (("one bit", np.full(256, 4, np.uint32)), ("a bit per query tile", per_tile)):
        md, ones = dev_u32(masks), dev_u32(np.full(256, ALL))
        want = model.topk_from_scores(sc, tags, masks, k, BASE)
        assert (want[1] >= 0).all()
        g.tag_stats()
        tagged_rows(g, qd, ones, k)
        visits, none = g.tag_stats()
        assert visits > 0 and none == 0
        assert g.tag_stats() == (0, 0)                              # the call resets
        got = tagged_rows(g, qd, md, k)
        scanned, skipped = g.tag_stats()
        assert skipped > 0 and scanned > 0 and scanned + skipped == visits, (what, scanned, skipped, visits)
        assert scanned < visits // 4, (what, scanned, visits)       # one group in eight (and the seed prefix) is multiplied
        assert_same(got, want, what)
        try:
            assert _lib.lib().fh_debug_tag_skip(0) == 0
            off = tagged_rows(g, qd, md, k)
            scanned, skipped = g.tag_stats()
            assert skipped == 0 and scanned == visits
            assert_same(off, got, what + ", skip off")
            assert_same(tagged_ids(g, qd, md, 5), model.topk_ids_from_scores(sc, ids, tags, masks, 5, BASE), what + " ids, skip off")
        finally:
            _lib.lib().fh_debug_tag_skip(1)
        assert_same(tagged_ids(g, qd, md, 5), model.topk_ids_from_scores(sc, ids, tags, masks, 5, BASE), what + " ids")
        assert g.tag_stats()[1] > 0


def test_scattered_tags_skip_nothing():
    dim, G, k = 64, G_SEED, 5
    rows, ids, q, sc = data(dim)
    tags = (np.uint32(1) << (np.arange(G) % 8).astype(np.uint32)).astype(np.uint32)     # every tile holds every bit
    masks = np.full(65, 4, np.uint32)
    g = gallery(rows, ids, tags)
    g.tag_stats()
    got = tagged_rows(g, dev(q[:65]), dev_u32(masks), k)
    scanned, skipped = g.tag_stats()
    assert skipped == 0 and scanned > 0
    assert_same(got, model.topk_from_scores(sc[:65], tags, masks, k, BASE), "scattered")


# ------------------------------------------------------------------------------------------ state
def test_set_tags_on_a_sub_range_get_tags_enroll_upload():
    dim, G, k = 64, 300, 5
    rows, ids, q, sc = data(dim)
    g = gallery(rows[:G])                                          # unlabelled
    qd = dev(q[:65])
    tags = np.full(G, ALL, np.uint32)
    tags[100:140] = 2                                               # straddles the border between tiles 0 and 1
    assert g.set_tags(np.full(40, 2, np.uint32), first=100) == 40
    assert np.array_equal(g.get_tags(), tags) and np.array_equal(g.get_tags(126, 4), tags[126:130])
    masks = np.where(np.arange(65) % 2 == 0, 1, 2).astype(np.uint32)
    md = dev_u32(masks)
    assert_same(tagged_rows(g, qd, md, k), model.topk_from_scores(sc[:65, :G], tags, masks, k, BASE), "sub-range")
    dt = dev_u32(np.full(28, 4))                                    # a device list, up to the last row
    assert g.set_tags(dt, first=272) == 28
    tags[272:] = 4
    assert np.array_equal(g.get_tags(), tags)
    # enrol: the new rows carry all ones, the old tags stay (across a capacity doubling)
    assert g.enroll(rows[G:G + 500]) == BASE + G
    tags = np.concatenate([tags, np.full(500, ALL, np.uint32)])
    assert np.array_equal(g.get_tags(), tags)
    for m in (2, 4, 8):
        masks = np.full(65, m, np.uint32)
        assert_same(tagged_rows(g, qd, dev_u32(masks), k), model.topk_from_scores(sc[:65, :G + 500], tags, masks, k, BASE), f"enrolled, mask {m}")
    # upload resets the tags
    rd = dev(rows[:G])
    g.upload(rd.data_ptr(), G, True, BASE)
    assert (g.get_tags() == ALL).all()
    assert_same(tagged_rows(g, qd, dev_u32(np.full(65, 8)), k), topk_rows(g, qd, k), "after upload")


def test_remove_ids_moves_the_tags_with_the_rows_and_rebuilds_the_tile_ors():
    dim, G, k = 64, 1000, 16
    rows, ids, q, sc = data(dim)
    ids = (np.arange(G) // 10).astype(np.int32)                    # identity j = rows 10 j .. 10 j + 9
    tags = np.full(G, 1, np.uint32)
    tags[384:512] = 2                                               # exactly tile 3
    g = gallery(rows[:G], ids, tags)
    sc = sc[:64]                                                    # one query tile: one workgroup per row tile
    qd = dev(q[:64])
    masks = np.full(64, 2, np.uint32)
    md = dev_u32(masks)
    assert_same(tagged_rows(g, qd, md, k), model.topk_from_scores(sc[:, :G], tags, masks, k, BASE), "before")
    gone = np.arange(3, 12, dtype=np.int32)                         # rows 30..119 go: the group now lies in rows 294..421, tiles 2 and 3
    keep = ~np.isin(ids, gone)
    assert g.remove_ids(gone) == 90 and len(g) == G - 90
    tags2 = tags[keep]
    assert np.array_equal(g.get_tags(), tags2) and list(np.flatnonzero(tags2 == 2)[[0, -1]]) == [294, 421]
    g.tag_stats()
    got = tagged_rows(g, qd, md, k)
    scanned, skipped = g.tag_stats()
    assert (scanned, skipped) == (2, 6)                             # eight tiles, one workgroup each: the two that hold the group
    assert_same(got, model.topk_from_scores(sc[:, :G][:, keep], tags2, masks, k, BASE), "after removal")
    assert_same(tagged_ids(g, qd, md, 5), model.topk_ids_from_scores(sc[:, :G][:, keep], ids[keep], tags2, masks, 5, BASE), "ids after removal")


def test_fuse_ors_the_tags_of_an_identity():
    dim, G = 64, 900
    rows, _, q, _ = data(dim)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 150, G).astype(np.int32) * 3 + 1
    tags = (np.uint32(1) << rng.integers(0, 6, G).astype(np.uint32)).astype(np.uint32)
    tags[rng.random(G) < 0.2] = 0
    src = gallery(rows[:G], ids, tags)
    dst = src.fuse()
    uniq = np.unique(ids)
    want_tags = np.array([np.bitwise_or.reduce(tags[ids == u]) for u in uniq], np.uint32)
    assert len(dst) == len(uniq) and np.array_equal(dst.ids(), uniq) and np.array_equal(dst.get_tags(), want_tags)
    assert len(set(want_tags.tolist())) > 8
    pooled = dst.rows()
    qd = dev(q[:65])
    masks = np.where(np.arange(65) % 2 == 0, 1, 0x24).astype(np.uint32)
    want = model.topk_ids(q[:65], pooled, uniq, want_tags, masks, 16, 0)
    assert_same(tagged_ids(dst, qd, dev_u32(masks), 16), want, "fused")
    plain = gallery(rows[:G], ids)                                  # a source without tags leaves the pooled gallery without tags
    d2 = plain.fuse(dst)
    assert (d2.get_tags() == ALL).all()
    assert_same(tagged_rows(d2, qd, dev_u32(np.full(65, 2)), 5), topk_rows(d2, qd, 5), "fused without tags")


def test_an_f16_rerank_gallery_answers_tagged_queries_with_the_fp32_scan():
    dim, G, k = 128, G_SEED, 16
    rows, ids, q, sc = data(dim)
    rng = np.random.default_rng(6)
    tags, masks = random_tags(rng, G), random_masks(rng, 65)
    g16 = gallery(rows, ids, tags, scan="f16")
    g32 = gallery(rows, ids, tags)
    qd, md = dev(q[:65]), dev_u32(masks)
    g16.scan_stats()
    got = tagged_rows(g16, qd, md, k)
    assert g16.scan_stats() == (0, 65)
    assert_same(got, tagged_rows(g32, qd, md, k), "rows")
    assert_same(got, model.topk_from_scores(sc[:65], tags, masks, k, BASE), "rows vs model")
    assert_same(tagged_ids(g16, qd, md, 1), tagged_ids(g32, qd, md, 1), "ids")
    assert g16.scan_stats() == (0, 65)
    assert g32.scan_stats() == (0, 0)


@pytest.mark.parametrize("labelled", [False, True])
def test_the_label_forms_are_strict_at_the_best_admitted_score(labelled):
    dim, G, Q = 64, 4097, 65
    rows, ids, q, sc = data(dim)
    sc = sc[:Q, :G]
    rng = np.random.default_rng(8)
    tags, masks = random_tags(rng, G), random_masks(rng, Q)
    masks[:3] = [0, 1, ALL]
    masks[40] = 4
    g = gallery(rows[:G], ids[:G] if labelled else None, tags)
    qd, md = dev(q[:Q]), dev_u32(masks)
    best = model.topk_from_scores(sc, tags, masks, 1, BASE)[0][:, 0]
    assert (best[[1, 2, 40]] > 0).all() and best[0] == -1.0
    for j in (1, 2, 40):
        for thr in (best[j], np.nextafter(best[j], np.float32(-np.inf))):
            want = model.label_from_scores(sc, tags, masks, thr, BASE, ids[:G] if labelled else None)
            got = tagged_label(g, qd, md, thr, ids=labelled)
            assert_same(got, want, f"labelled {labelled} query {j} thr {thr}")
            assert (got[0][j] == -1) == (thr == best[j]) and got[0][0] == -1 and got[1][0] == -1.0


def test_error_returns():
    dim, G = 64, 300
    rows, ids, q, _ = data(dim)
    L = fa.lib()
    g, u = gallery(rows[:G], ids[:G]), gallery(rows[:G])
    qd, md = dev(q[:9]), dev_u32(np.full(9, 1))
    s = torch.empty((9, 4), device="cuda"); i = torch.empty((9, 4), dtype=torch.int32, device="cuda"); r = torch.empty_like(i)
    a = (qd.data_ptr(), None, 9, 4, s.data_ptr(), i.data_ptr())
    assert L.fh_gallery_topk_tagged_dev(g._h, *a, None) == FH_ERR_ARG and "null" in _lib.last_error()          # NULL masks
    assert L.fh_gallery_topk_ids_tagged_dev(g._h, *a, r.data_ptr(), None) == FH_ERR_ARG
    assert L.fh_gallery_label_tagged_dev(g._h, qd.data_ptr(), None, 9, 0.5, i.data_ptr(), s.data_ptr(), None) == FH_ERR_ARG
    assert L.fh_gallery_label_ids_tagged_dev(g._h, qd.data_ptr(), None, 9, 0.5, i.data_ptr(), s.data_ptr(), None) == FH_ERR_ARG
    t = np.full(8, 1, np.uint32)
    for first, n in ((G - 7, 8), (-1, 2), (0, -1), (G, 1)):         # set_tags / get_tags out of range
        assert L.fh_gallery_set_tags(g._h, first, n, t.ctypes.data, 0) == FH_ERR_ARG
        assert L.fh_gallery_get_tags(g._h, first, n, t.ctypes.data) == FH_ERR_ARG
    assert L.fh_gallery_set_tags(g._h, 0, 2, None, 0) == FH_ERR_ARG and L.fh_gallery_set_tags(None, 0, 2, t.ctypes.data, 0) == FH_ERR_ARG
    assert L.fh_gallery_set_tags(g._h, G, 0, None, 0) == 0 and (g.get_tags() == ALL).all()
    assert L.fh_gallery_tag_stats(None, None, None) == FH_ERR_ARG
    b = (qd.data_ptr(), md.data_ptr(), 9)                           # the identity forms on an unlabelled gallery
    assert L.fh_gallery_topk_ids_tagged_dev(u._h, *b, 4, s.data_ptr(), i.data_ptr(), None, None) == FH_ERR_STATE
    assert L.fh_gallery_label_ids_tagged_dev(u._h, *b, 0.5, i.data_ptr(), s.data_ptr(), None) == FH_ERR_STATE
    assert L.fh_gallery_topk_tagged_dev(u._h, *b, 17, s.data_ptr(), i.data_ptr(), None) < 0          # k beyond 16
    torch.cuda.synchronize()
    e = fa.Gallery(dim)                                             # an empty gallery: empty answers
    got = tagged_rows(e, qd, md, 4)
    assert (got[0] == -1.0).all() and (got[1] == -1).all()
    got = tagged_ids(e, qd, md, 4)
    assert (got[0] == -1.0).all() and (got[1] == -1).all() and (got[2] == -1).all()
    lab, best = tagged_label(e, qd, md, 0.0)
    assert (lab == -1).all() and (best == -1.0).all()


def test_a_captured_tagged_call_reads_the_masks_at_replay():
    dim, Q, k = 64, 65, 16
    rows, ids, q, sc = data(dim)
    rng = np.random.default_rng(9)
    tags = random_tags(rng, G_SEED)
    g = gallery(rows, ids, tags)
    qd = dev(q[:Q])
    m1, m2 = random_masks(rng, Q), np.roll(random_masks(rng, Q), 3)
    m2[0] = 2 if m1[0] != 2 else 4
    md = dev_u32(m1)
    eager = tagged_ids(g, qd, md, k)                                # the warm-up call of the same (nq, k)
    assert_same(eager, model.topk_ids_from_scores(sc[:Q], ids, tags, m1, k, BASE), "eager")
    s = torch.zeros((Q, k), device="cuda"); d = torch.zeros((Q, k), dtype=torch.int32, device="cuda"); r = torch.zeros_like(d)
    side = side_stream_leaving_the_pool_as_it_was()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.topk_ids_tagged_dev(qd.data_ptr(), md.data_ptr(), Q, k, s.data_ptr(), d.data_ptr(), r.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    for masks in (m1, m2, m1):
        md.copy_(dev_u32(masks))                                    # new contents, same buffer
        s.fill_(3.0); d.fill_(-3); r.fill_(-3)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = model.topk_ids_from_scores(sc[:Q], ids, tags, masks, k, BASE)
        assert_same((s.cpu().numpy(), d.cpu().numpy(), r.cpu().numpy()), want, "replay")
    assert not np.array_equal(model.topk_ids_from_scores(sc[:Q], ids, tags, m2, k, BASE)[2], eager[2])
