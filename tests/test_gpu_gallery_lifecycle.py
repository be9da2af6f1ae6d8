"""One gallery handle with every per-row column live — labelled, tagged, F16_RERANK — walked through its whole life: upload, two
growths by enrolment (the first crosses the 128-row tile, the second is geometric), a tag change that straddles a tile border, a
removal that moves survivors across tile borders and shrinks the capacity, growth from the shrunken capacity, both scan-mode
switches, and template pooling into a second handle.

After every step the handle is held against a numpy mirror: rows, ids and tags bit for bit; the row top-k against
`oracle.gallery_topk_mfma`, the identity top-k (k = 1: the row top-1 of the scan mode; k = 4: the fp32 identity scan) against
tests/gallery_ids_model.py and both tagged forms against tests/gallery_tags_model.py, bit for bit as the tests of those paths assert;
scan_stats() must add up to the queries issued, and tag_stats() must report exactly the visits the mirror's tile ORs allow to be
skipped — so no tile is skipped while a row of it is admitted.  What this catches: a column left at a stale capacity, a tile_or word
not rebuilt, a wrong kernel picked for a (identities?, tags?) combination.

dim 128 certifies through the fp16 scan, dim 64 never does (the whole batch takes the fp32 route); Q = 5 and 65: one query tile and
two.  At most 470 rows: every gallery here is far below the seed pass, so every (query tile, row tile) pair is visited exactly once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from oracle import oracle                     # noqa: E402
from tests import gallery_fuse_model as fuse_model  # noqa: E402
from tests import gallery_ids_model as ids_model    # noqa: E402
from tests import gallery_tags_model as tags_model  # noqa: E402
from tests.test_gpu_gallery_tags import assert_same, dev, dev_u32, tagged_ids, tagged_rows, topk_ids, topk_rows  # noqa: E402

ALL = tags_model.TAG_ALL
BASE, K, TILE = 1000, 4, 128
N_UPLOAD, N_FIRST, N_SECOND, N_LAST = 100, 60, 300, 10
N_POOL = N_UPLOAD + N_FIRST + N_SECOND + N_LAST


def case(dim):
    """A pool of clustered rows whose 60 identities are scattered over all of it (so a removal takes rows from every tile), and 65
    queries: most near a row, some near nobody."""
    rng = np.random.default_rng(500 + dim)
    ids = (rng.integers(0, 60, N_POOL) * 7 + 3).astype(np.int32)
    centres = fuse_model.unit_rows(rng, 60 * 7 + 4, dim)
    rows = centres[ids] + np.float32(0.05) * rng.standard_normal((N_POOL, dim), dtype=np.float32)
    rows = np.ascontiguousarray(rows / np.linalg.norm(rows, axis=1, keepdims=True), np.float32)
    near = rows[rng.integers(0, N_POOL, 50)] + np.float32(0.05) * rng.standard_normal((50, dim), dtype=np.float32)
    q = np.concatenate([near / np.linalg.norm(near, axis=1, keepdims=True), fuse_model.unit_rows(rng, 15, dim)])
    return rows, ids, np.ascontiguousarray(q[rng.permutation(65)], np.float32), rng


class Mirror:
    def __init__(self, rows, ids, tags, base):
        self.rows, self.ids, self.tags, self.base = rows.copy(), ids.copy(), np.asarray(tags, np.uint32).copy(), base

    def append(self, rows, ids):
        self.rows = np.concatenate([self.rows, rows]); self.ids = np.concatenate([self.ids, ids])
        self.tags = np.concatenate([self.tags, np.full(len(ids), ALL, np.uint32)])

    def keep(self, mask):
        self.rows, self.ids, self.tags = self.rows[mask], self.ids[mask], self.tags[mask]

    def skippable(self, masks):
        """(visits, skips) of one tagged call: a (query tile, row tile) pair may be skipped iff no tag of the tile shares a bit with
        any mask of the query tile."""
        ors = [np.bitwise_or.reduce(self.tags[t:t + TILE]) for t in range(0, len(self.tags), TILE)]
        us = [np.bitwise_or.reduce(masks[t:t + 64]) for t in range(0, len(masks), 64)]
        return len(ors) * len(us), sum(1 for u in us for o in ors if (o & u) == 0)


def check(g, m, q, qd, mask_sets, certifies, what):
    G = len(m.ids)
    assert len(g) == G, what
    assert np.array_equal(g.rows().view(np.uint32), m.rows.view(np.uint32)), what
    assert np.array_equal(g.ids(), m.ids), what
    assert np.array_equal(g.get_tags(), m.tags), what
    sc = ids_model.scores(q, m.rows)
    want_rows = oracle.gallery_topk_mfma(q, m.rows, K, base=m.base)
    want_ids = ids_model.topk_ids_from_scores(sc, m.ids, K, m.base)
    g.scan_stats()
    issued = 0
    for Q in (5, 65):
        assert_same(topk_rows(g, qd[:Q], K), [w[:Q] for w in want_rows], f"{what}: rows Q{Q}")
        assert_same(topk_ids(g, qd[:Q], 1), [w[:Q, :1] for w in want_ids], f"{what}: ids k1 Q{Q}")
        assert_same(topk_ids(g, qd[:Q], K), [w[:Q] for w in want_ids], f"{what}: ids k{K} Q{Q}")
        issued += 3 * Q
        for name, masks in mask_sets:
            masks = masks[:Q]
            md = dev_u32(masks)
            visits, skips = m.skippable(masks)
            g.tag_stats()
            got = tagged_rows(g, qd[:Q], md, K)
            assert g.tag_stats() == (visits - skips, skips), (what, name, Q)
            assert_same(got, tags_model.topk_from_scores(sc[:Q], m.tags, masks, K, m.base), f"{what}: tagged rows, {name}, Q{Q}")
            got = tagged_ids(g, qd[:Q], md, K)
            assert g.tag_stats() == (visits - skips, skips), (what, name, Q)
            assert_same(got, tags_model.topk_ids_from_scores(sc[:Q], m.ids, m.tags, masks, K, m.base), f"{what}: tagged ids, {name}, Q{Q}")
            issued += 2 * Q
    c, f = g.scan_stats()
    if g.scan == "f16":
        assert c + f == issued and c <= 2 * (5 + 65), (what, c, f, issued)       # only the rows and the k = 1 identities can certify
        assert certifies or c == 0, (what, c)
    else:
        assert (c, f) == (0, 0), what


@pytest.mark.parametrize("dim", [128, 64])
def test_one_handle_through_its_whole_life(dim):
    rows, ids, q, rng = case(dim)
    qd = dev(q)
    narrow = np.full(65, 4, np.uint32); narrow[2] = 0                # one bit for every query: whole tiles without it are skipped
    mixed = rng.choice(np.array([0, ALL, 1, 2, 4, 8, 3, 0x10], np.uint64), 65).astype(np.uint32)
    mixed[64] = 8                                                     # the second query tile holds this query alone
    mask_sets = (("one bit", narrow), ("mixed", mixed))
    certifies = dim % 128 == 0

    # 1. upload with ids, then tags in runs of 50 rows: no row of the only tile carries bit 2
    a = N_UPLOAD
    tags = (np.uint32(1) << (np.arange(a) // 50).astype(np.uint32)).astype(np.uint32)
    g = fa.Gallery(dim, scan="f16")
    rd, idd = dev(rows[:a]), dev(ids[:a])
    g.upload(rd.data_ptr(), a, True, BASE, ids_ptr=idd.data_ptr())
    assert g.set_tags(tags) == a
    m = Mirror(rows[:a], ids[:a], tags, BASE)
    assert m.skippable(narrow[:5]) == (1, 1)
    check(g, m, q, qd, mask_sets, certifies, "upload")

    # 2. / 3. the first growth (across the 128-row tile), then a geometric one
    for n, what in ((N_FIRST, "first enrolment"), (N_SECOND, "second enrolment")):
        assert g.enroll(rows[a:a + n], ids[a:a + n]) == BASE + a
        m.append(rows[a:a + n], ids[a:a + n])
        a += n
        check(g, m, q, qd, mask_sets, certifies, what)

    # 4. tags of rows 120..139: both sides of the border between tiles 0 and 1
    assert g.set_tags(dev_u32(np.full(20, 8)), first=120) == 20
    m.tags[120:140] = 8
    check(g, m, q, qd, mask_sets, certifies, "set_tags")

    # 5. every third identity goes: survivors of every tile move to a lower one, and the capacity shrinks to the survivors
    gone = np.unique(ids)[::3]
    keep = ~np.isin(m.ids, gone)
    assert keep[:TILE].sum() < TILE - 20 and keep.sum() > 2 * TILE
    assert g.remove_ids(gone) == int((~keep).sum())
    m.keep(keep)
    check(g, m, q, qd, mask_sets, certifies, "remove_ids")

    # 6. growth from the shrunken capacity (ids that were removed come back)
    assert g.enroll(rows[a:a + N_LAST], ids[a:a + N_LAST]) == BASE + len(m.ids)
    m.append(rows[a:a + N_LAST], ids[a:a + N_LAST])
    check(g, m, q, qd, mask_sets, certifies, "third enrolment")

    # 7. the fp16 column goes and comes back
    for mode in ("fp32", "f16"):
        g.set_scan(mode)
        assert g.scan == mode
        check(g, m, q, qd, mask_sets, certifies, f"set_scan {mode}")

    # 8. pooled into a second handle with every column live: sums bit for bit, ascending ids, the OR of each identity's tags, base 0
    dst = g.fuse(fa.Gallery(dim, scan="f16"), mode="sum")
    sums, uniq, _ = fuse_model.fuse_sums(m.rows, m.ids)
    pooled_tags = np.array([np.bitwise_or.reduce(m.tags[m.ids == u]) for u in uniq], np.uint32)
    check(dst, Mirror(sums, uniq, pooled_tags, 0), q, qd, mask_sets, certifies, "fuse")
    check(g, m, q, qd, mask_sets, certifies, "the source after fuse")
