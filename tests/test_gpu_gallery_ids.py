"""The labelled gallery on the GPU, BIT FOR BIT (score bits, identity ids, representative rows) against the numpy model of
tests/gallery_ids_model.py (scores from `oracle.dot_mfma`, the scan's own fma order): identity top-k across dims, row counts, query
counts, k and cluster sizes; the list edges (one identity, fewer identities than k, a tile full of one identity's templates, exact
duplicate rows within and across identities, a NaN row); removal with both scan modes afterwards; label_ids at and just below the
best score; the identity merge (cached / uncached) against a numpy merge; the labelled / unlabelled state errors; graph capture."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from oracle import oracle                     # noqa: E402
from tests import gallery_ids_model as model  # noqa: E402

FH_ERR_STATE = -4
G_SEED = 70001                                # >= 65536 (seed pass); last 128-row tile holds 113 rows


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def labelled(rows, ids, base=0, scan="fp32"):
    g = fa.Gallery(rows.shape[1], scan=scan)
    rd, idd = dev(rows), dev(np.asarray(ids, np.int32))
    g.upload(rd.data_ptr(), rows.shape[0], True, base, ids_ptr=idd.data_ptr())
    return g


def topk_ids(g, qd, k, want_rows=True):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda")
    di = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    ri = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_ids_dev(qd.data_ptr(), Q, k, sc.data_ptr(), di.data_ptr(), ri.data_ptr() if want_rows else None, 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), di.cpu().numpy(), ri.cpu().numpy()


def topk_rows(g, qd, k):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda"); ix = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_dev(qd.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ix.cpu().numpy()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    for a, b, name in zip(got, want, ("scores", "ids", "rows")):
        a, b = bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b))
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:6], a[a != b][:6], b[a != b][:6])


def assert_same_rows(got, want, what):
    (s, i), (ms, mi) = got, want
    assert np.array_equal(i, mi), (what, np.argwhere(i != mi)[:8])
    assert np.array_equal(bits(s), bits(np.ascontiguousarray(ms))), what


def clustered(rng, G, dim, T, noise=0.02):
    """G rows in clusters of T templates (a centre plus small noise), shuffled; sparse unsorted ids."""
    n_ids = (G + T - 1) // T
    centres = unit(rng, n_ids, dim)
    rows = np.repeat(centres, T, axis=0)[:G] + np.float32(noise) * rng.standard_normal((G, dim), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    labels = (rng.permutation(4 * n_ids)[:n_ids] * 13 + 5).astype(np.int32)
    ids = np.repeat(labels, T)[:G]
    o = rng.permutation(G)
    return np.ascontiguousarray(rows[o], np.float32), ids[o], centres


def queries_near(rng, centres, Q, noise=0.02):
    c = centres[rng.integers(0, len(centres), Q)]
    q = c + np.float32(noise) * rng.standard_normal(c.shape, dtype=np.float32)
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), np.float32)


# ------------------------------------------------------------------------------------------ distinct ids = the row-level scan
@pytest.mark.timeout(300)
@pytest.mark.parametrize("base", [0, 2 ** 31 - 1 - G_SEED - 5])
def test_distinct_ids_answer_as_the_row_level_scan(base):
    rng = np.random.default_rng(11 + base % 97)
    dim = 512
    rows, q = unit(rng, G_SEED, dim), unit(rng, 256, dim)
    rows[40000] = rows[17] = q[3]                              # a tie across "identities"
    labels = (rng.permutation(8 * G_SEED)[:G_SEED] * 3 + 1).astype(np.int32)
    g = labelled(rows, labels, base)
    assert len(g) == G_SEED and np.array_equal(g.ids(), labels) and np.array_equal(g.ids(5, 3), labels[5:8])
    qd = dev(q)
    for Q, k in ((1, 1), (65, 5), (256, 16), (256, 1), (64, 16)):
        s, d, r = topk_ids(g, qd[:Q], k)
        rs, ri = topk_rows(g, qd[:Q], k)
        assert_same_rows((s, r), (rs, ri), f"Q{Q} k{k}")
        assert (r >= base).all() and np.array_equal(d, labels[r - base]), (Q, k)
        s2, d2, _ = topk_ids(g, qd[:Q], k, want_rows=False)     # d_rows = NULL
        assert np.array_equal(bits(s2), bits(s)) and np.array_equal(d2, d)
    assert r[3, 0] == base + 17 and r[3, 1] == base + 40000


# ------------------------------------------------------------------------------------------ clustered identities vs the model
@pytest.mark.timeout(600)
@pytest.mark.parametrize("T", [1, 3, 8, 40])
@pytest.mark.parametrize("dim", [64, 192, 512, 2048])
def test_clustered_identities_match_the_model(dim, T):
    """One identity's templates crowd a query's top: the row-level answer would be one person several times."""
    rng = np.random.default_rng(100 * dim + T)
    base = 1000 + T
    rows, ids, centres = clustered(rng, G_SEED, dim, T)
    q = queries_near(rng, centres, 256)
    q[200:] = unit(rng, 56, dim)                               # and some queries near nobody
    sc = model.scores(q, rows)
    qd, rd, idd = dev(q), dev(rows), dev(ids)
    g = fa.Gallery(dim)
    crowded = 0
    for G in (1, 31, 128, 129, 4097, G_SEED):
        g.upload(rd.data_ptr(), G, True, base, ids_ptr=idd.data_ptr())
        assert len(g) == G
        want = model.topk_ids_from_scores(sc[:, :G], ids[:G], 16, base)
        for Q in (1, 64, 65, 256):
            for k in (1, 5, 16):
                got = topk_ids(g, qd[:Q], k)
                assert_same(got, [w[:Q, :k] for w in want], f"dim{dim} T{T} G{G} Q{Q} k{k}")
        n_ids = len(np.unique(ids[:G]))
        assert ((want[1] >= 0).sum(1) == min(16, n_ids)).all()
        if G == G_SEED and T > 1:                               # the row-level list of the same gallery repeats people
            _, ri = topk_rows(g, qd, 16)
            crowded = sum(len(set(ids[ri[i] - base])) < 16 for i in range(200))
    assert T == 1 or crowded > 100, crowded


# ------------------------------------------------------------------------------------------ edges
@pytest.mark.timeout(300)
def test_every_row_of_one_identity():
    """One entry, then empty slots; nothing ever tightens the threshold, so every tile replays through the overflow path."""
    rng = np.random.default_rng(21)
    dim, G = 256, 20000
    rows, q = unit(rng, G, dim), unit(rng, 65, dim)
    ids = np.full(G, 77, np.int32)
    g = labelled(rows, ids, base=9)
    want = model.topk_ids(q, rows, ids, 16, base=9)
    assert (want[1][:, 0] == 77).all() and (want[1][:, 1:] == -1).all() and (want[2][:, 1:] == -1).all() and (want[0][:, 1:] == -1.0).all()
    for k in (1, 2, 16):
        assert_same(topk_ids(g, dev(q), k), [w[:, :k] for w in want], f"one identity k{k}")
    rs, ri = topk_rows(g, dev(q), 1)
    assert np.array_equal(ri[:, 0], want[2][:, 0])


@pytest.mark.timeout(300)
def test_fewer_identities_than_k():
    rng = np.random.default_rng(22)
    dim, G = 192, 5000
    rows, q = unit(rng, G, dim), unit(rng, 64, dim)
    ids = rng.choice(np.array([3, 1000000, 2 ** 31 - 1, 0, 42], np.int32), G)
    g = labelled(rows, ids)
    want = model.topk_ids(q, rows, ids, 16)
    assert ((want[1] >= 0).sum(1) == 5).all()
    for k in (3, 5, 6, 16):
        assert_same(topk_ids(g, dev(q), k), [w[:, :k] for w in want], f"five identities k{k}")


@pytest.mark.timeout(300)
def test_more_than_32_templates_of_one_identity_pass_in_one_tile():
    """Tile 300 (rows 38400..38527) holds 100 templates of identity 9 that all beat query 0's threshold, ascending in score (each
    replaces the listed one), and tile 301 forty more beside sixteen other strong identities."""
    rng = np.random.default_rng(23)
    dim = 512
    rows, q = unit(rng, G_SEED, dim), unit(rng, 65, dim)
    ids = (rng.permutation(G_SEED) + 100).astype(np.int32)
    near = q[0][None] + np.float32(0.3) * unit(rng, 140, dim)
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    near = near[np.argsort(oracle.dot_mfma(q[0], near), kind="stable")]
    rows[38400:38500], ids[38400:38500] = near[:100], 9
    rows[38528:38568], ids[38528:38568] = near[100:], 9
    other = q[0][None] + np.float32(0.5) * unit(rng, 16, dim)
    rows[38570:38586] = other / np.linalg.norm(other, axis=1, keepdims=True)
    g = labelled(rows, ids, base=5)
    want = model.topk_ids(q, rows, ids, 16, base=5)
    assert want[1][0, 0] == 9 and want[2][0, 0] == 5 + 38567 and set(want[2][0, 1:] - 5) <= set(range(38570, 38586))
    for k in (1, 5, 16):
        assert_same(topk_ids(g, dev(q), k), [w[:, :k] for w in want], f"crowded tile k{k}")


@pytest.mark.timeout(300)
def test_duplicate_rows_within_and_across_identities_and_a_nan_row():
    rng = np.random.default_rng(24)
    dim, G, base = 512, 30000, 77
    rows, q = unit(rng, G, dim), unit(rng, 65, dim)
    ids = np.repeat((rng.permutation(G // 4) * 5 + 2).astype(np.int32), 4)[rng.permutation(G)]
    # across identities: the same row under different ids in different tiles / parts -> the lower row wins the tie
    for r in (200, 9000, 9001, 29999):
        rows[r] = q[0]
    ids[[200, 9000, 9001, 29999]] = [50001, 50002, 50003, 50004]
    # within an identity: three copies -> the lowest row represents
    for r in (12345, 300, 25000):
        rows[r] = q[1]
    ids[[12345, 300, 25000]] = 60000
    rows[4000, 5] = np.nan                                      # a NaN row is never listed
    ids[4000] = 60001
    g = labelled(rows, ids, base)
    want = model.topk_ids(q, rows, ids, 16, base)
    assert list(want[2][0, :4] - base) == [200, 9000, 9001, 29999] and list(want[1][0, :4]) == [50001, 50002, 50003, 50004]
    assert want[2][1, 0] - base == 300 and want[1][1, 0] == 60000 and (want[1][1, 1:] != 60000).all()
    assert not (want[1] == 60001).any()
    for Q, k in ((65, 16), (65, 1), (2, 4)):
        got = topk_ids(g, dev(q[:Q]), k)
        assert_same(got, [w[:Q, :k] for w in want], f"duplicates Q{Q} k{k}")
    q2 = q.copy(); q2[7, 0] = np.nan                             # and a NaN query: all slots empty, the others untouched
    got = topk_ids(g, dev(q2), 16)
    assert (got[1][7] == -1).all() and (got[2][7] == -1).all() and (got[0][7] == -1.0).all()
    keep = np.arange(65) != 7
    assert_same([x[keep] for x in got], [w[keep] for w in want], "beside a NaN query")


# ------------------------------------------------------------------------------------------ removal
def check_all_modes(g, g16, q, qd, rows, ids, base, tag):
    """Row-level top-k in both scan modes against the oracle, identity top-k in both against the model, on the rows a gallery should
    hold now."""
    assert len(g) == len(ids) == len(g16) and np.array_equal(g.ids(), ids) and np.array_equal(g16.ids(), ids), tag
    ms, mi = oracle.gallery_topk_mfma(q, rows, 16, base=base)
    want = model.topk_ids(q, rows, ids, 16, base)
    for k in (16, 1):
        for gg, name in ((g, "fp32"), (g16, "f16")):
            assert_same_rows(topk_rows(gg, qd, k), (ms[:, :k], mi[:, :k]), f"{tag} rows {name} k{k}")
            assert_same(topk_ids(gg, qd, k), [w[:, :k] for w in want], f"{tag} ids {name} k{k}")


@pytest.mark.timeout(600)
def test_removal_compacts_rows_ids_and_the_fp16_copy():
    rng = np.random.default_rng(31)
    dim, G, T, base = 512, 30000, 5, 4321
    rows, ids, centres = clustered(rng, G, dim, T)
    q = queries_near(rng, centres, 65)
    qd = dev(q)
    g, g16 = labelled(rows, ids, base), labelled(rows, ids, base, scan="f16")
    g16.scan_stats()
    check_all_modes(g, g16, q, qd, rows, ids, base, "before")
    c, f = g16.scan_stats()
    assert f >= 65, (c, f)                                        # the k = 16 identity query is the fp32 scan: 65 fall-backs
    everyone = np.unique(ids)
    gone = set(rng.choice(everyone, len(everyone) // 3, replace=False).tolist()) | {int(ids[0]), int(ids[-1])}
    gone_list = np.array(sorted(gone) + [2 ** 31 - 2, int(ids[0])], np.int32)      # an id nobody has, and a duplicate
    keep = ~np.isin(ids, gone_list)
    n_gone = int((~keep).sum())
    assert g.remove_ids(gone_list) == n_gone and g16.remove_ids(gone_list) == n_gone
    assert g.remove_ids([2 ** 31 - 2]) == 0 and g.remove_ids(gone_list) == 0
    rows, ids = np.ascontiguousarray(rows[keep]), ids[keep]
    check_all_modes(g, g16, q, qd, rows, ids, base, "after removal")
    # enrol more, across a capacity doubling (the buffers hold exactly the survivors after a removal)
    more_rows, more_ids, _ = clustered(rng, len(ids) + 300, dim, 3)
    more_ids = more_ids + np.int32(10 ** 8)
    more_rows[5] = q[2]
    for gg in (g, g16):
        assert gg.enroll(more_rows, ids=more_ids) == base + len(ids)
    rows, ids = np.concatenate([rows, more_rows]), np.concatenate([ids, more_ids])
    check_all_modes(g, g16, q, qd, rows, ids, base, "after enrol")
    # remove everything: all answers -1, then enrol again
    for gg in (g, g16):
        assert gg.remove_ids(np.unique(ids)) == len(ids) and len(gg) == 0 and gg.ids().shape == (0,)
        s, d, r = topk_ids(gg, qd, 16)
        assert (s == -1.0).all() and (d == -1).all() and (r == -1).all()
        s, d, r = topk_ids(gg, qd, 1)
        assert (s == -1.0).all() and (d == -1).all() and (r == -1).all()
        lab = torch.full((65,), 5, dtype=torch.int32, device="cuda"); bs = torch.zeros(65, device="cuda")
        gg.label_ids_dev(qd.data_ptr(), 65, 0.0, lab.data_ptr(), bs.data_ptr(), 0)
        torch.cuda.synchronize()
        assert (lab.cpu().numpy() == -1).all() and (bs.cpu().numpy() == -1.0).all()
        assert gg.enroll(more_rows[:700], ids=more_ids[:700]) == base
    check_all_modes(g, g16, q, qd, more_rows[:700], more_ids[:700], base, "re-enrolled")


# ------------------------------------------------------------------------------------------ label_ids
@pytest.mark.timeout(300)
@pytest.mark.parametrize("scan", ["fp32", "f16"])
def test_label_ids_is_strict_at_the_best_score(scan):
    rng = np.random.default_rng(41)
    dim, G = 512, 20000
    rows, ids, centres = clustered(rng, G, dim, 4)
    q = queries_near(rng, centres, 100)
    g = labelled(rows, ids, base=50, scan=scan)
    want = model.topk_ids(q, rows, ids, 1, base=50)
    qd = dev(q)
    for Q in (1, 100):
        best = want[0][:Q, 0]
        for thr_of, expect in ((lambda b: b, -1), (lambda b: np.nextafter(b, np.float32(-np.inf)), None)):
            lab = torch.full((Q,), -5, dtype=torch.int32, device="cuda"); sc = torch.zeros(Q, device="cuda")
            # one threshold per call: query j's own best score decides query j only
            for j in range(0, Q, 17):
                thr = float(thr_of(best[j]))
                g.label_ids_dev(qd.data_ptr(), Q, thr, lab.data_ptr(), sc.data_ptr(), 0)
                torch.cuda.synchronize()
                l, s = lab.cpu().numpy(), sc.cpu().numpy()
                assert np.array_equal(bits(s), bits(np.ascontiguousarray(best)))
                assert np.array_equal(l, np.where(best > np.float32(thr), want[1][:Q, 0], -1))
                assert l[j] == (want[1][j, 0] if expect is None else expect)


# ------------------------------------------------------------------------------------------ merge
def crafted_parts(rng, W, Q, k):
    """[W][Q][k] identity lists as shards would write them: sorted, distinct ids within a list, the SAME id in several parts, equal
    scores across parts, -1 tails (score 7.0 there: emptiness is told by the row), rows distinct across the whole."""
    n_ids = max(k, (W * k) // 3)
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 0.5, 0.25, -1e30, 1.0], np.float32)
    s = np.where(rng.random((W, Q, k)) < 0.6, rng.choice(special, (W, Q, k)), rng.standard_normal((W, Q, k), dtype=np.float32)).astype(np.float32)
    r = np.stack([rng.permutation(2 * W * k)[:W * k] + 1 for _ in range(Q)]).reshape(Q, W, k).transpose(1, 0, 2).astype(np.int32)
    d = np.empty((W, Q, k), np.int32)
    for w in range(W):
        for qi in range(Q):
            d[w, qi] = rng.choice(n_ids, k, replace=False) * 7 + 1
    o = np.lexsort((r, -s.astype(np.float64)), axis=-1)
    s, r = np.take_along_axis(s, o, -1), np.take_along_axis(r, o, -1)
    fill = rng.integers(0, k + 1, (W, Q, 1))
    fill[0, :, 0] = k
    empty = np.arange(k)[None, None, :] >= fill
    s[empty], r[empty], d[empty] = 7.0, -1, -1
    return np.ascontiguousarray(s), np.ascontiguousarray(d), np.ascontiguousarray(r)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("W", [1, 2, 8, 600])
def test_merge_ids_matches_a_numpy_merge(W):
    """W * k = 9600 entries take the uncached path."""
    rng = np.random.default_rng(50 + W)
    Q = 5
    for k in (16, 1, 7):
        s, d, r = crafted_parts(rng, W, Q, k)
        want = model.merge_ids(s, d, r, k)
        if W > 1 and k > 1:
            assert any(len(set(d[:, qi][r[:, qi] >= 0].tolist())) < (r[:, qi] >= 0).sum() for qi in range(Q))     # ids do repeat
        sd, dd, rd = dev(s), dev(d), dev(r)
        os_ = torch.full((Q, k), 9.0, device="cuda")
        od = torch.full((Q, k), -9, dtype=torch.int32, device="cuda"); orow = torch.full((Q, k), -9, dtype=torch.int32, device="cuda")
        assert fa.topk_merge_ids_dev(sd.data_ptr(), dd.data_ptr(), rd.data_ptr(), W, Q, k, os_.data_ptr(), od.data_ptr(), orow.data_ptr()) == Q
        torch.cuda.synchronize()
        assert_same((os_.cpu().numpy(), od.cpu().numpy(), orow.cpu().numpy()), want, f"W{W} k{k}")


@pytest.mark.timeout(300)
def test_merge_of_shard_answers_is_the_whole_gallery_answer():
    rng = np.random.default_rng(61)
    dim, G, k = 256, 9000, 16
    rows, ids, centres = clustered(rng, G, dim, 8)
    q = queries_near(rng, centres, 33)
    qd = dev(q)
    whole = topk_ids(labelled(rows, ids, 100), qd, k)
    cuts = [0, 1000, 1001, 5000, G]
    parts = [topk_ids(labelled(rows[a:b], ids[a:b], 100 + a), qd, k) for a, b in zip(cuts[:-1], cuts[1:])]
    ps, pd, pr = (dev(np.stack([p[j] for p in parts])) for j in range(3))
    os_ = torch.empty((33, k), device="cuda"); od = torch.empty((33, k), dtype=torch.int32, device="cuda"); orow = torch.empty_like(od)
    fa.topk_merge_ids_dev(ps.data_ptr(), pd.data_ptr(), pr.data_ptr(), 4, 33, k, os_.data_ptr(), od.data_ptr(), orow.data_ptr())
    torch.cuda.synchronize()
    assert_same((os_.cpu().numpy(), od.cpu().numpy(), orow.cpu().numpy()), whole, "shards")
    assert_same(whole, model.topk_ids(q, rows, ids, k, 100), "whole")


# ------------------------------------------------------------------------------------------ state errors
@pytest.mark.timeout(300)
def test_mixing_labelled_and_unlabelled_is_a_state_error_and_changes_nothing():
    rng = np.random.default_rng(71)
    dim, G = 128, 500
    rows, q = unit(rng, G, dim), unit(rng, 9, dim)
    ids = (rng.permutation(G) // 3 + 10).astype(np.int32)
    L = fa.lib()
    qd, rd, idd = dev(q), dev(rows), dev(ids)
    out_s = torch.empty((9, 4), device="cuda"); out_i = torch.empty((9, 4), dtype=torch.int32, device="cuda")

    g = labelled(rows, ids, 3)
    before = topk_ids(g, qd, 4)
    assert L.fh_gallery_enroll(g._h, rows.ctypes.data, 5, 0) == FH_ERR_STATE and "labelled" in _lib.last_error()
    assert L.fh_gallery_upload(g._h, rd.data_ptr(), G, 1, 0) == FH_ERR_STATE
    bad = dev(np.array([1, -2, 3], np.int32))                    # a negative id in a DEVICE list
    assert L.fh_gallery_enroll_ids(g._h, rd.data_ptr(), bad.data_ptr(), 3, 1) == -1 and "negative id" in _lib.last_error()
    assert L.fh_gallery_upload_ids(g._h, rd.data_ptr(), bad.data_ptr(), 3, 1, 0) == -1
    assert len(g) == G and np.array_equal(g.ids(), ids)
    assert_same(topk_ids(g, qd, 4), before, "labelled gallery after refused calls")
    assert_same(before, model.topk_ids(q, rows, ids, 4, 3), "labelled gallery")

    u = fa.Gallery(dim)
    u.upload(rd.data_ptr(), G, True, 3)
    before_u = topk_rows(u, qd, 4)
    assert L.fh_gallery_enroll_ids(u._h, rows.ctypes.data, ids.ctypes.data, 5, 0) == FH_ERR_STATE and "unlabelled" in _lib.last_error()
    assert L.fh_gallery_topk_ids_dev(u._h, qd.data_ptr(), 9, 4, out_s.data_ptr(), out_i.data_ptr(), None, None) == FH_ERR_STATE
    assert L.fh_gallery_topk_ids_dev(u._h, qd.data_ptr(), 9, 1, out_s.data_ptr(), out_i.data_ptr(), None, None) == FH_ERR_STATE
    assert L.fh_gallery_label_ids_dev(u._h, qd.data_ptr(), 9, 0.5, out_i.data_ptr(), out_s.data_ptr(), None) == FH_ERR_STATE
    assert L.fh_gallery_remove_ids(u._h, ids.ctypes.data, 3) == FH_ERR_STATE
    assert L.fh_gallery_get_ids(u._h, 0, 1, ids[:1].copy().ctypes.data) == FH_ERR_STATE
    torch.cuda.synchronize()
    assert len(u) == G
    assert_same_rows(topk_rows(u, qd, 4), before_u, "unlabelled gallery after refused calls")
    assert_same_rows(before_u, oracle.gallery_topk_mfma(q, rows, 4, base=3), "unlabelled gallery")
    # upload decides afresh: ids make an unlabelled gallery labelled; plain enrol as today on the unlabelled one
    assert u.enroll(rows[:2]) == 3 + G
    u.upload(rd.data_ptr(), G, True, 3, ids_ptr=idd.data_ptr())
    assert_same(topk_ids(u, qd, 4), before, "upload_ids over an unlabelled gallery")
    # an empty gallery takes either kind
    e = fa.Gallery(dim)
    s, d, r = topk_ids(e, qd, 4)
    assert (s == -1.0).all() and (d == -1).all() and (r == -1).all() and e.remove_ids([1, 2]) == 0
    assert e.enroll(rows[:10], ids=ids[:10]) == 0 and np.array_equal(e.ids(), ids[:10])


# ------------------------------------------------------------------------------------------ graph capture
@pytest.mark.timeout(300)
def test_topk_ids_replays_from_a_captured_graph():
    rng = np.random.default_rng(81)
    dim, Q, k = 512, 65, 16
    rows, ids, centres = clustered(rng, G_SEED, dim, 8)
    q = queries_near(rng, centres, Q)
    g = labelled(rows, ids, 7)
    qd = dev(q)
    eager = topk_ids(g, qd, k)
    assert_same(eager, model.topk_ids(q, rows, ids, k, 7), "eager")
    sc = torch.zeros((Q, k), device="cuda"); di = torch.zeros((Q, k), dtype=torch.int32, device="cuda"); ri = torch.zeros_like(di)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.topk_ids_dev(qd.data_ptr(), Q, k, sc.data_ptr(), di.data_ptr(), ri.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    for _ in range(2):
        sc.fill_(3.0); di.fill_(-3); ri.fill_(-3)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_same((sc.cpu().numpy(), di.cpu().numpy(), ri.cpu().numpy()), eager, "replay")
