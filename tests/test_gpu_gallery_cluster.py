"""Exact DBSCAN over a gallery's rows on the GPU (fh_gallery_cluster_dev, gallery_cluster.hip).  Expected = the numpy rule of
tests/cluster_model.py on gallery_ids_model.scores(rows, rows) — the oracle.dot_mfma bits the fp32 scan reports; got = cluster_dev into
buffers prefilled with a sentinel.  Labels and the four counters must be IDENTICAL: there is no tolerance.  Shapes: dim 64 (the odd-chunk
tail), 128, 192 (even + tail), 256 (two loop rounds, the second without refetch or tail) and 512 (eight chunks: the production depth);
G around the 64-row B tile and the 128-row A tile, the diagonal inside a tile, several tiles each way;
runs of three and more A tiles per workgroup through the debug hook.  Then fh_gallery_set_ids and the cluster -> set_ids -> fuse flow."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import cluster_model as cm         # noqa: E402
from tests import gallery_ids_model as model  # noqa: E402

FH_ERR_ARG, FH_ERR_STATE = -1, -4
SENT = -7
PAD = 5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unit(x):
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), np.float32)


def gallery(rows, ids=None, base=0, scan="fp32"):
    g = fa.Gallery(rows.shape[1], scan=scan)
    if len(rows):
        rd, idd = dev(rows), None if ids is None else dev(np.asarray(ids, np.int32))      # (both alive until the synchronous upload returns)
        g.upload(rd.data_ptr(), rows.shape[0], True, base, ids_ptr=None if idd is None else idd.data_ptr())
    return g


def run(g, thr, min_pts, noise, want_info=True):
    """cluster_dev into sentinel-filled buffers; the pad behind the labels and around the counters must come back untouched."""
    n = len(g)
    labels = torch.full((n + PAD,), SENT, dtype=torch.int32, device="cuda")
    info = torch.full((4 + PAD,), SENT, dtype=torch.int32, device="cuda")
    g.cluster_dev(thr, min_pts, noise, labels.data_ptr(), info.data_ptr() if want_info else None, 0)
    torch.cuda.synchronize()
    labels, info = labels.cpu().numpy(), info.cpu().numpy()
    assert (labels[n:] == SENT).all() and (info[4:] == SENT).all()
    return labels[:n], info[:4]


def check(g, S, thr, min_pts, noise, what):
    want_l, want_i = cm.cluster(S, thr, min_pts, noise)
    got_l, got_i = run(g, thr, min_pts, noise)
    bad = np.flatnonzero(got_l != want_l)
    print(f"{what}: G {len(S)} thr {float(thr):.9g} min_pts {min_pts} noise {noise}: info got {got_i.tolist()} want {want_i.tolist()}, "
          f"{len(bad)} labels differ")
    assert len(bad) == 0, (what, min_pts, noise, bad[:8], got_l[bad[:8]], want_l[bad[:8]])
    assert np.array_equal(got_i, want_i), (what, min_pts, noise, got_i, want_i)
    return want_l, want_i


def mixed_rows(rng, G, dim):
    """Loose groups around ~G/5 centres plus a few lone rows: scores spread widely, so that a quantile threshold gives clusters, border
    rows and noise at once."""
    c = unit(rng.standard_normal((max(G // 5, 1), dim), dtype=np.float32))
    x = c[rng.integers(0, len(c), G)] + np.float32(0.9 / np.sqrt(dim)) * rng.standard_normal((G, dim), dtype=np.float32)
    return unit(x)


def sparse_threshold(S, per_row=3.0):
    """A threshold that leaves about per_row edges per row (an input choice: the comparison itself is exact)."""
    n = len(S)
    up = S[np.triu_indices(n, 1)]
    if len(up) == 0:
        return np.float32(0.5)
    keep = min(len(up) - 1, int(per_row * n / 2))
    return np.float32(np.sort(up)[::-1][keep])


SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300, 1100)
DEEP_SIZES = (65, 129, 300)         # dims 256 and 512: one partial B tile, a diagonal inside an A tile, several tiles each way


def sizes_for(dim):
    return SIZES if dim < 256 else DEEP_SIZES
_CASES = {}


def case(dim, G):
    """rows, their score matrix and a sparse threshold — computed once and shared, never modified"""
    if (dim, G) not in _CASES:
        rng = np.random.default_rng(1000 * dim + G)
        rows = mixed_rows(rng, G, dim)
        S = model.scores(rows, rows)
        assert np.array_equal(S.view(np.uint32), S.T.view(np.uint32))      # the chain is symmetric to the bit
        S.setflags(write=False)
        _CASES[(dim, G)] = (rows, S, sparse_threshold(S))
    return _CASES[(dim, G)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dim", [64, 128, 192, 256, 512])
def test_sizes_around_the_tiles(dim):
    seen = np.zeros(4, np.int64)
    for G in sizes_for(dim):
        rows, S, thr = case(dim, G)
        g = gallery(rows)
        for min_pts, noise in ((1, "none"), (3, "self"), (4, "none")):
            _, info = check(g, S, thr, min_pts, noise, f"dim {dim}")
            seen += info if min_pts > 1 else 0
    assert (seen > 0).all(), seen                              # clusters, core, border and noise rows all occurred


@pytest.mark.timeout(300)
@pytest.mark.parametrize("tiles", [3, 4, 9])
def test_runs_of_several_tiles_per_workgroup(tiles):
    rows, S, thr = case(128, 1100)                             # 9 A tiles: runs of 3 + 3 + 3, 4 + 4 + 1, 9
    g = gallery(rows)
    try:
        assert _lib.lib().fh_debug_cluster_tiles(tiles) == 0
        for min_pts, noise in ((1, "self"), (3, "none")):
            check(g, S, thr, min_pts, noise, f"runs of {tiles}")
    finally:
        _lib.lib().fh_debug_cluster_tiles(0)


@pytest.mark.timeout(300)
def test_planted_clusters():
    rng = np.random.default_rng(7)
    dim, planted, lone = 128, 60, 9
    sizes = rng.integers(4, 13, planted)
    centres = unit(rng.standard_normal((planted, dim), dtype=np.float32))
    x = np.repeat(centres, sizes, axis=0) + np.float32(0.02) * rng.standard_normal((int(sizes.sum()), dim), dtype=np.float32)
    rows = np.concatenate([unit(x), unit(rng.standard_normal((lone, dim), dtype=np.float32))])
    is_lone = np.arange(len(rows)) >= sizes.sum()
    perm = rng.permutation(len(rows))
    rows, is_lone = np.ascontiguousarray(rows[perm]), is_lone[perm]
    S = model.scores(rows, rows)
    g = gallery(rows)
    for min_pts in (1, 2, 4):
        want_l, want_i = check(g, S, np.float32(0.8), min_pts, "none", "planted")
        if min_pts == 1:
            assert want_i[0] == planted + lone
        else:
            assert want_i[0] == planted and (want_l[is_lone] == -1).all() and want_i[3] == lone
    labels, info = g.cluster(0.8, 4, "none")                   # the synchronous convenience
    assert np.array_equal(labels, want_l) and np.array_equal(info, want_i)


@pytest.mark.timeout(300)
def test_a_chain_across_tiles_is_one_cluster_with_the_minimum_position():
    G, dim = 300, 320
    rows = np.zeros((G, dim), np.float32)
    for t in range(G):
        rows[t, t] = rows[t, t + 1] = np.float32(1.0 / np.sqrt(2.0))
    perm = np.random.default_rng(11).permutation(G)
    rows = np.ascontiguousarray(rows[perm])
    S = model.scores(rows, rows)
    want_l, want_i = check(gallery(rows), S, np.float32(0.6), 1, "none", "chain")
    assert (want_l == 0).all() and tuple(want_i) == (1, G, 0, 0)
    want_l, want_i = check(gallery(rows), S, np.float32(0.6), 3, "none", "chain, min_pts 3")      # its two ends are border rows
    assert want_i[0] == 1 and want_i[2] == 2 and len(set(want_l.tolist())) == 1


@pytest.mark.timeout(300)
def test_identical_rows_are_one_cluster_under_maximal_contention():
    G, dim = 300, 128
    rows = np.repeat(unit(np.random.default_rng(13).standard_normal((1, dim), dtype=np.float32)), G, axis=0)
    S = model.scores(rows, rows)
    for min_pts in (1, 4):
        want_l, want_i = check(gallery(rows), S, np.float32(0.8), min_pts, "none", "identical")
        assert (want_l == 0).all() and tuple(want_i) == (1, G, 0, 0)


@pytest.mark.timeout(300)
def test_the_threshold_is_strict_to_the_bit():
    rows, S, _ = case(128, 300)
    up = np.triu(S, 1)
    i, j = np.unravel_index(np.argmax(up), up.shape)
    top = S[i, j]
    assert (up == top).sum() == 1 and i != j                    # one best pair, off the diagonal
    g = gallery(rows)
    _, info = check(g, S, top, 2, "none", "thr = the best pair's score")
    assert tuple(info) == (0, 0, 0, 300)                        # strict: not even that pair
    want_l, info = check(g, S, np.nextafter(top, np.float32(0)), 2, "none", "one ulp below")
    assert tuple(info) == (1, 2, 0, 298) and want_l[i] == want_l[j] == min(i, j)


@pytest.mark.timeout(300)
def test_a_nan_row_links_to_nothing():
    rows, _, _ = case(128, 129)
    rows = rows.copy()
    rows[70, 5] = np.nan
    S = model.scores(rows, rows)
    assert np.isnan(S[70]).all() and np.isnan(S[:, 70]).all()
    thr = sparse_threshold(np.nan_to_num(S, nan=0.0))
    g = gallery(rows)
    for min_pts, noise, want70 in ((1, "none", 70), (2, "none", -1), (3, "self", 70)):
        want_l, _ = check(g, S, thr, min_pts, noise, "NaN row")
        assert want_l[70] == want70
    check(g, S, np.float32(np.nan), 2, "none", "NaN threshold")


@pytest.mark.timeout(300)
def test_ids_scan_mode_and_index_base_play_no_part():
    rows, S, thr = case(128, 300)
    ids = np.random.default_rng(3).integers(0, 50, 300).astype(np.int32)
    for what, g in (("labelled", gallery(rows, ids)), ("f16 re-rank", gallery(rows, scan="f16")), ("index base 1000", gallery(rows, base=1000)),
                    ("labelled, f16, base", gallery(rows, ids, base=1000, scan="f16"))):
        for min_pts, noise in ((1, "none"), (3, "self")):
            check(g, S, thr, min_pts, noise, what)


@pytest.mark.timeout(300)
def test_two_calls_back_to_back_on_one_handle():
    rows, S, thr = case(192, 300)
    g = gallery(rows)
    n = len(g)
    a = torch.full((n,), SENT, dtype=torch.int32, device="cuda"); ai = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    b = torch.full((n,), SENT, dtype=torch.int32, device="cuda"); bi = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    g.cluster_dev(thr, 3, "none", a.data_ptr(), ai.data_ptr(), 0)            # no wait in between: the scratch is re-cleared on the stream
    g.cluster_dev(np.nextafter(thr, np.float32(1)), 1, "self", b.data_ptr(), bi.data_ptr(), 0)
    torch.cuda.synchronize()
    for (l, i), (min_pts, noise, t) in (((a, ai), (3, "none", thr)), ((b, bi), (1, "self", np.nextafter(thr, np.float32(1))))):
        want_l, want_i = cm.cluster(S, t, min_pts, noise)
        assert np.array_equal(l.cpu().numpy(), want_l) and np.array_equal(i.cpu().numpy(), want_i)
    # a smaller row set on the same handle, and without the counters
    rows2, S2, thr2 = case(192, 65)
    rd2 = dev(rows2)
    g.upload(rd2.data_ptr(), 65, True)
    got, info = run(g, thr2, 3, "none", want_info=False)
    assert np.array_equal(got, cm.cluster(S2, thr2, 3, "none")[0]) and (info == SENT).all()


@pytest.mark.timeout(120)
def test_errors_write_nothing_and_an_empty_gallery_writes_zero_counters():
    L = _lib.lib()
    rows, S, thr = case(128, 65)
    g = gallery(rows)
    labels = torch.full((65,), SENT, dtype=torch.int32, device="cuda"); info = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    lp, ip = labels.data_ptr(), info.data_ptr()
    for args in ((None, 0.5, 1, 0, lp, ip), (g._h, 0.5, 0, 0, lp, ip), (g._h, 0.5, -1, 1, lp, ip), (g._h, 0.5, 1, 2, lp, ip),
                 (g._h, 0.5, 1, -1, lp, ip), (g._h, 0.5, 1, 0, None, ip)):
        assert L.fh_gallery_cluster_dev(*args, None) == FH_ERR_ARG, args[1:4]
        assert _lib.last_error()
    with pytest.raises(ValueError):
        g.cluster_dev(0.5, 1, "other", lp, ip)
    torch.cuda.synchronize()
    assert (labels.cpu().numpy() == SENT).all() and (info.cpu().numpy() == SENT).all()
    empty = fa.Gallery(128)
    assert L.fh_gallery_cluster_dev(empty._h, 0.5, 1, 0, lp, ip, None) == 0
    torch.cuda.synchronize()
    assert (labels.cpu().numpy() == SENT).all() and (info.cpu().numpy() == 0).all()
    check(g, S, thr, 3, "none", "after the errors")            # the handle still works


@pytest.mark.timeout(300)
def test_set_ids_and_the_cluster_to_fuse_flow():
    L = _lib.lib()
    rows, S, thr = case(128, 300)
    want_l, want_i = cm.cluster(S, thr, 3, "self")
    g = gallery(rows)                                          # unlabelled
    n = len(g)
    labels = torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    g.cluster_dev(thr, 3, "self", labels.data_ptr(), None, 0)
    torch.cuda.synchronize()
    assert g.set_ids(labels) == n                              # a device list; the gallery becomes labelled
    assert np.array_equal(g.ids(), want_l)
    assert want_i[3] > 0 and want_i[0] > 1
    fused = g.fuse()
    assert len(fused) == want_i[0] + want_i[3] and np.array_equal(fused.ids(), np.unique(want_l))
    scores = torch.full((n,), 7.0, device="cuda")
    g.self_scores_dev(fused, scores.data_ptr(), 0)             # the audit takes the fused gallery
    torch.cuda.synchronize()
    sc = scores.cpu().numpy()
    noise_rows = cm.kinds(S, thr, 3)[2]
    assert ((sc > 0.5) & (sc <= 1.0001)).all() and np.allclose(sc[noise_rows], 1.0, atol=1e-5)     # a lone row is its own template
    # a negative id is refused and changes nothing, from the host and from the device
    bad = want_l.copy(); bad[17] = -1
    assert L.fh_gallery_set_ids(g._h, bad.ctypes.data, 0) == FH_ERR_ARG
    assert L.fh_gallery_set_ids(g._h, dev(bad).data_ptr(), 1) == FH_ERR_ARG
    assert L.fh_gallery_set_ids(g._h, None, 0) == FH_ERR_ARG and L.fh_gallery_set_ids(None, bad.ctypes.data, 0) == FH_ERR_ARG
    assert np.array_equal(g.ids(), want_l) and np.array_equal(g.rows().view(np.uint32), rows.view(np.uint32))
    # a host list; rows and the scan's answers are untouched
    other = (np.arange(n, dtype=np.int32) * 3) % 101
    assert g.set_ids(other) == n and np.array_equal(g.ids(), other)
    check(g, S, thr, 3, "none", "after set_ids")
    # set_ids clears the "fused" mark: the audit refuses such a template, and only such a one
    g.self_scores_dev(fused, scores.data_ptr(), 0)             # src's ids changed; the template is still a fused one
    torch.cuda.synchronize()
    assert fused.set_ids(fused.ids()) == len(fused)
    assert L.fh_gallery_self_scores_dev(g._h, fused._h, scores.data_ptr(), None) == FH_ERR_STATE
    refused = g.fuse()
    g.self_scores_dev(refused, scores.data_ptr(), 0)
    torch.cuda.synchronize()
    # an empty gallery: nothing to replace
    assert fa.Gallery(128).set_ids(np.zeros(0, np.int32)) == 0
