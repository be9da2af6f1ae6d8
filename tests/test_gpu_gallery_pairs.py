"""The pair audit on the GPU (fh_gallery_pairs_dev: the count and collect epilogues of gallery_cluster.hip, the cut and select kernels
of gallery_pairs.hip).  Expected = gallery_ids_model.scores(rows, rows) — the oracle.dot_mfma bits the fp32 scan reports — pushed through
the numpy rule of tests/pairs_model.py; got = pairs_dev into buffers prefilled with a sentinel.  Counts, score bits, positions and ids
must be IDENTICAL: there is no tolerance.  Shapes as for the clustering passes (the rows and score matrices are shared with
tests/test_gpu_gallery_cluster.py); runs of several A tiles through the debug hook; ties and bin edges; the cut through
fh_debug_pairs_room; the call's contract; histogram -> threshold -> the pairs end to end."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa                      # noqa: E402
from facerecognizeonnx_amd import _lib                  # noqa: E402
from tests import gallery_ids_model as model            # noqa: E402
from tests import pairs_model as pm                     # noqa: E402
from tests import test_gpu_gallery_cluster as tc        # noqa: E402   (its helpers and its cache of rows / score matrices)
from tests import test_gpu_gallery_hist as th           # noqa: E402   (the dyadic case, ids_for)

FH_ERR_ARG, FH_ERR_STATE = -1, -4
BINS = 2048
SENT = -7
PAD = 5


def buffers(cap):
    return (torch.full((4 + PAD,), SENT, dtype=torch.int64, device="cuda"), torch.full((cap + PAD,), float(SENT), dtype=torch.float32, device="cuda"),
            torch.full((2 * cap + PAD,), SENT, dtype=torch.int32, device="cuda"), torch.full((2 * cap + PAD,), SENT, dtype=torch.int32, device="cuda"))


def run(g, cls, side, thr, cap, lists=(True, True, True), stream=0, wait=None):
    """pairs_dev into sentinel-filled buffers; the pad behind every output must come back untouched, as must a list that was not passed"""
    info, s, r, d = buffers(cap)
    torch.cuda.synchronize()
    g.pairs_dev(cls, side, thr, cap, info.data_ptr(), s.data_ptr() if lists[0] else None, r.data_ptr() if lists[1] else None,
                d.data_ptr() if lists[2] else None, stream)
    (wait or torch.cuda.synchronize)()
    info, s, r, d = info.cpu().numpy(), s.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
    assert (info[4:] == SENT).all() and (s[cap:] == SENT).all() and (r[2 * cap:] == SENT).all() and (d[2 * cap:] == SENT).all()
    return info[:4].view(np.uint64), s[:cap], r[:2 * cap].reshape(cap, 2), d[:2 * cap].reshape(cap, 2)


def check(g, S, ids, cls, side, thr, cap, what, room=None, lists=(True, True, True), **kw):
    want = pm.pairs(S, ids, cls, side, thr, cap, room)
    got = run(g, cls, side, thr, cap, lists, **kw)
    print(f"{what}: G {len(S)} {cls} {side} thr {float(thr):.9g} cap {cap}: info got {got[0].tolist()} want {want[0].tolist()}")
    assert np.array_equal(got[0], want[0]), (what, cls, side, cap, got[0], want[0])
    for k, name in ((1, "scores"), (2, "rows"), (3, "ids")):
        if lists[k - 1]:
            bad = np.flatnonzero((got[k].view(np.uint32) != want[k].view(np.uint32)).reshape(cap, -1).any(axis=1))
            assert len(bad) == 0, (what, cls, side, cap, name, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
        else:
            assert (got[k] == SENT).all(), (what, name)
    return want


def thresholds(S, ids, cls, side, cap, ordered=None):
    """two thresholds from quantiles of the case's own scores (an input choice: the comparison itself is exact): one with fewer than
    cap selected pairs, one with a few times cap (or all there are).  ordered: every score of the class, most extreme first."""
    s = pm.selected(S, ids, cls, side, -np.inf if side == "above" else np.inf)[0] if ordered is None else ordered
    if len(s) == 0:
        return [np.float32(0.5)]
    few, many = s[min(len(s) - 1, max(cap // 2, 1))], s[min(len(s) - 1, 3 * cap)]
    if side == "not_above":                                      # s <= thr selects the entries up to and including that score
        few = s[min(len(s) - 1, max(cap // 2 - 1, 0))]
    return [np.float32(few), np.float32(many)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dim", [64, 128, 192, 256, 512])
def test_sizes_around_the_tiles(dim):
    regimes = set()
    for G in tc.sizes_for(dim):
        rows, S, _ = tc.case(dim, G)
        ids = th.ids_for(G, 7 * dim + G)
        g = tc.gallery(rows, ids)
        for cls in pm.CLASSES:
            for side in pm.SIDES:
                ordered = pm.selected(S, ids, cls, side, -np.inf if side == "above" else np.inf)[0]
                for cap in (16, 1024):
                    for thr in thresholds(S, ids, cls, side, cap, ordered):
                        info = check(g, S, ids, cls, side, thr, cap, f"dim {dim}")[0]
                        regimes.add((cap, "<" if info[0] < cap else ">=3x" if info[0] >= 3 * cap else "mid"))
    assert {(16, "<"), (16, ">=3x"), (1024, "<"), (1024, ">=3x")} <= regimes, regimes


@pytest.mark.timeout(300)
@pytest.mark.parametrize("tiles", [3, 4, 9])
def test_runs_of_several_tiles_per_workgroup(tiles):
    rows, S, _ = tc.case(128, 1100)                            # 9 A tiles: runs of 3 + 3 + 3, 4 + 4 + 1, 9
    ids = th.ids_for(1100, 99)
    g = tc.gallery(rows, ids)
    try:
        assert _lib.lib().fh_debug_cluster_tiles(tiles) == 0
        for cls, side, cap in (("impostor", "above", 1024), ("genuine", "not_above", 16), ("any", "above", 16)):
            check(g, S, ids, cls, side, thresholds(S, ids, cls, side, cap)[1], cap, f"runs of {tiles}")
    finally:
        _lib.lib().fh_debug_cluster_tiles(0)


_DUP = {}


def duplicates_case():
    """dim 64: 40 identical unit rows — 780 pairs with ONE score — among 60 random rows"""
    if not _DUP:
        rng = np.random.default_rng(23)
        rows = tc.unit(rng.standard_normal((100, 64), dtype=np.float32))
        where = np.sort(rng.choice(100, 40, replace=False))
        rows[where] = rows[where[0]]
        ids = th.ids_for(100, 31)
        S = model.scores(rows, rows)
        S.setflags(write=False)
        _DUP["case"] = (rows, ids, S, where)
    return _DUP["case"]


@pytest.mark.timeout(300)
def test_ties_are_listed_in_pair_order():
    rows, ids, S, where = duplicates_case()
    top = S[where[0], where[1]]
    iu = np.triu_indices(100, 1)
    assert (S[iu] == top).sum() == 780 and (S[iu] > top).sum() == 0
    g = tc.gallery(rows, ids)
    info, s, r, _ = check(g, S, ids, "any", "above", np.float32(0.9), 100, "40 duplicates")
    assert info.tolist() == [780, 0, 100, 1] and (s == top).all()
    first = [(int(where[a]), int(where[b])) for a in range(40) for b in range(a + 1, 40)][:100]
    assert [tuple(x) for x in r] == first                       # the first 100 in (i, j) order
    check(g, S, ids, "any", "above", np.float32(0.9), 1024, "40 duplicates, all of them")
    check(g, S, ids, "any", "not_above", top, 1024, "40 duplicates, from below")


@pytest.mark.timeout(300)
def test_scores_on_the_bin_edges_and_a_nan_row():
    rows, ids = th.dyadic_case()
    S = model.scores(rows, rows)
    g = tc.gallery(rows, ids)
    hist, nan = th.run(g)                                       # pair_hist_dev's own output on the same gallery
    planes = {"genuine": hist[0], "impostor": hist[1], "any": hist[0] + hist[1]}
    nans = {"genuine": int(nan[0]), "impostor": int(nan[1]), "any": int(nan.sum())}
    assert nans["genuine"] > 0 and nans["impostor"] > 0
    for cls in pm.CLASSES:
        suffix = np.cumsum(planes[cls][::-1].astype(np.int64))[::-1]
        total = pm.class_total(len(ids), ids, cls)
        for b in (1, 2, 512, 1023, 1024, 1025, 2046, 2047):
            thr = np.float32(b / BINS)
            above = check(g, S, ids, cls, "above", thr, 64, f"edge {b}")[0]
            below = check(g, S, ids, cls, "not_above", thr, 64, f"edge {b}")[0]
            assert int(above[0]) == int(suffix[b]) and int(above[1]) == int(below[1]) == nans[cls], (cls, b)
            assert int(above[0]) + int(below[0]) + nans[cls] == total, (cls, b)


@pytest.mark.timeout(300)
def test_the_cut():
    rows, ids, S, _ = duplicates_case()
    g = tc.gallery(rows, ids)
    L = _lib.lib()
    s_all = pm.selected(S, ids, "any", "above", 0.5)[0]
    b = pm.rm.bins(s_all)
    cap = 900                                                  # beyond the 780 of the top bin: the boundary bin lies further down
    bstar = b[cap - 1]
    need, strict = int((b >= bstar).sum()), int((b > bstar).sum())
    assert strict < cap < need
    try:
        assert L.fh_debug_pairs_room(8) == 0
        info, s, r, d = check(g, S, ids, "any", "above", np.float32(0.9), 8, "room 8", room=8)
        assert info.tolist() == [780, 0, 0, 0] and (s == -1).all() and (r == -1).all() and (d == -1).all()
        assert L.fh_debug_pairs_room(need) == 0
        assert check(g, S, ids, "any", "above", np.float32(0.5), cap, "the boundary bin fits exactly", room=need)[0].tolist()[2:] == [cap, 1]
        assert L.fh_debug_pairs_room(need - 1) == 0
        assert check(g, S, ids, "any", "above", np.float32(0.5), cap, "one short", room=need - 1)[0].tolist()[2:] == [strict, 0]
        assert L.fh_debug_pairs_room(3) == 0                       # below cap: the room in force is max(room, cap)
        check(g, S, ids, "impostor", "not_above", np.float32(0.5), 16, "room below cap", room=16)
    finally:
        L.fh_debug_pairs_room(0)
    check(g, S, ids, "any", "above", np.float32(0.9), 8, "the default room again")


@pytest.mark.timeout(120)
def test_errors_write_nothing_and_an_empty_gallery_writes_empty_lists():
    L = _lib.lib()
    rows, S, _ = tc.case(128, 65)
    ids = th.ids_for(65, 5)
    g, unlabelled, odd = tc.gallery(rows, ids), tc.gallery(rows), fa.Gallery(96)        # (96: not a multiple of 64)
    info, s, r, d = buffers(16)
    ip, sp, rp, dp = info.data_ptr(), s.data_ptr(), r.data_ptr(), d.data_ptr()
    for args in ((None, 0, 0, 0.5, 16, ip), (g._h, 0, 0, 0.5, 16, None), (g._h, 0, 0, float("nan"), 16, ip), (g._h, 3, 0, 0.5, 16, ip),
                 (g._h, -1, 0, 0.5, 16, ip), (g._h, 0, 2, 0.5, 16, ip), (g._h, 0, -1, 0.5, 16, ip), (g._h, 0, 0, 0.5, 0, ip),
                 (g._h, 0, 0, 0.5, _lib.PAIRS_MAX_CAP + 1, ip), (odd._h, 2, 0, 0.5, 16, ip)):
        assert L.fh_gallery_pairs_dev(*args, sp, rp, dp, None) == FH_ERR_ARG, args[1:5]
        assert _lib.last_error()
    for cls, idp in ((0, None), (1, None), (2, dp)):
        assert L.fh_gallery_pairs_dev(unlabelled._h, cls, 0, 0.5, 16, ip, sp, rp, idp, None) == FH_ERR_STATE and _lib.last_error()
    with pytest.raises(ValueError):
        g.pairs_dev("other", "above", 0.5, 16, ip)
    with pytest.raises(_lib.FaceHipError):
        unlabelled.pairs("genuine", "above", 0.5)
    torch.cuda.synchronize()
    for t in (info, s, r, d):
        assert (t.cpu().numpy() == SENT).all()
    # an unlabelled gallery answers class "any" without ids
    want = check(unlabelled, S, None, "any", "above", np.float32(0.55), 16, "unlabelled", lists=(True, True, False))
    d_info, d_s, d_r, d_d = unlabelled.pairs("any", "above", 0.55, 16)       # the synchronous convenience
    m = int(want[0][2])
    assert [d_info[k] for k in ("count", "nan", "returned", "complete")] == want[0].tolist() and d_d is None
    assert np.array_equal(d_s, want[1][:m]) and np.array_equal(d_r, want[2][:m])
    # an empty gallery: zeros with complete = 1, empty lists, either kind of class
    for cls in pm.CLASSES:
        got = run(fa.Gallery(128), cls, "not_above", 0.5, 16)
        assert got[0].tolist() == [0, 0, 0, 1] and (got[1] == -1).all() and (got[2] == -1).all() and (got[3] == -1).all()
    check(g, S, ids, "impostor", "above", np.float32(0.55), 16, "after the errors")      # the handle still works


@pytest.mark.timeout(300)
def test_any_subset_of_the_lists_may_be_null():
    rows, S, _ = tc.case(128, 300)
    ids = th.ids_for(300, 6)
    g = tc.gallery(rows, ids)
    thr = thresholds(S, ids, "impostor", "above", 16)[1]
    for mask in range(8):
        check(g, S, ids, "impostor", "above", thr, 16, f"lists {mask:03b}", lists=(bool(mask & 1), bool(mask & 2), bool(mask & 4)))


@pytest.mark.timeout(300)
def test_two_calls_back_to_back_give_identical_bytes():
    rows, S, _ = tc.case(192, 300)
    ids = th.ids_for(300, 3)
    g = tc.gallery(rows, ids)
    cap = 1024
    thr = thresholds(S, ids, "any", "above", cap)[1]
    a, b = buffers(cap), buffers(cap)
    g.pairs_dev("any", "above", thr, cap, *(t.data_ptr() for t in a))        # no wait in between: the scratch is re-cleared on the stream
    g.pairs_dev("any", "above", thr, cap, *(t.data_ptr() for t in b))
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    want = pm.pairs(S, ids, "any", "above", thr, cap)
    assert np.array_equal(a[0].cpu().numpy()[:4].view(np.uint64), want[0]) and int(want[0][0]) > cap
    assert np.array_equal(a[1].cpu().numpy()[:cap].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(a[2].cpu().numpy()[:2 * cap].reshape(cap, 2), want[2])
    # two different questions back to back
    c, e = buffers(16), buffers(16)
    g.pairs_dev("genuine", "not_above", 0.6, 16, *(t.data_ptr() for t in c))
    g.pairs_dev("impostor", "above", 0.6, 16, *(t.data_ptr() for t in e))
    torch.cuda.synchronize()
    for got, (cls, side) in ((c, ("genuine", "not_above")), (e, ("impostor", "above"))):
        want = pm.pairs(S, ids, cls, side, np.float32(0.6), 16)
        assert np.array_equal(got[0].cpu().numpy()[:4].view(np.uint64), want[0])
        assert np.array_equal(got[2].cpu().numpy()[:32].reshape(16, 2), want[2]) and np.array_equal(got[3].cpu().numpy()[:32].reshape(16, 2), want[3])


@pytest.mark.timeout(300)
def test_index_base_scan_mode_removal_and_stream_play_no_part():
    rows, S, _ = tc.case(128, 300)
    ids = th.ids_for(300, 6)
    thr = thresholds(S, ids, "impostor", "above", 16)[1]
    for what, g in (("base 0", tc.gallery(rows, ids)), ("index base 1000", tc.gallery(rows, ids, base=1000)),
                    ("f16 re-rank", tc.gallery(rows, ids, scan="f16")), ("f16, base", tc.gallery(rows, ids, base=1000, scan="f16"))):
        check(g, S, ids, "impostor", "above", thr, 16, what)
        check(g, S, ids, "genuine", "not_above", np.float32(0.6), 1024, what)
    g = tc.gallery(rows, ids)
    gone = int(np.bincount(ids).argmax())
    keep = np.flatnonzero(ids != gone)
    assert g.remove_ids([gone]) == 300 - len(keep) > 1
    check(g, S[np.ix_(keep, keep)], ids[keep], "impostor", "above", thr, 16, "after remove_ids")
    rows2, S2, _ = tc.case(128, 65)                             # a smaller upload on the same handle
    ids2 = th.ids_for(65, 4)
    rd, idd = tc.dev(rows2), tc.dev(ids2)
    g.upload(rd.data_ptr(), 65, True, 0, ids_ptr=idd.data_ptr())
    check(g, S2, ids2, "any", "above", np.float32(0.55), 1024, "after a smaller upload")
    # a non-default stream of the runtime's own, made and destroyed here, then a synchronise of that stream alone
    L = _lib.lib()
    side = C.c_void_p()
    assert L.hipStreamCreateWithFlags(C.byref(side), 1) == 0 and side.value            # hipStreamNonBlocking
    try:
        check(g, S2, ids2, "genuine", "not_above", np.float32(0.7), 16, "on a side stream", stream=side.value,
              wait=lambda: L.hipStreamSynchronize(side) == 0 or pytest.fail("hipStreamSynchronize"))
    finally:
        assert L.hipStreamDestroy(side) == 0


@pytest.mark.timeout(300)
def test_histogram_to_threshold_to_the_pairs():
    rng = np.random.default_rng(7)
    dim, planted = 128, 40
    sizes = rng.integers(4, 9, planted)
    centres = tc.unit(rng.standard_normal((planted, dim), dtype=np.float32))
    x = np.repeat(centres, sizes, axis=0) + np.float32(0.02) * rng.standard_normal((int(sizes.sum()), dim), dtype=np.float32)
    rows = tc.unit(x)
    centre = np.repeat(np.arange(planted), sizes)
    ids = (centre * 101 + 7).astype(np.int32)
    first = np.flatnonzero(centre == 3)
    ids[first[len(first) // 2:]] = 999983                      # one person enrolled under two ids: centre 3 split in two
    wrong = int(np.flatnonzero(centre == 11)[0])
    ids[wrong] = 17 * 101 + 7                                  # one row of centre 11 filed under centre 17's identity
    perm = rng.permutation(len(rows))
    rows, ids, centre = np.ascontiguousarray(rows[perm]), np.ascontiguousarray(ids[perm]), centre[perm]
    wrong = int(np.flatnonzero(perm == wrong)[0])
    g = tc.gallery(rows, ids)
    n = len(rows)
    i, j = np.triu_indices(n, 1)
    same_centre, same_id = centre[i] == centre[j], ids[i] == ids[j]
    S = model.scores(rows, rows)
    # the zero-false-accept threshold of this gallery sits just above its best impostor pair — a planted one; a little below it lie
    # the planted pairs and nothing else: every pair of two centres scores far lower, every pair of one centre higher
    hist, _ = g.pair_hist()
    op, _ = fa.roc_from_hist(hist, 0.0)
    assert op["bin"] >= 1 and op["false_accepts"] == 0
    thr = np.float32(op["threshold"] - 0.15)
    assert S[i, j][~same_centre].max() < thr < S[i, j][same_centre].min()
    info, s, r, d = g.pairs("impostor", "above", thr, 1024)
    want = {(int(a), int(b)) for a, b in zip(i[same_centre & ~same_id], j[same_centre & ~same_id])}
    assert info["complete"] == 1 and info["count"] == info["returned"] == len(want) > 0
    assert {tuple(x) for x in r.tolist()} == want and (np.diff(s) <= 0).all()
    assert all(centre[a] == centre[b] and ids[a] != ids[b] for a, b in r.tolist()) and np.array_equal(d, ids[r])
    info, s, r, d = g.pairs("genuine", "not_above", thr, 1024)
    want = {(int(a), int(b)) for a, b in zip(i[~same_centre & same_id], j[~same_centre & same_id])}
    assert info["complete"] == 1 and info["count"] == info["returned"] == len(want) > 0
    assert {tuple(x) for x in r.tolist()} == want and all(wrong in x for x in r.tolist()) and (np.diff(s) >= 0).all()
    check(g, S, ids, "impostor", "above", thr, 1024, "planted duplicates")      # and both lists are the model's, to the bit
    check(g, S, ids, "genuine", "not_above", thr, 1024, "planted mislabel")
