"""Template pooling on the GPU (fh_gallery_fuse_ids, gallery_fuse.hip): the fused rows, read back with fh_gallery_get_rows, BIT FOR BIT
against the numpy model of tests/gallery_fuse_model.py in sum mode and within its derived tolerance in unit mode; the chunked order on
skewed identities; zero and NaN sums; errors that change nothing; the fused gallery as an ordinary gallery in both scan modes; get_rows;
and the self scores (fh_gallery_self_scores_dev) against float64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from oracle import oracle                     # noqa: E402
from tests import gallery_fuse_model as fm    # noqa: E402
from tests import gallery_ids_model as model  # noqa: E402

FH_ERR_ARG, FH_ERR_STATE = -1, -4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def labelled(rows, ids, base=0, scan="fp32"):
    g = fa.Gallery(rows.shape[1], scan=scan)
    rd, idd = dev(rows), dev(np.asarray(ids, np.int32))
    g.upload(rd.data_ptr(), rows.shape[0], True, base, ids_ptr=idd.data_ptr())
    return g


def unlabelled(rows, base=0):
    g = fa.Gallery(rows.shape[1])
    g.upload(dev(rows).data_ptr(), rows.shape[0], True, base)
    return g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


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


def self_scores(src, tmpl):
    out = torch.full((max(len(src), 1),), 7.0, device="cuda")
    src.self_scores_dev(tmpl, out.data_ptr(), 0)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:len(src)]


def queries_near(rng, centres, Q, noise=0.05):
    c = centres[rng.integers(0, len(centres), Q)]
    q = c + np.float32(noise) * rng.standard_normal(c.shape, dtype=np.float32)
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), np.float32)


def check_against_model(src_rows, src_ids, g, what, dst=None):
    """Fuses g in both modes (into dst when given) and holds the results to the model of (src_rows, src_ids); returns the unit gallery."""
    sums, uniq, counts = fm.fuse_sums(src_rows, src_ids)
    dim = src_rows.shape[1]
    d = g.fuse(dst, mode="sum")
    assert dst is None or d is dst
    assert len(d) == len(uniq) and np.array_equal(d.ids(), uniq), what
    got = d.rows()
    bad = np.flatnonzero((bits(got) != bits(sums)).any(1))
    assert len(bad) == 0, (what, "sum mode", len(bad), uniq[bad[:5]], counts[bad[:5]])
    d = g.fuse(d, mode="unit")
    assert len(d) == len(uniq) and np.array_equal(d.ids(), uniq), what
    got = d.rows()
    ok = fm.within_unit_tolerance(got, fm.unit64(sums, counts), dim)
    err = np.abs(got.astype(np.float64) - fm.unit64(sums, counts))
    print(f"{what}: unit mode, worst absolute error {np.nanmax(err):.3e}; tolerance {fm.unit_tolerance(dim):.3e} relative per element")
    assert ok.all(), (what, "unit mode", int((~ok).sum()))
    one = counts == 1
    assert same_bits(got[one], sums[one]), (what, "a one-template identity is kept verbatim")
    return d


# ------------------------------------------------------------------------------------------ distinct ids
@pytest.mark.timeout(120)
def test_distinct_ids_fuse_to_the_rows_in_id_order():
    rng = np.random.default_rng(3)
    G, dim = 300, 128
    rows, q = fm.unit_rows(rng, G, dim), fm.unit_rows(rng, 9, dim)
    labels = (rng.permutation(8 * G)[:G] * 3 + 1).astype(np.int32)
    g = labelled(rows, labels, base=40)
    o = np.argsort(labels, kind="stable")
    qd = dev(q)
    for mode in ("unit", "sum"):
        d = g.fuse(mode=mode)
        assert len(d) == G and np.array_equal(d.ids(), labels[o]) and (np.diff(d.ids()) > 0).all()
        assert same_bits(d.rows(), rows[o]), mode                 # verbatim: not re-normalised
        for k in (1, 5):
            s, i, r = topk_ids(d, qd, k)
            ws, wi, wr = topk_ids(g, qd, k)
            assert same_bits(s, ws) and np.array_equal(i, wi), (mode, k)
            assert np.array_equal(labels[o][r], i)                # index base 0: the row index is the position
    assert len(g) == G and np.array_equal(g.ids(), labels) and same_bits(g.rows(), rows)          # the source is untouched


# ------------------------------------------------------------------------------------------ clustered ids vs the model
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dim", [64, 192, 512])
def test_clustered_identities_match_the_model(dim):
    rows, ids, _, _ = fm.clustered_case(dim)
    check_against_model(rows, ids, labelled(rows, ids, base=77), f"clustered dim{dim}")


# ------------------------------------------------------------------------------------------ skew
@pytest.mark.timeout(120)
def test_long_identities_are_summed_in_chunks_of_512():
    """Identities of 512, 513 and 1 300 rows: bit-exact against the CHUNKED model, which test_gallery_fuse_cpu.py shows to differ from the
    plain sequential order on the 1 300-row identity."""
    rows, ids, big = fm.skew_case()
    sums, uniq, _ = fm.fuse_sums(rows, ids)
    plain, _ = fm.plain_sums(rows, ids)
    j = int(np.searchsorted(uniq, big[2]))
    assert not same_bits(sums[j], plain[j])
    d = check_against_model(rows, ids, labelled(rows, ids), "skew")
    assert len(d) == len(uniq)


@pytest.mark.timeout(120)
def test_a_bucket_of_many_chunks_is_added_in_chunk_order():
    """2 700 rows of one id ("unknown"): six partials, more than the loads one wave keeps in flight, added by the second launch."""
    rng = np.random.default_rng(6)
    dim = 64
    rows = fm.unit_rows(rng, 2700 + 40, dim)
    ids = np.concatenate([np.full(2700, 999), rng.integers(0, 12, 40)]).astype(np.int32)
    o = rng.permutation(len(ids))
    rows, ids = np.ascontiguousarray(rows[o]), ids[o]
    sums, uniq, counts = fm.fuse_sums(rows, ids)
    plain, _ = fm.plain_sums(rows, ids)
    assert counts[-1] == 2700 and not same_bits(sums[-1], plain[-1])
    check_against_model(rows, ids, labelled(rows, ids), "many chunks")


# ------------------------------------------------------------------------------------------ the other forms of the kernel
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dim", [320, 1024, 2048, 2112])
def test_row_lengths_of_every_kernel_form(dim):
    """The sum kernel is built for 1, 2, 4 and 8 sixteen-byte columns per lane (dims up to 256, 512, 1024, 2048; 320 leaves 48 lanes idle in its second column); a longer row takes
    several passes of the eight-column form and is normalised from the sums it stored (2112 = 2048 + 64: a second pass of 16 lanes).
    One identity is longer than a chunk, so the partial path runs in every form; the self scores read the same rows."""
    rng = np.random.default_rng(dim)
    per = np.concatenate([[1, 2, 3, 4, 5, 9, 600], rng.integers(1, 12, 30)])
    labels = (rng.permutation(500)[:len(per)] * 3 + 2).astype(np.int32)
    G = int(per.sum())
    rows = fm.unit_rows(rng, G, dim)
    rows += np.repeat(fm.unit_rows(rng, len(per), dim), per, axis=0)          # templates of one identity lean the same way
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    o = rng.permutation(G)
    rows, ids = np.ascontiguousarray(rows[o], np.float32), np.repeat(labels, per)[o]
    src = labelled(rows, ids)
    d = check_against_model(rows, ids, src, f"dim{dim}")
    got = self_scores(src, d)
    trows, tids = d.rows().astype(np.float64), d.ids()
    want = ((rows.astype(np.float64) * trows[np.searchsorted(tids, ids)]).sum(1) + 1.0) / 2.0
    assert (np.abs(got - want) <= (dim + 4) * 2.0 ** -24).all()


# ------------------------------------------------------------------------------------------ edges
@pytest.mark.timeout(120)
def test_a_cancelled_sum_stays_zero_and_a_nan_stays_nan():
    rng = np.random.default_rng(8)
    dim = 128
    rows, ids, centres, _ = fm.clustered_case(dim, G=900)
    x = fm.unit_rows(rng, 2, dim)
    extra = np.stack([x[0], -x[0], x[1], fm.unit_rows(rng, 1, dim)[0]])
    extra[3, 17] = np.nan
    ZERO, NAN = 2 ** 31 - 1, 0                                    # the largest and the smallest id there is
    rows = np.concatenate([rows[:400], extra[:1], rows[400:], extra[1:]])
    ids = np.concatenate([ids[:400], [ZERO], ids[400:], [ZERO, NAN, NAN]]).astype(np.int32)
    g = labelled(rows, ids)
    sums, uniq, counts = fm.fuse_sums(rows, ids)
    assert uniq[0] == NAN and uniq[-1] == ZERO and np.isnan(sums[0, 17]) and not sums[-1].any()
    q = queries_near(rng, centres, 20)
    q[0] = x[1]
    for mode in ("sum", "unit"):
        d = g.fuse(mode=mode)
        got = d.rows()
        assert np.array_equal(d.ids(), uniq)
        assert same_bits(got[-1], np.zeros(dim, np.float32)), mode          # (x, -x): a zero row, not NaN from 0 / 0
        assert np.isnan(got[0, 17]), mode
        keep = np.arange(dim) != 17
        assert same_bits(got[0, keep], sums[0, keep]), mode       # unit mode too: a NaN norm is not > 0, the row is left as it is
        if mode == "sum":
            assert same_bits(got[1:], sums[1:])                   # the others exact
        else:
            ok = fm.within_unit_tolerance(got[1:], fm.unit64(sums, counts)[1:], dim)
            assert ok.all()
        s, i = topk_rows(d, dev(q), 16)
        assert (i != 0).all() and (i >= 0).all() and not np.isnan(s).any(), mode      # the NaN row is never listed
        ws, wi = oracle.gallery_topk_mfma(q, got, 16)
        assert same_bits(s, ws) and np.array_equal(i, wi), mode


@pytest.mark.timeout(120)
def test_errors_change_nothing_and_dst_may_have_held_anything():
    rng = np.random.default_rng(9)
    dim = 64
    rows, ids, _, _ = fm.clustered_case(dim, G=700)
    src = labelled(rows, ids)
    sums, uniq, _ = fm.fuse_sums(rows, ids)
    L = fa.lib()
    other_rows = fm.unit_rows(rng, 2000, dim)
    other_ids = rng.integers(0, 50, 2000).astype(np.int32)
    # dst held more rows and labels / fewer rows / unlabelled rows / nothing
    for name, dst in (("larger labelled", labelled(other_rows, other_ids, base=5)), ("smaller labelled", labelled(other_rows[:7], other_ids[:7])),
                      ("unlabelled", unlabelled(other_rows[:300], base=9)), ("fresh", fa.Gallery(dim))):
        assert src.fuse(dst, mode="sum") is dst
        assert len(dst) == len(uniq) and np.array_equal(dst.ids(), uniq) and same_bits(dst.rows(), sums), name
        s, i = topk_rows(dst, dev(other_rows[:3]), 4)
        ws, wi = oracle.gallery_topk_mfma(other_rows[:3], sums, 4)           # index base 0, whatever dst's was
        assert same_bits(s, ws) and np.array_equal(i, wi), name
    # refused calls leave dst as it is
    dst = labelled(other_rows, other_ids, base=5)
    before = (dst.ids().copy(), dst.rows().copy())

    def unchanged():
        return len(dst) == 2000 and np.array_equal(dst.ids(), before[0]) and same_bits(dst.rows(), before[1])

    u = unlabelled(other_rows[:10])
    assert L.fh_gallery_fuse_ids(u._h, dst._h, 0) == FH_ERR_STATE and "labelled" in _lib.last_error() and unchanged()
    wide = labelled(fm.unit_rows(rng, 4, 128), [1, 2, 1, 2])
    assert L.fh_gallery_fuse_ids(wide._h, dst._h, 0) == FH_ERR_ARG and unchanged()
    assert L.fh_gallery_fuse_ids(dst._h, dst._h, 0) == FH_ERR_ARG and unchanged()
    assert L.fh_gallery_fuse_ids(src._h, dst._h, 7) == FH_ERR_ARG and unchanged()
    s, i = topk_rows(dst, dev(other_rows[:3]), 4)
    ws, wi = oracle.gallery_topk_mfma(other_rows[:3], other_rows, 4, base=5)
    assert same_bits(s, ws) and np.array_equal(i, wi)
    # an empty source empties a full dst
    empty = fa.Gallery(dim)
    assert L.fh_gallery_fuse_ids(empty._h, dst._h, 0) == 0 and len(dst) == 0 and dst.ids().shape == (0,) and dst.rows().shape == (0, dim)
    s, i = topk_rows(dst, dev(other_rows[:3]), 4)
    assert (s == -1.0).all() and (i == -1).all()
    src.remove_ids(np.unique(ids))                                # emptied by removal: the same
    assert len(src) == 0 and len(src.fuse(dst)) == 0
    assert dst.enroll(other_rows[:5]) == 0 and len(dst) == 5      # and an emptied gallery takes either kind


# ------------------------------------------------------------------------------------------ dst is an ordinary gallery
def check_queries(d, q, what):
    """Row and identity top-k of a fused gallery against the models fed its read-back rows, bit for bit."""
    rows, ids = d.rows(), d.ids()
    for Q in (3, 64, 70):
        qd = dev(q[:Q])
        for k in (1, 5, 16):
            s, i = topk_rows(d, qd, k)
            ws, wi = oracle.gallery_topk_mfma(q[:Q], rows, k)
            assert same_bits(s, ws) and np.array_equal(i, wi), (what, "rows", Q, k)
            got = topk_ids(d, qd, k)
            want = model.topk_ids(q[:Q], rows, ids, k)
            for a, b, name in zip(got, want, ("scores", "ids", "rows")):
                assert same_bits(a, b), (what, name, Q, k)
            assert same_bits(got[0], s) and np.array_equal(got[2], i)        # one row per identity: the identity list IS the row list


@pytest.mark.timeout(300)
def test_the_fused_gallery_answers_as_any_gallery_in_both_scan_modes():
    rng = np.random.default_rng(10)
    dim = 128
    rows, ids, centres, labels = fm.clustered_case(dim, G=3000)
    q = queries_near(rng, centres, 70)
    src = labelled(rows, ids, base=123)
    d32 = fa.Gallery(dim)
    d16 = fa.Gallery(dim, scan="f16")                             # F16_RERANK set BEFORE fusing
    d16.scan_stats()
    for d in (d32, d16):
        check_against_model(rows, ids, src, f"scan {d.scan}", dst=d)
    assert d16.scan == "f16" and same_bits(d16.rows(), d32.rows())
    check_queries(d32, q, "fp32")
    check_queries(d16, q, "f16")
    certified, fallback = d16.scan_stats()
    print(f"F16_RERANK on the fused gallery: certified {certified}, fall-back {fallback}")
    assert certified > 0
    # enrol into src, remove from src, fuse again: the model of the new contents
    more = centres[:50] + np.float32(0.05) * rng.standard_normal((50, dim), dtype=np.float32)
    more = np.ascontiguousarray(more / np.linalg.norm(more, axis=1, keepdims=True), np.float32)
    more_ids = np.concatenate([labels[:40], np.arange(10, dtype=np.int32) + 10 ** 8]).astype(np.int32)
    src.enroll(more, ids=more_ids)
    gone = labels[100:130]
    src.remove_ids(gone)
    rows2, ids2 = np.concatenate([rows, more]), np.concatenate([ids, more_ids])
    keep = ~np.isin(ids2, gone)
    rows2, ids2 = np.ascontiguousarray(rows2[keep]), ids2[keep]
    assert same_bits(src.rows(), rows2) and np.array_equal(src.ids(), ids2)
    for d in (d32, d16):
        check_against_model(rows2, ids2, src, f"re-fused, scan {d.scan}", dst=d)
        assert not np.isin(d.ids(), gone).any() and np.isin(more_ids, d.ids()).all()
    check_queries(d16, q[:64], "f16 re-fused")


# ------------------------------------------------------------------------------------------ get_rows
@pytest.mark.timeout(120)
def test_get_rows_round_trip_sub_ranges_and_range_errors():
    rng = np.random.default_rng(11)
    dim, G = 192, 1000
    rows = fm.unit_rows(rng, G, dim)
    rows[5, 3], rows[6, 0] = np.nan, -0.0
    ids = rng.integers(0, 99, G).astype(np.int32)
    L = fa.lib()
    for g in (labelled(rows, ids, base=1000), unlabelled(rows, base=1000)):
        assert same_bits(g.rows(), rows)
        assert same_bits(g.rows(0, 1), rows[:1]) and same_bits(g.rows(G - 1), rows[G - 1:]) and same_bits(g.rows(17, 301), rows[17:318])
        assert g.rows(G, 0).shape == (0, dim) and g.rows(3, 0).shape == (0, dim)
        out = np.full((4, dim), 5.0, np.float32)
        for first, n in ((0, G + 1), (G, 1), (G - 3, 4), (-1, 2), (0, -1), (G + 1, 0)):
            assert L.fh_gallery_get_rows(g._h, first, n, out.ctypes.data) == FH_ERR_ARG, (first, n)
        assert L.fh_gallery_get_rows(g._h, 0, 2, None) == FH_ERR_ARG
        assert (out == 5.0).all()
        assert L.fh_gallery_get_rows(g._h, G - 4, 4, out.ctypes.data) == 4 and same_bits(out, rows[G - 4:])
    g = unlabelled(rows[:10])
    g.enroll(rows[10:25])                                         # across a capacity doubling
    assert same_bits(g.rows(), rows[:25])


# ------------------------------------------------------------------------------------------ self scores
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dim", [64, 512])
def test_self_scores_match_float64_and_find_a_planted_template(dim):
    rng = np.random.default_rng(12 + dim)
    rows, ids, centres, labels = fm.clustered_case(dim, G=2000)
    # a 10-template identity, one of whose templates is another person's face
    person = fm.unit_rows(rng, 2, dim)
    ten = person[0][None] + np.float32(0.05) * rng.standard_normal((10, dim), dtype=np.float32)
    ten[6] = person[1] + np.float32(0.05) * rng.standard_normal(dim, dtype=np.float32)
    ten = np.ascontiguousarray(ten / np.linalg.norm(ten, axis=1, keepdims=True), np.float32)
    PID = 10 ** 9
    at = np.sort(rng.choice(len(ids), 10, replace=False))
    rows, ids = np.insert(rows, at, ten, axis=0), np.insert(ids, at, PID).astype(np.int32)
    rows = np.ascontiguousarray(rows, np.float32)
    src = labelled(rows, ids, base=31)
    tmpl = src.fuse()
    trows, tids = tmpl.rows(), tmpl.ids()
    tol = (dim + 4) * 2.0 ** -24          # any-order fp32 dot product of rows of norm <= 1, plus the roundings of + 1 and / 2

    def want(trows, tids):
        pos = np.searchsorted(tids, ids)
        pos_ok = np.minimum(pos, len(tids) - 1)
        have = tids[pos_ok] == ids
        w = ((rows.astype(np.float64) * trows[pos_ok].astype(np.float64)).sum(1) + 1.0) / 2.0
        return np.where(have, w, -1.0), have

    got = self_scores(src, tmpl)
    w, have = want(trows, tids)
    assert have.all()
    print(f"self scores dim{dim}: worst |err| {np.abs(got - w).max():.3e}, tolerance {tol:.3e}")
    assert (np.abs(got - w) <= tol).all()
    mine = np.flatnonzero(ids == PID)
    planted = mine[6]
    others = np.delete(mine, 6)
    assert got[planted] < got[others].min() and np.argmin(got[mine]) == 6
    assert got[others].min() - got[planted] > got[others].max() - got[others].min()          # by a wide margin, not by rounding
    # ids removed from tmpl score -1; the others as before
    gone = np.concatenate([labels[:25], [PID]]).astype(np.int32)
    assert tmpl.remove_ids(gone) == 26
    got2 = self_scores(src, tmpl)
    lost = np.isin(ids, gone)
    assert lost.sum() > 26 and (got2[lost] == -1.0).all() and same_bits(got2[~lost], got[~lost])
    w2, have2 = want(tmpl.rows(), tmpl.ids())
    assert np.array_equal(~have2, lost) and (np.abs(got2 - w2) <= tol).all()
    # the pooled gallery against itself: every row is its own identity's row
    own = self_scores(tmpl, tmpl)
    # (|row|^2 + 1) / 2 of rows normalised in fp32: |row|^2 is within twice the unit-mode tolerance of 1, the mapping halves that
    assert (np.abs(own - 1.0) <= tol + fm.unit_tolerance(dim)).all()
    # a template gallery that was enrolled into is no longer one; nor is one that was uploaded, nor an unlabelled source
    L = fa.lib()
    out = torch.zeros(len(ids), device="cuda")
    tmpl.enroll(rows[:1], ids=[5])
    assert L.fh_gallery_self_scores_dev(src._h, tmpl._h, out.data_ptr(), None) == FH_ERR_STATE and "fh_gallery_fuse_ids" in _lib.last_error()
    assert L.fh_gallery_self_scores_dev(src._h, src._h, out.data_ptr(), None) == FH_ERR_STATE
    t2 = src.fuse()
    assert L.fh_gallery_self_scores_dev(unlabelled(rows[:10])._h, t2._h, out.data_ptr(), None) == FH_ERR_STATE
    assert L.fh_gallery_self_scores_dev(src._h, t2._h, out.data_ptr(), None) == 0
    idd = dev(t2.ids()); rd = dev(t2.rows())
    t2.upload(rd.data_ptr(), len(idd), True, 0, ids_ptr=idd.data_ptr())
    assert L.fh_gallery_self_scores_dev(src._h, t2._h, out.data_ptr(), None) == FH_ERR_STATE
    torch.cuda.synchronize()
