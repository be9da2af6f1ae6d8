"""The 1:N gallery held to an exact model: both scan modes (fp32, F16_RERANK) against `oracle.gallery_topk_mfma` — the k-ordered f32
fma chain of v_mfma_f32_32x32x2_f32 that gallery_topk_kernel and gal16_rescore_kernel compute, mapped (acc + 1) / 2 and ranked
(score desc, index asc) — BIT FOR BIT (score bits and indices), across dims with and without an odd chunk tail, row counts around
tile / part / seed-pass edges, operand scales down to fp16 / f32 subnormals, adversarial row orders, the certificate's fall-back,
non-finite values and the INT_MAX index edge; and the top-k merge (cached / uncached, packed and strided layouts) against a numpy
lexsort merge.  As an independent check every returned score also stays within 2 (gamma_d |q||g| / 2 + 2u) of an fp64 evaluation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from oracle import oracle                     # noqa: E402

INT_MAX = 2 ** 31 - 1
U = 2.0 ** -24
QM, KM = 256, 16                              # the model is computed once per (gallery, query set) at this size; smaller Q / k are prefixes
DIMS = [64, 128, 192, 256, 320, 384, 576, 640, 1024, 2048]
G_SEED = 70001                                # >= 65536 (seed pass); last 128-row tile holds 113 rows


def unit(rng, n, dim, lo=1.0, hi=1.0):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    if hi != lo:
        x *= rng.uniform(lo, hi, (n, 1)).astype(np.float32)
    return x


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def galleries(rows, base=0):
    """The same rows in an fp32-scan gallery and an F16_RERANK gallery."""
    rd = dev(rows)
    g32, g16 = fa.Gallery(rows.shape[1]), fa.Gallery(rows.shape[1], scan="f16")
    for g in (g32, g16):
        g.upload(rd.data_ptr(), rows.shape[0], True, base)
    g16.scan_stats()
    return g32, g16


def topk(g, qd, k):
    Q = qd.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda"); ix = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    g.topk_dev(qd.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ix.cpu().numpy()


def assert_bits(got, want, what):
    (s, i), (ms, mi) = got, want
    assert np.array_equal(i, mi), (what, np.argwhere(i != mi)[:8], i[i != mi][:8], mi[i != mi][:8])
    assert np.array_equal(s.view(np.uint32), ms.view(np.uint32)), (what, np.argwhere(s.view(np.uint32) != ms.view(np.uint32))[:8])


def assert_fp64_bound(q, rows, s, i, base):
    """|score - (dot64 + 1) / 2| <= 2 (gamma_d |q||g| / 2 + 2u max(1, |score|)) for every finite listed score."""
    dim = q.shape[1]
    gamma = dim * U / (1 - dim * U)
    qq, rr = np.nonzero(i >= 0)
    g = rows[i[qq, rr] - base].astype(np.float64)
    qv = q[qq].astype(np.float64)
    ok = np.isfinite(s[qq, rr]) & np.isfinite(g).all(1) & np.isfinite(qv).all(1)
    d = np.einsum("ij,ij->i", qv[ok], g[ok])
    ref = (d + 1.0) / 2.0
    bound = 2 * (0.5 * gamma * np.linalg.norm(qv[ok], axis=1) * np.linalg.norm(g[ok], axis=1) + 2 * U * np.maximum(1.0, np.abs(ref)))
    err = np.abs(s[qq, rr][ok].astype(np.float64) - ref)
    assert (err <= bound).all(), (err - bound).max()


def check_both(g32, g16, q, qd, model, cases, rows=None, base=0, f16_route=None, tag=""):
    """Both modes = the model (prefix [:Q, :k]) bit for bit, F16_RERANK = fp32; the certified / fall-back split of every F16 call is
    returned (and must add up to Q).  f16_route=False: the whole batch must take the fp32 route."""
    ms, mi = model
    stats = []
    for Q, k in cases:
        want = (np.ascontiguousarray(ms[:Q, :k]), np.ascontiguousarray(mi[:Q, :k]))
        r32 = topk(g32, qd[:Q], k)
        assert_bits(r32, want, f"{tag} fp32 Q={Q} k={k}")
        r16 = topk(g16, qd[:Q], k)
        assert_bits(r16, want, f"{tag} f16 Q={Q} k={k}")
        assert_bits(r16, r32, f"{tag} f16 vs fp32 Q={Q} k={k}")
        c, f = g16.scan_stats()
        assert c + f == Q, (c, f, Q)
        if f16_route is False:
            assert c == 0 and f == Q, (c, f)
        stats.append((Q, k, c, f))
        if rows is not None and Q == cases[-1][0] and k == cases[-1][1]:
            assert_fp64_bound(q[:Q], rows, *r32, base)
    print(f"[f16 stats] {tag}: " + " ".join(f"Q{Q}k{k}:c{c}/f{f}" for Q, k, c, f in stats))
    return stats


# ------------------------------------------------------------------------------------------ dims x shapes
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dim", DIMS)
def test_both_scans_are_the_model_bit_for_bit_across_dims(dim):
    """Odd 64-deep chunk counts (64, 192, 320, 576) run gallery_topk_kernel's tail; odd 128-deep counts (128, 384, 640) the f16 scan's;
    dims % 128 != 0 send F16_RERANK to the fp32 route for the whole batch."""
    rng = np.random.default_rng(100 + dim)
    rows, q = unit(rng, G_SEED, dim), unit(rng, QM, dim)
    model = oracle.gallery_topk_mfma(q, rows, KM)
    g32, g16 = galleries(rows)
    qd = dev(q)
    cases = [(Q, k) for Q in (1, 65) for k in (1, 16)] + [(129, k) for k in range(1, 17)] + [(256, 1), (256, 16)]
    check_both(g32, g16, q, qd, model, cases, rows=rows, f16_route=False if dim % 128 else None, tag=f"dim{dim}")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dim", [576, 128])
def test_row_count_edges(dim):
    rng = np.random.default_rng(200 + dim)
    q = unit(rng, 65, dim)
    qd = dev(q)
    for G in (1, 15, 16, 17, 127, 128, 129, 4097, 65535, 65536):
        rows = unit(rng, G, dim)
        model = oracle.gallery_topk_mfma(q, rows, 16, base=3)
        g32, g16 = galleries(rows, base=3)
        check_both(g32, g16, q, qd, model, [(1, 16), (64, 16), (65, 16)], rows=rows, base=3,
                   f16_route=False if dim % 128 else None, tag=f"dim{dim} G{G}")
        if G < 16:
            assert (model[1][:, G:] == -1).all() and (model[0][:, G:] == -1.0).all()


@pytest.mark.timeout(300)
def test_large_gallery_odd_chunk_count_many_parts():
    rng = np.random.default_rng(300)
    G, dim = (1 << 20) + 4097, 192
    rows, q = unit(rng, G, dim), unit(rng, 64, dim)
    for r in (7, (1 << 20) - 1, 1 << 20, G - 1):                 # exact copies of q[0] on both sides of the 2^20 boundary
        rows[r] = q[0]
    model = oracle.gallery_topk_mfma(q, rows, 16)
    assert list(model[1][0, :4]) == [7, (1 << 20) - 1, 1 << 20, G - 1]
    g32, g16 = galleries(rows)
    check_both(g32, g16, q, dev(q), model, [(64, 16), (64, 1)], rows=rows, f16_route=False, tag="2^20+4097 dim192")


# ------------------------------------------------------------------------------------------ operand scales
SCALES = {                                     # (row scale, query scale): both also carry random norms in [0.5, 2)
    "q2^-14": (1.0, 2.0 ** -14),               # query entries subnormal in fp16, scores still resolve above the ulp of 0.5
    "q2^-18": (1.0, 2.0 ** -18),
    "g2^-14": (2.0 ** -14, 1.0),
    "g2^-18": (2.0 ** -18, 1.0),
    "both2^-62": (2.0 ** -62, 2.0 ** -62),     # f32-subnormal products: every mapped score is 0.5, the answer is index order
    "both2^8": (2.0 ** 8, 2.0 ** 8),
    "g65504": (1.0, 1.0),                      # entries of exactly 65504: in fp16 range, certified path
    "g65504.01": (1.0, 1.0),                   # just beyond: the batch takes the fp32 route
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", list(SCALES))
@pytest.mark.parametrize("dim", [512, 384])
def test_operand_scales(dim, case):
    rng = np.random.default_rng(400 + dim + 7 * list(SCALES).index(case))
    G = 20000
    gs, qs = SCALES[case]
    rows = unit(rng, G, dim, 0.5, 2.0) * np.float32(gs)
    q = unit(rng, QM, dim, 0.5, 2.0) * np.float32(qs)
    if case.startswith("g65504"):
        big = rng.choice(G, 200, replace=False)
        rows[big, rng.integers(0, dim, 200)] = np.float32(65504.0 if case == "g65504" else 65504.01) * rng.choice([-1, 1], 200)
    model = oracle.gallery_topk_mfma(q, rows, KM)
    if case == "both2^-62":
        assert (model[0] == 0.5).all() and (model[1] == np.arange(KM)).all()
    g32, g16 = galleries(rows)
    check_both(g32, g16, q, dev(q), model, [(1, 1), (65, 16), (256, 1), (256, 16)], rows=rows,
               f16_route=False if case == "g65504.01" else None, tag=f"dim{dim} {case}")


# ------------------------------------------------------------------------------------------ adversarial orders
@pytest.mark.timeout(300)
@pytest.mark.parametrize("order", ["ascending", "tile_edge_copies", "one_row"])
def test_adversarial_row_orders(order):
    rng = np.random.default_rng(500)
    dim, base = 512, 0
    q = unit(rng, 65, dim)
    if order == "ascending":                   # every row beats query 0's running threshold: the queue overflows on every tile
        rows = unit(rng, G_SEED, dim)
        rows = rows[np.argsort(oracle.dot_mfma(q[0], rows), kind="stable")]
    elif order == "tile_edge_copies":          # q[0] on both sides of every 128-row boundary (part boundaries whatever the CU count)
        rows = unit(rng, G_SEED, dim)
        for t in range(128, G_SEED, 128):
            rows[t - 1] = rows[t] = q[0]
    else:
        rows = np.repeat(unit(rng, 1, dim), 5000, axis=0)
        base = 1000
    model = oracle.gallery_topk_mfma(q, rows, 16, base=base)
    if order == "tile_edge_copies":
        assert list(model[1][0, :4]) == [127, 128, 255, 256]
    if order == "one_row":
        assert (model[1] == np.arange(1000, 1016)).all()
    g32, g16 = galleries(rows, base)
    check_both(g32, g16, q, dev(q), model, [(65, 1), (65, 16), (1, 16)], rows=rows, base=base, tag=order)


# ------------------------------------------------------------------------------------------ the certificate's fall-back at tile edges
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 256])
def test_fallback_compaction_at_tile_edges(n):
    """n queries get a cluster of 48 rows within ~2e-7 of them: none of them can be certified, the compacted fall-back batch of n
    queries ends inside / at / just past a 64-query tile."""
    rng = np.random.default_rng(600 + n)
    dim = 512
    rows, q = unit(rng, G_SEED, dim), unit(rng, QM, dim)
    who = np.sort(rng.choice(QM, n, replace=False))
    pos = rng.choice(G_SEED, 48 * n, replace=False).reshape(n, 48)
    near = q[who][:, None, :] + np.float32(2e-7) * rng.standard_normal((n, 48, dim), dtype=np.float32)
    rows[pos] = near / np.linalg.norm(near, axis=2, keepdims=True)
    model = oracle.gallery_topk_mfma(q, rows, KM)
    g32, g16 = galleries(rows)
    stats = check_both(g32, g16, q, dev(q), model, [(256, 16)], rows=rows, tag=f"cluster n={n}")
    c, f = stats[0][2:]
    assert f >= n and c + f == QM, (c, f, n)


# ------------------------------------------------------------------------------------------ non-finite values, overflow
@pytest.mark.timeout(300)
def test_non_finite_queries_leave_the_others_alone():
    rng = np.random.default_rng(700)
    dim = 512
    rows, q = unit(rng, G_SEED, dim), unit(rng, 65, dim)
    clean = q.copy()
    q[5, 3] = np.nan
    q[40, 0] = np.inf
    model = oracle.gallery_topk_mfma(q, rows, 16)
    assert (model[1][5] == -1).all() and (model[0][5] == -1.0).all()
    g32, g16 = galleries(rows)
    stats = check_both(g32, g16, q, dev(q), model, [(65, 16), (65, 1)], rows=rows, tag="nan/inf queries")
    assert all(f >= 2 for _, _, _, f in stats)
    ref = topk(g32, dev(clean), 16)
    others = np.setdiff1d(np.arange(65), [5, 40])
    for g in (g32, g16):
        s, i = topk(g, dev(q), 16)
        assert np.array_equal(i[others], ref[1][others]) and np.array_equal(s[others].view(np.uint32), ref[0][others].view(np.uint32))


@pytest.mark.timeout(300)
def test_non_finite_and_overflowing_rows():
    rng = np.random.default_rng(701)
    dim, G = 512, 20000
    rows, q = unit(rng, G, dim), unit(rng, 65, dim)
    rows[10, 7] = np.nan
    rows[20, 3] = np.inf
    rows[30:40] = np.float32(1e19) * rng.choice([-1.0, 1.0], (10, dim)).astype(np.float32)
    q[7] = np.float32(1e19) * rng.choice([-1.0, 1.0], dim).astype(np.float32)       # against the 1e19 rows: products 1e38, sums overflow
    model = oracle.gallery_topk_mfma(q, rows, 16)
    assert np.isinf(model[0]).any()
    g32, g16 = galleries(rows)
    check_both(g32, g16, q, dev(q), model, [(65, 16), (65, 1)], f16_route=False, tag="nan/inf/1e19 rows")


# ------------------------------------------------------------------------------------------ index base at INT_MAX
@pytest.mark.timeout(300)
def test_index_base_next_to_int_max():
    rng = np.random.default_rng(800)
    dim = 512
    rows, q = unit(rng, G_SEED, dim), unit(rng, 65, dim)
    rows[-1] = q[0]
    base = INT_MAX - G_SEED
    model = oracle.gallery_topk_mfma(q, rows, 16, base=base)
    assert model[1][0, 0] == INT_MAX - 1
    g32, g16 = galleries(rows, base)
    check_both(g32, g16, q, dev(q), model, [(65, 16), (65, 1)], rows=rows, base=base, tag="base INT_MAX-G")
    g32, g16 = galleries(rows, base + 1)
    for g in (g32, g16):
        with pytest.raises(_lib.FaceHipError, match="31 bits"):
            topk(g, dev(q), 16)


# ------------------------------------------------------------------------------------------ merge
def merge_lists(rng, W, Q, k):
    """[W][Q][k] sorted lists with -1 tails (score 7.0 in the empty slots: emptiness is told by the index), distinct indices per
    query, many equal scores across parts, +-inf, scores << -1, -0.0 / +0.0."""
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 0.5, 0.25, -1e30, -5.0, 1.0], np.float32)
    n = W * k
    s = np.where(rng.random((W, Q, k)) < 0.6, rng.choice(special, (W, Q, k)), rng.standard_normal((W, Q, k), dtype=np.float32))
    s = s.astype(np.float32)
    idx = np.stack([rng.permutation(2 * n)[:n] + 1 for _ in range(Q)], axis=0).reshape(Q, W, k).transpose(1, 0, 2).astype(np.int32)
    o = np.lexsort((idx, -s), axis=-1)
    s, idx = np.take_along_axis(s, o, -1), np.take_along_axis(idx, o, -1)
    fill = rng.integers(0, k + 1, (W, Q, 1))
    fill[0, :, 0] = k                                            # at least one full list
    empty = np.arange(k)[None, None, :] >= fill
    s[empty], idx[empty] = 7.0, -1
    return np.ascontiguousarray(s), np.ascontiguousarray(idx)


def merge_ref(s, idx, k):
    W, Q, _ = s.shape
    out_s, out_i = np.full((Q, k), -1.0, np.float32), np.full((Q, k), -1, np.int32)
    for q in range(Q):
        ss, ii = s[:, q].reshape(-1), idx[:, q].reshape(-1)
        keep = ii >= 0
        ss, ii = ss[keep], ii[keep]
        o = np.lexsort((ii, -ss))[:k]
        out_s[q, :len(o)], out_i[q, :len(o)] = ss[o], ii[o]
    return out_s, out_i


@pytest.mark.timeout(300)
@pytest.mark.parametrize("W,k", [(1, 16), (3, 7), (512, 16), (513, 16), (8192, 1), (8193, 1), (4096, 16)])
def test_merge_matches_lexsort_packed_and_strided(W, k):
    """fh_topk_merge_dev (packed [W][Q][k]) and fh_debug_topk_merge_strided_dev with comm.cpp's gathered layout (rank w's score
    plane, then its index plane: part_stride = 2 Q k) and with a padded stride; nparts * k straddles the 8192-entry cached / uncached
    switch and reaches the 65536 limit."""
    rng = np.random.default_rng(900 + W * 17 + k)
    Q = 3
    s, idx = merge_lists(rng, W, Q, k)
    want = merge_ref(s, idx, k)
    L = fa.lib()
    plane = Q * k

    def run(call):
        os_ = torch.full((Q, k), 9.0, device="cuda"); oi = torch.full((Q, k), -9, dtype=torch.int32, device="cuda")
        assert call(os_.data_ptr(), oi.data_ptr()) == Q, _lib.last_error()
        torch.cuda.synchronize()
        return os_.cpu().numpy(), oi.cpu().numpy()

    ps, pi = dev(s), dev(idx)
    assert_bits(run(lambda a, b: L.fh_topk_merge_dev(ps.data_ptr(), pi.data_ptr(), W, Q, k, a, b, None)), want, "packed")
    gathered = np.empty((W, 2, plane), np.float32)                  # comm.cpp (3): per rank [scores | indices as raw words]
    gathered[:, 0] = s.reshape(W, plane)
    gathered[:, 1] = idx.reshape(W, plane).view(np.float32)
    gd = dev(gathered)
    assert_bits(run(lambda a, b: L.fh_debug_topk_merge_strided_dev(gd.data_ptr(), gd.data_ptr() + 4 * plane, W, Q, k, 2 * plane, a, b,
                                                                   None)), want, "comm layout")
    stride = plane + 13                                             # padding that would win if it were read: score 1e30, index 0
    sp = np.full((W, stride), 1e30, np.float32); ip = np.zeros((W, stride), np.int32)
    sp[:, :plane], ip[:, :plane] = s.reshape(W, plane), idx.reshape(W, plane)
    spd, ipd = dev(sp), dev(ip)
    assert_bits(run(lambda a, b: L.fh_debug_topk_merge_strided_dev(spd.data_ptr(), ipd.data_ptr(), W, Q, k, stride, a, b, None)), want,
                "padded stride")
