"""The gallery's F16_RERANK scan (fh_gallery_set_scan): fp16 candidate scan, exact fp32 re-score, per-query certificate, fp32
fallback on the device.  Every test compares it with the FP32 scan on the same rows BIT FOR BIT (scores and indices)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unit_rows(n, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, dim), device="cuda", generator=g)
    return x / x.norm(dim=1, keepdim=True)


def topk(gal, q, k, stream=0):
    Q = q.shape[0]
    sc = torch.full((Q, k), 7.0, device="cuda"); ix = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    gal.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), stream)
    return sc, ix


def assert_same(a, b):
    torch.cuda.synchronize()
    (s1, i1), (s2, i2) = a, b
    s1, i1, s2, i2 = s1.cpu().numpy(), i1.cpu().numpy(), s2.cpu().numpy(), i2.cpu().numpy()
    assert np.array_equal(i1, i2), np.argwhere(i1 != i2)[:8]
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)), np.argwhere(s1 != s2)[:8]


def pair(rows, base=0):
    g32, g16 = fa.Gallery(rows.shape[1]), fa.Gallery(rows.shape[1], scan="f16")
    for g in (g32, g16):
        g.upload(rows.data_ptr(), rows.shape[0], True, base)
    assert g16.scan == "f16" and g32.scan == "fp32"
    return g32, g16


@pytest.mark.parametrize("G", [1, 31, 4097, 300001, (1 << 20) + 4097])
def test_f16_rerank_equals_fp32_on_random_unit_rows(G):
    rows = unit_rows(G, 512, G)
    qall = unit_rows(256, 512, G + 1)
    big = G == (1 << 20) + 4097
    if big:                                                   # exact duplicates of q[0] on both sides of the 2^20 boundary
        for r in (5, (1 << 20) - 1, 1 << 20, G - 1):
            rows[r] = qall[0]
    for base in (0, 1000):
        g32, g16 = pair(rows, base)
        g16.scan_stats()
        per_k = {}
        for Q in (1, 64, 200, 256):
            q = qall[:Q].contiguous()
            for k in (1, 5, 16):
                r16 = topk(g16, q, k)
                assert_same(topk(g32, q, k), r16)
                c, f = g16.scan_stats()
                assert c + f == Q
                pc, pf = per_k.get(k, (0, 0)); per_k[k] = (pc + c, pf + f)
                if k > G:
                    assert (r16[1][:, G:] == -1).all() and (r16[0][:, G:] == -1.0).all()
                if big:
                    want = [base + 5, base + (1 << 20) - 1, base + (1 << 20), base + G - 1][:min(k, 4)]
                    assert list(r16[1][0, :min(k, 4)].cpu().numpy()) == want
        if big:                                               # the fast path provably ran
            for k, (c, f) in per_k.items():
                assert c >= (0.99 if k == 1 else 0.90) * (c + f), (k, c, f)


def test_crafted_cluster_fails_the_certificate_and_falls_back():
    G, Q, k = 50000, 64, 16
    rows = unit_rows(G, 512, 3)
    q = unit_rows(Q, 512, 4)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for j in range(48):                                       # 48 rows within ~1e-6 of query 0's best match (q[0] itself)
        r = q[0] + 2e-7 * torch.randn(512, device="cuda", generator=gen)
        rows[100 + 997 * j] = r / r.norm()
    g32, g16 = pair(rows, 0)
    g16.scan_stats()
    assert_same(topk(g32, q, k), topk(g16, q, k))
    c, f = g16.scan_stats()
    assert f > 0 and c + f == Q, (c, f)


def test_enroll_growth_set_scan_after_upload_and_round_trip():
    rows = unit_rows(70000, 512, 8)
    q = unit_rows(100, 512, 9)
    g32, g16 = fa.Gallery(512), fa.Gallery(512, scan="f16")
    for a, b in ((0, 1000), (1000, 6000), (6000, 70000)):    # geometric growth of both copies
        chunk = rows[a:b].cpu().numpy()
        assert g32.enroll(chunk) == a and g16.enroll(chunk) == a
        assert_same(topk(g32, q, 16), topk(g16, q, 16))
    c, f = g16.scan_stats()
    assert c > 0
    g = fa.Gallery(512)
    g.upload(rows.data_ptr(), rows.shape[0], True, 0)
    ref = topk(g, q, 5)
    g.set_scan("f16")                                          # after upload
    assert g.scan == "f16"
    assert_same(ref, topk(g, q, 5))
    c, f = g.scan_stats()
    assert c > 0 and c + f == 100
    g.set_scan("fp32")                                         # and back
    assert g.scan == "fp32"
    assert_same(ref, topk(g, q, 5))
    g.set_scan("f16")
    assert_same(ref, topk(g, q, 5))


def test_label_dev_equal():
    rows = unit_rows(200000, 512, 11)
    q = unit_rows(77, 512, 12)
    q[:10] = rows[1000:1010]                                   # some matches, the rest unknown
    g32, g16 = pair(rows, 0)
    out = []
    for g in (g32, g16):
        lab = torch.zeros(77, dtype=torch.int32, device="cuda"); sc = torch.zeros(77, device="cuda")
        g.label_dev(q.data_ptr(), 77, 0.6, lab.data_ptr(), sc.data_ptr())
        out.append((sc, lab))
    assert_same(out[0], out[1])
    assert (out[1][1][:10].cpu().numpy() == np.arange(1000, 1010)).all()


def test_rows_beyond_fp16_range_take_the_fp32_route():
    rng = np.random.default_rng(13)
    G, Q, k = 20000, 64, 16
    rows = rng.standard_normal((G, 512)).astype(np.float32) * rng.uniform(0.1, 40.0, (G, 1)).astype(np.float32)
    rows[777, 3] = 70000.0                                     # not representable in fp16
    q = rng.standard_normal((Q, 512)).astype(np.float32)
    rd, qd = dev(rows), dev(q)
    g32, g16 = pair(rd, 0)
    g16.scan_stats()
    assert_same(topk(g32, qd, k), topk(g16, qd, k))
    c, f = g16.scan_stats()
    assert c == 0 and f == Q


def test_non_unit_rows_within_fp16_range_are_equal():
    rng = np.random.default_rng(14)
    G, Q, k = 100000, 200, 5
    rows = rng.standard_normal((G, 512)).astype(np.float32) * rng.uniform(0.1, 4.0, (G, 1)).astype(np.float32)
    q = rng.standard_normal((Q, 512)).astype(np.float32) * 0.5
    g32, g16 = pair(dev(rows), 0)
    qd = dev(q)
    assert_same(topk(g32, qd, k), topk(g16, qd, k))


def test_graph_capture_after_one_warm_up():
    rows = unit_rows(300001, 512, 15)
    Q, k = 64, 16
    q = unit_rows(Q, 512, 16)
    g32, g16 = pair(rows, 0)
    ref = topk(g32, q, k)
    side = torch.cuda.Stream()
    sc = torch.zeros((Q, k), device="cuda"); ix = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
    with torch.cuda.stream(side):
        g16.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), side.cuda_stream)       # warm-up: sizes the buffers
    side.synchronize()
    sc.fill_(0); ix.fill_(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g16.topk_dev(q.data_ptr(), Q, k, sc.data_ptr(), ix.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert_same(ref, (sc, ix))
    c, f = g16.scan_stats()
    assert c > 0 and c + f == 2 * Q                             # warm-up + replay (capture itself runs nothing)
