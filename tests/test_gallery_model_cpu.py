"""CPU tests of `oracle.gallery_topk_mfma`, the exact model of the gallery scan's arithmetic that tests/test_gpu_gallery_exact.py holds
the GPU to bit for bit.  They pin the model itself: its fma chain against an independent exact-rational evaluation, its error against
fp64, that it is fused and that it follows the kernel's k order (not just any order), and its selection rules."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle

U = 2.0 ** -24


def f32_round(x: Fraction) -> float:
    """x rounded to binary32, round to nearest even, subnormals and overflow included."""
    if x == 0:
        return 0.0
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    r = round(a / ulp) * ulp                                   # Fraction.__round__: ties to even
    v = math.inf if r >= Fraction(2) ** 128 else float(r)
    return -v if x < 0 else v


def fma32(a, b, c) -> float:
    return f32_round(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def kernel_order(dim):
    """The k sequence of gallery_topk_kernel's multiply: kc, s = 0..7, e = 0..3; k0 = 64 kc + 8 s + e, then k1 = k0 + 4."""
    return [kc + 8 * s + e + 4 * h for kc in range(0, dim, 64) for s in range(8) for e in range(4) for h in range(2)]


def chain(q, g, order, fused=True):
    acc = 0.0
    for kk in order:
        if fused:
            acc = fma32(g[kk], q[kk], acc)
        else:
            acc = float(np.float32(acc) + np.float32(g[kk]) * np.float32(q[kk]))
    return np.float32(acc)


def mapped(acc):
    return (np.float32(acc) + np.float32(1.0)) / np.float32(2.0)


@pytest.mark.parametrize("dim", [64, 192])
def test_model_equals_exact_rational_fma_chain(dim):
    rng = np.random.default_rng(dim)
    n = 24
    g = rng.standard_normal((n, dim)) * np.exp2(rng.integers(-12, 13, (n, dim)))
    q = rng.standard_normal((3, dim))
    g[-4:] = rng.standard_normal((4, dim)) * 2.0 ** -135       # subnormal rows: products and partial sums on the 2^-149 grid
    g, q = g.astype(np.float32), q.astype(np.float32)
    order = kernel_order(dim)
    s_all, i_all = oracle.gallery_topk_mfma(q, g, n)
    for qi in range(3):
        raw = oracle.dot_mfma(q[qi], g)
        score = np.empty(n, np.float32)
        score[i_all[qi]] = s_all[qi]
        assert sorted(i_all[qi]) == list(range(n))
        for r in range(n):
            want = chain(q[qi], g[r], order)
            assert raw[r].view(np.uint32) == want.view(np.uint32), (qi, r, raw[r], want)
            assert score[r].view(np.uint32) == mapped(want).view(np.uint32), (qi, r)
    assert (np.abs(oracle.dot_mfma(q[0], g[-4:])) < 2.0 ** -126).any()     # the subnormal rows did produce subnormal sums


@pytest.mark.parametrize("dim", [64, 192, 512, 2048])
def test_model_error_within_gamma_bound_of_fp64(dim):
    rng = np.random.default_rng(7 + dim)
    g = (rng.standard_normal((200, dim)) * rng.uniform(0.1, 10.0, (200, 1))).astype(np.float32)
    q = (rng.standard_normal((4, dim)) * rng.uniform(0.1, 10.0, (4, 1))).astype(np.float32)
    gamma = dim * U / (1 - dim * U)
    g64, q64 = g.astype(np.float64), q.astype(np.float64)
    for qi in range(4):
        raw = oracle.dot_mfma(q[qi], g).astype(np.float64)
        exact = g64 @ q64[qi]
        bound = 2 * gamma * np.linalg.norm(q64[qi]) * np.linalg.norm(g64, axis=1)
        assert (np.abs(raw - exact) <= bound).all()
        assert (raw != exact.astype(np.float32)).any()         # (not a correctly rounded dot product: the chain's rounding shows)


def test_model_is_fused():
    dim = 64
    q, g = np.zeros(dim, np.float32), np.zeros(dim, np.float32)
    q[0], g[0] = -(1 + 2.0 ** -11), 1.0                       # k0 = 0: acc = -(1 + 2^-11)
    q[4] = g[4] = 1 + 2.0 ** -12                               # k1 = 4: product 1 + 2^-11 + 2^-24, its low bit lost when rounded alone
    raw = oracle.dot_mfma(q, g[None])[0]
    assert raw == np.float32(2.0 ** -24) == chain(q, g, kernel_order(dim))
    assert chain(q, g, kernel_order(dim), fused=False) == 0.0


def test_model_follows_the_kernel_k_order():
    # within one MFMA: k0 before k1 (k = 1 before k = 5) — 1 + 2^24 rounds to 2^24, 1 - 2^24 is exact
    dim = 64
    q, g = np.zeros(dim, np.float32), np.ones(dim, np.float32)
    q[0], q[1], q[5] = 1.0, 2.0 ** 24, -(2.0 ** 24)
    swapped = [o for kk in kernel_order(dim)[::2] for o in (kk + 4, kk)]
    want = chain(q, g, kernel_order(dim))
    assert oracle.dot_mfma(q, g[None])[0] == want == 0.0
    assert chain(q, g, swapped) == 1.0
    # chunks in ascending order: chunk 0's 1 is absorbed by chunk 1's 2^24 before the cancellation
    dim = 128
    q, g = np.zeros(dim, np.float32), np.ones(dim, np.float32)
    q[0], q[64], q[68] = 1.0, 2.0 ** 24, -(2.0 ** 24)
    order = kernel_order(dim)
    rev = order[64:] + order[:64]
    assert oracle.dot_mfma(q, g[None])[0] == chain(q, g, order) == 0.0
    assert chain(q, g, rev) == 1.0


def test_model_selection_rules():
    dim = 64
    rng = np.random.default_rng(3)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    g = rng.standard_normal((9, dim)).astype(np.float32)
    g[0, 5] = np.nan                                           # never listed
    g[2] = g[4] = g[7] = q[0]                                  # identical scores: ties by index
    g[3] = 0.0                                                 # score exactly 0.5
    g[8] = q[0] * np.float32(1e38)                             # +inf for query 0
    s, i = oracle.gallery_topk_mfma(q, g, 12, base=100)
    assert i[0, 0] == 108 and s[0, 0] == np.inf
    assert list(i[0, 1:4]) == [102, 104, 107] and s[0, 1] == s[0, 2] == s[0, 3]
    for qi in range(2):
        assert 100 not in i[qi] and not np.isnan(s[qi]).any()
        assert list(i[qi, 8:]) == [-1] * 4 and (s[qi, 8:] == -1.0).all()
        assert sorted(i[qi, :8]) == [101, 102, 103, 104, 105, 106, 107, 108]
        order = np.lexsort((i[qi, :8], -s[qi, :8]))
        assert (order == np.arange(8)).all()                  # (score desc, index asc)
    assert 0.5 in s[0]
    s1, i1 = oracle.gallery_topk_mfma(q, g, 3, base=100)
    assert (i1 == i[:, :3]).all() and (s1.view(np.uint32) == s[:, :3].view(np.uint32)).all()     # k is a prefix
    s0, i0 = oracle.gallery_topk_mfma(q, g[:0], 2)
    assert (i0 == -1).all() and (s0 == -1.0).all()
