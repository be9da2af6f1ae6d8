"""The three-piece bf16 ("x3") model (tests/wino_x3_model.py) pinned in exact rational arithmetic, and the power of the GPU bars of
tests/test_gpu_wino_x3.py: a kernel that drops one of the six products, adds a seventh, exchanges two pieces or two k positions must
fall outside them on the very operand sets those tests use.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import wino_x3_model as xm

F = Fraction


def _frac(a):
    return [F(float(v)) for v in np.asarray(a, np.float32).ravel()]


def _check_exact(words):
    x = words.view(np.float32)
    h, m, l = xm.split3(x)
    for p in (h, m, l):
        assert np.isfinite(p).all()                                        # finite in, finite pieces out
        assert (xm.is_bf16_normal(p) | (p == 0)).all()
        assert ((p.view(np.uint32) & 0xFFFF) == 0).all()                   # every piece is a bf16 value
    xs, hs, ms, ls = _frac(x), _frac(h), _frac(m), _frac(l)
    bad = [hex(int(w)) for w, a, b, c, d in zip(words, xs, hs, ms, ls) if a != b + c + d]
    assert not bad, bad[:8]
    ax = np.abs(x.astype(np.float64))
    assert (np.abs(m.astype(np.float64)) <= ax * 2.0 ** -7).all() and (np.abs(l.astype(np.float64)) <= ax * 2.0 ** -16).all()


def test_split_reconstructs_crafted_words_exactly():
    """+-0, ties of m both ways, m carrying into the next binade, negative l, negative values, the largest finite f32 (and the values a
    rounded h would overflow on), the smallest value whose l is still bf16-normal: x == h + m + l in exact arithmetic."""
    w = xm.crafted_words()
    for must in (0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x0C000101, 0x3F80FFFF, 0x3F808080, 0x3F808180):
        assert must in w, hex(must)
    _check_exact(w)
    h, m, l = xm.split3(np.array([0x3F808080, 0x3F808180, 0x3F80FFFF, 0x0C000101], np.uint32).view(np.float32))
    assert l[0] > 0 and l[1] < 0                                           # the two ties of m round to even: one down, one up
    assert m[2] == np.float32(2.0 ** -7) and l[2] == np.float32(-2.0 ** -23)   # carry into the next binade, negative l
    assert l[3] == np.float32(2.0 ** -126)                                 # the smallest bf16 normal


def test_split_reconstructs_random_words_exactly():
    """10^5 seeded bit patterns (finite; pieces zero or bf16-normal)"""
    _check_exact(xm.random_words(np.random.default_rng(31), 100000))


def test_finite_inputs_give_finite_pieces():
    """every finite f32 of the top binades, where a rounded h would become Inf, and a seeded sample of all finite patterns"""
    rng = np.random.default_rng(32)
    w = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    w = np.concatenate([w[((w >> 23) & 0xFF) != 0xFF], np.arange(0x7F7F0000, 0x7F800000, dtype=np.uint32), np.arange(0xFF7F0000, 0xFF800000, dtype=np.uint32)])
    for p in xm.split3(w.view(np.float32)):
        assert np.isfinite(p).all()


def test_non_finite_inputs_stay_non_finite():
    w = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF, 0xFF800001], np.uint32)
    h, m, l = xm.split3(w.view(np.float32))
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(h + m + l).any()
    assert np.isnan(m).all() and np.isnan(l).all()                         # a NaN piece meets every one of the six products (m: mm, mh, hm)


# c of the six-term bound, derived from the rule: |m| <= 2^-7 |x| (x - h is below one bf16 ulp of the truncated h, and rounding it to
# bf16 can at most reach that ulp), |l| <= 2^-16 |x| (half a bf16 ulp of x - h < 2^-7 |x|).  The six products leave out
# u_m v_l + u_l v_m + u_l v_l, so per product |six - u v| <= (2^-7 2^-16 + 2^-16 2^-7 + 2^-32) |u v| = (2^-22 + 2^-32) |u v|, and summed
# over k: |six-term - exact| <= c sum |u v| with
C_SIX = F(1, 2 ** 22) + F(1, 2 ** 32)


@pytest.mark.parametrize("K", (32, 160, 256))
@pytest.mark.parametrize("kind", ("normal", "positive"))
def test_six_term_error_bound_in_exact_arithmetic(K, kind):
    """|six-term - exact| <= c sum_k |u v| with c = 2^-22 + 2^-32 (derivation above), everything in Fractions: only the dropped terms
    show.  A few outputs per K: the bound is per output."""
    rng = np.random.default_rng(40 + K)
    V, U = xm.dense_operands(rng, 3, K, 2, kind)
    vp = [np.reshape(_frac(p), (3, K)) for p in xm.split3(V)]
    up = [np.reshape(_frac(p), (2, K)) for p in xm.split3(U[0])]
    ix = {"h": 0, "m": 1, "l": 2}
    worst = F(0)
    for r in range(3):
        for n in range(2):
            six = sum(up[ix[t[0]]][n][k] * vp[ix[t[1]]][r][k] for t in xm.ORDER for k in range(K))
            exact = sum(F(float(U[0][n][k])) * F(float(V[r][k])) for k in range(K))
            sabs = sum(abs(F(float(U[0][n][k])) * F(float(V[r][k]))) for k in range(K))
            assert abs(six - exact) <= C_SIX * sabs
            worst = max(worst, abs(six - exact) / sabs)
            # and the fp64 model agrees with the rational six-term sum to fp64 accuracy
            M, S = xm.gemm_model(V[r:r + 1], U[0][n:n + 1])
            assert abs(F(float(M[0, 0])) - six) <= F(float(S[0, 0])) * F(K + 6, 2 ** 52)
    print(f"K={K} {kind}: worst |six - exact| / sum|uv| = {float(worst):.3g} (c = {float(C_SIX):.3g})")


# ---------------------------------------------------------------------------------------------------------------- power of the bars
VARIANTS = {
    "drop hl": dict(terms=("lh", "mm", "mh", "hm", "hh")),
    "drop lh": dict(terms=("hl", "mm", "mh", "hm", "hh")),
    "drop mm": dict(terms=("lh", "hl", "mh", "hm", "hh")),
    "ml added": dict(terms=("ml",) + xm.ORDER),
    "h<->m in V": dict(v_swap=True),
    "h<->m in U": dict(u_swap=True),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_wrong_variants_fail_the_one_hot_bitwise_bar(name):
    """the 24 x 24-bit one-hot set of the GPU test (K = 32, N = 64): the variant's value differs in bits from the model's on a large share
    of the outputs — the bitwise bar has no slack to hide it in"""
    rng = np.random.default_rng(32 * 1000 + 64 + 256)
    V, wv = xm.one_hot_operands(rng, 512, 32, 64, "f")
    kk = xm.one_hot_kk(32, 64)
    v = V[:, kk[3]]
    good = xm.one_hot_chain(v, wv[3][None])
    bad = xm.one_hot_chain(v, wv[3][None], **VARIANTS[name])
    share = float((good.view(np.uint32) != bad.view(np.uint32)).mean())
    print(f"{name}: {100 * share:.1f} % of the outputs differ in bits")
    assert share > 0.05


def test_exchanged_k_fails_the_one_hot_bar():
    """k <-> k ^ 1: every output then sees its neighbour's V value"""
    rng = np.random.default_rng(5)
    V, wv = xm.one_hot_operands(rng, 256, 32, 64, "c")
    kk = xm.one_hot_kk(32, 64)
    good = V[:, kk[0]].astype(np.float64) * wv[0][None]
    bad = V[:, kk[0] ^ 1].astype(np.float64) * wv[0][None]
    assert (good != bad).mean() > 0.99


def test_dense_bar_sees_a_dropped_mm_and_nothing_smaller():
    """the all-positive dense set at K = 32 (the GPU test's smallest K, where the bar 2 gamma_{6K+5} S = 2^-15.4 S is tightest): without
    u_m v_m (up to 2^-14 of a product, coherent here) the exact value lies outside the bar around the model.  Every other variant moves
    an output by one l-term, at most 2^-16 of S — below the dense bar at every K; those are the bitwise one-hot bar's to catch (above),
    and the assertion below records that the dense bar does not."""
    K, N = 32, 64
    rng = np.random.default_rng(K * 1000 + N + 256 + 1)
    V, U = xm.dense_operands(rng, 64, K, N, "positive")
    M, S = xm.gemm_model(V, U[0])
    bar = 2 * xm.gamma(6 * K + 5) * S
    ratios = {}
    for name in ("drop hl", "drop lh", "drop mm", "h<->m in V", "h<->m in U"):
        v = VARIANTS[name]
        vp, up = list(xm.split3(V)), list(xm.split3(U[0]))
        if v.get("v_swap"):
            vp[0], vp[1] = vp[1], vp[0]
        if v.get("u_swap"):
            up[0], up[1] = up[1], up[0]
        Mv, _ = xm.gemm_pieces(vp, up, v.get("terms", xm.ORDER))
        ratios[name] = float((np.abs(Mv - M) / bar).max())
    print({k: round(r, 3) for k, r in ratios.items()})
    assert ratios["drop mm"] > 1.0
    assert all(r < 1.0 for k, r in ratios.items() if k != "drop mm")
