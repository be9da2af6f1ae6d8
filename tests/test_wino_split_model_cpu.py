"""Pins tests/wino_split_model.py (the exact model of the split-bf16 Winograd path) and proves that the bars of
tests/test_gpu_wino_bf16x2.py have power: on that file's own operand sets every wrong variant of the GEMM is far outside them.

CPU only.  The variants (terms named u-half then v-half, the kernel computes um*vh + uh*vm + uh*vh):
  drop_hm   uh*vm missing              drop_mh   um*vh missing               add_mm   um*vm added back
  swap_v    hi and mid of V exchanged  swap_u    the same in U               kswap_v / kswap_u   k and k^1 exchanged in one operand only
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import wino_split_model as wm

# the shapes of C.2 / C.3 of tests/test_gpu_wino_bf16x2.py (rows cut to one 128-row tile per plane: the power is a per-element property)
KS = (32, 64, 160, 256)
NS = (64, 192)


# ------------------------------------------------------------------------------------------------------------------- split()
def _frac(bits):
    """the exact value of a finite f32 bit pattern"""
    s = -1 if bits >> 31 else 1
    e, m = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    return s * (Fraction(m, 1 << 23) * Fraction(2) ** -126 if e == 0 else (1 + Fraction(m, 1 << 23)) * Fraction(2) ** (e - 127))


def _rne8(x):
    """x (Fraction) rounded to 8 significant bits, ties to even (bf16 inside its normal range)"""
    if x == 0:
        return Fraction(0)
    a, e = abs(x), 0
    while a >= 2:
        a /= 2; e += 1
    while a < 1:
        a *= 2; e -= 1
    ulp = Fraction(2) ** (e - 7)
    q = abs(x) / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return (1 if x > 0 else -1) * n * ulp


def _f32_frac(a):
    return _frac(int(np.float32(a).view(np.uint32)))


def test_split_matches_exact_rational_arithmetic_on_the_crafted_words():
    words = wm.crafted_words()
    hi, mid, word = wm.split(words.view(np.float32))
    for i, b in enumerate(words):
        x = _frac(int(b))
        h = _rne8(x)
        m = _rne8(x - h)
        assert _f32_frac(hi[i]) == h and _f32_frac(mid[i]) == m, hex(int(b))
        assert int(word[i]) == (int(hi[i].view(np.uint32)) >> 16) | (int(mid[i].view(np.uint32)) & 0xFFFF0000), hex(int(b))
        assert abs(x - h - m) <= abs(x) * Fraction(1, 1 << 16), hex(int(b))                  # 16 bits carried
    named = {int(b): (float(hi[i]), float(mid[i]), int(word[i])) for i, b in enumerate(words)}
    assert named[0x00000000][2] == 0x00000000 and named[0x80000000][2] == 0x00008000          # -0: hi keeps the sign, r = +0
    assert named[0x3F808000][:2] == (1.0, 2.0 ** -8)                                          # tie -> even, hi stays
    assert named[0x3F818000][:2] == (1.0 + 2.0 ** -6, -(2.0 ** -8))                           # tie -> even, hi goes up, mid negative
    assert named[0x3F7FFFFF][:2] == (1.0, -(2.0 ** -24))                                      # carry into the next binade
    assert named[0x3F800101][:2] == (1.0, 2.0 ** -15) and named[0x3F800103][1] == 2.0 ** -15 * (1 + 2.0 ** -6)   # ties of mid -> even
    assert named[0x0C000001][:2] == (2.0 ** -103, 2.0 ** -126)                                # the smallest bf16-normal mid
    assert named[0x7F7F7FFF][0] == float(np.uint32(0x7F7F0000).view(np.float32))              # the largest finite hi
    # everything crafted stays inside the range the GPU test compares bitwise: halves zero or normal
    assert ((wm.is_bf16_normal(hi) | (hi == 0)) & (wm.is_bf16_normal(mid) | (mid == 0))).all()


def test_split_overflows_to_inf_minus_inf_from_0x7f7f8000():
    x = np.array([0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000], np.uint32).view(np.float32)
    hi, mid, _ = wm.split(x)
    assert np.isinf(hi).all() and np.isinf(mid).all() and (np.sign(hi) == -np.sign(mid)).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(hi + mid).all()


def test_values_of_at_most_16_significant_bits_split_exactly():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1 << 16).astype(np.float32) * np.float32(2.0) ** rng.integers(-40, 40, 1 << 16).astype(np.float32)
    for bits in (1, 8, 9, 12, 16):
        q = wm.quantize(x, bits)
        hi, mid, _ = wm.split(q)
        assert (hi.astype(np.float64) + mid.astype(np.float64) == q.astype(np.float64)).all(), bits
    hi, mid, _ = wm.split(x)                                                                  # 24 bits: not exact, 16 bits carried
    err = np.abs(hi.astype(np.float64) + mid.astype(np.float64) - x)
    assert (err > 0).any() and (err <= np.abs(x) * 2.0 ** -16).all()
    # random_words: the population the GPU compares bitwise
    w = wm.random_words(np.random.default_rng(1), 4096)
    hi, mid, _ = wm.split(w.view(np.float32))
    assert np.isfinite(w.view(np.float32)).all() and (np.abs(w.view(np.float32)) < 2.0 ** 127).all()
    assert ((wm.is_bf16_normal(hi) | (hi == 0)) & (wm.is_bf16_normal(mid) | (mid == 0))).all()
    assert wm.unpack(wm.split(w.view(np.float32))[2])[0].tobytes() == hi.tobytes()


def test_conv_model_is_the_convolution():
    """Small integer inputs and weights that are multiples of 576 = 24^2 make U = G g G^T integral with <= 8 significant bits (um = 0)
    and V an integer of <= 16 bits (splits exactly): nothing is dropped or rounded, so the model must BE the convolution — on a ragged
    map with overhanging tiles.  On ordinary operands it is the convolution to about 2^-17."""
    rng = np.random.default_rng(2)
    x = rng.integers(-40, 41, (2, 32, 7, 10)).astype(np.float32)
    w = (rng.integers(-3, 4, (8, 32, 3, 3)) * 576).astype(np.float32)
    b = rng.integers(-9, 10, 8).astype(np.float64)
    U = wm.filter_transform(w)
    V, _ = wm.input_transform(x)
    assert (U == np.rint(U)).all() and (wm.split(U)[1] == 0).all()
    vh, vm, _ = wm.split(V)
    assert (vh.astype(np.float64) + vm == V).all() and (vm != 0).any()
    assert (wm.conv_model(x, w, b) == wm.conv_fp64(x, w, b)).all()
    x = rng.standard_normal((2, 32, 7, 10)).astype(np.float32)
    w = (rng.standard_normal((8, 32, 3, 3)) / np.sqrt(288)).astype(np.float32)
    got, ref = wm.conv_model(x, w, None), wm.conv_fp64(x, w, None)
    assert 0 < np.abs(got - ref).max() < 1e-3 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------------- power of the GPU bars
def _variants(vh, vm, uh, um):
    ks = np.arange(vh.shape[-1]) ^ 1
    return {
        "drop_hm": ((vh, vm, uh, um), ("mh", "hh")),
        "drop_mh": ((vh, vm, uh, um), ("hm", "hh")),
        "add_mm": ((vh, vm, uh, um), ("mh", "hm", "hh", "mm")),
        "swap_v": ((vm, vh, uh, um), ("mh", "hm", "hh")),
        "swap_u": ((vh, vm, um, uh), ("mh", "hm", "hh")),
        "kswap_v": ((vh[..., ks], vm[..., ks], uh, um), ("mh", "hm", "hh")),
        "kswap_u": ((vh, vm, uh[..., ks], um[..., ks]), ("mh", "hm", "hh")),
    }


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# C.2: which variants each operand class must expose (class a has um = 0 and class b has vm = 0: they isolate one cross term each)
ONE_HOT_EXPOSES = {"a": {"drop_hm", "swap_u", "kswap_v", "kswap_u"},
                   "b": {"drop_mh", "swap_v", "kswap_v", "kswap_u"},
                   "c": {"drop_hm", "drop_mh", "add_mm", "swap_v", "swap_u", "kswap_v", "kswap_u"}}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_one_hot_sets_expose_every_wrong_variant(K, N):
    """C.2's bar is bit equality with the exact three-term product.  A wrong variant must move the result by at least 8 f32 ulps somewhere
    and change more than 80 % of the elements.  Measured, worst shape (ulps of the expected value, max over elements / fraction of
    elements changed), classes a | b | c:

        drop_hm   6.4e4 / 0.995 |  0              | 6.5e4 / 0.93
        drop_mh   0             |  6.1e4 / 0.994  | 6.4e4 / 0.93
        add_mm    0             |  0              | 128   / 0.87
        swap_v    0             |  6.1e4 / 0.994  | 6.4e4 / 0.93
        swap_u    6.4e4 / 0.995 |  0              | 6.5e4 / 0.93
        kswap_v   8.0e7 / 1.0   |  8.0e7 / 0.997  | 8.0e7 / 1.0
        kswap_u   8.0e7 / 1.0   |  8.0e7 / 0.997  | 8.0e7 / 1.0

    The zeros are by construction and are asserted as zeros: um = 0 in class a and vm = 0 in class b, so each isolates one cross term
    (and an exchange of the halves of the operand whose mid is zero merely renames a term).  Class c exposes all seven."""
    rng = np.random.default_rng(K * 7 + N)
    kk = wm.one_hot_kk(K, N)
    assert set(np.unique(kk)) == set(range(K)) and (kk[1:] != kk[:-1]).all()
    if N >= K:
        assert all(set(np.unique(kk[f])) == set(range(K)) for f in range(36))
    for cls, exposes in ONE_HOT_EXPOSES.items():
        V, wv, _ = wm.one_hot_operands(rng, 128, K, N, cls)
        U = np.zeros((36, N, K), np.float32)
        f, n = np.meshgrid(np.arange(36), np.arange(N), indexing="ij")
        U[f, n, kk] = wv
        vh, vm, _ = wm.split(V)
        uh, um, _ = wm.split(U)
        assert (vh.astype(np.float64) + vm == V).all() and (uh.astype(np.float64) + um == U).all()         # operands split exactly
        exp = wm.one_hot_expected(V[:, kk], wv[None])                                                      # [rows, 36, N]
        exp = np.moveaxis(exp, 0, 1)
        assert (exp.astype(np.float32).astype(np.float64) == exp).all()                                   # exact in f32
        M, _ = wm.gemm_halves(vh, vm, uh, um)
        assert (M == exp).all()
        if cls == "c":                                                                                     # three terms, not the rounded product
            prod = V[:, kk].astype(np.float64) * wv[None]
            assert (np.moveaxis(prod, 0, 1) != exp).mean() > 0.8
        for name, (halves, terms) in _variants(vh, vm, uh, um).items():
            Mv, _ = wm.gemm_halves(*halves, terms=terms)
            ulps = np.abs(Mv - exp) / _ulp32(exp)
            print(f"K={K} N={N} class {cls} {name:8s} max ulps {ulps.max():.3g} changed {(ulps > 0).mean():.3f}")
            if name in exposes:
                assert ulps.max() >= 8 and (ulps > 0).mean() > 0.8, (cls, name, ulps.max(), (ulps > 0).mean())
            else:
                assert ulps.max() == 0, (cls, name)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_dense_sets_put_wrong_variants_far_outside_the_derived_bound(K, N):
    """C.3's bar is |M - model| <= 2 gamma_{3K+2} S per element.  max(|variant - model| / bound) measured, the smaller of the two N, for
    K = 32 / 64 / 160 / 256 (the bound grows with K, a coherent error does not, so K = 256 is the hardest):

        variant     positive set                 N(0,1) set
        drop_hm     238 / 116 / 46 / 28.7        160 / 55 / 15.7 / 7.3
        drop_mh     170 / 118 / 37 / 29.1        166 / 63 / 15.6 / 6.6
        swap_v      170 / 118 / 37 / 29          166 / 63 / 15.6 / 6.6
        swap_u      238 / 116 / 46 / 28.7        160 / 55 / 15.7 / 7.3
        kswap_v     407 / 145 / 35 / 16.3        1.4e5 / 4.5e4 / 1.3e4 / 6.2e3
        kswap_u     407 / 145 / 35 / 16.3        1.4e5 / 4.5e4 / 1.3e4 / 6.2e3
        add_mm      0.47 / 0.32 / 0.10 / 0.08    0.30 / 0.12 / 0.025 / 0.013

    The positive set puts a lost cross term (an exchange of halves loses one too) at least 16x outside the bar at every shape.  On the
    N(0,1) set the lost term is a random walk of signed products and falls to 6.6x at K = 256 — below the 8x asked for, which is why
    the positive set exists; asserted there as >= 8 up to K = 160 and > 4 at K = 256.  add_mm CANNOT be seen by this bar at any shape:
    |um*vm| <= 2^-18 |uh*vh| while the bound is at least 2 gamma_98 = 2^-16.4 of S; asserted as < 1, and held by C.2's class c (bitwise)
    alone."""
    rng = np.random.default_rng(K * 11 + N)
    for kind in ("positive", "normal"):
        V, U = wm.dense_operands(rng, 128, K, N, kind)
        U = U[:4]                                                            # (four of the 36 weight planes are population enough)
        vh, vm, _ = wm.split(V)
        uh, um, _ = wm.split(U)
        assert wm.is_bf16_normal(vh).all() and wm.is_bf16_normal(vm).all() and wm.is_bf16_normal(uh).all() and wm.is_bf16_normal(um).all()
        if kind == "positive":
            assert (vh > 0).all() and (vm > 0).all() and (uh > 0).all() and (um > 0).all()
        M, S = wm.gemm_model(V[None], U)
        bound = 2 * wm.gamma(3 * K + 2) * S
        for name, (halves, terms) in _variants(vh[None], vm[None], uh, um).items():
            Mv, _ = wm.gemm_halves(*halves, terms=terms)
            ratio = (np.abs(Mv - M) / bound).max()
            print(f"K={K} N={N} {kind:8s} {name:8s} ratio {ratio:.3g}")
            if name == "add_mm":
                assert ratio < 1, (kind, name, ratio)                    # invisible to this bar (see the docstring)
            elif kind == "positive" or name.startswith("kswap"):
                assert ratio >= 8, (kind, name, ratio)
            else:
                assert ratio >= (8 if K <= 160 else 4), (kind, name, ratio)


def test_plane_layouts():
    """the Python restatement of the plane layouts the GEMM hook is driven with (docs/kernels.md 3.1c, 3.1j)"""
    pl = wm.uniform_planes(300)
    assert len(pl) == 36 and pl[1] == (512, 300, 512, 1) and pl[35][0] + pl[35][2] == 36 * 512
    pl = wm.mixed_planes(64, 14, 14)                                  # 9 / 3 / 3 / 1 tiles per image, 36 / 24 / 24 / 16 planes
    assert len(pl) == 100 and [p[2] for p in pl[:1] + pl[36:37] + pl[60:61] + pl[84:85]] == [640, 256, 256, 128]
    assert pl[-1][0] + pl[-1][2] == 36 * 640 + 24 * 256 + 24 * 256 + 16 * 128 == 128 * 292
    assert [p[3] for p in pl[36:40]] == [0, 1, 2, 5] and [p[3] for p in pl[60 + 18:60 + 24]] == [30, 31, 32, 33, 34, 35]
    assert [p[3] for p in pl[84:]] == [0, 1, 2, 5, 6, 7, 8, 11, 12, 13, 14, 17, 30, 31, 32, 35]
    pl = wm.mixed_planes(64, 16, 14)                                  # only the columns are mixed: two classes
    assert len(pl) == 60 and {p[1] for p in pl} == {64 * 12, 64 * 4}
