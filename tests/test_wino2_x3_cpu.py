"""wino2_x3_kernel without a GPU: the model of tests/wino2_x3_model.py against exact arithmetic, the host pack of the three-piece weight
image (wino2_pack_weights_x3 through fh_debug_wino2_pack_x3) against the model's statement of where every piece sits, and the launch
predicate wino2_x3_pays (question 8 of fh_debug_conv_plan)."""
from fractions import Fraction

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import wino2_x3_model as w2
from tests import wino_x3_model as xm


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def direct_conv(x, w_ohwi):
    """x [B][H][W][64], w [N][9][64] -> the 3x3 pad-1 convolution [B][H][W][N] in fp64"""
    x = np.asarray(x, np.float64); w = np.asarray(w_ohwi, np.float64)
    B, H, W, C = x.shape
    p = np.zeros((B, H + 2, W + 2, C)); p[:, 1:-1, 1:-1] = x
    out = np.zeros((B, H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += p[:, ky:ky + H, kx:kx + W] @ w[:, 3 * ky + kx].T
    return out


def test_transforms_are_winograd_f2x2():
    """the model's transforms in fp64 give the direct convolution (B^T, G, A^T and their index tables are F(2x2, 3x3)'s), odd sizes too"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 5, 7, 64)); w = rng.standard_normal((3, 9, 64))
    g = w.reshape(3, 3, 3, 64)
    U = np.einsum("ia,nabc,jb->ijnc", w2.G, g, w2.G).reshape(16, 3, 64)
    d = w2.patches(x)
    Bt = np.zeros((4, 4))
    for i in range(4):
        Bt[i, w2.YA[i]] += 1; Bt[i, w2.YB[i]] += w2.SB[i]
    V = np.einsum("ia,...abc,jb->ij...c", Bt, d, Bt).reshape((16,) + d.shape[:3] + (64,))
    M = np.stack([V[f] @ U[f].T for f in range(16)])
    A = np.array(w2.AT, np.float64)
    Y = np.einsum("ai,bj,ij...->ab...", A, A, M.reshape((4, 4) + M.shape[1:]))
    np.testing.assert_allclose(w2.untile(Y, 5, 7), direct_conv(x, w), rtol=0, atol=1e-11)
    # ... and the fp32 statements of the two transforms are those, rounded
    np.testing.assert_allclose(w2.input_transform(d.astype(np.float32)), V, rtol=0, atol=1e-5)
    np.testing.assert_allclose(w2.filter_transform(w.astype(np.float32)), U, rtol=0, atol=1e-6)
    np.testing.assert_allclose(w2.input_transform(d, absolute=True), np.einsum("ia,...abc,jb->ij...c", np.abs(Bt), np.abs(d), np.abs(Bt))
                               .reshape(V.shape), rtol=0, atol=1e-12)


def one_hot_layer(rng, B, H, W, N, cls):
    """one non-zero input channel per output channel ((7 n + 3) mod 64: every channel is used).  Class c: integer inputs (|x| <= 127,
    channels 0 mod 8 all zero) and integer filters (|g| <= 15, nine taps) — V <= 9 bits, 4 U <= 8 bits, every partial sum of an output
    < 2^20 quarter units: all exact.  Class f: 24 x 24 significand bits, ONE tap per filter (tap n mod 9), so that U_f = +-g / {1, 2, 4}
    keeps its 24 bits."""
    cin_of = (7 * np.arange(N) + 3) % 64
    w = np.zeros((N, 9, 64), np.float32)
    if cls == "c":
        x = rng.integers(-127, 128, (B, H, W, 64)).astype(np.float32)
        x[..., ::8] = 0
        w[np.arange(N), :, cin_of] = rng.integers(-15, 16, (N, 9)).astype(np.float32)
    else:
        xv, wv = xm.one_hot_operands(rng, B * H * W, 64, N, "f")
        x = xv.reshape(B, H, W, 64)
        w[np.arange(N), np.arange(N) % 9, cin_of] = wv[0]
    return x, w, cin_of


def test_model_one_hot_class_c_is_the_exact_convolution():
    rng = np.random.default_rng(2)
    x, w, cin_of = one_hot_layer(rng, 2, 5, 6, 64, "c")
    got = w2.layer_one_hot(x, w, cin_of)
    exact = direct_conv(x, w)
    assert (got.astype(np.float64) == exact).all()
    zero = exact == 0
    assert zero[..., cin_of % 8 == 0].all() and (_bits(got)[zero] == 0).all()          # +0, never -0


def test_model_one_hot_class_f_is_near_the_convolution():
    """24 x 24 bits: the model is the kernel's statement, not the exact product — but it must lie within the dense bound of it"""
    rng = np.random.default_rng(3)
    x, w, cin_of = one_hot_layer(rng, 1, 4, 4, 64, "f")
    got = w2.layer_one_hot(x, w, cin_of)
    assert (np.abs(got - direct_conv(x, w)) <= w2.dense_bound(x, w)).all()
    assert (got != direct_conv(x, w).astype(np.float32)).any()


@pytest.mark.parametrize("cout", [64, 192])
def test_packed_image(cout):
    """For every (cout, cin, f): the three pieces sit where lane (m, kq), step s, element j of wave / block (wv, cb) reads them, they are
    the model's split of the fp32 U, and h + m + l is that U exactly (in rational arithmetic).  Every word of the image is one of them."""
    rng = np.random.default_rng(cout)
    w = (rng.standard_normal((cout, 9, 64)) / 24).astype(np.float32)
    img = np.full(16 * 64 * cout * 3, 0xFFFF, np.uint16)
    assert fa.lib().fh_debug_wino2_pack_x3(w.ctypes.data, cout, 64, img.ctypes.data) == 0, _lib.last_error()
    U = w2.filter_transform(w)                                                       # [16][cout][64]
    pieces = [(_bits(p) >> 16).astype(np.uint16) for p in xm.split3(U)]
    assert all((_bits(p) & 0xFFFF == 0).all() for p in xm.split3(U))
    f, co, ci = np.meshgrid(np.arange(16), np.arange(cout), np.arange(64), indexing="ij")
    pos, plane = w2.image_index(co, ci, f)
    seen = np.zeros(img.size, bool)
    for pl in range(3):
        assert (img[pos + pl * plane] == pieces[pl]).all(), f"plane {pl}"
        seen[pos + pl * plane] = True
    assert seen.all()
    # the lane's view: element j of lane (m, kq) of step s is the channel the kernel's patch reads hand to the B operand
    nw = cb_n = 2
    view = img.reshape(cout // 64, 16, 2, nw, 3, cb_n, 4, 16, 8)                       # [tn][f][s][wv][plane][cb][kq][m][j]
    for s in range(2):
        for kq in range(4):
            for j in range(8):
                c = w2.lane_channel(s, kq, j)
                got = view[:, :, s, :, 0, :, kq, :, j]                                 # [tn][f][wv][cb][m]
                want = pieces[0][:, :, c].reshape(16, cout // 64, nw, cb_n, 16).transpose(1, 0, 2, 3, 4)
                assert (got == want).all(), (s, kq, j)
    assert sorted(w2.lane_channel(s, kq, j) for s in range(2) for kq in range(4) for j in range(8)) == list(range(64))
    # exact sums, on a sample (Fraction is slow)
    h, m, l = xm.split3(U)
    for idx in rng.integers(0, U.size, 2000):
        i = np.unravel_index(idx, U.shape)
        assert Fraction(float(h[i])) + Fraction(float(m[i])) + Fraction(float(l[i])) == Fraction(float(U[i]))


def test_pack_refuses_layers_without_the_form():
    w = np.zeros((64, 9, 64), np.float32); img = np.zeros(16 * 64 * 64 * 3, np.uint16)
    L = fa.lib()
    for cout, cin in ((32, 64), (96, 64), (64, 32), (64, 128)):
        assert L.fh_debug_wino2_pack_x3(w.ctypes.data, cout, cin, img.ctypes.data) < 0
        assert "three-piece" in _lib.last_error()


def pays(workgroups, cus):
    a = np.asarray([workgroups, cus], np.int32); out = np.zeros(1, np.int64)
    assert fa.lib().fh_debug_conv_plan(8, a.ctypes.data, 2, out.ctypes.data, 1) == 1, _lib.last_error()
    return bool(out[0])


@pytest.mark.parametrize("cus", [1, 8, 64, 256, 304])
def test_predicate_is_monotone_and_off_below_its_threshold(cus):
    """wino2_x3_pays(workgroups, CUs): off for an empty launch and up to the threshold, on from there for every larger launch; the
    threshold is three workgroups per two CUs, the smallest launch that was measured (profiles/wino2_x3.md)."""
    answers = [pays(n, cus) for n in range(0, 8 * cus + 2)]
    first = answers.index(True)
    assert first == (3 * cus + 1) // 2 and not any(answers[:first]) and all(answers[first:])
    assert pays(1 << 30, cus)
