"""The three-piece bf16 ("x3") form of the 1x1 stride-1 convolutions (csrc/conv_mfma.hip: conv_pw_x3_kernel; gemm_tile.h's gemm_split3 /
gemm_mma_x3 / gemm_load_chunk_x3) held to the exact operand model of tests/wino_x3_model.py through the single-layer entry point
(fh_conv_forward_ex_dev; fh_conv_forward_ep_dev is the same call with the epilogue's activation and residual):

  1  one-hot weights, bit for bit: one chunk, K tails of 8 and 24 floats, nine chunks, all three tile widths — with NaN planted where a
     K tail would read on if its columns did not come from the zero line
  2  dense operands inside a derived bound, with bias + ReLU and with a residual; same bits twice, other bits than the f32 kernel
  3  locality: plants, aggressors, guards on a layer with a K tail
  4  layers without the form are refused
  5  a small SCRFD with the detector's switch on, off, on
  6  a small MobileFaceNet with the recogniser's switch on, off, on

`cus` = 1 or 2 everywhere: the form wants a tile per CU, and the layers here have two to ten tiles."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402
from oracle import oracle              # noqa: E402
from tests import util                        # noqa: E402
from tests import locality as loc             # noqa: E402
from tests import wino_x3_model as xm         # noqa: E402

FP32, X3 = 0, 2                                 # FH_PREC_FP32, FH_PREC_F32X3
PW_X3 = 6                                       # question 6 of fh_debug_conv_plan
# (M, K, N): one chunk / a K tail of 8 floats in chunk 3 and padded columns / a tail of 24 / nine chunks and the N = 288 tiling / a tail of 8
# in chunk 2 on 64-wide tiles
SHAPES = [(128, 32, 32), (256, 72, 152), (256, 152, 152), (256, 288, 288), (128, 40, 64)]
HW = 8                                          # every layer is B = M / 64 images of 8 x 8 pixels


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared operands are read-only)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kpad(K):
    return -(-K // 32) * 32


def weight_image(w):
    """w [N][K] -> the kernel's [fh_conv_wt_rows(N)][kpad(K)] image, zero behind N and K"""
    N, K = w.shape
    img = np.zeros((fa.lib().fh_conv_wt_rows(N), kpad(K)), np.float32)
    img[:N, :K] = w
    return img


def plan_width(M, K, N, cus):
    a = np.asarray([M // (HW * HW), HW, HW, K, N, 1, 1, 0, 0, 0, cus], np.int32)
    out = np.zeros(3, np.int64)
    assert fa.lib().fh_debug_conv_plan(PW_X3, a.ctypes.data, 11, out.ctypes.data, 3) == 3, _lib.last_error()
    return int(out[0])


def run_layer(M, K, N, x_ptr, wd, bd, out_ptr, precision, act=0, res_ptr=None, cus=1):
    rc = fa.lib().fh_conv_forward_ep_dev(x_ptr, wd.data_ptr(), bd.data_ptr() if bd is not None else None, out_ptr, M // (HW * HW), HW, HW, K, N,
                                         1, 1, kpad(K), -1, precision, None, 0, 0, 0, 0, cus, act, res_ptr, 0)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()


def layer(M, K, N, x, img, b, precision, act=0, res=None):
    """x [M, K], img = weight_image(w), b [N] or None, res [M, N] or None (numpy) -> out [M, N]"""
    xd, wd = dev(x), dev(img)
    bd = dev(b) if b is not None else None
    rd = dev(res) if res is not None else None
    out = torch.full((M, N), float("nan"), device="cuda")
    run_layer(M, K, N, xd.data_ptr(), wd, bd, out.data_ptr(), precision, act, rd.data_ptr() if rd is not None else None)
    return out.cpu().numpy()


def test_shapes_reach_every_tile_width():
    """the five shapes run on 32-, 64- and 96-wide x3 tiles between them, each with at least a tile per CU at cus = 1"""
    widths = {s: plan_width(*s, 1) for s in SHAPES}
    assert all(widths.values()), widths
    assert widths[(256, 288, 288)] == 96 and widths[(128, 40, 64)] == 64 and widths[(128, 32, 32)] == 32, widths


# ====================================================================================================== 1: one-hot weights
@pytest.mark.parametrize("M,K,N", SHAPES, ids=lambda v: str(v))
def test_one_hot_weights_bitwise(M, K, N):
    """Every output channel n has ONE non-zero weight, at k = (7 n + 3) mod K — every k of every chunk, the tail's included, is some
    channel's — so an output is one input value times one weight value: with 12 x 12 significand bits the exact product, with 24 x 24 bits,
    bit for bit, the model's six piece products added to a zero accumulator in the documented order.  No bias.
    The zero-line rule: the float4 columns behind K in the last chunk of pixel row m are, in memory, the first kpad(K) - K channels of row
    m + 1.  Every odd row gets NaN there.  Those are real inputs of the odd rows (all their outputs must be NaN — a NaN times a zero weight
    is a NaN: the values were read where they belong) and no input of the even rows, whose outputs must be the clean run's bits."""
    kk = (7 * np.arange(N) + 3) % K
    assert set(kk) == set(range(K)) or N < K
    assert set(kk // 32) == set(range(kpad(K) // 32))
    tail = kpad(K) - K
    rng = np.random.default_rng(M * 100000 + K * 1000 + N)
    for cls in "cf":
        x, wv = xm.one_hot_operands(rng, M, K, N, cls)
        wv = wv[0]
        w = np.zeros((N, K), np.float32)
        w[np.arange(N), kk] = wv
        exp = xm.one_hot_chain(x[:, kk], wv[None])
        if cls == "c":
            assert (exp.astype(np.float64) == x[:, kk].astype(np.float64) * wv.astype(np.float64)).all()
        xp = x.copy()
        xp[1::2, :tail] = np.nan
        poisoned = np.zeros((M, N), bool)
        poisoned[1::2] = tail > 0
        assert poisoned.any() == (tail > 0)
        got = layer(M, K, N, xp, weight_image(w), None, X3)
        assert np.isnan(got[poisoned]).all(), "a planted NaN was not read by its own pixel"
        bad = np.argwhere((_bits(got) != _bits(exp)) & ~poisoned)
        assert bad.size == 0, (f"class {cls}: {len(bad)} of {got.size} differ, first (m, n) {bad[0]}: got {got[tuple(bad[0])]!r} "
                               f"expected {exp[tuple(bad[0])]!r} k = {kk[bad[0][1]]}")


# ====================================================================================================== 2: dense operands
@functools.lru_cache(maxsize=None)
def dense_operands(M, K, N):
    """x, w, b, r and the fp64 products (computed once, read only): y = x w^T + b and S = |x| |w|^T + |b|"""
    rng = np.random.default_rng(M * 1000 + K * 10 + N)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    r = rng.standard_normal((M, N)).astype(np.float32)
    y = x.astype(np.float64) @ w.astype(np.float64).T + b
    S = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T + np.abs(b)
    for a in (x, w, b, r, y, S):
        a.setflags(write=False)
    return x, w, b, r, y, S


@pytest.mark.parametrize("form", ["bias_relu", "residual"])
@pytest.mark.parametrize("M,K,N", SHAPES, ids=lambda v: str(v))
def test_dense_within_derived_bound(M, K, N, form):
    """x ~ N(0,1), w ~ N(0,1)/sqrt(K), against fp64.  The bar, with S = sum |w x| + |b| per output in fp64, derived as
    tests/test_gpu_conv_x3.py derives its own:
      * dropped products: the split is exact, the kernel leaves out m l, l m, l l <= (2^-23 + 2^-23 + 2^-32) |w x|: (2^-22 + 2^-32) S;
      * additions: every bf16 x bf16 product is exact in f32 and none passes through more than 6 K f32 additions inside the K loop (the
        columns behind K add exact zeros), 1 for the bias and 1 for the residual: gamma_(6K+2), on the six terms' magnitudes
        <= (1 + 2 * 2^-7 + 2^-14 + 2 * 2^-16) S < 1.016 S, with the factor 2 of that test for the rounding inside the instruction.
    ReLU is exact and never grows an error.  Beside the bar, printed and used by no assertion: the f32 kernel's own error.  Same bits on a
    second call; different bits from the f32 kernel (the x3 kernel really ran)."""
    x, w, b, r, y, S = dense_operands(M, K, N)
    act, res = (1, None) if form == "bias_relu" else (0, r)
    ref = np.maximum(y, 0.0) if act else y + r
    img = weight_image(w)
    got = layer(M, K, N, x, img, b, X3, act, res)
    again = layer(M, K, N, x, img, b, X3, act, res)
    f32 = layer(M, K, N, x, img, b, FP32, act, res)
    assert np.isfinite(got).all()
    bound = ((2.0 ** -22 + 2.0 ** -32) + 2 * xm.gamma(6 * K + 2) * 1.016) * S
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    d3, d0 = got - ref, f32 - ref
    print(f"dense 1x1 {form} {(M, K, N)}: |x3 - fp64| / bound max {ratio.max():.4f} | x3 - fp64 max {np.abs(d3).max():.3g} rms {np.sqrt((d3 ** 2).mean()):.3g}"
          f" | f32 kernel - fp64 max {np.abs(d0).max():.3g} rms {np.sqrt((d0 ** 2).mean()):.3g}")
    assert ratio.max() <= 1.0, (form, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    if act:
        assert (got == 0).any() and (got > 0).any()
    assert (_bits(got) == _bits(again)).all()
    assert (_bits(got) != _bits(f32)).any()


# ====================================================================================================== 3: locality
def test_pw_layer_locality_x3():
    """plants (NaN / +-Inf), aggressors, guards, radius 0 — the legs of tests/test_gpu_locality.py on an x3 1x1 layer with a K tail of 8
    floats (4 images of 8 x 8 pixels, 72 -> 152 channels, two row tiles): bitwise outside a plant's own pixel, non-finite inside it."""
    from tests.test_gpu_locality import _single_layer_legs
    M, K, N = 256, 72, 152
    B = M // (HW * HW)
    x, w, b, _, y, S = dense_operands(M, K, N)
    wd, bd = dev(weight_image(w)), dev(b)

    def launch(xp, _rp, outs):
        run_layer(M, K, N, xp, wd, bd, outs[0], X3, cus=2)

    def clean_check(clean):
        assert np.isfinite(clean[0]).all()
        bound = ((2.0 ** -22 + 2.0 ** -32) + 2 * xm.gamma(6 * K + 2) * 1.016) * S          # (test_dense_within_derived_bound)
        assert (np.abs(clean[0].reshape(M, N) - y) <= bound).all()

    _single_layer_legs("pw x3", np.array(x).reshape(B, HW, HW, K), None, [(B, HW, HW, N)], launch, 1, loc.R_1X1, 1, [True], clean_check)


# ====================================================================================================== 4: refusals
def test_layers_without_the_form_are_refused():
    t = torch.zeros(1 << 16, device="cuda")
    L, p = fa.lib(), t.data_ptr()

    def call(batch, cin, cout, ks=1, stride=1, kp=None, cus=1, prec=X3):
        return L.fh_conv_forward_ex_dev(p, p, None, p, batch, 8, 8, cin, cout, ks, stride, kp if kp is not None else kpad(ks * ks * cin), -1, prec,
                                        None, 0, 0, 0, 0, cus, 0)

    for cin, cout in ((30, 64), (34, 32), (32, 30), (64, 150)):            # cin % 4, or a Cout the form has no width for
        assert call(2, cin, cout) < 0
        assert "three-piece" in _lib.last_error(), (cin, cout)
    assert call(3, 32, 64) < 0 and "three-piece" in _lib.last_error()      # 192 rows: no whole 128-row tiles
    assert call(2, 32, 64, cus=64) < 0 and "three-piece" in _lib.last_error()   # one tile for 64 CUs
    assert call(2, 32, 64, stride=2) < 0 and "three-piece" in _lib.last_error()
    assert call(2, 32, 96, ks=3, stride=2) < 0 and "three-piece" in _lib.last_error()      # what ksize = 3 refused before, it still refuses
    assert call(2, 16, 64, ks=3, stride=2) < 0 and "three-piece" in _lib.last_error()
    assert call(2, 32, 64) == 0, _lib.last_error()                          # ... and the form itself is accepted
    assert call(2, 32, 64, prec=1) < 0                                      # FH_PREC_BF16X2: no such form here
    torch.cuda.synchronize()


# ====================================================================================================== 5: a small SCRFD
def _read_dev(ptr, shape):
    out = np.empty(shape, np.float32)
    assert fa.lib().fh_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0, _lib.last_error()
    return out


def _det_outputs(det, n):
    import ctypes as C
    outs = []
    for i in range(fa.lib().fh_det_num_outputs(det.handle)):
        r, c = C.c_int(), C.c_int()
        p = fa.lib().fh_det_output_dev(det.handle, i, C.byref(r), C.byref(c))
        outs.append(_read_dev(p, (n, r.value, c.value)))
    return outs


def test_small_scrfd_with_the_switch_on_off_on(models_dir):
    """The tiny SCRFD of test_scrfd_network_and_postprocess (640 x 640), eight frames, planned for 8 CUs: at that batch its 20 x 20 x 48 -> 48
    layer (two chunks, 50 tiles) is one conv_pw_x3_pays admits — the one-chunk 1x1s stay on the f32 kernel at either setting.  Off: the f32
    kernels — the same bytes from this handle and from a second one that was switched off before its first run.  On: other bytes (an x3
    launch ran), the same on the second "on", and the nine heads within the standing 1e-4 abs / rel of the oracle (one frame: the oracle
    is the slow side).  fh_det_get_x3 = the number of layers that have the form while on, 0 while off."""
    L = fa.lib()
    path = util.tiny_scrfd(models_dir, hw=None, cls_bias=-2.0)
    n = 8
    frames = util.frames_u8(n, 640, 640, seed=5, smooth=True)
    d = dev(frames)

    def run(det):
        assert L.fh_det_run_network_dev(det.handle, d.data_ptr(), n, 640, 640, 640 * 3, 640 * 640 * 3, 0) == n, _lib.last_error()
        torch.cuda.synchronize()
        return _det_outputs(det, n)

    det = fa.FaceDetector()
    assert det.loadModel(path)
    assert L.fh_det_set_cus(det.handle, 8) == 0
    layers = L.fh_det_set_x3(det.handle, 1)
    assert layers > 0, _lib.last_error()
    assert L.fh_det_get_x3(det.handle) == layers
    on1 = run(det)
    assert L.fh_det_set_x3(det.handle, 0) == 0 and L.fh_det_get_x3(det.handle) == 0
    off = run(det)
    assert L.fh_det_set_x3(det.handle, 1) == layers and L.fh_det_get_x3(det.handle) == layers
    on2 = run(det)
    other = fa.FaceDetector()
    assert other.loadModel(path)
    assert L.fh_det_set_cus(other.handle, 8) == 0 and L.fh_det_set_x3(other.handle, 0) == 0
    off_other = run(other)
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(on1, on2))
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(off, off_other))
    assert any((_bits(a) != _bits(b)).any() for a, b in zip(on1, off)), "no x3 launch ran: conv_pw_x3_pays admitted no layer of this graph"
    odet = oracle.OracleDetector()
    assert odet.loadModel(path)
    inp, _ = oracle.det_preprocess(frames[5], 640, 640)
    ref = odet.run_network(inp)
    for i in range(9):
        np.testing.assert_allclose(on1[i][5], ref[i], rtol=1e-4, atol=1e-4, err_msg=f"x3 on, output {i}")
        np.testing.assert_allclose(off[i][5], ref[i], rtol=1e-4, atol=1e-4, err_msg=f"x3 off, output {i}")
    print("small SCRFD: x3 on - off max", max(float(np.abs(a - b).max()) for a, b in zip(on1, off)), "layers", layers)


# ====================================================================================================== 6: a small MobileFaceNet
def test_small_mobilefacenet_with_the_switch_on_off_on(models_dir):
    """A small MobileFaceNet (blocks (1, 1, 1, 1), 64 base channels, 128-d), two crops, planned for 8 CUs: its 1x1 expansions have the form
    while the recogniser's switch (fh_rec_set_wino_x3) is on — fh_rec_get_pw_x3 — and the two-chunk one on the 56 x 56 map (64 -> 64 channels,
    49 tiles of 128 rows) is a launch conv_pw_x3_pays admits.  On and off both meet the oracle at the standing 1e-4 abs / rel,
    on / off / on returns the bits of the first "on", and on differs from off in bits (an x3 launch ran)."""
    L = fa.lib()
    n, size = 2, 112
    path = models.make_mobilefacenet(os.path.join(models_dir, "m_small_64.onnx"), (1, 1, 1, 1), 64, size, 128, seed=5)
    rec = fa.FaceRecognizer()
    assert rec.loadModel(path)
    assert L.fh_rec_set_cus(rec.handle, 8) == 0
    dim = rec.feature_dim()
    crops = util.frames_u8(n, size, size, seed=131)
    cd = dev(crops)

    def raw_out():
        out = torch.zeros((n, dim), device="cuda"); raw = torch.zeros((n, dim), device="cuda")
        assert rec.embed_aligned_dev(cd.data_ptr(), n, out.data_ptr(), raw.data_ptr()) == n, _lib.last_error()
        torch.cuda.synchronize()
        return raw.cpu().numpy()

    was = L.fh_rec_get_pw_x3(rec.handle) > 0 or L.fh_rec_get_wino_x3(rec.handle)
    runs = []
    try:
        for on in (1, 0, 1):
            assert L.fh_rec_set_wino_x3(rec.handle, on) >= 0, _lib.last_error()
            assert (L.fh_rec_get_pw_x3(rec.handle) > 0) == bool(on)
            runs.append(raw_out())
    finally:
        L.fh_rec_set_wino_x3(rec.handle, 1 if was else 0)
    on1, off, on2 = runs
    assert (_bits(on1) == _bits(on2)).all()
    assert (_bits(on1) != _bits(off)).any(), "no x3 launch ran: conv_pw_x3_pays admitted no layer of this graph"
    orec = oracle.OracleRecognizer()
    assert orec.loadModel(path)
    for i in range(n):                                                       # test_tiny_mobilefacenet_embeddings' bar
        r = oracle.run_graph(orec.g, {orec.g.inputs[0][0]: oracle.rec_preprocess(crops[i])[None]})[orec.g.outputs[0][0]].reshape(-1)
        np.testing.assert_allclose(on1[i], r, rtol=1e-4, atol=1e-4, err_msg="x3 on")
        np.testing.assert_allclose(off[i], r, rtol=1e-4, atol=1e-4, err_msg="x3 off")
    print(f"small MobileFaceNet: x3 on - off max {np.abs(on1 - off).max():.3g} of {np.abs(off).max():.3g}")
