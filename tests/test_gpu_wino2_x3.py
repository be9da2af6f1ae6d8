"""The three-piece bf16 ("x3") form of the fused Winograd F(2x2, 3x3) layer (csrc/conv_wino2.hip: wino2_x3_kernel) held to the model of
tests/wino2_x3_model.py through the single-layer entry point fh_conv_wino2_prec_dev:

  1  one non-zero input channel per output channel, bit for bit: the exact convolution (12 x 12 bits), the model (24 x 24 bits)
  2  dense operands against the fp64 direct convolution: PReLU + residual + nine bias classes, and the second output
  3  locality at radius 2, with a residual
  4  layers without the form are refused
  5  a small IResNet with the recogniser's switch on / off / on / off"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402
from oracle import oracle, onnx_min, torch_graph  # noqa: E402
from tests import util                        # noqa: E402
from tests import locality as loc             # noqa: E402
from tests import wino2_x3_model as w2        # noqa: E402
from tests.test_wino2_x3_cpu import direct_conv, one_hot_layer  # noqa: E402

FP32, X3 = 0, 2                                 # FH_PREC_FP32, FH_PREC_F32X3
# (B, H, W, Cout): one partly empty tile group / whole groups / odd sizes, two groups a side, two column tiles / three column tiles
CASES = [(1, 2, 2, 64), (2, 8, 8, 64), (3, 9, 7, 128), (2, 10, 13, 192)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared operands are read-only)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def run_layer(shape, x_ptr, w, out_ptr, precision, bias=None, slope=None, res_ptr=None, out2_ptr=None, s2=None, t2=None, act=0, bias_cls=0):
    B, H, W, N = shape
    rc = fa.lib().fh_conv_wino2_prec_dev(x_ptr, w.ctypes.data, _ptr(bias), _ptr(slope), res_ptr, out_ptr, out2_ptr, _ptr(s2), _ptr(t2), B, H, W, 64, N,
                                         act, bias_cls, precision, 1, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()


def layer(shape, x, w, precision, **kw):
    xd = dev(x)
    out = torch.full(shape, float("nan"), device="cuda")
    run_layer(shape, xd.data_ptr(), w, out.data_ptr(), precision, **kw)
    return out.cpu().numpy()


# ====================================================================================================== 1: one-hot weights
@pytest.mark.parametrize("B,H,W,N", CASES, ids=lambda v: str(v))
def test_one_hot_weights_bitwise(B, H, W, N):
    """Output channel n reads input channel (7 n + 3) mod 64 alone, so every MFMA adds one non-zero product.  Class c (integers of
    12 x 12 bits and fewer): every step is exact and the layer is the exact convolution, +0 where it is zero (the channels 0 mod 8 are all
    zero, and the padding adds +0).  Class f (24 x 24 bits, one tap per filter): bit for bit the model — V in the kernel's order of
    additions, the split, the six products in the documented order, y_update in frequency order."""
    rng = np.random.default_rng(1000 * B + 100 * H + 10 * W + N)
    for cls in "cf":
        x, w, cin_of = one_hot_layer(rng, B, H, W, N, cls)
        exp = w2.layer_one_hot(x, w, cin_of)
        if cls == "c":
            exact = direct_conv(x, w)
            assert (exp.astype(np.float64) == exact).all()
            assert (exact == 0).any() and (exact != 0).any()
        got = layer((B, H, W, N), x, w, X3)
        bad = np.argwhere(_bits(got) != _bits(exp))
        assert bad.size == 0, (f"class {cls}: {len(bad)} of {got.size} differ, first (b, y, x, n) {bad[0]}: got {got[tuple(bad[0])]!r} "
                               f"expected {exp[tuple(bad[0])]!r} cin = {cin_of[bad[0][3]]}")


# ====================================================================================================== 2: dense operands
@functools.lru_cache(maxsize=None)
def dense_operands(B, H, W, N):
    """x, w, the nine bias vectors, slope, residual, s2, t2 and the fp64 references (computed once, read only)"""
    rng = np.random.default_rng(B * 1000 + H * 100 + W * 10 + N)
    x = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    w = (rng.standard_normal((N, 9, 64)) / np.sqrt(9 * 64)).astype(np.float32)
    b9 = rng.standard_normal((9, N)).astype(np.float32)
    slope = rng.uniform(0.1, 0.4, N).astype(np.float32)
    r = rng.standard_normal((B, H, W, N)).astype(np.float32)
    s2 = rng.uniform(0.5, 1.5, N).astype(np.float32)
    t2 = rng.standard_normal(N).astype(np.float32)
    bias = b9.astype(np.float64)[w2.bias_classes(H, W)]                             # [H][W][N]
    y = direct_conv(x, w) + bias
    y = np.where(y >= 0, y, y * slope.astype(np.float64)) + r
    y2 = y * s2.astype(np.float64) + t2
    extra = np.abs(bias) + np.abs(r)
    bound = w2.dense_bound(x, w, extra)
    bound2 = bound * s2 + 2.0 ** -23 * (np.abs(y) * s2 + np.abs(t2))               # (out2: one rounding of out1, one multiply-add)
    out = (x, w, b9, slope, r, s2, t2, y, y2, bound, bound2)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("B,H,W,N", CASES, ids=lambda v: str(v))
def test_dense_within_the_bars(B, H, W, N):
    """x ~ N(0,1), w ~ N(0,1) / sqrt(576) (O(1) outputs) through PReLU + residual + nine bias classes + the second output, against the fp64
    direct convolution: within the documented bars of this layer form (docs/tolerances.md: 5e-5 abs, 1e-4 on the second output) AND within
    the bound derived in tests/wino2_x3_model.py (dense_bound).  PReLU's slope is below 1: it never grows an error.  Same bits on a second
    call; other bits than the f32 kernel (the x3 kernel really ran)."""
    x, w, b9, slope, r, s2, t2, y, y2, bound, bound2 = dense_operands(B, H, W, N)
    shape = (B, H, W, N)
    xd, rd = dev(x), dev(r)
    kw = dict(bias=dev(b9), slope=dev(slope), res_ptr=rd.data_ptr(), s2=dev(s2), t2=dev(t2), act=2, bias_cls=1)

    def run(precision):
        o1 = torch.full(shape, float("nan"), device="cuda"); o2 = torch.full(shape, float("nan"), device="cuda")
        run_layer(shape, xd.data_ptr(), w, o1.data_ptr(), precision, out2_ptr=o2.data_ptr(), **kw)
        return o1.cpu().numpy(), o2.cpu().numpy()

    got, got2 = run(X3)
    again, again2 = run(X3)
    f32, f32_2 = run(FP32)
    assert np.isfinite(got).all() and np.isfinite(got2).all()
    e1, e2 = np.abs(got - y), np.abs(got2 - y2)
    print(f"dense wino2 x3 {shape}: |x3 - fp64| max {e1.max():.3g} (second output {e2.max():.3g}), of the derived bound {(e1 / bound).max():.4f} "
          f"({(e2 / bound2).max():.4f}) | f32 kernel - fp64 max {np.abs(f32 - y).max():.3g} ({np.abs(f32_2 - y2).max():.3g})")
    assert e1.max() <= 5e-5 and e2.max() <= 1e-4, (float(e1.max()), float(e2.max()))
    assert (e1 <= bound).all() and (e2 <= bound2).all()
    assert (_bits(got) == _bits(again)).all() and (_bits(got2) == _bits(again2)).all()
    assert (_bits(got) != _bits(f32)).any()


# ====================================================================================================== 3: locality
def test_wino2_x3_locality():
    """plants (NaN / +-Inf), aggressors, guards at radius 2 — the legs of tests/test_gpu_locality.py on (3, 9, 7, 128) with a residual and no
    activation: bitwise outside a plant's radius, non-finite inside it."""
    from tests.test_gpu_locality import _single_layer_legs
    B, H, W, N = shape = (3, 9, 7, 128)
    x, w, b9, _, r, _, _, _, _, bound, _ = dense_operands(*shape)
    bd = dev(b9[4])
    ref = direct_conv(x, w) + b9[4].astype(np.float64) + r

    def launch(xp, rp, outs):
        run_layer(shape, xp, w, outs[0], X3, bias=bd, res_ptr=rp)

    def clean_check(clean):
        e = np.abs(clean[0] - ref)
        assert e.max() <= 5e-5 and (e <= bound).all(), float(e.max())

    _single_layer_legs("wino2 x3", np.array(x), np.array(r), [shape], launch, 1, loc.R_WINO2, 3, [True], clean_check)


# ====================================================================================================== 4: refusals
def test_layers_without_the_form_are_refused():
    t = torch.zeros(1 << 16, device="cuda")
    L, p = fa.lib(), t.data_ptr()
    w = np.zeros((192, 9, 64), np.float32)

    def call(cin, cout, prec=X3, out=p):
        return L.fh_conv_wino2_prec_dev(p, w.ctypes.data, None, None, None, out, None, None, None, 1, 4, 4, cin, cout, 0, 0, prec, 1, None)

    for cin, cout in ((32, 64), (128, 64), (64, 32), (64, 30), (64, 96)):        # Cin != 64; Cout % 64 != 0 (30: the merged heads' width)
        assert call(cin, cout) < 0
        assert "no three-piece bf16 form" in _lib.last_error(), (cin, cout)
    assert call(64, 64, prec=1) < 0                                              # FH_PREC_BF16X2: no such form here
    assert call(64, 64, out=None) < 0                                            # no output
    # (merged outputs — Cout <= 32, the 30 above — exist on fh_conv_wino2_ex_dev alone, which has no precision argument)
    assert call(64, 64) == 0, _lib.last_error()
    assert call(64, 64, prec=FP32) == 0, _lib.last_error()
    torch.cuda.synchronize()


# ====================================================================================================== 5: a small IResNet
def test_small_iresnet_with_the_switch_on_off_on_off(tmp_path):
    """widths (64, 64, 128, 128), 112 x 112, 16 crops, planned for 8 CUs: the stride-1 3x3 layers of the first three stages (64 -> 64 on 112 x
    112 and 56 x 56, 64 -> 128 on 28 x 28) have the form (fh_rec_get_wino2_x3 > 0 while the switch is on, 0 while off) and launches that
    wino2_x3_pays admits.  Returning to a setting restores its bits; on differs from off; both meet torch fp64 at the chain bar of the fp32
    path (2e-4 of scale).  FACEHIP_WINO2_X3 is expected unset."""
    n, size = 16, 112
    path = models.make_iresnet(str(tmp_path / "w2x3.onnx"), (1, 1, 1, 1), (64, 64, 128, 128), size, 64, seed=37)
    g = onnx_min.load(path)
    rec = fa.FaceRecognizer()
    assert rec.loadModel(path)
    L = fa.lib()
    assert L.fh_rec_set_cus(rec.handle, 8) == 0
    crops = util.frames_u8(n, size, size, seed=137)
    cd = dev(crops)

    def raw_out():
        out = torch.zeros((n, 64), device="cuda"); raw = torch.zeros((n, 64), device="cuda")
        assert rec.embed_aligned_dev(cd.data_ptr(), n, out.data_ptr(), raw.data_ptr()) == n, _lib.last_error()
        torch.cuda.synchronize()
        return raw.cpu().numpy()

    was = L.fh_rec_get_wino_x3(rec.handle)
    runs = []
    try:
        for on in (1, 0, 1, 0):
            assert L.fh_rec_set_wino_x3(rec.handle, on) >= 0, _lib.last_error()
            assert (L.fh_rec_get_wino2_x3(rec.handle) > 0) == bool(on)
            runs.append(raw_out())
    finally:
        L.fh_rec_set_wino_x3(rec.handle, was)
    on1, off1, on2, off2 = runs
    assert (_bits(on1) == _bits(on2)).all() and (_bits(off1) == _bits(off2)).all()
    assert (_bits(on1) != _bits(off1)).any()
    tg = torch_graph.TorchGraph(path)
    slots = (0, n // 2, n - 1)
    feeds = {g.inputs[0][0]: np.stack([oracle.rec_preprocess(crops[i]) for i in slots])}
    plain = tg.run(feeds)[g.outputs[0][0]].reshape(len(slots), -1)
    scale = np.abs(plain).max()
    d_on = float(np.abs(on1[list(slots)] - plain).max() / scale)
    d_off = float(np.abs(off1[list(slots)] - plain).max() / scale)
    print(f"small IResNet: wino2 x3 on - fp64 {d_on:.3g} of scale, off - fp64 {d_off:.3g}, on - off {np.abs(on1 - off1).max() / scale:.3g}")
    assert d_on <= 2e-4 and d_off <= 2e-4, (d_on, d_off)
