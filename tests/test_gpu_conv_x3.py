"""The three-piece bf16 ("x3") K loop of the direct convolution kernel (csrc/conv_mfma.hip: conv_igemm_kernel<.., X3>; gemm_tile.h's
gemm_split3 / gemm_mma_x3) — the form the recogniser's folded-shortcut stride-2 3x3 layers take — held to the exact operand model of
tests/wino_x3_model.py through fh_conv_forward_ex_dev:

  1  one-hot weights, bit for bit: both tile widths, every tap and channel chunk and the shortcut tap, ragged M
  2  dense operands inside a derived bound, one launch per stream-K role (plain tiles / owners and helpers / fix-up kernel)
  3  locality: plants, aggressors, guards on a layer with a shortcut
  4  a small IResNet with the switch on, off, on

The cases and the role each dense case reaches are in tests/conv_x3_cases.py; tests/test_conv_x3_cpu.py checks the roles without a GPU.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402
from oracle import onnx_min, oracle, torch_graph  # noqa: E402
from tests import util                        # noqa: E402
from tests import locality as loc             # noqa: E402
from tests import conv_x3_cases as cx         # noqa: E402
from tests import wino_x3_model as xm         # noqa: E402

NAN = np.float32("nan")
FP32, X3 = 0, 2                                 # FH_PREC_FP32, FH_PREC_F32X3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared operands are read-only)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def weight_image(w9, wsc, cout):
    """w9 [Cout][9][Cin], wsc [Cout][sc] or None -> the kernel's [fh_conv_wt_rows(Cout)][9 Cin + sc] image, k = tap Cin + ci, shortcut last"""
    k9 = w9.shape[1] * w9.shape[2]
    K = k9 + (wsc.shape[1] if wsc is not None else 0)
    img = np.zeros((fa.lib().fh_conv_wt_rows(cout), K), np.float32)
    img[:cout, :k9] = w9.reshape(cout, k9)
    if wsc is not None:
        img[:cout, k9:] = wsc
    return img


def run_layer(c, x_ptr, wd, bd, sc_ptr, out_ptr, precision):
    """one 3x3 stride-2 pad-1 layer of case c (device pointers; wd = the f32 weight image)"""
    rc = fa.lib().fh_conv_forward_ex_dev(x_ptr, wd.data_ptr(), bd.data_ptr() if bd is not None else None, out_ptr, c.B, c.H, c.W, c.Cin,
                                         c.Cout, 3, 2, cx.kpad(c), -1, precision, sc_ptr if c.sc else None, c.H, c.W, c.sc, 2, c.cus, 0)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()


def layer(c, x, img, b, xs, precision):
    """x [B,H,W,Cin], xs [B,H,W,sc] or None (numpy, channels last) -> out [B,Ho,Wo,Cout]"""
    ho, wo = cx.out_hw(c)
    xd, wd = dev(x), dev(img)
    bd = dev(b) if b is not None else None
    sd = dev(xs) if xs is not None else None
    out = torch.full((c.B, ho, wo, c.Cout), float("nan"), device="cuda")
    run_layer(c, xd.data_ptr(), wd, bd, sd.data_ptr() if sd is not None else 0, out.data_ptr(), precision)
    return out.cpu().numpy()


def im2col(c, x, xs):
    """the K-long row every output pixel multiplies: [B, Ho, Wo, 9 Cin + sc], zero where a tap falls on the padding"""
    ho, wo = cx.out_hw(c)
    xp = np.zeros((c.B, c.H + 2, c.W + 2, c.Cin), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    cols = [xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2][:, :ho, :wo] for ky in range(3) for kx in range(3)]
    if xs is not None:
        cols.append(xs[:, 0:2 * ho:2, 0:2 * wo:2][:, :ho, :wo])
    return np.concatenate(cols, axis=3)


# ====================================================================================================== 1: one-hot weights
def one_hot_kk(K, N):
    """the single k of output channel n: chunk n mod (K / 32) — every tap's every 32-channel chunk and the shortcut's — at a position in the
    chunk that walks with n"""
    n = np.arange(N)
    chunks = K // 32
    return 32 * (n % chunks) + (5 * (n // chunks) + 3 * n) % 32


@pytest.mark.parametrize("c", cx.ONE_HOT, ids=lambda c: f"{c.H}x{c.W}-cin{c.Cin}-cout{c.Cout}-sc{c.sc}")
def test_one_hot_weights_bitwise(c):
    """Every output channel has ONE non-zero weight, so an output is one input value times one weight value (or nothing, where the tap lies
    on the padding): with 12 x 12 significand bits it must be the exact product, with 24 x 24 bits — bit for bit — the model's six piece
    products added to a zero accumulator in the documented order (one_hot_chain).  No bias."""
    K = cx.kpad(c)
    kk = one_hot_kk(K, c.Cout)
    assert set(kk // 32) == set(range(K // 32))                            # every (tap, chunk) and the shortcut's chunks
    rng = np.random.default_rng(c.H * 100000 + c.Cin * 1000 + c.Cout + c.sc)
    for cls in "cf":
        xv, wv = xm.one_hot_operands(rng, c.B * c.H * c.W, c.Cin, c.Cout, cls)
        x = xv.reshape(c.B, c.H, c.W, c.Cin)
        xs = xm.one_hot_operands(rng, c.B * c.H * c.W, c.sc, c.Cout, cls)[0].reshape(c.B, c.H, c.W, c.sc) if c.sc else None
        wv = wv[0]
        full = np.zeros((c.Cout, K), np.float32)
        full[np.arange(c.Cout), kk] = wv
        img = weight_image(full[:, :9 * c.Cin].reshape(c.Cout, 9, c.Cin), full[:, 9 * c.Cin:] if c.sc else None, c.Cout)
        got = layer(c, x, img, None, xs, X3)
        v = im2col(c, x, xs)[..., kk]                                      # [B, Ho, Wo, Cout]: the one input value each output sees
        exp = xm.one_hot_chain(v, wv[None, None, None])
        if cls == "c":
            assert (exp.astype(np.float64) == v.astype(np.float64) * wv.astype(np.float64)).all()
        assert (v == 0).any() and (v != 0).any()                           # padded taps and real ones
        bad = np.argwhere(_bits(got) != _bits(exp))
        assert bad.size == 0, (f"class {cls}: {len(bad)} of {got.size} differ, first (b, oy, ox, n) {bad[0]}: got {got[tuple(bad[0])]!r} "
                               f"expected {exp[tuple(bad[0])]!r} k = {kk[bad[0][3]]}")


# ====================================================================================================== 2: dense operands
@functools.lru_cache(maxsize=None)
def dense_operands(role):
    """operands of a dense case and their fp64 reference (computed once, read only): x, xs, w9, wsc, b, ref, S = sum |w x| + |b|"""
    c = cx.DENSE[role]
    rng = np.random.default_rng(c.B * 1000 + c.H * 10 + c.Cin)
    K = cx.kpad(c)
    x = rng.standard_normal((c.B, c.H, c.W, c.Cin)).astype(np.float32)
    xs = rng.standard_normal((c.B, c.H, c.W, c.sc)).astype(np.float32) if c.sc else None
    w9 = (rng.standard_normal((c.Cout, 9, c.Cin)) / np.sqrt(K)).astype(np.float32)
    wsc = (rng.standard_normal((c.Cout, c.sc)) / np.sqrt(K)).astype(np.float32) if c.sc else None
    b = rng.standard_normal(c.Cout).astype(np.float32)

    def conv64(x, xs, w9, wsc, b):
        F = torch.nn.functional
        with torch.no_grad():
            wt = torch.from_numpy(w9.reshape(c.Cout, 3, 3, c.Cin).transpose(0, 3, 1, 2).copy()).double()
            y = F.conv2d(torch.from_numpy(x.transpose(0, 3, 1, 2).copy()).double(), wt, torch.from_numpy(b).double(), stride=2, padding=1)
            if xs is not None:
                y = y + F.conv2d(torch.from_numpy(xs.transpose(0, 3, 1, 2).copy()).double(), torch.from_numpy(wsc[:, :, None, None].copy()).double(), stride=2)
        return y.numpy().transpose(0, 2, 3, 1)

    ref = conv64(x, xs, w9, wsc, b)
    S = conv64(np.abs(x), None if xs is None else np.abs(xs), np.abs(w9), None if wsc is None else np.abs(wsc), np.abs(b))
    for a in (x, xs, w9, wsc, b, ref, S):
        if a is not None:
            a.setflags(write=False)
    return x, xs, w9, wsc, b, ref, S


@pytest.mark.parametrize("role", sorted(cx.DENSE))
def test_dense_within_derived_bound(role):
    """x ~ N(0,1), w ~ N(0,1)/sqrt(K), one launch per stream-K role, against the fp64 convolution (torch).  The bar, with S = sum |w x| + |b|
    per output in fp64, derived as test_gemm_dense_within_derived_bound derives its own:
      * dropped products: the split is exact, the kernel leaves out m l, l m, l l <= (2^-23 + 2^-23 + 2^-32) |w x|: (2^-22 + 2^-32) S;
      * additions: every bf16 x bf16 product is exact in f32 and none passes through more than 6 K + 5 f32 additions inside the K loop, at
        most 3 more where a remainder tile's slabs are summed and 1 for the bias: gamma_(6K+9), on the six terms' magnitudes
        <= (1 + 2 * 2^-7 + 2^-14 + 2 * 2^-16) S < 1.016 S, with the factor 2 of that test for the rounding inside the instruction.
    Beside the bar, printed and used by no assertion: the f32 kernel's own error.  Same bits on a second call; different bits from the f32
    kernel (the x3 kernel really ran)."""
    c = cx.DENSE[role]
    x, xs, w9, wsc, b, ref, S = dense_operands(role)
    K = cx.kpad(c)
    img = weight_image(w9, wsc, c.Cout)
    got = layer(c, x, img, b, xs, X3)
    again = layer(c, x, img, b, xs, X3)
    f32 = layer(c, x, img, b, xs, FP32)
    assert np.isfinite(got).all()
    bound = ((2.0 ** -22 + 2.0 ** -32) + 2 * xm.gamma(6 * K + 9) * 1.016) * S
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    d3, d0 = got - ref, f32 - ref
    print(f"dense conv {role} {tuple(c)}: |x3 - fp64| / bound max {ratio.max():.4f} | x3 - fp64 max {np.abs(d3).max():.3g} rms {np.sqrt((d3 ** 2).mean()):.3g}"
          f" | f32 kernel - fp64 max {np.abs(d0).max():.3g} rms {np.sqrt((d0 ** 2).mean()):.3g}")
    assert ratio.max() <= 1.0, (role, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    assert (_bits(got) == _bits(again)).all()
    assert (_bits(got) != _bits(f32)).any()


def test_layers_without_the_form_are_refused():
    t = torch.zeros(1 << 16, device="cuda")
    L, p = fa.lib(), t.data_ptr()
    for cin, cout in ((16, 64), (32, 96), (48, 64)):
        assert L.fh_conv_forward_ex_dev(p, p, None, p, 1, 8, 8, cin, cout, 3, 2, 9 * cin, -1, X3, None, 0, 0, 0, 0, 0, 0) < 0
        assert "three-piece" in _lib.last_error()
    assert L.fh_conv_forward_ex_dev(p, p, None, p, 1, 8, 8, 32, 64, 3, 2, 288, -1, 1, None, 0, 0, 0, 0, 0, 0) < 0      # FH_PREC_BF16X2: no such form here


# ====================================================================================================== 3: locality
def test_conv_layer_locality_x3():
    """plants (NaN / +-Inf), aggressors, guards, radius 1 — the legs of tests/test_gpu_locality.py on an x3 layer with a shortcut: bitwise
    outside a plant's receptive field, non-finite inside it (the split rule leaves a NaN piece for every non-finite value)."""
    from tests.test_gpu_locality import _single_layer_legs
    c = cx.LOCALITY
    rng = np.random.default_rng(77)
    K = cx.kpad(c)
    x = rng.standard_normal((c.B, c.H, c.W, c.Cin)).astype(np.float32)
    xs = rng.standard_normal((c.B, c.H, c.W, c.sc)).astype(np.float32)
    w9 = (rng.standard_normal((c.Cout, 9, c.Cin)) / np.sqrt(K)).astype(np.float32)
    wsc = (rng.standard_normal((c.Cout, c.sc)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(c.Cout).astype(np.float32)
    wd, bd, sd = dev(weight_image(w9, wsc, c.Cout)), dev(b), dev(xs)
    ho, wo = cx.out_hw(c)
    A = im2col(c, x, xs).astype(np.float64)
    W = np.concatenate([w9.reshape(c.Cout, -1), wsc], axis=1).astype(np.float64)
    ref, S = A @ W.T + b, np.abs(A) @ np.abs(W).T + np.abs(b)

    def launch(xp, _rp, outs):
        run_layer(c, xp, wd, bd, sd.data_ptr(), outs[0], X3)

    def clean_check(clean):
        assert np.isfinite(clean[0]).all()
        bound = ((2.0 ** -22 + 2.0 ** -32) + 2 * xm.gamma(6 * K + 9) * 1.016) * S          # (test_dense_within_derived_bound)
        assert (np.abs(clean[0] - ref) <= bound).all()

    _single_layer_legs("conv x3", x, None, [(c.B, ho, wo, c.Cout)], launch, 2, loc.R_DIRECT3, 3, [True], clean_check)


# ====================================================================================================== 4: a small IResNet
def strided_layers_with_form(g):
    """3x3 stride-2 convolutions of the graph with Cin % 32 == 0 and Cout % 64 == 0 (each carries its block's folded shortcut)"""
    count = 0
    for nd in g.nodes:
        if nd.op != "Conv":
            continue
        cout, cin, kh, kw = g.inits[nd.inputs[1]].shape
        count += (kh, kw) == (3, 3) and tuple(nd.attrs.get("strides", [1, 1])) == (2, 2) and cin % 32 == 0 and cout % 64 == 0
    return count


def test_small_iresnet_with_the_switch_on_off_on(tmp_path):
    """widths (64, 64, 128, 128), 112 x 112, 16 crops: the four stride-2 blocks have the x3 form while the switch is on (fh_rec_get_conv_x3),
    on and off both meet torch fp64 at the chain bar of the fp32 path (2e-4 of scale), on / off / on returns the same bits at each setting.
    With the Winograd form off every other layer is an f32 kernel at either setting, so bits that differ between on and off show that a
    direct x3 launch ran."""
    n, size = 16, 112
    path = models.make_iresnet(str(tmp_path / "x3.onnx"), (1, 1, 1, 1), (64, 64, 128, 128), size, 64, seed=31)
    g = onnx_min.load(path)
    rec = fa.FaceRecognizer()
    assert rec.loadModel(path)
    L = fa.lib()
    crops = util.frames_u8(n, size, size, seed=131)
    cd = dev(crops)

    def raw_out():
        out = torch.zeros((n, 64), device="cuda"); raw = torch.zeros((n, 64), device="cuda")
        assert rec.embed_aligned_dev(cd.data_ptr(), n, out.data_ptr(), raw.data_ptr()) == n
        torch.cuda.synchronize()
        return raw.cpu().numpy()

    want = strided_layers_with_form(g)
    assert want == 4
    was = L.fh_rec_get_wino_x3(rec.handle)
    runs, direct = [], []
    try:
        for on in (1, 0, 1, 0):
            assert L.fh_rec_set_wino_x3(rec.handle, on) >= 0, _lib.last_error()
            assert L.fh_rec_get_conv_x3(rec.handle) == (want if on else 0)
            runs.append(raw_out())
            L.fh_rec_set_winograd(rec.handle, 0)
            direct.append(raw_out())
            L.fh_rec_set_winograd(rec.handle, 1)
    finally:
        L.fh_rec_set_winograd(rec.handle, 1)
        L.fh_rec_set_wino_x3(rec.handle, was)
    on1, off1, on2, off2 = runs
    assert (_bits(on1) == _bits(on2)).all() and (_bits(off1) == _bits(off2)).all()
    assert (_bits(direct[0]) == _bits(direct[2])).all() and (_bits(direct[1]) == _bits(direct[3])).all()
    assert (_bits(direct[0]) != _bits(direct[1])).any()
    tg = torch_graph.TorchGraph(path)
    slots = (0, n // 2, n - 1)
    feeds = {g.inputs[0][0]: np.stack([oracle.rec_preprocess(crops[i]) for i in slots])}
    plain = tg.run(feeds)[g.outputs[0][0]].reshape(len(slots), -1)
    scale = np.abs(plain).max()
    d_on = float(np.abs(on1[list(slots)] - plain).max() / scale)
    d_off = float(np.abs(off1[list(slots)] - plain).max() / scale)
    print(f"small IResNet: x3 on - fp64 {d_on:.3g} of scale, off - fp64 {d_off:.3g}, on - off {np.abs(on1 - off1).max() / scale:.3g}")
    assert d_on <= 2e-4 and d_off <= 2e-4, (d_on, d_off)
