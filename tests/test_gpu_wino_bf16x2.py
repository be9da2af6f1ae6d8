"""The split-bf16 ("bf16x2") Winograd path held to an exact operand model (tests/wino_split_model.py), stage by stage:

  C.1  the pack format, bit for bit                                          (wino_pack_bf16x2 through pack_bf16x2_kernel)
  C.2  the GEMM stage on one-hot weights, bit for bit                        (wino_gemm_bf16x2_kernel<64,3>; the f32 kernels with class c)
  C.3  the GEMM stage on dense operands, inside a derived rounding bound
  C.4  one whole layer against the fp64 convolution, bar from the model      (wino_input_kernel / wino_mix_kernel packing V)
  C.5  chains in which the producer of V and its reader must agree           (Net::run: bf2 / pack_next; wino_fused / wino_slice / wino_mix)

tests/test_wino_split_model_cpu.py pins the model and shows that a kernel which loses a cross term, adds mid*mid back, exchanges the
halves or two k positions is far outside the bars of C.2 / C.3.  Bars of C.4 / C.5 are computed in the test from the reference side only
(e = model - fp64); measured deviations are recorded in docs/tolerances.md, not used.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402
from oracle import onnx_min, oracle, torch_graph  # noqa: E402
from tests import util                        # noqa: E402
from tests import wino_split_model as wm      # noqa: E402
from tests.test_gpu_parity import dev, pack_weights  # noqa: E402

NAN = np.float32("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ====================================================================================================== C.1 the pack format
def _pack_gpu(words):
    x = dev(words.view(np.float32))
    out = torch.zeros_like(x)
    rc = fa.lib().fh_debug_pack_bf16x2_dev(x.data_ptr(), out.data_ptr(), x.numel())
    assert rc == 0, _lib.last_error()
    return _bits(out.cpu().numpy())


def test_pack_format_is_the_model_bit_for_bit():
    """4096 words: the crafted edge words of the model + seeded random bit patterns (finite, |x| < 2^127, hi and mid zero or bf16-normal).
    The kernel's word must be split()'s word.  Subnormal halves are left out: whether the conversion flushes them is a mode, not a format."""
    crafted = wm.crafted_words()
    words = np.concatenate([crafted, wm.random_words(np.random.default_rng(20), 4096 - crafted.size)])
    assert words.size == 4096
    got = _pack_gpu(words)
    _, _, ref = wm.split(words.view(np.float32))
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, [(hex(int(words[i])), hex(int(got[i])), hex(int(ref[i]))) for i in bad[:8]]
    t = torch.zeros(8, device="cuda")
    assert fa.lib().fh_debug_pack_bf16x2_dev(t.data_ptr(), t.data_ptr(), 6) < 0                # n % 4 == 0 is the contract


def test_pack_keeps_non_finite_values_non_finite():
    """NaN, +-Inf and the finite values that round to a bf16 infinity (|x| >= 0x7F7F8000 -> (Inf, -Inf)): the unpacked hi + mid is not
    finite — such a value cannot turn into an ordinary number on its way through the format."""
    words = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF,
                      0x7F7F8001, 0x7FA00000], np.uint32)
    got = _pack_gpu(words)
    hi, mid = wm.unpack(got)
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(hi + mid).any(), [(hex(int(w)), hex(int(g))) for w, g in zip(words, got)]
    fin = np.isin(words, np.array([0x7F7F8000, 0x7F7FFFFF, 0x7F7F8001], np.uint32))
    assert (got[fin] == 0xFF807F80).all(), [hex(int(g)) for g in got[fin]]                    # (+Inf, -Inf), as the kernel's comment states


# ====================================================================================================== the GEMM stage alone
# (B, H, W) of the uniform rows: 4 x 4 maps, one tile per image.  300 tiles pad every plane to 512 rows.
GEMM_SHAPES = [(K, N, tiles) for K in (32, 64, 160, 256) for N in (64, 192) for tiles in (256, 300)]
MIXED = (64, 14, 14, 128, 128)                                         # B, H, W, K, N: 100 planes, 292 row tiles


def _gemm_gpu(V, U, B, H, W, K, N, precision, mixed):
    """V [rows, K], U [36, N, K] (numpy f32) -> M [rows, N]; rows come from the library's own count"""
    L = fa.lib()
    rows = L.fh_debug_wino_gemm_rows(B, H, W, K, N, mixed)
    assert rows == V.shape[0], (rows, V.shape, _lib.last_error())
    wt_rows = L.fh_conv_wt_rows(N)
    Up = np.zeros((36, wt_rows, K), np.float32)
    Up[:, :N] = U
    vd, ud = dev(V), dev(Up)
    md = torch.full((rows, N), float("nan"), device="cuda")
    rc = L.fh_debug_wino_gemm_dev(vd.data_ptr(), ud.data_ptr(), md.data_ptr(), B, H, W, K, N, precision, mixed, 0)
    assert rc == 0, _lib.last_error()
    return md.cpu().numpy()


def _planes(B, H, W, mixed):
    return wm.mixed_planes(B, H, W) if mixed else wm.uniform_planes(B * ((H + 3) // 4) * ((W + 3) // 4))


def _spread(planes, Vreal, K, pad):
    """Vreal [real rows of all planes, K] -> the full V with `pad` in the padded rows of every plane"""
    rows = planes[-1][0] + planes[-1][2]
    V = np.full((rows, K), pad, np.float32)
    o = 0
    for r0, real, _, _ in planes:
        V[r0:r0 + real] = Vreal[o:o + real]
        o += real
    return V


def _one_hot_case(B, H, W, K, N, mixed, precision, classes):
    planes = _planes(B, H, W, mixed)
    nreal = sum(p[1] for p in planes)
    rng = np.random.default_rng(K * 1000 + N + B)
    kk = wm.one_hot_kk(K, N)
    assert set(np.unique(kk)) == set(range(K))
    f, n = np.meshgrid(np.arange(36), np.arange(N), indexing="ij")
    for cls in classes:
        Vreal, wv, _ = wm.one_hot_operands(rng, nreal, K, N, cls)
        U = np.zeros((36, N, K), np.float32)
        U[f, n, kk] = wv
        V = _spread(planes, Vreal, K, NAN)                             # padded rows of every plane are NaN
        got = _gemm_gpu(V, U, B, H, W, K, N, precision, mixed)
        for r0, real, _, fq in planes:
            v = V[r0:r0 + real][:, kk[fq]]                             # [real, N]: the one V value each output sees
            exp = wm.one_hot_expected(v, wv[fq][None]) if precision else v.astype(np.float64) * wv[fq][None]
            e32 = exp.astype(np.float32)
            assert (e32.astype(np.float64) == exp).all()               # the expected value is exact in f32
            g = got[r0:r0 + real]
            bad = np.argwhere(_bits(g) != _bits(e32))
            assert bad.size == 0, (f"class {cls} plane at row {r0} (frequency {fq}): {len(bad)} of {g.size} differ, first (row, n) "
                                   f"{bad[0]}: got {g[tuple(bad[0])]!r} expected {e32[tuple(bad[0])]!r} k = {kk[fq][bad[0][1]]}")


@pytest.mark.parametrize("K,N,tiles", GEMM_SHAPES)
def test_gemm_one_hot_weights_bitwise(K, N, tiles):
    """U[f][n][:] holds one value w(f, n) at k = kk(f, n) and zeros: M[row][n] is the three-term product of V[row][kk] and w whatever the
    order of summation, and the operand classes make it exact in f32 (a: 16-bit V x 8-bit w isolates uh*vm; b: 8 x 16 isolates um*vh;
    c: 12 x 12 gives v*w - vm*wm, not the product: exactly three terms).  kk walks every k, a different walk per frequency.  At 300 tiles
    the rows 300 .. 511 of every plane of V are NaN and the real rows must still be exact."""
    _one_hot_case(tiles, 4, 4, K, N, 0, 1, "abc")


def test_gemm_one_hot_weights_bitwise_mixed_layout():
    """The mixed F(4x4) / F(2x2) plane layout (100 planes in four classes): the weight values differ per frequency, so a wrong
    plane -> frequency lookup shows in every row tile of that plane."""
    B, H, W, K, N = MIXED
    _one_hot_case(B, H, W, K, N, 1, 1, "abc")
    _one_hot_case(B, H, W, K, N, 1, 0, "c")


@pytest.mark.parametrize("K,N,tiles", GEMM_SHAPES + [(64, 96, 300), (32, 128, 1536)])
def test_gemm_one_hot_weights_bitwise_f32_kernels(K, N, tiles):
    """precision = 0 with class c operands: one f32 product of two 12-bit values is exact and order-free too.  N = 64 / 192 run
    wino_gemm_kernel<64,3>, N = 96 runs <32,4>, and 1536 tiles x 128 columns (432 row tiles: one round of 128 x 128 tiles against two of
    128 x 64) run <128,2>."""
    _one_hot_case(tiles, 4, 4, K, N, 0, 0, "c")


def _dense_case(B, H, W, K, N, mixed, pad_check):
    planes = _planes(B, H, W, mixed)
    nreal = sum(p[1] for p in planes)
    bound_c = 2 * wm.gamma(3 * K + 2)
    for kind in ("normal", "positive"):
        rng = np.random.default_rng(K * 1000 + N + B + (kind == "positive"))
        Vreal, U = wm.dense_operands(rng, nreal, K, N, kind)
        for a in (Vreal, U):
            hi, mid, _ = wm.split(a)
            assert wm.is_bf16_normal(hi).all() and wm.is_bf16_normal(mid).all()              # no subnormal half reaches the MFMA
            assert kind == "normal" or ((hi > 0).all() and (mid > 0).all())
        got = _gemm_gpu(_spread(planes, Vreal, K, 0.0), U, B, H, W, K, N, 1, mixed)
        if pad_check:
            got_nan = _gemm_gpu(_spread(planes, Vreal, K, NAN), U, B, H, W, K, N, 1, mixed)
        worst, o = 0.0, 0
        for r0, real, _, fq in planes:
            M, S = wm.gemm_model(Vreal[o:o + real], U[fq])
            o += real
            g = got[r0:r0 + real].astype(np.float64)
            assert np.isfinite(g).all()
            ratio = np.abs(g - M) / (bound_c * S)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (kind, r0, fq, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
            if pad_check:                                              # NaN in the padded rows of V changes no bit of a real row of M
                assert (_bits(got_nan[r0:r0 + real]) == _bits(got[r0:r0 + real])).all(), (kind, r0)
        print(f"dense GEMM K={K} N={N} rows={nreal} {kind}: max |gpu - model| / (2 gamma_(3K+2) S) = {worst:.4f}")


@pytest.mark.parametrize("K,N,tiles", GEMM_SHAPES)
def test_gemm_dense_within_derived_bound(K, N, tiles):
    """V ~ N(0,1), U ~ N(0,1)/sqrt(K), and a second set with every value and every mid positive (a lost cross term is coherent there).
    Every bf16 x bf16 product is exact in f32, so the kernel's only roundings are those of adding 3K terms (+ 2 for the accumulator
    hand-over between the three MFMAs of a step): |M - model| <= gamma_{3K+2} S for ANY order of f32 additions; the factor 2 covers the
    undocumented rounding of the additions inside the instruction, as in the gallery tests."""
    _dense_case(tiles, 4, 4, K, N, 0, tiles == 300)


def test_gemm_dense_within_derived_bound_mixed_layout():
    B, H, W, K, N = MIXED
    _dense_case(B, H, W, K, N, 1, True)


@pytest.mark.parametrize("K", (32, 160))
def test_conv_pw_and_wino_gemm_give_one_bit_pattern(K):
    """conv_pw_kernel and wino_gemm_kernel run the same tile body (gemm_tile.h) and add every output's products in the same order: with
    K % 32 == 0, no bias and no activation, a 1x1 convolution over 9216 rows is the GEMM of the uniform Winograd layout of 256 tiles
    (36 planes x 256 rows) whose 36 frequencies all carry the same weight matrix.  K = 32 is one chunk, 160 an odd number of chunks;
    B = 36 maps of 16 x 16 give 72 x 4 tiles of 128 x 64, at least one per CU, so the convolution takes conv_pw_kernel.  Equality of
    VALUES: the epilogue's + 0 may turn a -0 into +0."""
    N, tiles = 256, 256
    rng = np.random.default_rng(7000 + K)
    V = rng.standard_normal((36 * tiles, K)).astype(np.float32)
    Wm = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    wino = _gemm_gpu(V, np.broadcast_to(Wm, (36, N, K)), tiles, 4, 4, K, N, 0, 0)
    wp, kpad = pack_weights(Wm[:, :, None, None])
    assert kpad == K
    xd, wd = dev(V), dev(wp)
    out = torch.full((36 * tiles, N), float("nan"), device="cuda")
    rc = fa.lib().fh_conv_forward_dev(xd.data_ptr(), wd.data_ptr(), None, out.data_ptr(), 36, 16, 16, K, N, 1, 1, kpad, -1, 0)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    conv = out.cpu().numpy()
    assert np.isfinite(wino).all() and np.abs(wino).max() > 1.0
    bad = np.argwhere(conv != wino)
    assert np.array_equal(conv, wino), (len(bad), bad[:4], conv[tuple(bad[0])], wino[tuple(bad[0])])


def test_gemm_hook_checks_its_arguments():
    L = fa.lib()
    assert L.fh_debug_wino_gemm_rows(256, 4, 4, 32, 64, 0) == 36 * 256 and L.fh_debug_wino_gemm_rows(300, 4, 4, 32, 64, 0) == 36 * 512
    assert L.fh_debug_wino_gemm_rows(64, 14, 14, 128, 128, 1) == 128 * 292
    assert L.fh_debug_wino_gemm_rows(2, 14, 14, 128, 128, 1) < 0 and "mixed" in _lib.last_error()       # B < 64: uniform tiling
    assert L.fh_debug_wino_gemm_rows(256, 4, 4, 48, 64, 0) < 0
    t = torch.zeros(36 * 256 * 128, device="cuda")
    assert L.fh_debug_wino_gemm_dev(t.data_ptr(), t.data_ptr(), t.data_ptr(), 256, 4, 4, 32, 96, 1, 0, 0) < 0
    assert "no split-bf16 GEMM" in _lib.last_error()
    assert L.fh_debug_wino_gemm_dev(t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 14, 14, 128, 128, 1, 1, 0) < 0


# ====================================================================================================== C.4 one whole layer
LAYER_CASES = [
    # B, H,  W,  Cin, Cout
    (2, 14, 14, 256, 256),       # base shape
    (2, 13, 10, 128, 64),        # ragged map
    (3, 7, 7, 512, 128),         # 7x7 stage
    (64, 14, 14, 128, 64),       # mixed tiling
    (70, 13, 14, 64, 128),       # mixed tiling, ragged
]


def layer_operands(B, H, W, Cin, Cout):
    rng = np.random.default_rng(B * 1000 + H * 10 + Cin)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    return x, w, b


def conv_fp64(x, w, b):
    with torch.no_grad():
        return torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                                          padding=1).numpy()


def layer_bars(x, w, b, ref):
    """(max bar, rms bar, max|e|, rms(e)) with e = split model - fp64: 3 max|e| + 2e-4 and 2 rms(e) + 2e-5.  The additive parts are the
    fp32 Winograd bars; the factors allow for the kernel's V differing from the model's by an f32 ulp before it is packed."""
    e = wm.conv_model(x, w, b) - ref
    emax, erms = float(np.abs(e).max()), float(np.sqrt((e ** 2).mean()))
    return 3 * emax + 2e-4, 2 * erms + 2e-5, emax, erms


def _layer_gpu(x, w, b, precision):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1))
    xd, bd = dev(x.transpose(0, 2, 3, 1)), dev(b)
    out = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    rc = fa.lib().fh_conv_winograd_ex_dev(xd.data_ptr(), ohwi.ctypes.data, bd.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, precision, 0)
    assert rc == 0, _lib.last_error()
    return out.cpu().numpy().transpose(0, 3, 1, 2)


@pytest.mark.parametrize("B,H,W,Cin,Cout", LAYER_CASES)
def test_layer_against_fp64_with_the_bar_from_the_model(B, H, W, Cin, Cout):
    x, w, b = layer_operands(B, H, W, Cin, Cout)
    ref = conv_fp64(x, w, b)
    bar_max, bar_rms, emax, erms = layer_bars(x, w, b, ref)
    got = _layer_gpu(x, w, b, 1)
    f32 = _layer_gpu(x, w, b, 0)
    assert np.isfinite(got).all()
    dmax, drms = float(np.abs(got - ref).max()), float(np.sqrt(((got - ref) ** 2).mean()))
    print(f"layer {(B, H, W, Cin, Cout)}: model - fp64 max {emax:.3g} rms {erms:.3g} | gpu - fp64 max {dmax:.3g} rms {drms:.3g} "
          f"(bars {bar_max:.3g} / {bar_rms:.3g}) | fp32 path - fp64 max {np.abs(f32 - ref).max():.3g}")
    assert dmax <= bar_max and drms <= bar_rms, (dmax, bar_max, drms, bar_rms)
    assert (_bits(got) != _bits(f32)).any()                            # the mode really ran
    assert np.abs(f32 - ref).max() < 2e-4                              # and precision = 0 is the fp32 path (its own bar)


def test_layer_without_a_split_form_is_refused():
    x, w, b = layer_operands(2, 8, 8, 128, 96)
    out = torch.zeros((2, 8, 8, 96), device="cuda")
    ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1))
    rc = fa.lib().fh_conv_winograd_ex_dev(dev(x.transpose(0, 2, 3, 1)).data_ptr(), ohwi.ctypes.data, dev(b).data_ptr(), out.data_ptr(),
                                          2, 8, 8, 128, 96, 1, 0)
    assert rc < 0 and "no split-bf16 GEMM" in _lib.last_error()
    assert np.abs(_layer_gpu(x, w, b, 0) - conv_fp64(x, w, b)).max() < 2e-4       # the fp32 form of the same layer is fine


# ====================================================================================================== C.5 chains
CHAINS = [
    # name, layers, widths, size, batch, seed
    ("mixed-roles", (1, 1, 2, 1), (32, 64, 128, 128), 112, 64, 9),        # wino_mix_kernel in its three roles, packing
    ("sliced-28x28", (1, 3, 1, 1), (32, 128, 128, 128), 112, 24, 21),     # wino_slice_kernel
    ("to-ineligible", (1, 1, 2, 2), (32, 64, 128, 160), 112, 64, 33),     # eligible -> ineligible: pack_next false, <32,4> after a packed layer
    ("to-eligible", (1, 1, 2, 2), (32, 64, 160, 128), 112, 64, 34),       # ineligible -> eligible: an f32 layer writes packed V
]


def _eligible(wshape, stride, pads):
    cout, cin, kh, kw = wshape
    return (kh, kw) == (3, 3) and tuple(stride) == (1, 1) and tuple(pads[:2]) == (1, 1) and cin >= 128 and cin % 32 == 0 and cout % 64 == 0


def _model_run(tg, feeds, batch, patched):
    """the fp64 graph with F.conv2d replaced by conv_model on the convolutions the engine runs split at `batch`; patched collects them"""
    F = torch_graph.F
    real = F.conv2d

    def conv2d(x, w, b=None, stride=1, padding=0, groups=1, **kw):
        st = (stride, stride) if isinstance(stride, int) else tuple(stride)
        pd = (padding, padding) if isinstance(padding, int) else tuple(padding)
        H, W = x.shape[2], x.shape[3]
        if groups == 1 and _eligible(tuple(w.shape), st, pd) and batch * ((H + 3) // 4) * ((W + 3) // 4) >= 256:
            patched.append(tuple(w.shape) + (H, W))
            return torch.from_numpy(wm.conv_model(x.numpy(), w.numpy(), None if b is None else b.numpy()))
        return real(x, w, b, stride=stride, padding=padding, groups=groups, **kw)

    F.conv2d = conv2d
    try:
        return tg.run(feeds)
    finally:
        F.conv2d = real


@pytest.mark.parametrize("name,layers,widths,size,n,seed", CHAINS, ids=[c[0] for c in CHAINS])
def test_chain_producer_and_reader_of_v_agree(tmp_path, name, layers, widths, size, n, seed):
    path = models.make_iresnet(str(tmp_path / f"{name}.onnx"), layers, widths, size, 64, seed=seed)
    g = onnx_min.load(path)
    convs = [nd for nd in g.nodes if nd.op == "Conv"]
    count = sum(_eligible(g.inits[nd.inputs[1]].shape, nd.attrs.get("strides", [1, 1]), nd.attrs.get("pads", [0] * 4)) for nd in convs)
    assert count >= 2, count
    rec = fa.FaceRecognizer()
    assert rec.loadModel(path)
    L = fa.lib()
    crops = util.frames_u8(n, size, size, seed=seed + 100)
    cd = dev(crops)

    def raw_out():
        out = torch.zeros((n, 64), device="cuda"); raw = torch.zeros((n, 64), device="cuda")
        assert rec.embed_aligned_dev(cd.data_ptr(), n, out.data_ptr(), raw.data_ptr()) == n
        torch.cuda.synchronize()
        return raw.cpu().numpy()

    try:
        fp32 = raw_out()
        worst = C.c_float(0)
        got_layers = L.fh_rec_set_precision(rec.handle, 1, C.byref(worst))
        assert got_layers == count, (got_layers, count, _lib.last_error())
        split = {}
        for fusion in (1, 0):
            assert L.fh_rec_set_wino_fusion(rec.handle, fusion) == 0
            split[fusion] = raw_out()
        assert L.fh_rec_set_wino_fusion(rec.handle, 1) == 0
        assert L.fh_rec_set_precision(rec.handle, 0, None) == 0
        assert (_bits(raw_out()) == _bits(fp32)).all()                 # back to the fp32 bits
    finally:
        L.fh_rec_set_wino_fusion(rec.handle, 1)
        L.fh_rec_set_precision(rec.handle, 0, None)
    assert (_bits(split[1]) != _bits(fp32)).any()

    tg = torch_graph.TorchGraph(path)
    slots = (0, n // 2, n - 1)
    feeds = {g.inputs[0][0]: np.stack([oracle.rec_preprocess(crops[i]) for i in slots])}
    plain = tg.run(feeds)[g.outputs[0][0]].reshape(len(slots), -1)
    patched = []
    model = _model_run(tg, feeds, n, patched)[g.outputs[0][0]].reshape(len(slots), -1)
    assert 1 <= len(patched) <= count, patched
    scale = np.abs(plain).max()
    e = float(np.abs(model - plain).max() / scale)
    bar = 3 * e + 2e-4
    devs = {f: float(np.abs(split[f][list(slots)] - plain).max() / scale) for f in (1, 0)}
    between = float(np.abs(split[1] - split[0]).max() / np.abs(split[1]).max())
    print(f"chain {name}: {count} eligible layers, {len(patched)} run split at B = {n}; model - fp64 {e:.3g} of scale (bar {bar:.3g}); "
          f"gpu - fp64 fused {devs[1]:.3g} unfused {devs[0]:.3g}; fused - unfused {between:.3g}; fp32 path - fp64 "
          f"{np.abs(fp32[list(slots)] - plain).max() / scale:.3g}; gate 1 - cos {worst.value:.3g}")
    assert devs[1] <= bar and devs[0] <= bar, (devs, bar)
    assert between <= bar, (between, bar)
