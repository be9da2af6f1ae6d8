"""The three-piece bf16 ("x3") Winograd GEMM — the fp32 mode's default on the recogniser — held to its exact operand model
(tests/wino_x3_model.py), stage by stage:

  X.2  the GEMM stage on one-hot weights, bit for bit      (wino_gemm_x3_kernel<64,2>, <128,2>; wino_gemm_pers_kernel<.., true> through
                                                            fh_debug_wino_slots; uniform and mixed plane layouts)
  X.3  the GEMM stage on dense operands, inside a derived rounding bound; (gpu - fp64) of the x3 and of the f32 kernel measured beside it
  X.4  whole layers against the fp64 convolution at the fp32 Winograd bar, and their locality
  X.5  small IResNets with the switch on, off, on

tests/test_wino_x3_model_cpu.py pins the model and shows the power of the bars of X.2 / X.3.
"""
import hashlib

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
from tests import wino_x3_model as xm         # noqa: E402
from tests.test_gpu_parity import dev         # noqa: E402

NAN = np.float32("nan")
X3 = 2                                          # FH_PREC_F32X3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ====================================================================================================== the GEMM stage alone
# (B, H, W) of the uniform rows: 4 x 4 maps, one tile per image.  300 tiles pad every plane to 512 rows.  N = 64 / 192 and, at these
# sizes, N = 128 run the 128 x 64 tile; 2048 tiles x 128 columns (576 row tiles: at least one 128 x 128 tile per workgroup slot of a 256-CU part)
# run the 128 x 128 tile.
GEMM_SHAPES = [(K, N, tiles) for K in (32, 64, 160) for N in (64, 128, 192) for tiles in (256, 300)]
WIDE = (64, 128, 2048)
MIXED = (64, 14, 14, 128, 128)                                         # B, H, W, K, N: 100 planes, 292 row tiles
WALKS = [(160, 128, 300), (64, 64, 300)]                               # under fh_debug_wino_slots(8): <128,2,true> and <64,2,true>, 18 / 36 tiles per workgroup


def _gemm_gpu(V, U, B, H, W, K, N, precision, mixed):
    """V [rows, K], U [36, N, K] (numpy f32) -> M [rows, N]; rows come from the library's own count"""
    L = fa.lib()
    rows = L.fh_debug_wino_gemm_rows(B, H, W, K, N, mixed)
    assert rows == V.shape[0], (rows, V.shape, _lib.last_error())
    Up = np.zeros((36, L.fh_conv_wt_rows(N), K), np.float32)
    Up[:, :N] = U
    vd, ud = dev(V), dev(Up)
    md = torch.full((rows, N), float("nan"), device="cuda")
    rc = L.fh_debug_wino_gemm_dev(vd.data_ptr(), ud.data_ptr(), md.data_ptr(), B, H, W, K, N, precision, mixed, 0)
    assert rc == 0, _lib.last_error()
    return md.cpu().numpy()


def _planes(B, H, W, mixed):
    return xm.mixed_planes(B, H, W) if mixed else xm.uniform_planes(B * ((H + 3) // 4) * ((W + 3) // 4))


def _spread(planes, Vreal, K, pad):
    """Vreal [real rows of all planes, K] -> the full V with `pad` in the padded rows of every plane"""
    V = np.full((planes[-1][0] + planes[-1][2], K), pad, np.float32)
    o = 0
    for r0, real, _, _ in planes:
        V[r0:r0 + real] = Vreal[o:o + real]
        o += real
    return V


def _one_hot_case(B, H, W, K, N, mixed):
    planes = _planes(B, H, W, mixed)
    nreal = sum(p[1] for p in planes)
    rng = np.random.default_rng(K * 1000 + N + B)
    kk = xm.one_hot_kk(K, N)
    assert set(np.unique(kk)) == set(range(K))
    f, n = np.meshgrid(np.arange(36), np.arange(N), indexing="ij")
    for cls in "cf":
        Vreal, wv = xm.one_hot_operands(rng, nreal, K, N, cls)
        assert xm.pieces_ok(Vreal).all() and xm.pieces_ok(wv).all()
        U = np.zeros((36, N, K), np.float32)
        U[f, n, kk] = wv
        V = _spread(planes, Vreal, K, NAN)                             # padded rows of every plane are NaN
        got = _gemm_gpu(V, U, B, H, W, K, N, X3, mixed)
        for r0, real, _, fq in planes:                                 # every real row of every plane
            v = V[r0:r0 + real][:, kk[fq]]                             # [real, N]: the one V value each output sees
            exp = xm.one_hot_chain(v, wv[fq][None])
            if cls == "c":                                             # 12 x 12 bits: the exact product
                assert (exp.astype(np.float64) == v.astype(np.float64) * wv[fq][None].astype(np.float64)).all()
            g = got[r0:r0 + real]
            bad = np.argwhere(_bits(g) != _bits(exp))
            assert bad.size == 0, (f"class {cls} plane at row {r0} (frequency {fq}): {len(bad)} of {g.size} differ, first (row, n) "
                                   f"{bad[0]}: got {g[tuple(bad[0])]!r} expected {exp[tuple(bad[0])]!r} k = {kk[fq][bad[0][1]]}")


@pytest.mark.parametrize("K,N,tiles", GEMM_SHAPES + [WIDE])
def test_gemm_one_hot_weights_bitwise(K, N, tiles):
    """U[f][n][:] holds one value w(f, n) at k = kk(f, n) and zeros, so M[row][n] is built from ONE V value and ONE weight value: with
    12 x 12 significand bits the result must be the exact product; with 24 x 24 bits it must be, bit for bit, the model's six piece
    products added to a zero accumulator in the documented order (one_hot_chain).  kk walks every k, a different walk per frequency.
    Every real row of every plane is compared; at 300 tiles rows 300 .. 511 of every plane of V are NaN."""
    _one_hot_case(tiles, 4, 4, K, N, 0)


def test_gemm_one_hot_weights_bitwise_mixed_layout():
    """The mixed F(4x4) / F(2x2) plane layout (100 planes in four classes): the weight values differ per frequency, so a wrong
    plane -> frequency lookup shows in every row tile of that plane."""
    B, H, W, K, N = MIXED
    _one_hot_case(B, H, W, K, N, 1)


@pytest.mark.parametrize("K,N,tiles", WALKS)
def test_gemm_one_hot_weights_bitwise_multi_tile_walk(K, N, tiles):
    """fh_debug_wino_slots(8): eight workgroups walk all tiles of the launch (wino_gemm_pers_kernel with the x3 step, both tile shapes)"""
    L = fa.lib()
    try:
        assert L.fh_debug_wino_slots(8) == 0
        _one_hot_case(tiles, 4, 4, K, N, 0)
    finally:
        L.fh_debug_wino_slots(0)


MEASURED = []


def _dense_case(B, H, W, K, N, mixed, pad_check):
    planes = _planes(B, H, W, mixed)
    nreal = sum(p[1] for p in planes)
    bound_c = 2 * xm.gamma(6 * K + 5)
    for kind in ("normal", "positive"):
        rng = np.random.default_rng(K * 1000 + N + B + (kind == "positive"))
        Vreal, U = xm.dense_operands(rng, nreal, K, N, kind)
        for a in (Vreal, U):
            assert all(xm.is_bf16_normal(p).all() for p in xm.split3(a))                        # no zero or subnormal piece reaches the MFMA
            assert kind == "normal" or all((p > 0).all() for p in xm.split3(a))
        V0 = _spread(planes, Vreal, K, 0.0)
        got = _gemm_gpu(V0, U, B, H, W, K, N, X3, mixed)
        f32 = _gemm_gpu(V0, U, B, H, W, K, N, 0, mixed)
        if pad_check:
            got_nan = _gemm_gpu(_spread(planes, Vreal, K, NAN), U, B, H, W, K, N, X3, mixed)
        worst, o, d3, d0 = 0.0, 0, [], []
        for r0, real, _, fq in planes:
            v = Vreal[o:o + real]
            M, S = xm.gemm_model(v, U[fq])
            ref = v.astype(np.float64) @ U[fq].astype(np.float64).T
            o += real
            g = got[r0:r0 + real].astype(np.float64)
            assert np.isfinite(g).all()
            ratio = np.abs(g - M) / (bound_c * S)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (kind, r0, fq, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
            d3.append((g - ref).ravel()); d0.append((f32[r0:r0 + real] - ref).ravel())
            if pad_check:                                              # NaN in the padded rows of V changes no bit of a real row of M
                assert (_bits(got_nan[r0:r0 + real]) == _bits(got[r0:r0 + real])).all(), (kind, r0)
        d3, d0 = np.concatenate(d3), np.concatenate(d0)
        line = (f"dense GEMM K={K} N={N} rows={nreal} {kind}: |gpu - model| / (2 gamma_(6K+5) S) = {worst:.4f} | x3 - fp64 max {np.abs(d3).max():.3g} "
                f"rms {np.sqrt((d3 ** 2).mean()):.3g} | f32 kernel - fp64 max {np.abs(d0).max():.3g} rms {np.sqrt((d0 ** 2).mean()):.3g}")
        MEASURED.append(line)
        print(line)


@pytest.mark.parametrize("K,N,tiles", GEMM_SHAPES + [WIDE])
def test_gemm_dense_within_derived_bound(K, N, tiles):
    """V ~ N(0,1), U ~ N(0,1)/sqrt(K), and a second set with every value and every piece positive.  The bar: every bf16 x bf16 product is
    exact in f32, so the kernel's only roundings are those of ADDING: per output 6 K products — each v_mfma_f32_32x32x16_bf16 adds its 16
    products and the accumulator, 6 K / 16 instructions in a chain — plus the 5 accumulator hand-overs between the six MFMAs of a step.
    However the instruction orders its 16-deep additions, no product passes through more than 6K + 5 f32 additions, so
    |M - model| <= gamma_{6K+5} S with S the sum of the six terms' magnitudes; the factor 2 covers the undocumented rounding of the additions
    INSIDE the instruction (not round-to-nearest: see one_hot_chain), as in the split-bf16 and gallery tests.
    Beside the bar, MEASURED and used by no assertion: max and rms of (gpu - fp64) for the x3 kernel and for the native f32 kernel on the
    same operands (docs/tolerances.md)."""
    _dense_case(tiles, 4, 4, K, N, 0, tiles == 300)


def test_gemm_dense_within_derived_bound_mixed_layout():
    B, H, W, K, N = MIXED
    _dense_case(B, H, W, K, N, 1, True)


def test_gemm_hook_refuses_layers_without_the_form():
    t = torch.zeros(36 * 256 * 128, device="cuda")
    assert fa.lib().fh_debug_wino_gemm_dev(t.data_ptr(), t.data_ptr(), t.data_ptr(), 256, 4, 4, 32, 96, X3, 0, 0) < 0
    assert fa.lib().fh_debug_wino_gemm_dev(t.data_ptr(), t.data_ptr(), t.data_ptr(), 256, 4, 4, 32, 64, 3, 0, 0) < 0


# ====================================================================================================== whole layers
LAYER_CASES = [
    # B, H,  W,  Cin, Cout        (the cases of tests/test_gpu_wino_bf16x2.py)
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
def test_layer_against_fp64_at_the_fp32_winograd_bar(B, H, W, Cin, Cout):
    """fh_conv_winograd_ex_dev(precision = 2) against the fp64 direct convolution at the Winograd layer bar of the fp32 path, 2e-4 abs /
    2e-5 rms; the result differs in bits from precision 0 (the kernel really ran) and is the same bits on a second call."""
    x, w, b = layer_operands(B, H, W, Cin, Cout)
    ref = conv_fp64(x, w, b)
    got = _layer_gpu(x, w, b, X3)
    again = _layer_gpu(x, w, b, X3)
    f32 = _layer_gpu(x, w, b, 0)
    assert np.isfinite(got).all()
    dmax, drms = float(np.abs(got - ref).max()), float(np.sqrt(((got - ref) ** 2).mean()))
    print(f"layer {(B, H, W, Cin, Cout)}: x3 - fp64 max {dmax:.3g} rms {drms:.3g} | f32 kernels - fp64 max {np.abs(f32 - ref).max():.3g} "
          f"rms {np.sqrt(((f32 - ref) ** 2).mean()):.3g} | x3 - f32 kernels max {np.abs(got - f32).max():.3g}")
    assert dmax <= 2e-4 and drms <= 2e-5, (dmax, drms)
    assert (_bits(got) != _bits(f32)).any()
    assert (_bits(got) == _bits(again)).all()
    assert np.abs(f32 - ref).max() <= 2e-4


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 14, 14, 256, 256), (64, 14, 14, 128, 64)], ids=["uniform", "mixed"])
def test_winograd_layer_locality_x3(B, H, W, Cin, Cout):
    """plants (NaN / +-Inf), aggressors, guards, radius 4 — the legs of tests/test_gpu_locality.py for precision 2: bitwise outside the
    radius, non-finite inside a plant's receptive field; the clean run at the fp32 Winograd bar."""
    from tests.test_gpu_locality import _single_layer_legs
    x, w, b = layer_operands(B, H, W, Cin, Cout)
    ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1))
    bd = dev(b)
    ref = conv_fp64(x, w, b)

    def launch(xp, _rp, outs):
        rc = fa.lib().fh_conv_winograd_ex_dev(xp, ohwi.ctypes.data, bd.data_ptr(), outs[0], B, H, W, Cin, Cout, X3, 0)
        assert rc == 0, _lib.last_error()

    def clean_check(clean):
        got = clean[0].transpose(0, 3, 1, 2)
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= 2e-4 and np.sqrt(((got - ref) ** 2).mean()) <= 2e-5

    _single_layer_legs("winograd F(4x4) x3", np.ascontiguousarray(x.transpose(0, 2, 3, 1)), None, [(B, H, W, Cout)], launch, 1, loc.R_WINO4, 3,
                       [True], clean_check)


# ====================================================================================================== small IResNets
CHAINS = [
    # name, layers, widths, size, batch, seed            (two chains of tests/test_gpu_wino_bf16x2.py)
    ("mixed-roles", (1, 1, 2, 1), (32, 64, 128, 128), 112, 64, 9),        # wino_mix_kernel in its three roles
    ("sliced-28x28", (1, 3, 1, 1), (32, 128, 128, 128), 112, 24, 21),     # wino_slice_kernel
]
# sha256 of the raw outputs [n][64] (f32 bytes) with the switch OFF, recorded from the library of the commit before this kernel existed
PARENT_SHA256 = {
    "mixed-roles": "f4cbf1bc3e2b9cacc6fe2e5dd545ccee3c3ca4bb91e589815126f610d4602c97",
    "sliced-28x28": "8c89cc648fd566b5e24b6ad8c1db2be1b1f6f7fc2fcbb3002f1de267388a4e7e",
}


@pytest.mark.parametrize("name,layers,widths,size,n,seed", CHAINS, ids=[c[0] for c in CHAINS])
def test_chain_with_the_switch_on_off_on(tmp_path, name, layers, widths, size, n, seed):
    """A small IResNet through the recogniser: x3 on (the default) and off both meet torch fp64 at the chain bar of the fp32 path (2e-4 of
    scale: the additive part of the split-bf16 chain bar, whose model term is zero for an fp32 path); on, off, on gives the same bits each
    time it returns to a setting; and OFF reproduces, bit for bit, what the library computed before this kernel existed (PARENT_SHA256:
    recorded once by running the parent commit's library on the same crops; only the hashes are kept)."""
    path = models.make_iresnet(str(tmp_path / f"{name}.onnx"), layers, widths, size, 64, seed=seed)
    g = onnx_min.load(path)
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

    was = L.fh_rec_get_wino_x3(rec.handle)
    runs = []
    try:
        for on in (1, 0, 1, 0):
            layers_x3 = L.fh_rec_set_wino_x3(rec.handle, on)
            assert layers_x3 == (layers_with_form(g) if on else 0), (layers_x3, _lib.last_error())
            assert L.fh_rec_get_wino_x3(rec.handle) == on and L.fh_rec_get_precision(rec.handle) == 0
            runs.append(raw_out())
    finally:
        L.fh_rec_set_wino_x3(rec.handle, was)
    on1, off1, on2, off2 = runs
    assert (_bits(on1) == _bits(on2)).all() and (_bits(off1) == _bits(off2)).all()
    assert (_bits(on1) != _bits(off1)).any()
    sha = hashlib.sha256(np.ascontiguousarray(off1, np.float32).tobytes()).hexdigest()
    tg = torch_graph.TorchGraph(path)
    slots = (0, n // 2, n - 1)
    feeds = {g.inputs[0][0]: np.stack([oracle.rec_preprocess(crops[i]) for i in slots])}
    plain = tg.run(feeds)[g.outputs[0][0]].reshape(len(slots), -1)
    scale = np.abs(plain).max()
    d_on = float(np.abs(on1[list(slots)] - plain).max() / scale)
    d_off = float(np.abs(off1[list(slots)] - plain).max() / scale)
    print(f"chain {name}: x3 on - fp64 {d_on:.3g} of scale, off - fp64 {d_off:.3g}, on - off {np.abs(on1 - off1).max() / scale:.3g}; sha256(off) = {sha}")
    assert d_on <= 2e-4 and d_off <= 2e-4, (d_on, d_off)
    assert sha == PARENT_SHA256[name], sha


def layers_with_form(g):
    """convolutions of the graph that have the x3 form: 3x3, stride 1, pad 1, Cin >= 128, Cin % 32 == 0, Cout % 64 == 0"""
    count = 0
    for nd in g.nodes:
        if nd.op != "Conv":
            continue
        cout, cin, kh, kw = g.inits[nd.inputs[1]].shape
        st, pd = nd.attrs.get("strides", [1, 1]), nd.attrs.get("pads", [0] * 4)
        count += (kh, kw) == (3, 3) and tuple(st) == (1, 1) and tuple(pd[:2]) == (1, 1) and cin >= 128 and cin % 32 == 0 and cout % 64 == 0
    return count
