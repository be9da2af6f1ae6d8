"""Locality / isolation on the GPU: values outside an output's receptive field must not reach it.

Every other GPU test feeds finite values in tight allocations whose surroundings are zero, so a border tap masked by a multiply, a
fragment read across a batch boundary, a halo read that runs off a tensor or a row-end dword that picks up pitch padding all return
exactly the right numbers.  Here the surroundings are hostile.  Each leg is DIFFERENTIAL and BITWISE (uint32 compare, no tolerance): a
dirty run differs from the clean run only where the result may not depend on it —

  (a) plants      NaN / +Inf / -Inf at the fixed positions of locality.plant_list; outside the allowed set (Chebyshev radius R of the
                  convolution form around each plant, locality.allowed_mask — at most (2R+1)^2 exempted pixels per plant) the output is
                  the clean run's; layers without activation also prove the poison was read (every output whose direct receptive field
                  holds a plant is non-finite);
  (b) aggressors  every element of every non-victim image is NaN; the victims' outputs are the clean run's.  Behind a ReLU a NaN image
                  is an all-zero map (`v > 0 ? v : 0`), the value of zero padding, so the graph legs run a second aggressor set that
                  survives it (locality.hostile_images: large noise with sparse +Inf pixels), and every aggressor run asserts that
                  the aggressor images' own outputs changed — something hostile did arrive;
  (c) guards      tensors sit in [guard | tensor | guard] allocations (>= 64 KiB each side, all allocated: a correct kernel never reads
                  unallocated memory); input / residual guards NaN instead of 0 change nothing, output guards keep their canary bytes
                  in EVERY run;
  (u8)            row-pitch padding, guard bytes and the other frames of a batch change (0x00 / 0xFF, smooth / all-255 / noise).

The clean run is also held to the oracle at the bar its layer already has (docs/tolerances.md), which anchors the differential.
Radii: tests/locality.py, derived in tests/test_locality_model_cpu.py.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402
from oracle import onnx_min, oracle           # noqa: E402
from tests import graphgen, util              # noqa: E402
from tests import locality as loc             # noqa: E402
from tests.test_gpu_parity import CONV_CASES, DWPW_CASES, HALO_CASES, WINO_CASES, _det_outputs, dev, pack_weights  # noqa: E402
from tests.test_gpu_round4 import WINO2_CASES                                                                      # noqa: E402
from tests.test_gpu_round5 import WINO2_MERGED_CASES                                                               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32("nan")

# leg -> [cases, exempted output elements, compared output elements]
STATS = {}


def _count(leg, exempt, compared, case=0):
    s = STATS.setdefault(leg, [0, 0, 0])
    s[0] += case; s[1] += int(exempt); s[2] += int(compared)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)
    oracle.set_threads(8)
    yield
    lines = [f"locality leg {leg:<28} cases {c:4d}  exempted {e:12d}  compared {n:14d}" for leg, (c, e, n) in sorted(STATS.items())]
    print("\n" + "\n".join(lines))                                      # (pytest -s shows the per-leg table)


# ================================================================================================== 3. single layers, float inputs
def _single_layer_legs(leg, x, res, out_shapes, launch, stride, R, k, nonvacuous, clean_check):
    """x [B,H,W,Cin] f32, res [B,Ho,Wo,Cres] or None, out_shapes = [[B,Ho,Wo,C], ...]; launch(x_ptr, res_ptr or 0, [out ptrs]) runs the
    layer (and synchronises).  nonvacuous = [bool per output]: the output has no activation.  clean_check(list of clean outputs) holds the
    clean run to the oracle."""
    B, H, W, Cin = x.shape
    Ho, Wo = out_shapes[0][1:3]
    xb = loc.GuardedBuffer(x, 0)
    rb = loc.GuardedBuffer(res, 0) if res is not None else None

    def run(tag):
        xb.upload()
        if rb is not None:
            rb.upload()
        outs = [loc.GuardedBuffer(np.full(s, NAN, np.float32), loc.CANARY_BITS).upload() for s in out_shapes]
        launch(xb.ptr, rb.ptr if rb is not None else 0, [o.ptr for o in outs])
        torch.cuda.synchronize()
        return [o.read_checked(f"{leg} {tag}") for o in outs]                 # (asserts the canaries of both output guards)

    clean = run("clean")
    clean_check(clean)
    _count(leg, 0, 0, case=1)

    # (a) within-image plants, one dirty run per pattern group
    read = 0
    for group in loc.plant_groups(B, H, W, Cin):
        Q = sorted({(b, y, xx) for _, b, y, xx, *_ in group})
        allowed = loc.allowed_mask((B, Ho, Wo), Q, stride, R)
        xb.set(loc.apply_plants(x, group))
        if rb is not None:                                                    # same positions in the residual: R = 0 there
            rplants = [(t, b, y, xx, c, nm, bits) for (t, b, y, xx, _, nm, bits) in group for c in sorted({0, res.shape[3] - 1})]
            rb.set(loc.apply_plants(res, rplants))
            allowed |= loc.allowed_mask((B, Ho, Wo), Q, 1, 0)
        dirty = run(f"plants {group[0][5]}")
        for o, (d, c) in enumerate(zip(dirty, clean)):
            _count(leg + " (a) plants", *loc.assert_bitwise_outside(d, c, allowed, f"{leg} plants {group[0][5]} output {o}"))
            if nonvacuous[o]:
                read += loc.assert_poison_was_read(d, Q, (H, W), stride, k, f"{leg} plants {group[0][5]} output {o}")
    assert read > 0 or not any(nonvacuous)
    xb.set(x)
    if rb is not None:
        rb.set(res)

    # (b) aggressor images
    if B > 1:
        for victims in loc.aggressor_victim_sets(B):
            agg = np.ones(B, bool); agg[victims] = False
            xd = x.copy(); xd[agg] = NAN
            xb.set(xd)
            if rb is not None:
                rd = res.copy(); rd[agg] = NAN
                rb.set(rd)
            dirty = run("aggressors")
            for o, (d, c) in enumerate(zip(dirty, clean)):
                _count(leg + " (b) aggressors", *loc.assert_bitwise_outside(d, c, agg, f"{leg} aggressors output {o}"))
                if nonvacuous[o]:
                    assert not np.isfinite(d[agg]).any(), f"{leg}: an aggressor image's output stayed finite"
                loc.assert_images_changed(d, c, agg, f"{leg} aggressors output {o}")
        xb.set(x)
        if rb is not None:
            rb.set(res)

    # (c) guards
    xb.fill_guards(loc.NAN_BITS)
    if rb is not None:
        rb.fill_guards(loc.NAN_BITS)
    dirty = run("guards")
    for o, (d, c) in enumerate(zip(dirty, clean)):
        _count(leg + " (c) guards", *loc.assert_bitwise_outside(d, c, np.zeros(B, bool), f"{leg} guards output {o}"))


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,cfg", CONV_CASES)
def test_conv_layer_locality(B, H, W, Cin, Cout, k, stride, cfg):
    """conv_igemm (all cfgs, stream-K remainder rounds, tile0 > 0), conv_tall 256x64 / 128x32, conv_pw with its K tail."""
    rng = np.random.default_rng(B * 1000 + H * 10 + Cin)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ref = oracle.conv2d(x, w, b, stride, k // 2, 1)
    wp, kpad = pack_weights(w)
    wd, bd = dev(wp), dev(b)
    Ho, Wo = ref.shape[2], ref.shape[3]

    def launch(xp, _rp, outs):
        rc = fa.lib().fh_conv_forward_dev(xp, wd.data_ptr(), bd.data_ptr(), outs[0], B, H, W, Cin, Cout, k, stride, kpad, cfg, 0)
        assert rc == 0, _lib.last_error()

    def clean_check(clean):
        np.testing.assert_allclose(clean[0].transpose(0, 3, 1, 2), ref, rtol=0, atol=2e-5)       # test_conv_layer_matches_oracle's bar

    _single_layer_legs("conv", np.ascontiguousarray(x.transpose(0, 2, 3, 1)), None, [(B, Ho, Wo, Cout)], launch, stride,
                       loc.R_DIRECT3 if k == 3 else loc.R_1X1, k, [True], clean_check)


def _winograd_layer_locality(B, H, W, Cin, Cout, precision):
    """precision = 1: the split-bf16 operand format through fh_conv_winograd_ex_dev — the same plants, aggressors, guards and radius; a
    plant's word holds a NaN mid beside its NaN / Inf hi, nothing else changes."""
    rng = np.random.default_rng(B * 1000 + H * 10 + Cin)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1))
    bd = dev(b)
    if precision:                                                                                  # test_layer_against_fp64_...'s bars
        from tests.test_gpu_wino_bf16x2 import conv_fp64, layer_bars
        ref = conv_fp64(x, w, b)
        bar_max, bar_rms, _, _ = layer_bars(x, w, b, ref)
    else:
        ref = oracle.conv2d(x, w, b, 1, 1, 1)

    def launch(xp, _rp, outs):
        rc = fa.lib().fh_conv_winograd_ex_dev(xp, ohwi.ctypes.data, bd.data_ptr(), outs[0], B, H, W, Cin, Cout, precision, 0)
        assert rc == 0, _lib.last_error()

    def clean_check(clean):                                                                        # test_winograd_conv_matches_oracle's bars
        got = clean[0].transpose(0, 3, 1, 2)
        assert np.isfinite(got).all()
        if precision:
            assert np.abs(got - ref).max() <= bar_max and np.sqrt(((got - ref) ** 2).mean()) <= bar_rms
            return
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-4)
        assert np.sqrt(((got - ref) ** 2).mean()) < 2e-5

    _single_layer_legs("winograd F(4x4) bf16x2" if precision else "winograd F(4x4)", np.ascontiguousarray(x.transpose(0, 2, 3, 1)), None,
                       [(B, H, W, Cout)], launch, 1, loc.R_WINO4, 3, [True], clean_check)


@pytest.mark.parametrize("B,H,W,Cin,Cout", WINO_CASES)
def test_winograd_layer_locality(B, H, W, Cin, Cout):
    """F(4x4,3x3), uniform and mixed F(4) / F(2) tiling: wino_input_kernel / wino_mix_kernel -> GEMM -> output transform."""
    _winograd_layer_locality(B, H, W, Cin, Cout, 0)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [c for c in WINO_CASES if c[3] % 32 == 0 and c[4] % 64 == 0])
def test_winograd_layer_locality_bf16x2(B, H, W, Cin, Cout):
    """The same layers in the split-bf16 operand format (those that have that form): the packing writers of V and
    wino_gemm_bf16x2_kernel under the same plants, aggressors and guards."""
    _winograd_layer_locality(B, H, W, Cin, Cout, 1)


@pytest.mark.parametrize("B,H,W,Cin,Cout,act,with_res,cls", WINO2_CASES)
def test_wino2_layer_locality(B, H, W, Cin, Cout, act, with_res, cls):
    """wino2_kernel: residual, bias classes, ReLU / PReLU."""
    rng = np.random.default_rng(B * 1000 + H * 10 + Cin + Cout)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    ref = oracle.conv2d(x, w, None, 1, 1, 1)
    if cls:
        b9 = rng.standard_normal((9, Cout)).astype(np.float32)
        ys = np.ones(H, int); ys[0] = 0; ys[-1] = 2 if H > 1 else 0
        xs = np.ones(W, int); xs[0] = 0; xs[-1] = 2 if W > 1 else 0
        ref = ref + b9[3 * ys[:, None] + xs[None, :]].transpose(2, 0, 1)[None]
        bias = b9
    else:
        bias = rng.standard_normal(Cout).astype(np.float32)
        ref = ref + bias[None, :, None, None]
    slope = (0.25 * rng.uniform(0.5, 1.5, Cout)).astype(np.float32)
    if act == 1:
        ref = np.maximum(ref, 0)
    elif act == 2:
        ref = np.where(ref >= 0, ref, ref * slope[None, :, None, None])
    res = rng.standard_normal((B, H, W, Cout)).astype(np.float32) if with_res else None
    if with_res:
        ref = ref + res.transpose(0, 3, 1, 2)
    bd, sd = dev(bias), dev(slope)
    w_ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(Cout, 9, Cin))

    def launch(xp, rp, outs):
        rc = fa.lib().fh_conv_wino2_dev(xp, w_ohwi.ctypes.data, bd.data_ptr(), sd.data_ptr(), rp, outs[0], B, H, W, Cin, Cout, act,
                                        1 if cls else 0, 0)
        assert rc == 0, _lib.last_error()

    def clean_check(clean):                                                                        # test_wino2_fused_conv_layer_matches_oracle's bar
        got = clean[0].transpose(0, 3, 1, 2)
        assert not np.isnan(got).any()
        np.testing.assert_allclose(got, ref.astype(np.float32), rtol=0, atol=5e-5)

    _single_layer_legs("wino2 F(2x2)", np.ascontiguousarray(x.transpose(0, 2, 3, 1)), res, [(B, H, W, Cout)], launch, 1, loc.R_WINO2, 3,
                       [act == 0], clean_check)


@pytest.mark.parametrize("B,H,W,splits,acts", WINO2_MERGED_CASES)
def test_wino2_merged_siblings_locality(B, H, W, splits, acts):
    """The CB = 2 form of wino2_kernel: merged sibling convolutions, one destination per channel range."""
    cout = sum(splits)
    rng = np.random.default_rng(B * 100 + H + cout)
    x = rng.standard_normal((B, 64, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, 64, 3, 3)) / np.sqrt(64 * 9)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    ref = oracle.conv2d(x, w, None, 1, 1, 1) + bias[None, :, None, None]
    oc0 = np.concatenate([[0], np.cumsum(splits)]).astype(np.int32)
    oact = np.array(acts, np.int32)
    bd = dev(bias)
    w_ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(cout, 9, 64))

    def launch(xp, _rp, outs):
        ptrs = (C.c_void_p * len(splits))(*outs)
        rc = fa.lib().fh_conv_wino2_ex_dev(xp, w_ohwi.ctypes.data, bd.data_ptr(), None, None, None, None, None, None, len(splits),
                                           C.cast(ptrs, C.c_void_p), oc0.ctypes.data, oact.ctypes.data, B, H, W, 64, cout, 0, 0, None)
        assert rc == 0, _lib.last_error()

    def clean_check(clean):                                                                        # test_wino2_merged_sibling_epilogue_matches_oracle's bars
        for g, (c, a) in enumerate(zip(splits, acts)):
            r = ref[:, oc0[g]:oc0[g + 1]]
            r = np.maximum(r, 0) if a == 1 else 1.0 / (1.0 + np.exp(-r.astype(np.float64))) if a == 3 else r
            got = clean[g].transpose(0, 3, 1, 2)
            assert not np.isnan(got).any(), g
            np.testing.assert_allclose(got, r.astype(np.float32), rtol=0, atol=5e-5 if a != 3 else 2e-5, err_msg=f"destination {g}")

    _single_layer_legs("wino2 merged", np.ascontiguousarray(x.transpose(0, 2, 3, 1)), None, [(B, H, W, c) for c in splits], launch, 1,
                       loc.R_WINO2, 3, [a == 0 for a in acts], clean_check)


def test_wino2_second_output_locality():
    """`out2 = out1 * s2 + t2` beside out1, with a residual (IResNet's `+bn2nd` layers): both outputs are held to the property."""
    B, H, W, Cc = 2, 24, 24, 64
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, Cc, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cc, Cc, 3, 3)) / np.sqrt(Cc * 9)).astype(np.float32)
    bias = rng.standard_normal(Cc).astype(np.float32); s2 = rng.uniform(0.5, 1.5, Cc).astype(np.float32); t2 = rng.standard_normal(Cc).astype(np.float32)
    res = rng.standard_normal((B, H, W, Cc)).astype(np.float32)
    ref = oracle.conv2d(x, w, None, 1, 1, 1) + bias[None, :, None, None] + res.transpose(0, 3, 1, 2)
    ref2 = ref * s2[None, :, None, None] + t2[None, :, None, None]
    bd, s2d, t2d = dev(bias), dev(s2), dev(t2)
    w_ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(Cc, 9, Cc))

    def launch(xp, rp, outs):
        rc = fa.lib().fh_conv_wino2_ex_dev(xp, w_ohwi.ctypes.data, bd.data_ptr(), None, rp, outs[0], outs[1], s2d.data_ptr(), t2d.data_ptr(), 0,
                                           None, None, None, B, H, W, Cc, Cc, 0, 0, None)
        assert rc == 0, _lib.last_error()

    def clean_check(clean):                                                                        # test_wino2_second_output_and_argument_checks' bars
        np.testing.assert_allclose(clean[0].transpose(0, 3, 1, 2), ref, rtol=0, atol=5e-5)
        np.testing.assert_allclose(clean[1].transpose(0, 3, 1, 2), ref2, rtol=0, atol=1e-4)

    _single_layer_legs("wino2 second output", np.ascontiguousarray(x.transpose(0, 2, 3, 1)), res, [(B, H, W, Cc), (B, H, W, Cc)], launch, 1,
                       loc.R_WINO2, 3, [True, True], clean_check)


# ================================================================================================== 4. kernels reachable only through graphs
def _nhwc4(x):
    """[n,3,H,W] -> the engine's input layout [n,H,W,4], lane 3 = 0."""
    n, _, H, W = x.shape
    out = np.zeros((n, H, W, 4), np.float32)
    out[..., :3] = x.transpose(0, 2, 3, 1)
    return out


def _det_graph_legs(leg, det, g, x, plants, clean_check):
    """A detector handle on a caller-supplied float input (fh_det_run_input_dev): aggressor images and input guards, and for the
    direct-form graphs within-image plants with the allowed set taken from locality.propagate_graph_mask."""
    n, _, H, W = x.shape
    x4 = _nhwc4(x)
    xb = loc.GuardedBuffer(x4, 0)
    L = fa.lib()
    onames = [name for name, _ in g.outputs]
    cap = (2 * sum(1 for nd in g.nodes if nd.op == "Conv" and nd.attrs["kernel_shape"][0] == 3) + 1) ** 2

    def run():
        xb.upload()
        assert L.fh_det_run_input_dev(det.handle, xb.ptr, n, 0) == n, _lib.last_error()
        torch.cuda.synchronize()
        return [o.copy() for o in _det_outputs(det, n)]

    clean = run()
    clean_check(clean)
    _count(leg, 0, 0, case=1)
    if plants:
        for group in loc.plant_groups(n, H, W, 3):
            m = np.zeros((n, H, W), bool)
            for _, b, y, xx, *_ in group:
                m[b, y, xx] = True
            allowed = loc.propagate_graph_mask(g, m)
            xb.set(loc.apply_plants(x4, group))                                   # (channels 0 and 2: lane 3 stays 0)
            dirty = run()
            for name, d, c in zip(onames, dirty, clean):
                a = allowed[name]
                assert a.sum() <= cap * len(group)                                # the exemption cap: (2R+1)^2 per plant, R = 1 per 3x3 layer
                shape = a.shape + (d.shape[-1],)
                _count(leg + " (a) plants", *loc.assert_bitwise_outside(d.reshape(shape), c.reshape(shape), a, f"{leg} plants {group[0][5]} {name}"))
                if group[0][5] != "nan":                                          # +-Inf survives the stem's ReLU in some channels: it must show
                    planted = sorted({b for _, b, *_ in group})
                    touched = np.zeros(n, bool); touched[planted] = True
                    loc.assert_images_changed(d, c, touched, f"{leg} plants {group[0][5]} {name}")
        xb.set(x4)
    hostile = loc.hostile_images(x4.shape, 3, seed=n + H)
    for victims in loc.aggressor_victim_sets(n):
        agg = np.ones(n, bool); agg[victims] = False
        for kind in ("nan", "hostile"):
            xd = x4.copy()
            if kind == "nan":
                xd[agg, :, :, :3] = NAN
            else:
                xd[agg] = hostile[agg]
            xb.set(xd)
            dirty = run()
            for name, d, c in zip(onames, dirty, clean):
                _count(leg + " (b) aggressors", *loc.assert_bitwise_outside(d, c, agg, f"{leg} aggressors {kind} {name}"))
                if kind == "hostile":                                             # (a NaN image may legitimately end as the clean image's bias map)
                    loc.assert_images_changed(d, c, agg, f"{leg} aggressors {kind} {name}")
    xb.set(x4)
    xb.fill_guards(loc.NAN_BITS)
    dirty = run()
    for name, d, c in zip(onames, dirty, clean):
        _count(leg + " (c) guards", *loc.assert_bitwise_outside(d, c, np.zeros(n, bool), f"{leg} guards {name}"))


@pytest.mark.parametrize("H,W,Cc,Cout,ds", DWPW_CASES)
def test_depthwise_pointwise_graph_locality(tmp_path, H, W, Cc, Cout, ds):
    """dwpw_mfma.hip's depthwise -> pointwise kernels (LDS and register-fed forms, both strides) behind a generic stem convolution: the
    front kernel is off for float input."""
    path = util.dwpw_graph(str(tmp_path / "dwpw.onnx"), H, W, Cc, Cout, ds)
    assert "DW+PW" in fa.plan_describe(path, H, W)
    det = fa.FaceDetector(); odet = oracle.OracleDetector()
    assert det.loadModel(path) and odet.loadModel(path)
    assert fa.lib().fh_det_set_fused_front(det.handle, 0) == 0
    n = 3
    x = (np.random.default_rng(Cout).standard_normal((n, 3, H, W)) * 0.5).astype(np.float32)

    def clean_check(clean):                                                       # test_depthwise_pointwise_block_matches_oracle's bar
        for i in (0, n - 1):
            ref = odet.run_network(x[i])[0]
            np.testing.assert_allclose(clean[0][i], ref.reshape(clean[0][i].shape), rtol=1e-5, atol=2e-5)

    _det_graph_legs("graph dw->pw", det, odet.g, x, True, clean_check)


@pytest.mark.parametrize("H,W,CH,stride,act", [
    (20, 20, 288, 1, "relu"), (40, 40, 152, 2, "relu"), (7, 9, 8, 1, "none"), (9, 7, 8, 2, "prelu"), (13, 31, 20, 1, "prelu"),
    (33, 17, 64, 2, "none"), (5, 5, 4, 1, "relu"),           # the cases of test_depthwise_lean_kernel_matches_oracle
])
def test_depthwise_graph_locality(tmp_path, H, W, CH, stride, act):
    """dwconv3x3_lean_kernel and the generic dwconv3x3_kernel (C = 4), both strides."""
    path = util.dw_graph(str(tmp_path / "dw.onnx"), H, W, CH, stride, act, seed=H * 100 + W + CH)
    det = fa.FaceDetector()
    assert det.loadModel(path)
    g = onnx_min.load(path)
    n = 3
    x = (np.random.default_rng(7 + CH).standard_normal((n, 3, H, W)) * 0.5).astype(np.float32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1

    def clean_check(clean):                                                       # test_depthwise_lean_kernel_matches_oracle's bar
        assert clean[0].shape == (n, Ho * Wo, CH)
        for i in range(n):
            ref = oracle.run_graph(g, {"input.1": x[i][None]})["out"]
            np.testing.assert_allclose(clean[0][i], np.asarray(ref).reshape(Ho * Wo, CH), rtol=1e-5, atol=1e-5, err_msg=f"image {i}")

    _det_graph_legs("graph depthwise", det, g, x, True, clean_check)


@pytest.mark.parametrize("H,W,Cin,Cout,res", HALO_CASES)
def test_halo_conv_graph_locality(tmp_path, H, W, Cin, Cout, res):
    """conv_halo.hip's spatial-tile 3x3 kernels (32x32 and 16x16x4 MFMA forms), with and without the residual."""
    path = util.halo_graph(str(tmp_path / "halo.onnx"), H, W, Cin, Cout, res)
    det = fa.FaceDetector(); odet = oracle.OracleDetector()
    assert det.loadModel(path) and odet.loadModel(path)
    assert fa.lib().fh_det_set_halo_conv(det.handle, 1) == 0
    n = 3
    x = (np.random.default_rng(Cout).standard_normal((n, 3, H, W)) * 0.5).astype(np.float32)

    def clean_check(clean):                                                       # test_halo_conv_matches_oracle's bar
        for i in range(n):
            ref = odet.run_network(x[i])[0]
            np.testing.assert_allclose(clean[0][i], ref.reshape(clean[0][i].shape), rtol=1e-5, atol=3e-5)

    _det_graph_legs("graph halo conv", det, odet.g, x, True, clean_check)


def test_fpn_upsampled_residual_graph_locality(tmp_path):
    """The `up2` motif of the graph corpus: conv + x2-upsampled residual (+res(up2x)), standalone upsample / ACT / ADD / AFFINE ops."""
    path, spec = graphgen.make_graph(1020, str(tmp_path))
    H, W = graphgen.MOTIFS[1020][1]
    assert "+res(up2x)" in fa.plan_describe(path, H, W) and "UPSAMPLE" in fa.plan_describe(path, H, W), fa.plan_describe(path, H, W)
    det = fa.FaceDetector(); odet = oracle.OracleDetector()
    assert det.loadModel(path) and odet.loadModel(path)
    n = 3
    x = np.random.default_rng(1020).uniform(-1, 1, (n, 3, H, W)).astype(np.float32)

    def clean_check(clean):                                                       # the graph corpus' bar: 1e-4 of the output's scale
        for i in range(n):
            for got, ref in zip(clean, odet.run_network(x[i])):
                ref = np.asarray(ref).reshape(got[i].shape)
                assert np.abs(got[i] - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), spec

    _det_graph_legs("graph fpn up2", det, odet.g, x, False, clean_check)


def _rec_graph_legs(leg, path, size, n, oracle_slots):
    """A recogniser handle on a caller-supplied float input (fh_rec_run_input_dev), Winograd fusion on and off: aggressor images and input
    guards; raw outputs AND embeddings of the victims are bitwise the clean run's (l2norm_kernel: rows are independent)."""
    rec = fa.FaceRecognizer(); orec = oracle.OracleRecognizer()
    assert rec.loadModel(path) and orec.loadModel(path)
    L = fa.lib()
    dim = L.fh_rec_feature_dim(rec.handle)
    x = (np.random.default_rng(size + n).standard_normal((n, 3, size, size)) * 0.5).astype(np.float32)
    x4 = _nhwc4(x)
    xb = loc.GuardedBuffer(x4, 0)
    refs = {i: oracle.run_graph(orec.g, {orec.g.inputs[0][0]: x[i][None]})[orec.g.outputs[0][0]].reshape(-1) for i in oracle_slots}
    try:
        for fusion in (1, 0):
            assert L.fh_rec_set_wino_fusion(rec.handle, fusion) == 0
            tag = f"{leg} fusion={fusion}"

            def run():
                xb.upload()
                emb = loc.GuardedBuffer(np.full((n, dim), NAN, np.float32), loc.CANARY_BITS).upload()
                raw = loc.GuardedBuffer(np.full((n, dim), NAN, np.float32), loc.CANARY_BITS).upload()
                assert L.fh_rec_run_input_dev(rec.handle, xb.ptr, n, emb.ptr, raw.ptr, 0) == n, _lib.last_error()
                torch.cuda.synchronize()
                return raw.read_checked(tag + " raw"), emb.read_checked(tag + " emb")

            xb.set(x4).fill_guards(0)
            craw, cemb = run()
            assert np.isfinite(craw).all() and np.isfinite(cemb).all()
            for i, r in refs.items():                                             # the bar of the tests these graphs come from
                np.testing.assert_allclose(craw[i], r, rtol=2e-4, atol=2e-4 * np.abs(r).max(), err_msg=f"{tag} slot {i}")
            np.testing.assert_allclose(np.linalg.norm(cemb.astype(np.float64), axis=1), 1.0, rtol=0, atol=1e-5)
            _count(leg, 0, 0, case=1)
            hostile = loc.hostile_images(x4.shape, 3, seed=n + size)
            for victims in loc.aggressor_victim_sets(n):
                agg = np.ones(n, bool); agg[victims] = False
                for kind in ("nan", "hostile"):
                    xd = x4.copy()
                    if kind == "nan":
                        xd[agg, :, :, :3] = NAN
                    else:
                        xd[agg] = hostile[agg]
                    xb.set(xd)
                    draw, demb = run()
                    _count(leg + " (b) aggressors", *loc.assert_bitwise_outside(draw, craw, agg, f"{tag} aggressors {kind} raw"))
                    _count(leg + " (b) aggressors", *loc.assert_bitwise_outside(demb, cemb, agg, f"{tag} aggressors {kind} emb"))
                    # PReLU keeps NaN / Inf (u >= 0 ? u : u * slope): both kinds must arrive at the end of the network non-finite
                    loc.assert_images_changed(draw, craw, agg, f"{tag} aggressors {kind} raw", need_nonfinite=True)
            xb.set(x4).fill_guards(loc.NAN_BITS)
            draw, demb = run()
            _count(leg + " (c) guards", *loc.assert_bitwise_outside(draw, craw, np.zeros(n, bool), tag + " guards raw"))
            _count(leg + " (c) guards", *loc.assert_bitwise_outside(demb, cemb, np.zeros(n, bool), tag + " guards emb"))
    finally:
        L.fh_rec_set_wino_fusion(rec.handle, 1)


@pytest.mark.timeout(600)
def test_mixed_winograd_iresnet_locality(tmp_path):
    """The graph of test_mixed_winograd_tiling_in_its_three_transform_roles at B = 64: wino_mix_kernel as image -> V, M -> V and
    M -> output, wino_fused_kernel on the 7x7 stage."""
    path = models.make_iresnet(str(tmp_path / "mix.onnx"), (1, 1, 2, 1), (32, 64, 128, 128), 112, 64, seed=9)
    _rec_graph_legs("graph iresnet mixed", path, 112, 64, (0, 17, 63))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("size", [112, 104])
def test_channel_sliced_winograd_iresnet_locality(tmp_path, size):
    """The graph of test_channel_sliced_fused_transform_on_28x28_maps...: wino_slice_kernel on 28x28 / 26x26 maps at B = 24."""
    m = size // 4
    path = models.make_iresnet(str(tmp_path / f"s{m}.onnx"), (1, 3, 1, 1), (32, 128, 128, 128), size, 64, seed=21)
    assert fa.plan_describe(path, size, size).count(f"k3s1 {m}x{m}x128 -> {m}x{m}x128") >= 5
    _rec_graph_legs("graph iresnet sliced", path, size, 24, (0, 12, 23))


def test_input_entry_points_check_their_arguments(models_dir):
    L = fa.lib()
    det = fa.FaceDetector(); rec = fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128)) and rec.loadModel(util.tiny_iresnet(models_dir))
    x = torch.zeros((1, 128, 128, 4), device="cuda")
    out = torch.zeros((1, 512), device="cuda")
    assert L.fh_det_run_input_dev(None, x.data_ptr(), 1, 0) == -1 and L.fh_det_run_input_dev(det.handle, None, 1, 0) == -1
    assert L.fh_det_run_input_dev(det.handle, x.data_ptr(), 0, 0) == -1
    assert L.fh_rec_run_input_dev(None, x.data_ptr(), 1, out.data_ptr(), None, 0) == -1
    assert L.fh_rec_run_input_dev(rec.handle, None, 1, out.data_ptr(), None, 0) == -1
    assert L.fh_rec_run_input_dev(rec.handle, x.data_ptr(), 1, None, None, 0) == -1
    assert L.fh_rec_run_input_dev(rec.handle, x.data_ptr(), -1, out.data_ptr(), None, 0) == -1
    # and the float path computes what the u8 path computes with the fused stem off (same kernels on the same input)
    frames = util.frames_u8(2, 128, 128, seed=5)
    assert L.fh_det_set_fused_stem(det.handle, 0) == 0
    d = dev(frames)
    assert L.fh_det_run_network_dev(det.handle, d.data_ptr(), 2, 128, 128, 384, 128 * 384, 0) == 2
    torch.cuda.synchronize()
    want = [o.copy() for o in _det_outputs(det, 2)]
    x4 = _nhwc4(np.stack([oracle.det_preprocess(f, 128, 128)[0] for f in frames]))
    assert L.fh_det_run_input_dev(det.handle, dev(x4).data_ptr(), 2, 0) == 2
    torch.cuda.synchronize()
    for a, b in zip(_det_outputs(det, 2), want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ================================================================================================== 5. byte-level isolation, u8 paths
class U8Frames:
    """n frames [rows][step] in one guarded allocation: guard | frame 0 | ... | frame n-1 | guard.  Pixels, row padding and guards are set
    independently; everything is allocated."""

    def __init__(self, n, rows, cols, step):
        assert step >= cols * 3
        self.n, self.rows, self.cols, self.step = n, rows, cols, step
        self.buf = loc.GuardedBuffer(np.zeros((n, rows, step), np.uint8), 0)

    def fill(self, frames, pad_byte, guard_byte):
        img = np.full((self.n, self.rows, self.step), pad_byte, np.uint8)
        img[:, :, :self.cols * 3] = np.asarray(frames, np.uint8).reshape(self.n, self.rows, self.cols * 3)
        self.buf.set(img).fill_guards(guard_byte * 0x01010101)
        self.buf.upload()
        return self.buf.ptr


def _other_frames(kind, n, rows, cols, seed):
    if kind == "smooth":
        return util.frames_u8(n, rows, cols, seed=seed, smooth=min(rows, cols) >= 32)
    if kind == "255":
        return np.full((n, rows, cols, 3), 255, np.uint8)
    return util.frames_u8(n, rows, cols, seed=seed + 1, smooth=False)


def _u8_variants(n, rows, cols, victims, seed):
    """-> [(tag, frames, pad byte, guard byte, frames that must not change)]: the baseline, then padding + guards 0xFF, then the
    non-victim frames all-255 and noise (padding / guards 0xFF too)."""
    base = _other_frames("smooth", n, rows, cols, seed)
    out = [("base", base, 0x00, 0x00, None), ("pad+guards 0xFF", base, 0xFF, 0xFF, list(range(n)))]
    for kind in ("255", "noise"):
        f = _other_frames(kind, n, rows, cols, seed)
        f[victims] = base[victims]
        out.append((f"others {kind}", f, 0xFF, 0x00 if kind == "noise" else 0xFF, victims))
    return out


DET_FRAMES = [
    # rows, cols, row pitch - cols * 3   (the shapes of test_det500m_letterboxed_frame_heads_match_oracle, + two pitches off the dword grid)
    (375, 500, 0), (640, 401, 0), (640, 3, 0), (640, 2, 0), (640, 1, 0), (2, 640, 0), (375, 500, 5), (640, 401, 2),
]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("front,stem", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_det500m_u8_path_byte_isolation(front, stem):
    """det_500m heads through fh_det_run_network_dev (front_kernel / stem kernels / preprocess + resize): the 9 heads of a frame depend on
    that frame's pixels only — not on pitch padding, guard bytes or the other frames."""
    path = models.cached("det_500m_seed100.onnx", models.make_det_500m)
    det = fa.FaceDetector()
    assert det.loadModel(path)
    L = fa.lib()
    assert L.fh_det_set_fused_front(det.handle, front) == 0 and L.fh_det_set_fused_stem(det.handle, stem) == 0
    n, victims = 3, [1]
    for rows, cols, pad in DET_FRAMES:
        step = cols * 3 + pad
        fr = U8Frames(n, rows, cols, step)
        base = None
        for tag, frames, pb, gb, same in _u8_variants(n, rows, cols, victims, rows + cols):
            ptr = fr.fill(frames, pb, gb)
            assert L.fh_det_run_network_dev(det.handle, ptr, n, rows, cols, step, rows * step, 0) == n, _lib.last_error()
            torch.cuda.synchronize()
            outs = [o.copy() for o in _det_outputs(det, n)]
            if base is None:
                base = outs
                assert all(np.isfinite(o).all() for o in outs)
                _count("u8 det_500m", 0, 0, case=1)
                continue
            allowed = np.ones(n, bool); allowed[same] = False
            for i, (d, c) in enumerate(zip(outs, base)):
                _count("u8 det_500m", *loc.assert_bitwise_outside(d, c, allowed, f"front={front} stem={stem} {rows}x{cols} step {step} {tag} head {i}"))


def _r50_stem_leg(dump=None):
    """Body of test_r50_stem_u8_path_byte_isolation (also run in a child process with the matrix-core stem switched off).  Returns the
    baseline raw outputs, and saves them to `dump` when given."""
    torch.cuda.set_device(0)
    fa.lib().fh_init(0)
    rec = fa.FaceRecognizer()
    assert rec.loadModel(models.cached("w600k_r50_seed200.onnx", models.make_w600k_r50))
    n, victims = 4, [0, 3]
    fr = U8Frames(n, 112, 112, 336)
    base = None
    for tag, crops, pb, gb, same in _u8_variants(n, 112, 112, victims, 9):
        ptr = fr.fill(crops, pb, gb)
        emb = loc.GuardedBuffer(np.full((n, 512), NAN, np.float32), loc.CANARY_BITS).upload()
        raw = loc.GuardedBuffer(np.full((n, 512), NAN, np.float32), loc.CANARY_BITS).upload()
        assert fa.lib().fh_rec_embed_aligned_dev(rec.handle, ptr, n, emb.ptr, raw.ptr, 0) == n, _lib.last_error()
        torch.cuda.synchronize()
        outs = [raw.read_checked(tag), emb.read_checked(tag)]
        if base is None:
            base = outs
            assert all(np.isfinite(o).all() for o in outs)
            continue
        allowed = np.ones(n, bool); allowed[same] = False
        for d, c in zip(outs, base):
            _count("u8 r50 stem", *loc.assert_bitwise_outside(d, c, allowed, f"r50 stem {tag}"))
    _count("u8 r50 stem", 0, 0, case=1)
    if dump:
        np.save(dump, base[0])
    return base[0]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mfma", [1, 0])
def test_r50_stem_u8_path_byte_isolation(tmp_path, mfma):
    """w600k_r50 through fh_rec_embed_aligned_dev: stem_mfma_kernel, and (FACEHIP_STEM_MFMA=0, read once per process: a fresh child) the
    stem kernel launch_stem falls back to at 64 output channels, the LDS-tile stem_conv_u8_kernel (the thread-per-pixel form is
    what det_500m takes with the front off and the stem on, test_det500m_u8_path_byte_isolation[0-1]).  The child's raw outputs must
    differ from the matrix-core stem's in some bit (another kernel ran: a different summation order) and agree to 1e-4 of scale (the bar of
    test_winograd_switch_changes_only_rounding: rounding-only changes through the whole IResNet-50).
    Crops are tight [n][112][112][3]: the neighbours are the other crops and the guards."""
    if mfma:
        _r50_stem_leg()
        return
    env = dict(os.environ, FACEHIP_STEM_MFMA="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    dump = str(tmp_path / "raw_no_mfma.npy")
    r = subprocess.run([sys.executable, "-c", f"from tests.test_gpu_locality import _r50_stem_leg; _r50_stem_leg({dump!r}); print('LEG_OK')"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0 and "LEG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    other, here = np.load(dump), _r50_stem_leg()
    assert not np.array_equal(other.view(np.uint32), here.view(np.uint32)), "FACEHIP_STEM_MFMA=0 ran the same stem kernel"
    assert np.abs(other - here).max() <= 1e-4 * np.abs(here).max()
    _count("u8 r50 stem", 0, 0, case=1)


def _border_faces(rows, cols):
    """Faces whose 112x112 crop hangs over the left / right / top / bottom frame border, one over all four (a crop larger than the
    frame), and one inside: landmarks = template x similarity."""
    T = util.TEMPLATE
    specs = [(1.0, -30.0, 60.0), (1.0, cols - 80.0, 60.0), (1.0, 100.0, -30.0), (1.0, 100.0, rows - 80.0), (4.0, -60.0, -100.0),
             (1.5, 60.0, 30.0), (1.0, -40.0, -40.0), (1.0, cols - 70.0, rows - 70.0)]
    faces = np.zeros(len(specs), fa.FACE_DTYPE)
    for i, (s, tx, ty) in enumerate(specs):
        faces["lm"][i] = (T * s + np.array([tx, ty], np.float32)).reshape(10)
    faces["x"], faces["y"], faces["w"], faces["h"] = 30, 40, 90, 100
    return faces


def test_align_u8_path_byte_isolation(models_dir):
    """fh_rec_align_dev: crops of faces on frame `v` whose taps reach all four borders depend on frame v's pixels only (bit-exact vs the
    oracle's alignFace, and unchanged by padding / guards / the other frames)."""
    rec = fa.FaceRecognizer()
    assert rec.loadModel(util.tiny_iresnet(models_dir))
    nfr, rows, cols, v = 3, 240, 320, 1
    faces = _border_faces(rows, cols)
    n = len(faces)
    frame_of = np.full(n, v, np.int32)
    facd, fo = dev(faces.view(np.uint8).reshape(n, 60)), dev(frame_of)
    for pad in (0, 5):
        step = cols * 3 + pad
        fr = U8Frames(nfr, rows, cols, step)
        base = None
        for tag, frames, pb, gb, _ in _u8_variants(nfr, rows, cols, [v], 11):
            ptr = fr.fill(frames, pb, gb)
            crops = loc.GuardedBuffer(np.zeros((n, 112, 112, 3), np.uint8), loc.CANARY_BITS).upload()
            ok = loc.GuardedBuffer(np.zeros(n, np.int32), loc.CANARY_BITS).upload()
            rc = fa.lib().fh_rec_align_dev(rec.handle, ptr, rows, cols, step, rows * step, facd.data_ptr(), fo.data_ptr(), n, crops.ptr, ok.ptr, 0)
            assert rc == n, _lib.last_error()
            torch.cuda.synchronize()
            got, gok = crops.read_checked(tag), ok.read_checked(tag)
            if base is None:
                base = (got, gok)
                for i in range(n):                                                # test_align_bit_exact's bar
                    ref = oracle.align_face(frames[v], faces[i])
                    assert ref is not None and gok[i] in (1, 2), i
                    assert np.array_equal(got[i], ref), f"face {i}"
                # taps on all four borders: the over-sized crop replicates / pads every edge of the frame
                _count("u8 align", 0, 0, case=1)
                continue
            assert np.array_equal(gok, base[1]), tag
            assert np.array_equal(got, base[0]), f"align {tag} step {step}: crops of frame {v} changed"
            _count("u8 align", 0, got.size)


def test_resize_u8_path_byte_isolation():
    """fh_resize_u8c3_dev with sstep > sw * 3 and dstep > dw * 3: source padding / guards do not matter, destination padding bytes and
    guards are untouched, pixels bit-exact vs the oracle."""
    rng = np.random.default_rng(0)
    for (sh, sw, dh, dw, sp, dp) in ((480, 640, 112, 112, 4, 8), (37, 53, 112, 112, 1, 3), (123, 77, 61, 200, 5, 2), (64, 64, 128, 128, 7, 1),
                                     (100, 100, 50, 50, 2, 6)):
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        ref = oracle.resize_bilinear(img, dw, dh)
        sstep, dstep = sw * 3 + sp, dw * 3 + dp
        src = U8Frames(1, sh, sw, sstep)
        for pb, gb in ((0x00, 0x00), (0xFF, 0xFF)):
            ptr = src.fill(img[None], pb, gb)
            dst = loc.GuardedBuffer(np.full((dh, dstep), 0x5A, np.uint8), loc.CANARY_BITS).upload()
            assert fa.lib().fh_resize_u8c3_dev(ptr, sh, sw, sstep, dst.ptr, dh, dw, dstep, 0) == 0, _lib.last_error()
            torch.cuda.synchronize()
            got = dst.read_checked(f"resize {sh}x{sw}")
            assert np.array_equal(got[:, :dw * 3].reshape(dh, dw, 3), ref), (sh, sw, dh, dw, pb)     # test_resize_bit_exact's bar
            assert (got[:, dw * 3:] == 0x5A).all(), f"resize {sh}x{sw} -> {dh}x{dw}: destination padding bytes written"
            _count("u8 resize", 0, got.size)
        _count("u8 resize", 0, 0, case=1)
