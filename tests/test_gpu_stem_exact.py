"""The u8 stems (csrc/stem.hip over csrc/stem_tile.h) and front_kernel (csrc/dwpw_mfma.hip) held to exact models: docs/kernels.md promises
"hi + mid + lo = w exactly", "every product is exact in fp32" and "the fp32 FMA chain's value up to summation order" — here the output must
EQUAL tests/stem_model.py's value, every element of every image, on operands for which any summation order gives the same f32:

  class I  integer weights k = w / 128 in -7..7 (-3..3 in front of the block), integer biases, noise frames: the whole stem — and the whole
           stem -> depthwise -> pointwise block — is an integer convolution in halves.  All five kernels of launch_stem, strides 1 and 2,
           ReLU / PReLU 1/4 / none, with and without the second output y / 2 + t2, cus = 0 and 1; front_kernel<true> and <false>.
           A wrong byte, padding 127 for 127.5, canvas taken for padding.
  class P  two taps +w, -w per channel, w of three non-zero bf16 pieces, bytes 0..15: w (x1 - x2) fits 24 bits.  stem_mfma_kernel and
           front_kernel.  A dropped or doubled piece.  The outputs whose window touches the convolution padding are class I's (127.5 takes
           more bits): the border ring of the map, its size asserted in tests/test_stem_model_cpu.py.
  class D  dense 24-bit weights against fp64 at 2 gamma_100 S (stem_model.d_bound: derived, not measured); the worst ratio is printed.

Frames are pasted at letterbox scale 1 into a static net input (tests/stem_cases.py: 64 x 64 and 56 x 72, twice that where the planner
fuses the block only at the larger map; fh_debug_det_run_pasted_dev pastes the frames that the detector's letterbox would enlarge); pitch
bytes that are no pixel are 255.  The preconditions of I and P and the power of both against
nine wrong kernels are tests/test_stem_model_cpu.py's.  Values are compared with ==, so that +0 and -0 count as equal.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import stem_cases as sc            # noqa: E402
from tests import stem_model as sm            # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def stem_kernel(c):
    """launch_stem's choice (stem.hip)"""
    return "stem_mfma_kernel" if c in (48, 64) else "stem_conv_px_kernel" if c in (16, 32) else "stem_conv_u8_kernel"


def plan_ops(path, H, W):
    desc = fa.plan_describe(path, H, W)
    return [ln for ln in desc.splitlines() if ln[:1].isdigit()], desc


class Net:
    """a loaded graph with the fused u8 paths switched on; run() -> its outputs [B][rows][cols] for frames staged at `pitch`"""

    def __init__(self, path, hw, front=None):
        self.hw = hw
        self.det = fa.FaceDetector()
        assert self.det.loadModel(path), _lib.last_error()
        L = fa.lib()
        assert L.fh_det_set_fused_stem(self.det.handle, 1) == 0
        if front is not None:
            assert L.fh_det_set_fused_front(self.det.handle, 1 if front else 0) == 0

    def run(self, fr, pitch, cus=0):
        L, h = fa.lib(), self.det.handle
        n, rows, cols, _ = fr.shape
        d = torch.from_numpy(sc.staged(fr, pitch)).cuda()
        try:
            assert L.fh_det_set_cus(h, cus) == 0
            # the detector's own entry wherever its letterbox leaves the frame as it is (a side that fills the net input); the other
            # frames are pasted by the debug entry, which skips the resize
            _, nw, nh, scale = fa.letterbox_plan(rows, cols, self.hw[1], self.hw[0])
            run = L.fh_det_run_network_dev if (nw, nh, scale) == (cols, rows, 1.0) else L.fh_debug_det_run_pasted_dev
            assert run(h, d.data_ptr(), n, rows, cols, pitch, rows * pitch, 0) == n, _lib.last_error()
            torch.cuda.synchronize()
        finally:
            L.fh_det_set_cus(h, 0)
        outs = []
        for i in range(L.fh_det_num_outputs(h)):
            r, c = C.c_int(), C.c_int()
            p = L.fh_det_output_dev(h, i, C.byref(r), C.byref(c))
            out = np.empty((n, r.value, c.value), np.float32)
            assert L.fh_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0, _lib.last_error()
            outs.append(out)
        return outs


def assert_equal(got, want, tag, keep=None):
    """got [B][Ho * Wo][C] f32 == want [B][Ho][Wo][C] (fp64 values that are f32s), every element (or every element of `keep` [Ho][Wo])"""
    want = np.asarray(want, np.float64)
    got = got.reshape(want.shape).astype(np.float64)
    bad = got != want
    if keep is not None:
        bad &= keep[None, :, :, None]
    if bad.any():
        n, y, x, c = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} outputs differ; first at image {n}, output ({y}, {x}), channel {c}: "
                             f"gpu {got[n, y, x, c]!r}, model {want[n, y, x, c]!r}")


def stem_line(H, W, c, s, act, bn=False):
    Ho, Wo = sm.out_hw(H, W, s)
    tail = {"relu": "+relu", "prelu": "+prelu", "none": ""}[act] + (" +bn2nd" if bn else "") + " "
    return f"0 CONV k3s{s} {H}x{W}x4 -> {Ho}x{Wo}x{c}{tail}"


def front_net(tmp, name, H, W, w, b, ss, relus, dw, dwb, ds, pw, pwb):
    """the block's graph, its plan asserted: DW+PW (front_kernel) where sc.front_fused says so, three separate layers otherwise"""
    path = sc.front_graph(str(tmp / f"{name}_{H}x{W}.onnx"), H, W, w, b, ss, relus, dw, dwb, ds, pw, pwb)
    ops, desc = plan_ops(path, H, W)
    Hs, Ws = sm.out_hw(H, W, ss)
    Ho, Wo = sm.out_hw(Hs, Ws, ds)
    r = ["+relu " if on else " " for on in relus]
    assert ops[0].startswith(f"0 CONV k3s{ss} {H}x{W}x4 -> {Hs}x{Ws}x16{r[0]}"), desc
    fused = sc.front_fused(H, W, ss, ds)
    if fused:
        assert len(ops) == 2 and ops[1].startswith(f"1 DW+PW k1s1 {Hs}x{Ws}x16 -> {Ho}x{Wo}x{len(pwb)}{r[2]}"), desc
        assert len(pwb) <= 32 and len(pwb) % 4 == 0                     # front_fused_ok (dwpw_mfma.hip)
    else:
        assert len(ops) == 3 and ops[1].startswith(f"1 DWCONV k3s{ds} {Hs}x{Ws}x16 -> {Ho}x{Wo}x16{r[1]}"), desc
        assert ops[2].startswith(f"2 CONV k1s1 {Ho}x{Wo}x16 -> {Ho}x{Wo}x{len(pwb)}{r[2]}"), desc
    return Net(path, (H, W), front=True if fused else None), fused


def pitches(cols, pitch, fused):
    """front_kernel<STEP4>: the table's pitch and the other instantiation's"""
    return (pitch, sc.other_pitch(cols, pitch)) if fused else (pitch,)


# ------------------------------------------------------------------------------------------------------------------------ class I
@pytest.mark.parametrize("c,s,act,bn", sc.I_STEMS, ids=[f"c{c}-s{s}-{a}{'-bn' if b else ''}" for c, s, a, b in sc.I_STEMS])
def test_class_I_stem_is_the_integer_convolution_bit_for_bit(tmp_path, c, s, act, bn):
    k, b, t2 = sc.i_stem(c, s, act, bn)
    for (H, W), frames in sc.inputs():
        path = sc.stem_graph(str(tmp_path / f"i_{H}x{W}.onnx"), H, W, 128.0 * k, b, s, act, t2)
        ops, desc = plan_ops(path, H, W)
        assert len(ops) == 1 and ops[0].startswith(stem_line(H, W, c, s, act, bn)), desc
        net = Net(path, (H, W))
        for i, (rows, cols, pitch) in enumerate(frames):
            fr = sc.frames("I", (H, W), i, rows, cols)
            want = sm.epilogue_int(sm.stem_int(fr, rows, cols, H, W, s, k, b), act, t2)
            for cus in (0, 1):
                outs = net.run(fr, pitch, cus)
                assert len(outs) == 1 + bn
                for o, (got, w) in enumerate(zip(outs, want)):
                    assert_equal(got, w / sm.UNIT, f"{stem_kernel(c)} {H}x{W} frame {rows}x{cols} pitch {pitch} cus {cus} output {o}")


FRONT_IDS = [f"s{ss}-{'relu' if r[0] else 'none'}-dw{ds}-c{co}" for ss, r, ds, co in sc.I_FRONTS]


@pytest.mark.parametrize("ss,relus,ds,co", sc.I_FRONTS, ids=FRONT_IDS)
def test_class_I_block_is_the_integer_model_bit_for_bit(tmp_path, ss, relus, ds, co):
    k, b, dw, dwb, pw, pwb = sc.i_front(ss, relus, ds, co)
    ran_fused = set()
    for (H, W), frames in sc.inputs(True, ss):
        net, fused = front_net(tmp_path, "if", H, W, 128.0 * k, b, ss, relus, dw, dwb, ds, pw, pwb)
        for i, (rows, cols, pitch) in enumerate(frames):
            fr = sc.frames("I", (H, W), i, rows, cols)
            want = sm.front_int(fr, rows, cols, H, W, ss, k, b, relus[0], dw, dwb, ds, relus[1], pw, pwb, relus[2]) / 2
            for pt in pitches(cols, pitch, fused):
                for cus in (0, 1):
                    (got,) = net.run(fr, pt, cus)
                    assert_equal(got, want, f"{'front_kernel' if fused else 'separate layers'} {H}x{W} frame {rows}x{cols} pitch {pt} cus {cus}")
                if fused:
                    ran_fused.add(pt % 4 == 0)
    assert ran_fused == ({True, False} if ds == 1 else set())           # both front_kernel<STEP4> wherever the block has the one-kernel form


# ------------------------------------------------------------------------------------------------------------------------ class P
@pytest.mark.parametrize("c,s", sc.P_STEMS, ids=[f"c{c}-s{s}" for c, s in sc.P_STEMS])
def test_class_P_stem_gives_the_exact_product_of_all_three_pieces(tmp_path, c, s):
    K, _ = sc.p_stem(c, s)
    assert stem_kernel(c) == "stem_mfma_kernel"
    for (H, W), frames in sc.inputs():
        path = sc.stem_graph(str(tmp_path / f"p_{H}x{W}.onnx"), H, W, sm.onnx_from_window(K), np.zeros(c), s, "none")
        ops, desc = plan_ops(path, H, W)
        assert len(ops) == 1 and ops[0].startswith(stem_line(H, W, c, s, "none")), desc
        net = Net(path, (H, W))
        keep = ~sm.ring(H, W, s)
        for i, (rows, cols, pitch) in enumerate(frames):
            fr = sc.frames("P", (H, W), i, rows, cols)
            want = sm.stem_exact(fr, H, W, s, K)
            for cus in (0, 1):
                (got,) = net.run(fr, pitch, cus)
                assert_equal(got, want, f"stem_mfma_kernel {H}x{W} frame {rows}x{cols} pitch {pitch} cus {cus}", keep)


@pytest.mark.parametrize("ss,mode", sc.P_FRONTS, ids=[f"s{ss}-{m}" for ss, m in sc.P_FRONTS])
def test_class_P_front_kernel_gives_the_exact_product_of_all_three_pieces(tmp_path, ss, mode):
    for rnd in range(sc.P_ROUNDS[mode]):
        K, _, relus, dw, pw = sc.p_front(ss, mode, rnd)
        zero = np.zeros(16)
        for (H, W), frames in sc.inputs(True, ss, fused_only=True):
            net, fused = front_net(tmp_path, f"pf{rnd}", H, W, sm.onnx_from_window(K), zero, ss, relus, dw, zero, 1, pw, np.zeros(len(pw)))
            assert fused
            keep = ~sm.ring(H, W, ss)
            for i, (rows, cols, pitch) in enumerate(frames):
                fr = sc.frames("P", (H, W), i, rows, cols)
                want = sc.front_exact(sm.stem_exact(fr, H, W, ss, K), relus, pw)
                for pt in pitches(cols, pitch, True):
                    (got,) = net.run(fr, pt)
                    assert_equal(got, want, f"front_kernel round {rnd} {H}x{W} frame {rows}x{cols} pitch {pt}", keep)


# ------------------------------------------------------------------------------------------------------------------------ class D
def assert_within(got, ref, bound, tag):
    ratio = np.abs(got.reshape(ref.shape).astype(np.float64) - ref) / bound
    assert np.isfinite(ratio).all() and ratio.max() <= 1.0, f"{tag}: |gpu - fp64| / bound = {ratio.max():.3f}"
    return float(ratio.max())


@pytest.mark.parametrize("c,s,act", sc.D_STEMS, ids=[f"c{c}-s{s}-{a}" for c, s, a in sc.D_STEMS])
def test_class_D_stem_dense_weights_within_the_derived_bar_of_fp64(tmp_path, c, s, act):
    w, b = sc.d_stem(c, s, act)
    wf, bf = sm.fold(w, b)
    worst = 0.0
    for (H, W), frames in sc.inputs():
        path = sc.stem_graph(str(tmp_path / f"d_{H}x{W}.onnx"), H, W, w, b, s, act)
        ops, desc = plan_ops(path, H, W)
        assert len(ops) == 1 and ops[0].startswith(stem_line(H, W, c, s, act)), desc
        net = Net(path, (H, W))
        for i, (rows, cols, pitch) in enumerate(frames):
            fr = sc.frames("D", (H, W), i, rows, cols)
            ref = sm.stem_fp64(fr, H, W, s, w, b)
            if act == "relu":
                ref = np.maximum(ref, 0)                               # (1-Lipschitz: the bar holds behind it)
            (got,) = net.run(fr, pitch)
            worst = max(worst, assert_within(got, ref, sm.d_bound(fr, H, W, s, wf, bf), f"{H}x{W} frame {rows}x{cols}"))
    print(f"class D stem_mfma_kernel c{c} s{s} {act}: worst |gpu - fp64| / bound = {worst:.4f}")


@pytest.mark.parametrize("ss,mode", sc.D_FRONTS, ids=[f"s{ss}-{m}" for ss, m in sc.D_FRONTS])
def test_class_D_front_kernel_dense_weights_within_the_derived_bar_of_fp64(tmp_path, ss, mode):
    w, b, relus, dw, pw = sc.d_front(ss, mode)
    wf, bf = sm.fold(w, b)
    zero = np.zeros(16)
    worst = 0.0
    for (H, W), frames in sc.inputs(True, ss, fused_only=True):
        net, fused = front_net(tmp_path, "df", H, W, w, b, ss, relus, dw, zero, 1, pw, np.zeros(len(pw)))
        assert fused
        for i, (rows, cols, pitch) in enumerate(frames):
            fr = sc.frames("D", (H, W), i, rows, cols)
            ref = sc.front_exact(sm.stem_fp64(fr, H, W, ss, w, b), relus, pw)
            bound = sm.d_bound(fr, H, W, ss, wf, bf) @ np.abs(pw).T.astype(np.float64)      # one stem value per output, sign +-1
            for pt in pitches(cols, pitch, True):
                (got,) = net.run(fr, pt)
                worst = max(worst, assert_within(got, ref, bound, f"{H}x{W} frame {rows}x{cols} pitch {pt}"))
    print(f"class D front_kernel s{ss} {mode}: worst |gpu - fp64| / bound = {worst:.4f}")
