"""The cases, operands and graphs of tests/test_gpu_stem_exact.py, drawn here so that tests/test_stem_model_cpu.py asserts the classes'
preconditions and runs the power test on exactly the operands the GPU sees (classes I, P, D: tests/stem_model.py)."""
from __future__ import annotations

import zlib

import numpy as np

from tests import stem_model as sm

B = 3
# net input (H, W) -> the frames pasted into it at letterbox scale 1
INPUTS = [((64, 64), sm.FRAMES), ((56, 72), [sm.FRAME_FULL])]
# The planner fuses the block (DW+PW, front_kernel) from 1600 outputs on: behind a stride-2 stem that takes a net input of twice the
# side.  The same frames, one that reaches the lower edge with canvas on its right, and the full frame of a ragged map (56 x 72).
BIG_INPUTS = [((128, 128), sm.FRAMES + [(128, 83, 83 * 3 + 2)]), ((112, 144), [(112, 144, 432)])]
CHANNELS = (8, 24, 16, 32, 48, 64)                  # stem_conv_u8_kernel | stem_conv_px_kernel + stem_conv_border_kernel | stem_mfma_kernel
MFMA_CHANNELS = (48, 64)
ACTS = ("relu", "prelu", "none")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def inputs(front=False, ss=1, fused_only=False):
    """[((H, W) of the net input, [(rows, cols, pitch)])] of a stem case, or of a block case behind a stem of stride `ss` (frames of two
    pixels' width and more; fused_only: only the inputs at which the block runs in front_kernel)"""
    if not front:
        return INPUTS
    src = INPUTS if ss == 1 else BIG_INPUTS if fused_only else INPUTS + BIG_INPUTS
    return [(hw, [f for f in fr if f[1] >= 2]) for hw, fr in src]


def front_fused(H, W, ss, ds):
    """does the planner hand the block to front_kernel?  (plan.cpp: stride-1 depthwise, >= 1600 outputs; front_fused_ok)"""
    Hs, Ws = sm.out_hw(H, W, ss)
    return ds == 1 and Hs * Ws >= 1600


def frames(cls, hw, k, rows, cols):
    """noise frames [B][rows][cols][3]; class P: bytes 0..15"""
    rng = np.random.default_rng(_seed("frames", cls, hw, k))
    return rng.integers(0, sm.P_BYTES if cls == "P" else 256, (B, rows, cols, 3), dtype=np.uint8)


def staged(fr, pitch):
    """frames -> [B][rows][pitch] u8, the pitch bytes that are no pixel = 255"""
    n, rows, cols, _ = fr.shape
    img = np.full((n, rows, pitch), 255, np.uint8)
    img[:, :, :cols * 3] = fr.reshape(n, rows, cols * 3)
    return img


def other_pitch(cols, pitch):
    """the front kernel's other instantiation for the same frame: a multiple of 4 where the table's pitch is none, and the reverse"""
    return pitch + 1 if pitch % 4 == 0 else (pitch + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------------------------------ graphs
def stem_graph(path, H, W, w, b, stride, act, t2=None):
    """input [1,3,H,W] -> y = Conv3x3(w, b) stride `stride` (+ReLU | +PReLU 1/4 | nothing) -> out0 [H'W', C]; with t2 also
    BatchNormalization(y) = y / 2 + t2 -> out1 (epsilon 0, variance 4: the scale is 1/2 exactly).  The stem's maps ARE the outputs."""
    from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder
    C = len(b)
    g = OnnxBuilder("stem_exact")
    x = g.add_input("input.1", [1, 3, H, W])
    y = g.node("Conv", [x, g.init("stem.w", np.asarray(w, np.float32)), g.init("stem.b", np.asarray(b, np.float32))],
               kernel_shape=[3, 3], strides=[stride, stride], pads=[1, 1, 1, 1], dilations=[1, 1], group=1)
    if act == "relu":
        y = g.node("Relu", [y])
    elif act == "prelu":
        y = g.node("PRelu", [y, g.init("stem.slope", np.full((C, 1, 1), 0.25, np.float32))])
    outs = [y]
    if t2 is not None:
        outs.append(g.node("BatchNormalization", [y, g.init("bn.weight", np.ones(C, np.float32)), g.init("bn.bias", np.asarray(t2, np.float32)),
                                                  g.init("bn.running_mean", np.zeros(C, np.float32)),
                                                  g.init("bn.running_var", np.full(C, 4.0, np.float32))], epsilon=0.0, momentum=0.9))
    for i, z in enumerate(outs):
        z = g.node("Transpose", [z], perm=[0, 2, 3, 1])
        g.node("Reshape", [z, g.init(f"shape{i}", np.array([-1, C], np.int64))], outputs=[f"out{i}"])
        g.add_output(f"out{i}", ["A", C])
    return g.save(path)


def front_graph(path, H, W, w, b, stride, relus, dw, dw_b, dw_stride, pw, pw_b):
    """util.dwpw_graph with given weights: Conv3x3(3 -> 16) -> depthwise 3x3 stride `dw_stride` -> pointwise, a ReLU behind each where
    relus = (stem, depthwise, pointwise) says so -> [H'W', Cout]"""
    from facerecognizeonnx_amd.synth.onnx_writer import OnnxBuilder
    Cc, Cout = len(b), len(pw_b)
    g = OnnxBuilder("front_exact")
    x = g.add_input("input", [1, 3, H, W])

    def conv(x, tag, w, bias, relu, **kw):
        y = g.node("Conv", [x, g.init(tag + ".w", np.asarray(w, np.float32)), g.init(tag + ".b", np.asarray(bias, np.float32))], **kw)
        return g.node("Relu", [y]) if relu else y
    y = conv(x, "stem", w, b, relus[0], kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[stride, stride])
    y = conv(y, "dw", np.asarray(dw).reshape(Cc, 1, 3, 3), dw_b, relus[1], kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[dw_stride, dw_stride], group=Cc)
    y = conv(y, "pw", np.asarray(pw).reshape(Cout, Cc, 1, 1), pw_b, relus[2], kernel_shape=[1, 1], strides=[1, 1])
    y = g.node("Transpose", [y], perm=[0, 2, 3, 1])
    g.node("Reshape", [y, g.init("shape", np.array([-1, Cout], np.int64))], outputs=["out"])
    g.add_output("out", ["A", Cout])
    return g.save(path)


# ------------------------------------------------------------------------------------------------------------------------ class I
I_STEMS = [(c, s, act, bn) for c in CHANNELS for s in (1, 2) for act in ACTS for bn in (False, True)]
#           stem stride, ReLUs (stem, depthwise, pointwise), depthwise stride, pointwise channels
I_FRONTS = [(ss, relus, ds, co) for ss in (1, 2) for relus in ((1, 1, 1), (0, 0, 0)) for ds in (1, 2) for co in (16, 24, 32)]


def i_stem(c, s, act, bn):
    """-> (k [C][3][3][3], b [C], t2 [C] or None), integers"""
    rng = np.random.default_rng(_seed("I", c, s, act, bn))
    k, b = sm.draw_int(rng, c, 7)
    return k, b, rng.integers(-8, 9, c) if bn else None


def i_front(ss, relus, ds, co):
    """-> (k, b, dw [16][3][3], dw_b, pw [co][16], pw_b), integers"""
    rng = np.random.default_rng(_seed("IF", ss, relus, ds, co))
    return sm.draw_int(rng, 16, 3) + sm.draw_front(rng, co)


# ------------------------------------------------------------------------------------------------------------------------ class P
P_STEMS = [(c, s) for c in MFMA_CHANNELS for s in (1, 2)]
# front_kernel: the stem's value in sign and magnitude behind the block.  "pm": nothing between stem and output but (first) the stem's
# ReLU, pointwise = [+1 one-hot; -1 one-hot] -> 32 outputs +-act(y).  "dup": a ReLU behind every layer, the stem's channels 8..15 are the
# negated filters of 0..7, pointwise = identity -> relu(y), relu(-y).
P_FRONTS = [(ss, mode) for ss in (1, 2) for mode in ("pm", "pm-relu", "dup")]
P_ROUNDS = {"stem": 1, "pm": 2, "pm-relu": 2, "dup": 4}             # draws until 27 consecutive channels have been dealt


def p_stem(c, s, rnd=0):
    """-> (K [C][3][9] f32 = wf in window order, its pieces as drawn)"""
    return sm.draw_pieces(np.random.default_rng(_seed("P", c, s, rnd)), c, first=c * rnd)


def p_front(ss, mode, rnd):
    """-> (K [16][3][9], pieces, relus, depthwise taps, pointwise [Cout][16]); depthwise = centre tap 1, all biases 0"""
    rng = np.random.default_rng(_seed("PF", ss, mode, rnd))
    dw = np.zeros((16, 3, 3), np.int64)
    dw[:, 1, 1] = 1
    eye = np.eye(16, dtype=np.int64)
    if mode == "dup":
        K, P = sm.draw_pieces(rng, 8, first=8 * rnd)
        return np.concatenate([K, -K]), tuple(np.concatenate([p, -p]) for p in P), (1, 1, 1), dw, eye
    K, P = sm.draw_pieces(rng, 16, first=16 * rnd)
    return K, P, (1 if mode == "pm-relu" else 0, 0, 0), dw, np.concatenate([eye, -eye])


def front_exact(y, relus, pw):
    """the block behind an exact stem map y [..][16] (fp64) for p_front's / d_front's depthwise copy and one-hot pointwise, zero biases"""
    relu = lambda v, on: np.maximum(v, 0) if on else v                 # noqa: E731
    return relu(relu(relu(y, relus[0]), relus[1]) @ np.asarray(pw, np.float64).T, relus[2])


# ------------------------------------------------------------------------------------------------------------------------ class D
D_STEMS = [(c, s, act) for c in MFMA_CHANNELS for s in (1, 2) for act in ("relu", "none")]
D_FRONTS = [(ss, mode) for ss in (1, 2) for mode in ("pm", "dup")]


def d_stem(c, s, act):
    """dense weights as util.stem_graph draws them -> (w [C][3][3][3] f32, b [C] f32)"""
    rng = np.random.default_rng(_seed("D", c, s, act))
    return (rng.standard_normal((c, 3, 3, 3)) / 5).astype(np.float32), (rng.standard_normal(c) / 10).astype(np.float32)


def d_front(ss, mode):
    """-> (w [16][3][3][3], b [16], relus, depthwise taps, pointwise); "dup": filters AND biases of channels 8..15 negate 0..7"""
    rng = np.random.default_rng(_seed("DF", ss, mode))
    n = 8 if mode == "dup" else 16
    w, b = (rng.standard_normal((n, 3, 3, 3)) / 5).astype(np.float32), (rng.standard_normal(n) / 10).astype(np.float32)
    dw = np.zeros((16, 3, 3), np.int64)
    dw[:, 1, 1] = 1
    eye = np.eye(16, dtype=np.int64)
    if mode == "dup":
        return np.concatenate([w, -w]), np.concatenate([b, -b]), (1, 1, 1), dw, eye
    return w, b, (0, 0, 0), dw, np.concatenate([eye, -eye])
