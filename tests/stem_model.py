"""Exact models of the u8 entry of both networks: the fused stems (csrc/stem.hip over csrc/stem_tile.h) and the stem -> depthwise ->
pointwise block of front_kernel (csrc/dwpw_mfma.hip).

THE WEIGHTS.  engine.cpp folds the preprocess (v - 127.5) / 128 into the filter (`fold`): wf = w / 128 in the byte order of a BGR pixel,
bf = b - 127.5 / 128 * sum(w).  The matrix-core kernels carry every wf as three bf16 terms (`split_rne3`, stem_pack_wfrag's rule — round
to nearest even three times, NOT the truncating rule of tests/wino_x3_model.py) laid out as the A fragments of v_mfma_f32_16x16x32_bf16
(`pack_wfrag`).

THE WINDOW.  An output pixel reads three rows of nine bytes (`windows`): byte j of row g is byte j % 3 (B, G, R) of the pixel in window
column j // 3.  A position outside the net input is the convolution's zero padding = the byte value 127.5 of the folded form; inside the
net input but outside the pasted frame it is the letterbox canvas, byte 0; otherwise the frame's byte.

THREE CLASSES OF OPERANDS hold the kernels to that (tests/test_stem_model_cpu.py pins the model and their preconditions,
tests/test_gpu_stem_exact.py runs them):
  I  integer k = w / 128 and integer biases: 2 y = sum k (2 x - 255) + 2 b is an integer and every partial sum of every kernel, in any
     order, is a multiple of 1/2 far below 2^23 — the output is `stem_int` / `front_int` bit for bit.  Wrong bytes, wrong padding.
  P  two taps +w, -w per channel, w of three non-zero pieces, bytes 0..15: w (x1 - x2) fits 24 bits — the output is the exact
     product.  A lost, doubled or misplaced piece.
  D  dense 24-bit weights against fp64 at a derived bar (`d_bound`).
Everything here is numpy and Python ints on the CPU; tests/test_stem_model_cpu.py checks it in exact rational arithmetic.
"""
from __future__ import annotations

import numpy as np

from tests import wino_split_model as wm

gamma = wm.gamma
UNIT = 16                                           # `epilogue_int` counts in 1/16: 2 y is an integer, PReLU 1/4 and s2 = 1/2 take three more bits
FRAMES = [(64, 41, 125), (41, 64, 192), (64, 2, 7), (64, 3, 10), (64, 1, 5), (33, 47, 47 * 3)]      # rows, cols, pitch on the 64 x 64 net input
FRAME_FULL = (56, 72, 216)                          # the whole 56 x 72 net input: ragged 16 x 16 and 8 x 16 tiles at both strides


# ---------------------------------------------------------------------------------------------------------------- weights: split, pack, fold
def bf16_rne(x):
    """f32 (finite) -> the nearest bf16, ties to even, as f32"""
    x = np.ascontiguousarray(x, np.float32)
    return (wm._rne_bf16_bits(x.view(np.uint32)) << 16).astype(np.uint32).view(np.float32)


def split_rne3(w):
    """w (f32) -> (hi, mid, lo) as f32: hi = bf16_rne(w), mid = bf16_rne(w - hi), lo = bf16_rne(w - hi - mid), the differences in f32"""
    w = np.ascontiguousarray(w, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = bf16_rne(w)
        r1 = (w - hi).astype(np.float32)
        mid = bf16_rne(r1)
        r2 = (r1 - mid).astype(np.float32)
        return hi, mid, bf16_rne(r2)


W_MIN, W_MAX = 2.0 ** -103, float(np.array([0x7F7F7FFF], np.uint32).view(np.float32)[0])


def split_domain(w):
    """True where "hi + mid + lo = w exactly" is promised: w = 0, or 2^-103 <= |w| <= 0x7F7F7FFF (the last f32 that does not round to
    the bf16 Inf).  Every bit of such a w lies at 2^-126 or above, so each remainder is zero or a normal number and each piece — at most
    8, 8 and 8 of w's 24 bits — is zero or a bf16 normal.  Below 2^-103 a remainder may fall under the normal range, where bf16 has
    fewer bits than f32 (and the matrix cores read subnormals as zero)."""
    a = np.abs(np.ascontiguousarray(w, np.float32).astype(np.float64))
    return (a == 0) | ((a >= W_MIN) & (a <= W_MAX))


def bf16_bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint32)


def k_source(k):
    """K index 0..31 of the MFMA -> row of wf [27][Cout] (window row g, byte j -> g * 9 + j), or -1 for the zero columns 27..31"""
    if k < 24:
        return (k >> 3) * 9 + (k & 7)
    return (k - 24) * 9 + 8 if k < 27 else -1


def pack_wfrag(wf, Cout, pieces=split_rne3):
    """wf [27][Cout] (f32) -> the [Cout / 16][3][64][4] dword image: lane l = channel l & 15, K block l >> 4, its eight bf16 = K indices
    8 g .. 8 g + 7, two per dword (even K in the low half); blocks in the order hi, mid, lo"""
    wf = np.ascontiguousarray(wf, np.float32).reshape(27, Cout)
    wk = np.zeros((32, Cout), np.float32)
    for k in range(27):
        wk[k] = wf[k_source(k)]
    bits = [bf16_bits(p) for p in pieces(wk)]                          # [32][Cout] each
    out = np.zeros((Cout // 16, 3, 64, 4), np.uint32)
    for cb in range(Cout // 16):
        for q in range(3):
            for l in range(64):
                co, g = cb * 16 + (l & 15), l >> 4
                for d in range(4):
                    out[cb, q, l, d] = bits[q][8 * g + 2 * d, co] | (bits[q][8 * g + 2 * d + 1, co] << 16)
    return out


def fold(w_onnx, b_onnx):
    """ONNX stem filter [Cout][3 R, G, B][3][3] and bias (f32) -> (wf [27][Cout], bf [Cout]) as engine.cpp forms them: wf[(ky * 3 + kx) * 3
    + j] = w[2 - j] / 128 in f32 (j = byte of the BGR pixel), bf = float(double(b) - 127.5 / 128 * sum(w)), the sum in fp64 in tap order"""
    w = np.ascontiguousarray(w_onnx, np.float32)
    Cout = w.shape[0]
    wf = np.empty((27, Cout), np.float32)
    bf = np.empty(Cout, np.float32)
    for co in range(Cout):
        s = 0.0
        for t in range(9):
            for j in range(3):
                v = w[co, 2 - j, t // 3, t % 3]
                wf[t * 3 + j, co] = v / np.float32(128.0)
                s += float(v)
        bf[co] = np.float32(float(np.float32(b_onnx[co])) - 127.5 / 128.0 * s)
    return wf, bf


def window_weights(w):
    """[Cout][3 R, G, B][3][3] (any dtype) -> K [Cout][3 rows][9 bytes]: the weight of byte j of window row g, K[co][g][3 kx + jb] =
    w[co][2 - jb][g][kx]"""
    w = np.asarray(w)
    return np.ascontiguousarray(w[:, ::-1].transpose(0, 2, 3, 1).reshape(w.shape[0], 3, 9))


# ---------------------------------------------------------------------------------------------------------------- the window
def out_hw(inH, inW, stride):
    return (inH - 1) // stride + 1, (inW - 1) // stride + 1


def windows2(frames, inH, inW, stride, pad2=255, canvas2=0, shift=(0, 0, 0)):
    """frames [B][rows][cols][3] u8 (BGR), pasted at the net input's origin -> TWICE the byte value of every window position,
    int64 [B][Ho][Wo][3][9].  pad2 / canvas2: twice the value of the convolution padding (127.5) and of the canvas (0); shift[g]: window
    row g starts that many bytes late (all three are the model's own — the wrong variants of the power test change them)."""
    frames = np.asarray(frames)
    B, rows, cols, _ = frames.shape
    assert rows <= inH and cols <= inW
    plane = np.full((B, inH + 2, 3 * (inW + 2) + 3), pad2, np.int64)
    plane[:, 1:inH + 1, 3:3 * (inW + 1)] = canvas2
    plane[:, 1:rows + 1, 3:3 * (cols + 1)] = 2 * frames.reshape(B, rows, cols * 3).astype(np.int64)
    Ho, Wo = out_hw(inH, inW, stride)
    g = np.arange(3)
    yy = (np.arange(Ho) * stride)[:, None, None, None] + g[None, None, :, None]
    xx = (3 * stride * np.arange(Wo))[None, :, None, None] + np.asarray(shift)[None, None, :, None] + np.arange(9)[None, None, None, :]
    return plane[:, yy, xx]


def ring(inH, inW, stride):
    """bool [Ho][Wo]: outputs whose window touches the convolution padding (row / column -1, or inH / inW)"""
    Ho, Wo = out_hw(inH, inW, stride)
    oy, ox = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    return (oy == 0) | (ox == 0) | (oy * stride + 1 >= inH) | (ox * stride + 1 >= inW)


# ---------------------------------------------------------------------------------------------------------------- class I: integers
def stem_int(frames, rows, cols, inH, inW, stride, k, b, **variant):
    """2 y as int64 [B][Ho][Wo][Cout] for integer k = w_onnx / 128 [Cout][3][3][3] and integer b: 2 y = sum k (2 x - 255) + 2 b; a tap
    outside the net input has 2 x = 255 and contributes 0, a tap on the canvas x = 0"""
    frames = np.asarray(frames)
    assert frames.shape[1:] == (rows, cols, 3)
    K = np.asarray(variant.pop("K") if "K" in variant else window_weights(np.asarray(k, np.int64)), np.float64)
    X2 = windows2(frames, inH, inW, stride, **variant)
    y2 = (X2 - 255).reshape(-1, 27).astype(np.float64) @ K.reshape(-1, 27).T       # (integers far below 2^53: exact, and quick)
    return np.rint(y2).astype(np.int64).reshape(X2.shape[:3] + (K.shape[0],)) + 2 * np.asarray(b, np.int64)


def epilogue_int(y2, act, t2=None):
    """2 y -> (UNIT * out1, UNIT * out2 or None): ReLU | PReLU with slope 1/4 | none, out2 = out1 / 2 + t2 (integer t2)"""
    y = np.asarray(y2, np.int64) * (UNIT // 2)
    if act == "relu":
        y = np.maximum(y, 0)
    elif act == "prelu":
        y = np.where(y >= 0, y, y // 4)                                # (a multiple of 8: the division is exact)
    else:
        assert act == "none"
    return y, None if t2 is None else y // 2 + UNIT * np.asarray(t2, np.int64)


def dw_int(m, taps, bias2, stride):
    """depthwise 3x3, zero padding of the MAP m [B][H][W][C] (int64), integer taps [C][3][3], bias2 = twice the bias"""
    B, H, W, Cc = m.shape
    Ho, Wo = out_hw(H, W, stride)
    p = np.zeros((B, H + 2, W + 2, Cc), np.int64)
    p[:, 1:-1, 1:-1] = m
    out = np.zeros((B, Ho, Wo, Cc), np.int64) + np.asarray(bias2, np.int64)
    for ky in range(3):
        for kx in range(3):
            out += p[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] * np.asarray(taps, np.int64)[:, ky, kx]
    return out


def front_int(frames, rows, cols, inH, inW, stride, k, b, stem_relu, dw, dw_b, dw_stride, dw_relu, pw, pw_b, pw_relu, **variant):
    """2 x the block's output, int64 [B][Ho][Wo][Cout]: stem_int -> (ReLU) -> depthwise 3x3 (integer taps dw [C][3][3], bias dw_b) ->
    (ReLU) -> pointwise (integer pw [Cout][C], bias pw_b) -> (ReLU)"""
    relu = lambda v, on: np.maximum(v, 0) if on else v                 # noqa: E731
    m = relu(stem_int(frames, rows, cols, inH, inW, stride, k, b, **variant), stem_relu)
    m = relu(dw_int(m, dw, 2 * np.asarray(dw_b, np.int64), dw_stride), dw_relu)
    return relu(m @ np.asarray(pw, np.int64).T + 2 * np.asarray(pw_b, np.int64), pw_relu)


def draw_int(rng, Cout, kmax):
    """class I stem operands: k uniform in -kmax..kmax [Cout][3][3][3], bias in -8..8"""
    return rng.integers(-kmax, kmax + 1, (Cout, 3, 3, 3)), rng.integers(-8, 9, Cout)


def draw_front(rng, Cout):
    """class I block operands behind a 16-channel stem: depthwise taps and pointwise weights in {-1, 0, 1}, biases in -8..8"""
    return rng.integers(-1, 2, (16, 3, 3)), rng.integers(-8, 9, 16), rng.integers(-1, 2, (Cout, 16)), rng.integers(-8, 9, Cout)


# ---------------------------------------------------------------------------------------------------------------- class P: pieces
P_BYTES = 16                                        # frame bytes 0..15


def draw_pieces(rng, n, first=0):
    """class P, n channels: channel c has exactly two non-zero taps, +w at window position (first + c) % 27 and -w thirteen positions
    further (mod 27; position = 9 g + j), so that 27 consecutively dealt channels use every position as + and as -.
    w = (h + m + l) 2^e with h in {1.25, 1.5, 1.75}, m = +-2^-9, l = +-2^-19, e in -3..0: 20 bits, three non-zero pieces, no tie.
    -> (wf K [n][3][9] f32, the pieces (hi, mid, lo) of K as they were drawn)"""
    K = np.zeros((n, 27), np.float32)
    P = [np.zeros((n, 27), np.float32) for _ in range(3)]
    for c in range(n):
        e = int(rng.integers(-3, 1))
        h = (1.25, 1.5, 1.75)[int(rng.integers(3))] * 2.0 ** e
        m = (1, -1)[int(rng.integers(2))] * 2.0 ** (e - 9)
        l = (1, -1)[int(rng.integers(2))] * 2.0 ** (e - 19)
        plus = (first + c) % 27
        for pos, sg in ((plus, 1), ((plus + 13) % 27, -1)):
            K[c, pos] = np.float32(sg * (h + m + l))
            for q, v in enumerate((h, m, l)):
                P[q][c, pos] = np.float32(sg * v)
    return K.reshape(n, 3, 9), tuple(p.reshape(n, 3, 9) for p in P)


def onnx_from_window(K):
    """K [Cout][3][9] = wf in window order -> the ONNX filter [Cout][3 R, G, B][3][3] = 128 wf (exact)"""
    K = np.asarray(K, np.float32)
    return np.ascontiguousarray((K * np.float32(128.0)).reshape(K.shape[0], 3, 3, 3)[..., ::-1].transpose(0, 3, 1, 2))


def stem_exact(frames, inH, inW, stride, K, bf=None, **variant):
    """sum K x (+ bf) over the window in fp64, [B][Ho][Wo][Cout] — exact wherever the caller's operands make every product and sum fit
    (class P: 24 bits; asserted there), the fp64 reference otherwise"""
    X = windows2(frames, inH, inW, stride, **variant).astype(np.float64) / 2
    y = np.einsum("byxgj,cgj->byxc", X, np.asarray(K, np.float64))
    return y if bf is None else y + np.asarray(bf, np.float64)


# ---------------------------------------------------------------------------------------------------------------- class D: dense
def d_bound(frames, inH, inW, stride, wf, bf):
    """class D's bar per element, 2 gamma_100 S with S = sum |wf| x + |bf| on the folded form the kernel computes (padding = 127.5): 100 =
    three MFMAs of 32 exact products + three accumulator hand-overs + the rounding of bf; the factor 2 covers the instruction's internal
    additions, as in the x3 bars"""
    K = np.abs(np.asarray(wf, np.float64)).reshape(3, 9, -1).transpose(2, 0, 1)
    S = stem_exact(frames, inH, inW, stride, K) + np.abs(np.asarray(bf, np.float64))
    return 2 * gamma(100) * S


def stem_fp64(frames, inH, inW, stride, w_onnx, b_onnx):
    """the ONNX form sum w (x - 127.5) / 128 + b in fp64: padding taps contribute 0, the canvas is x = 0"""
    K = window_weights(np.asarray(w_onnx, np.float32).astype(np.float64))
    X = windows2(frames, inH, inW, stride).astype(np.float64) / 2
    return np.einsum("byxgj,cgj->byxc", (X - 127.5) / 128.0, K) + np.asarray(b_onnx, np.float32).astype(np.float64)


def stem_f32(frames, inH, inW, stride, wf, bf):
    """the folded form in plain f32, one fused-free chain per output: acc = bf, then acc = fl(acc + fl(wf x)) over the 27 bytes (each
    product of a 24-bit weight and a byte is NOT exact in f32 — this is the vector kernels' arithmetic, the model's own check of the bar)"""
    X = (windows2(frames, inH, inW, stride).astype(np.float64) / 2).astype(np.float32)
    K = np.asarray(wf, np.float32).reshape(3, 9, -1)
    acc = np.broadcast_to(np.asarray(bf, np.float32), X.shape[:3] + (K.shape[2],)).copy()
    for g in range(3):
        for j in range(9):
            acc = (acc + (X[..., g, j, None] * K[g, j]).astype(np.float32)).astype(np.float32)
    return acc
