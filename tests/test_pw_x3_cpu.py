"""The host side of the 1x1 convolutions' three-piece bf16 form (csrc/conv_plan.h: conv_pw_x3_bn, conv_pw_x3_pays through questions 6 and
7 of fh_debug_conv_plan), no GPU: the tile width's and the per-launch predicate's shape, swept over the 1x1 stride-1 geometries of SCRFD
det_500m (640 x 640) and MobileFaceNet (112 x 112) at B = 1 .. 256.  The operand model of the kernel is tests/wino_x3_model.py as it is: a
1x1 convolution is the GEMM that model states."""
import numpy as np

import facerecognizeonnx_amd as fa

PW, PW_X3, PW_X3_PAYS = 1, 6, 7

# (H = W, Cin, Cout): SCRFD det_500m's 1x1 stride-1 convolutions at 640 x 640 (the 288 / 152 / 72-deep ones, the FPN laterals) ...
SCRFD = [(20, 288, 288), (40, 152, 152), (40, 72, 152), (80, 72, 16), (40, 152, 16), (20, 288, 16)]
# ... and MobileFaceNet's (scale 2: expand / project / conv_sep)
MBF = [(56, 128, 128), (28, 128, 128), (28, 128, 256), (14, 256, 256), (14, 256, 512), (7, 512, 256), (7, 256, 256), (7, 256, 512)]
BATCHES = sorted(set(list(range(1, 33)) + [48, 64, 96, 100, 128, 192, 200, 255, 256]))
CUS = (1, 8, 64, 208, 256, 304)


def ask(what, args, n_out):
    a = np.asarray(args, np.int32)
    out = np.zeros(max(n_out, 1), np.int64)
    rc = fa.lib().fh_debug_conv_plan(what, a.ctypes.data, a.size, out.ctypes.data, n_out)
    assert rc == n_out, fa._lib.last_error()
    return [int(v) for v in out[:n_out]]


def geom(B, hw, cin, cout, cus, ks=1, stride=1, pad=0, n_outs=0, up2x=0):
    return [B, hw, hw, cin, cout, ks, stride, pad, n_outs, up2x, cus]


def kpad(cin):
    return -(-cin // 32) * 32


def test_width_divides_padded_cout_and_never_without_the_f32_form():
    """every geometry x batch x CU count: a width of 96 / 64 / 32 or none; none wherever conv_pw_bn has none; the tiles are whole (the width
    divides the padded Cout, the padded columns stay inside the weight image's rows) and at least one per CU; 288 columns are three exact
    96-wide tiles"""
    seen = set()
    for hw, cin, cout in SCRFD + MBF:
        for B in BATCHES:
            for cus in CUS:
                g = geom(B, hw, cin, cout, cus)
                f32 = ask(PW, g, 1)[0]
                bn, tiles, on = ask(PW_X3, g, 3)
                assert bn in (0, 32, 64, 96), (g, bn)
                if f32 == 0:
                    assert bn == 0 and tiles == 0 and on == 0, g
                if bn:
                    M = B * hw * hw
                    cols = -(-cout // bn) * bn
                    assert M % 128 == 0 and cols % bn == 0 and cols - cout < bn and cols <= -(-cout // 128) * 128, g
                    assert tiles == (M // 128) * (cols // bn) and tiles >= cus, (g, tiles)
                    if cout == 288:
                        assert bn == 96 and cols == 288
                    seen.add(bn)
                else:
                    assert on == 0
    assert seen == {32, 64, 96} or seen == {64, 96}, seen


def test_layers_without_the_form():
    """3x3, strided, merged outputs, Cin or Cout not a multiple of 4, ragged M: no width"""
    for g in (geom(128, 20, 288, 288, 8, ks=3, pad=1), geom(128, 20, 288, 288, 8, stride=2), geom(128, 20, 288, 288, 8, n_outs=2),
              geom(128, 20, 286, 288, 8), geom(128, 20, 288, 30, 8), geom(3, 20, 288, 288, 1), geom(1, 20, 288, 288, 1)):
        assert ask(PW_X3, g, 3) == [0, 0, 0], g
    assert ask(PW_X3, geom(8, 20, 288, 288, 8), 3)[0] == 96


def test_width_is_monotone_in_batch_along_whole_tiles():
    """with the batch growing along whole 128-row tiles a form, once there, stays, and keeps its width"""
    for hw, cin, cout in SCRFD + MBF:
        for cus in CUS:
            last = 0
            for B in range(8, 257, 8):                       # (7 x 7 maps: every 128th image count closes a tile; 8 x n does for the rest)
                if (B * hw * hw) % 128:
                    continue
                bn = ask(PW_X3, geom(B, hw, cin, cout, cus), 3)[0]
                assert bn == last or last == 0, (hw, cin, cout, cus, B, bn, last)
                last = bn


def test_pays_is_monotone_in_tiles_and_depth():
    grid = sorted(set(list(range(0, 700)) + [784, 1568, 3136, 6400, 1 << 20]))
    kpads = (32, 64, 96, 128, 160, 256, 288, 512, 1024)
    for cout in (16, 64, 128, 152, 256, 288, 512):
        for cus in CUS:
            last_thr = None
            for kp in kpads:                                   # deeper: the threshold in tiles never rises
                on = [ask(PW_X3_PAYS, [t, kp, cout, cus], 1)[0] for t in grid]
                assert on[0] == 0 and on == sorted(on), (kp, cout, cus)
                thr = grid[on.index(1)] if 1 in on else None
                if last_thr is not None:
                    assert thr is not None and thr <= last_thr, (kp, cout, cus, thr, last_thr)
                if thr is not None:
                    assert thr >= cus                              # never with less than a tile per CU
                    last_thr = thr
            for t in (1, cus, 4 * cus, 100 * cus):
                on = [ask(PW_X3_PAYS, [t, kp, cout, cus], 1)[0] for kp in kpads]
                assert on == sorted(on), (t, cout, cus, on)


def test_pays_refuses_what_the_kernel_lacks():
    L = fa.lib()
    for cout in (1, 3, 30, 150):
        for kp in (32, 96, 288):
            assert ask(PW_X3_PAYS, [1 << 20, kp, cout, 8], 1) == [0]
    assert ask(PW_X3_PAYS, [1 << 20, 72, 152, 8], 1) == [0]           # Kpad is whole chunks
    out = np.zeros(3, np.int64)
    for bad in ([-1, 96, 152, 256], [10, 0, 152, 256], [10, 96, 0, 256], [10, 96, 152, 0]):
        a = np.asarray(bad, np.int32)
        assert L.fh_debug_conv_plan(PW_X3_PAYS, a.ctypes.data, 4, out.ctypes.data, 1) < 0
    a = np.asarray(geom(8, 20, 288, 288, 8), np.int32)
    assert L.fh_debug_conv_plan(PW_X3, a.ctypes.data, 10, out.ctypes.data, 3) < 0
    assert L.fh_debug_conv_plan(PW_X3, a.ctypes.data, 11, out.ctypes.data, 2) < 0


def test_question_6_agrees_with_question_7():
    """the third answer of question 6 is conv_pw_x3_pays of the launch's own tiles and padded depth"""
    for hw, cin, cout in SCRFD + MBF:
        for B in (8, 64, 128, 256):
            for cus in (8, 256):
                bn, tiles, on = ask(PW_X3, geom(B, hw, cin, cout, cus), 3)
                if bn:
                    assert on == ask(PW_X3_PAYS, [tiles, kpad(cin), cout, cus], 1)[0]
