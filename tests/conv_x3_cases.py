"""The layers tests/test_gpu_conv_x3.py runs through fh_conv_forward_ex_dev, and the launch arithmetic that says which stream-K role each
reaches.  No GPU here: tests/test_conv_x3_cpu.py holds every dense case to the role it claims through fh_debug_conv_plan.

All layers are 3x3, stride 2, pad 1; `sc` = channels of the folded 1x1 stride-2 shortcut (0 = none), which reads an input of the same
map size as the 3x3's.  The x3 kernel's tile is 128 x 128 where Cout % 128 == 0 and 128 x 64 otherwise; it holds two workgroups per CU."""
from __future__ import annotations

from collections import namedtuple

Case = namedtuple("Case", "B H W Cin Cout sc cus")

# One-hot cases: both tile widths (Cout 64, 192: 128 x 64; 128: 128 x 128), a last column tile behind the first (192 = 3 x 64), both chunk
# counts per tap (Cin 32: one, 64: two), an odd map (9 x 7 -> 5 x 4) and an even one whose last input row and column are never a window's
# centre (16 x 16 -> 8 x 8), B = 3: M = 60 and 192 rows, ragged against 128; with and without a shortcut of another channel count.
ONE_HOT = [Case(3, H, W, Cin, Cout, sc, 0) for (H, W) in ((9, 7), (16, 16)) for Cin in (32, 64) for Cout in (64, 128, 192) for sc in (0, 32)]

# Dense cases by stream-K role (the f32 plan's constants hold for x3 launches too):
#   plain   8 tiles on 8 slots: one whole round, nothing to cut
#   owners  22 tiles of 40 chunks on 16 slots: 16 whole, 6 remainder tiles with an owner each (16 chunks of its own) and 10 helpers
#   fixup   2 tiles of 19 chunks on 16 slots: an owner would keep 4 chunks (< 12), so every segment goes to a slab and conv_fixup_kernel sums
DENSE = {
    "plain": Case(2, 32, 32, 32, 256, 0, 4),
    "owners": Case(27, 14, 14, 128, 256, 128, 8),
    "fixup": Case(3, 9, 7, 64, 256, 32, 8),
}
# The locality legs: a layer with a shortcut, several tiles, the device's own CU count.
LOCALITY = Case(3, 16, 16, 64, 128, 32, 0)


def out_hw(c):
    return (c.H + 2 - 3) // 2 + 1, (c.W + 2 - 3) // 2 + 1


def kpad(c):
    return 9 * c.Cin + c.sc


def x3_bn(cout):
    return 128 if cout % 128 == 0 else 64


def plan_inputs(c):
    """question 0 of fh_debug_conv_plan for the x3 launch of case c: T tiles, S slots, chunks, accumulators per tile, CUs, Kpad, tile0, slabs"""
    ho, wo = out_hw(c)
    bn = x3_bn(c.Cout)
    tiles = -(-c.B * ho * wo // 128) * (c.Cout // bn)
    return [tiles, 2 * c.cus, kpad(c) // 32, 128 * bn, c.cus, kpad(c), 0, 1]
