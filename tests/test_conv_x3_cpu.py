"""The host side of the direct convolutions' three-piece bf16 K loop (csrc/conv_plan.h: conv_x3_pays, conv_x3_bn through question 5 of
fh_debug_conv_plan), no GPU: the per-launch predicate's shape, and — for every dense case of tests/test_gpu_conv_x3.py — that the
stream-K plan of the `cus` the case passes puts its launch into the role the case is there for."""
import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from tests import conv_x3_cases as cx

STREAMK, X3 = 0, 5
FIELDS = ("full", "rem", "helpers", "owners", "fixup", "units", "q", "owner_chunks", "maxp")
MIN_OWNER = 12                                                             # ConvKnobs::sk_min_owner's default


def ask(what, args, n_out):
    a = np.asarray(args, np.int32)
    out = np.zeros(max(n_out, 1), np.int64)
    rc = fa.lib().fh_debug_conv_plan(what, a.ctypes.data, a.size, out.ctypes.data, n_out)
    assert rc == n_out, fa._lib.last_error()
    return [int(v) for v in out[:n_out]]


def pays(tiles, kpad, cout, cus):
    return ask(X3, [tiles, kpad, cout, cus], 2)


COUTS_WITH = (64, 128, 192, 256, 512)
COUTS_WITHOUT = (1, 3, 32, 48, 96, 100, 130, 160, 200)
KPADS = (32, 288, 320, 608, 640, 1216, 1280, 2432, 4864)
CUS = (1, 8, 64, 208, 256, 304)


def test_tile_width_follows_cout():
    for cout in COUTS_WITH:
        assert pays(1000, 1280, cout, 256)[1] == (128 if cout % 128 == 0 else 64)
    for cout in COUTS_WITHOUT:
        assert pays(1000, 1280, cout, 256)[1] == 0


def test_never_on_for_a_shape_the_kernel_lacks():
    """Cout % 64 != 0 has no x3 tile, whatever the launch looks like"""
    for cout in COUTS_WITHOUT:
        for kpad in KPADS:
            for cus in CUS:
                for tiles in (0, 1, cus, 2 * cus, 100 * cus, 1 << 20):
                    assert pays(tiles, kpad, cout, cus) == [0, 0], (tiles, kpad, cout, cus)


def test_monotone_in_tiles_with_a_threshold():
    """for every (Kpad, Cout, CUs): off at 0 tiles and below a threshold, on from the threshold up — never on, off, on — and the
    threshold does not fall when the chip grows.  A deep layer on a full chip (the headline's stride-2 layers) is on."""
    grid = sorted(set(list(range(0, 700)) + [784, 1568, 3136, 6272, 1 << 20]))
    for cout in COUTS_WITH:
        for kpad in KPADS:
            last_thr = -1
            for cus in CUS:
                on = [pays(t, kpad, cout, cus)[0] for t in grid]
                assert on[0] == 0
                flips = sum(a != b for a, b in zip(on, on[1:]))
                assert flips <= 1 and on == sorted(on), (kpad, cout, cus)
                thr = grid[on.index(1)] if 1 in on else None
                if thr is not None:
                    assert thr >= 1 and thr >= last_thr, (kpad, cout, cus, thr, last_thr)
                    last_thr = thr
    for tiles, kpad, cout in ((3136, 640, 64), (784, 1216, 128), (392, 2432, 256), (196, 4864, 512)):      # IResNet-50's four at B = 128
        assert pays(tiles, kpad, cout, 256)[0] == 1


def test_monotone_in_depth():
    for cout in COUTS_WITH:
        for cus in CUS:
            for tiles in (1, cus // 2, cus, 4 * cus):
                on = [pays(tiles, k, cout, cus)[0] for k in sorted(KPADS)]
                assert on == sorted(on), (tiles, cout, cus, on)


def test_bad_arguments_are_refused():
    L = fa.lib()
    out = np.zeros(2, np.int64)
    for bad in ([-1, 320, 64, 256], [10, 0, 64, 256], [10, 320, 0, 256], [10, 320, 64, 0]):
        a = np.asarray(bad, np.int32)
        assert L.fh_debug_conv_plan(X3, a.ctypes.data, 4, out.ctypes.data, 2) < 0
    a = np.asarray([10, 320, 64, 256], np.int32)
    assert L.fh_debug_conv_plan(X3, a.ctypes.data, 3, out.ctypes.data, 2) < 0
    assert L.fh_debug_conv_plan(X3, a.ctypes.data, 4, out.ctypes.data, 1) < 0


@pytest.mark.parametrize("role", sorted(cx.DENSE))
def test_dense_gpu_cases_reach_the_role_they_claim(role):
    c = cx.DENSE[role]
    args = cx.plan_inputs(c)
    p = dict(zip(FIELDS, ask(STREAMK, args, 9)))
    T, S, chunks = args[0], args[1], args[2]
    assert cx.kpad(c) % 32 == 0 and c.Cin % 32 == 0 and c.sc % 32 == 0 and c.Cout % 64 == 0
    if role == "plain":
        assert p["full"] == T and p["helpers"] == 0 and p["owners"] == 0 and p["fixup"] == 0, p
    elif role == "owners":
        assert p["owners"] > 0 and p["owners"] == p["rem"] == T - p["full"] and p["helpers"] > 0 and p["fixup"] == 0, p
        assert MIN_OWNER <= p["owner_chunks"] < chunks and p["maxp"] <= 3 and p["full"] > 0, p      # plain tiles, owners and helpers in ONE launch
        assert p["full"] + p["helpers"] + p["owners"] <= 2 * S
    else:
        assert p["fixup"] == 1 and p["owners"] == 0 and p["helpers"] > 0 and p["owner_chunks"] == 0 and p["rem"] == T - p["full"], p
        assert p["q"] < chunks                                                                   # a tile really is cut


def test_one_hot_cases_cover_what_they_name():
    """both tile widths, a column tile behind the first, one and two chunks per tap, ragged M, with and without the shortcut"""
    cs = cx.ONE_HOT
    assert {cx.x3_bn(c.Cout) for c in cs} == {64, 128} and any(c.Cout // cx.x3_bn(c.Cout) > 1 for c in cs)
    assert {c.Cin // 32 for c in cs} == {1, 2} and {c.sc for c in cs} == {0, 32}
    for c in cs:
        ho, wo = cx.out_hw(c)
        assert (c.B * ho * wo) % 128 != 0
    assert any(c.sc and c.sc != c.Cin for c in cs)                                               # a shortcut of another channel count
    assert any(c.B * cx.out_hw(c)[0] * cx.out_hw(c)[1] > 128 for c in cs)                        # more than one row tile
