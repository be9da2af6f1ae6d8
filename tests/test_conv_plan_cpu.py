"""The launch arithmetic of the direct convolutions on the host (csrc/conv_plan.h through fh_debug_conv_plan), no GPU: the properties
conv_igemm_kernel / conv_fixup_kernel rely on over a sweep of tile shapes, chip sizes, K depths and tile counts, and the decisions
themselves against tests/golden/conv_streamk_plan.json — the answers of the arithmetic as it stood inside conv_mfma.hip before it moved
(the parent is the reference there, not the code under test)."""
import json
import os

import numpy as np

import facerecognizeonnx_amd as fa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_streamk_plan.json")
STREAMK, PW, TALL, NPARTS, LIMITS = range(5)
TILES = [(128, 128, 2), (256, 64, 2), (128, 32, 4), (64, 64, 5)]          # cfg -> BM, BN, resident workgroups per CU (launch_conv)
FIELDS = ("full", "rem", "helpers", "owners", "fixup", "units", "q", "owner_chunks", "maxp")
MIN_OWNER = 12                                                             # ConvKnobs::sk_min_owner's default


def ask(what, args, n_out):
    a = np.asarray(args, np.int32)
    out = np.zeros(max(n_out, 1), np.int64)
    rc = fa.lib().fh_debug_conv_plan(what, a.ctypes.data, a.size, out.ctypes.data, n_out)
    assert rc == n_out, fa._lib.last_error()
    return [int(v) for v in out[:n_out]]


def streamk(cfg, cus, chunks, T, tile0):
    bm, bn, res = TILES[cfg]
    return dict(zip(FIELDS, ask(STREAMK, [T, cus * res, chunks, bm * bn, cus, chunks * 32, tile0, 1], 9)))


def nparts_range(r0, r1, Kh, q):
    """(min, max) of conv_sk_nparts(r, Kh, q) over remainder tiles r0 <= r < r1"""
    return ask(NPARTS, [r0, r1, Kh, q], 2)


def sweep():
    for cfg, (_, _, res) in enumerate(TILES):
        for cus in (1, 9, 64, 100, 208, 255, 256):
            S = cus * res
            Ts = sorted({t for t in list(range(1, 41)) + [S + d for d in range(-6, 7)] + [2 * S + d for d in range(-6, 7)] +
                         [392, 784, 811, 1568, 6400] if t >= 1})
            for chunks in (1, 2, 5, 9, 18, 36, 72, 144, 288, 784):
                for T in Ts:
                    for tile0 in (0, 1):
                        yield cfg, cus, chunks, T, tile0


def test_streamk_plan_keeps_what_the_kernels_rely_on():
    slab_floats, counters = ask(LIMITS, [], 2)
    seen = {"owner": 0, "fixup": 0, "uncut": 0}
    for cfg, cus, chunks, T, tile0 in sweep():
        bm, bn, res = TILES[cfg]
        S = cus * res
        p = streamk(cfg, cus, chunks, T, tile0)
        ctx = (cfg, cus, chunks, T, tile0, p)
        assert p["full"] + p["rem"] == T, ctx
        assert not (p["owners"] and p["fixup"]), ctx
        if not p["helpers"]:
            assert p["rem"] == 0 and not p["owners"] and not p["fixup"] and p["units"] == 0, ctx
            seen["uncut"] += 1
            continue
        assert bool(p["owners"]) != bool(p["fixup"]), ctx
        assert p["full"] % S == 0 and 0 < p["rem"] < S, ctx
        Kh = chunks - p["owner_chunks"]                                    # chunks of a remainder tile the helpers compute
        assert Kh >= 1 and p["q"] >= 1, ctx
        assert p["units"] == p["rem"] * Kh and p["helpers"] == -(-p["units"] // p["q"]), ctx
        # every slab a tile's segments go to exists: 1 <= pieces <= maxp (the owner's / fix-up kernel's loop, the helpers' `part`)
        lo, hi = nparts_range(0, p["rem"], Kh, p["q"])
        assert 1 <= lo and hi <= p["maxp"], (ctx, lo, hi)
        assert p["rem"] * p["maxp"] * bm * bn <= slab_floats, ctx
        if p["owners"]:
            assert p["owners"] == p["rem"] <= counters, ctx
            assert p["helpers"] <= S - p["rem"], ctx                       # every helper is resident before the owners wait for it
            assert p["maxp"] <= 3 and p["owner_chunks"] >= MIN_OWNER, ctx
            seen["owner"] += 1
        else:
            assert p["owner_chunks"] == 0, ctx
            seen["fixup"] += 1
    assert min(seen.values()) > 0, seen                                    # a plan that never cuts cannot pass


def test_nparts_counts_the_runs_that_touch_a_tile():
    for Kh in (1, 3, 8, 17):
        for q in (1, 2, 5, 8, 40):
            for r in range(12):
                runs = {u // q for u in range(r * Kh, (r + 1) * Kh)}
                assert nparts_range(r, r + 1, Kh, q) == [len(runs)] * 2, (r, Kh, q)


def test_decisions_are_the_parents():
    with open(GOLDEN) as f:
        g = json.load(f)
    forms = set()
    for row in g["plans"]:
        got = streamk(*row["in"])
        assert [got[k] for k in FIELDS] == row["out"], (row, got)
        forms.add("owner" if got["owners"] else "fixup" if got["fixup"] else "uncut")
    assert forms == {"owner", "fixup", "uncut"} and len(g["plans"]) >= 90
    npw = ntall = 0
    for row in g["predicates"]:
        B, H, W, Cin, Cout, k, stride, cfg, n_outs, up2x = row["in"]
        shape = [B, H, W, Cin, Cout, k, stride, k // 2, n_outs, up2x, 256]
        assert ask(PW, shape, 1) == [row["pw"]], row
        assert ask(TALL, shape + [cfg], 3) == row["tall"], row
        npw += row["pw"] > 0
        ntall += row["tall"][0] > 0
    assert npw and ntall


def test_bad_arguments_are_refused():
    L = fa.lib()
    out = np.zeros(9, np.int64)
    a = np.zeros(8, np.int32)                                              # S = 0
    assert L.fh_debug_conv_plan(STREAMK, a.ctypes.data, 8, out.ctypes.data, 9) < 0
    assert L.fh_debug_conv_plan(STREAMK, a.ctypes.data, 7, out.ctypes.data, 9) < 0
    assert L.fh_debug_conv_plan(99, a.ctypes.data, 8, out.ctypes.data, 9) < 0
    assert "fh_debug_conv_plan" in fa._lib.last_error()
