"""The model of the u8 stems and of front_kernel's block (tests/stem_model.py) held to exact rational arithmetic, the host packer
(stem_pack_wfrag through fh_debug_stem_pack) held to the layout comment, the preconditions of the GPU test's bitwise classes asserted on
the operands it uses (tests/stem_cases.py), and the power of those classes against nine wrong kernels.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import stem_cases as sc
from tests import stem_model as sm
from tests import wino_x3_model as x3

F = Fraction


def f32(*v):
    return np.array(v, np.float32)


def frac_sum(parts):
    return [sum((F(float(p[i])) for p in parts), F(0)) for i in range(len(parts[0]))]


def pieces_normal(parts):
    return np.logical_and.reduce([sm.wm.is_bf16_normal(p) | (p == 0) for p in parts])


def assert_split_exact(w):
    w = np.ascontiguousarray(w, np.float32).reshape(-1)
    parts = [p.reshape(-1) for p in sm.split_rne3(w)]
    for p in parts:                                                    # every piece IS a bf16
        assert not (p.view(np.uint32) & 0xFFFF).any()
    assert pieces_normal(parts).all()
    got = frac_sum(parts)
    bad = [i for i in range(w.size) if got[i] != F(float(w[i]))]
    assert not bad, [(float(w[i]).hex(), [float(p[i]).hex() for p in parts]) for i in bad[:4]]


# ---------------------------------------------------------------------------------------------------------------- split_rne3
def test_split_rne3_crafted_words():
    u = 2.0 ** -7                                                      # bf16 ulp in [1, 2)
    inside = {
        "zeros": f32(0.0, -0.0),
        "hi ties": f32(1 + u / 2, 1 + 3 * u / 2, -(1 + u / 2), -(1 + 3 * u / 2)),               # to even: down to 1, up to 1 + 2 u
        "mid ties": f32(1 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -9 + 3 * 2.0 ** -17, 1 - 2.0 ** -10 - 2.0 ** -18),
        "mid carries": f32(1 + 2.0 ** -8 - 2.0 ** -17, 1 + 2.0 ** -9 * (2 - 2.0 ** -7) + 2.0 ** -18),
        "negative mid, lo": f32(1 - 2.0 ** -10 - 2.0 ** -20, 1 + 2.0 ** -9 - 2.0 ** -19, -1.5 + 2.0 ** -9 + 2.0 ** -19),
        "all 24 bits": f32(1 + (2 ** 23 - 1) * 2.0 ** -23, 2 - 2.0 ** -23, np.float32(1) / np.float32(3)),
        "edges of the domain": f32(sm.W_MIN, -sm.W_MIN * (2 - 2.0 ** -23), sm.W_MAX, -sm.W_MAX),
    }
    for name, w in inside.items():
        assert sm.split_domain(w).all(), name
        assert_split_exact(w)
    hi, mid, lo = sm.split_rne3(inside["hi ties"])
    assert hi.tolist() == [1.0, 1 + 2 * u, -1.0, -(1 + 2 * u)] and (mid != 0).all() and (lo == 0).all()
    hi, mid, lo = sm.split_rne3(inside["mid ties"])
    assert (hi == 1).all() and mid.tolist() == [2.0 ** -9, 2.0 ** -9 + 2.0 ** -15, -2.0 ** -10] and (lo != 0).all()
    hi, mid, lo = sm.split_rne3(inside["mid carries"][:1])
    assert (hi[0], mid[0], lo[0]) == (1.0, 2.0 ** -8, -2.0 ** -17)
    hi, mid, lo = sm.split_rne3(inside["negative mid, lo"])
    assert (mid[:2] * [-1, 1] > 0).all() and (lo[:2] < 0).all() and (hi[2], mid[2], lo[2]) == (-1.5, 2.0 ** -9, 2.0 ** -19)
    # outside: a remainder below the bf16 normal range is lost or travels as a subnormal; above W_MAX hi is Inf
    outside = f32(2.0 ** -120 * (1 + 2.0 ** -23), 2.0 ** -110 * (1 + 2.0 ** -9 + 2.0 ** -18), -2.0 ** -104 * (1 + 2.0 ** -23), 2.0 ** -126 * (1 + 2.0 ** -23))
    assert not sm.split_domain(outside).any()
    parts = sm.split_rne3(outside)
    exact = np.array([s == F(float(w)) for s, w in zip(frac_sum(parts), outside)])
    assert (~exact | ~pieces_normal(parts)).all() and not exact[0]
    over = np.array([0x7F7F8000], np.uint32).view(np.float32)
    assert not sm.split_domain(over).any() and np.isinf(sm.split_rne3(over)[0]).all()


def test_split_rne3_random_bit_patterns():
    rng = np.random.default_rng(20240521)
    w = rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    w = w[np.isfinite(w)]
    dom = sm.split_domain(w)
    assert dom.mean() > 0.85                                           # (exponents 24..254 of 0..254)
    assert_split_exact(w[dom])
    # the magnitudes of the pieces: mid within half a bf16 ulp of hi, lo within half a bf16 ulp of mid
    hi, mid, lo = (np.abs(p.astype(np.float64)) for p in sm.split_rne3(w[dom]))
    assert (mid <= hi * 2.0 ** -8).all() and (lo <= np.maximum(mid, hi * 2.0 ** -9) * 2.0 ** -8).all()


def _first_conv(path):
    from oracle import onnx_min
    g = onnx_min.load(path)
    n = next(n for n in g.nodes if n.op == "Conv")
    return g.inits[n.inputs[1]], g.inits[n.inputs[2]]


def test_stem_weights_of_the_synthetic_models_lie_in_the_split_domain():
    from facerecognizeonnx_amd.synth import models
    for name, maker in (("det_500m_seed100.onnx", models.make_det_500m), ("w600k_r50_seed200.onnx", models.make_w600k_r50),
                        ("w600k_mbf_seed300.onnx", models.make_w600k_mbf)):
        w, b = _first_conv(models.cached(name, maker))
        assert w.shape[1:] == (3, 3, 3), (name, w.shape)
        wf, bf = sm.fold(w, b)
        assert (wf != 0).all() and sm.split_domain(wf).all(), name
        assert (wf.astype(np.float64) * 128 == w[:, ::-1].transpose(2, 3, 1, 0).reshape(27, -1)).all()        # w / 128 is exact
        assert_split_exact(wf)
    for cases, draw in ((sc.D_STEMS, sc.d_stem), (sc.D_FRONTS, lambda *a: sc.d_front(*a)[:2])):               # ... and class D's
        for case in cases:
            wf, _ = sm.fold(*draw(*case))
            assert sm.split_domain(wf).all()
            assert_split_exact(wf)


# ---------------------------------------------------------------------------------------------------------------- the packer
def _lib_pack(wf, cout):
    wf = np.ascontiguousarray(wf, np.float32)
    out = np.full((cout // 16, 3, 64, 4), 0xDEADBEEF, np.uint32)
    assert fa.lib().fh_debug_stem_pack(wf.ctypes.data, cout, out.ctypes.data) == 0, _lib.last_error()
    return out


@pytest.mark.parametrize("cout", (16, 48, 64))
def test_stem_pack_wfrag_is_the_layout_comment_word_for_word(cout):
    rng = np.random.default_rng(cout)
    wf = (rng.standard_normal((27, cout)) / 640).astype(np.float32)
    wf[rng.integers(27, size=8), rng.integers(cout, size=8)] = 0.0
    got = _lib_pack(wf, cout)
    assert np.array_equal(got, sm.pack_wfrag(wf, cout))
    # where the kernel reads them: lane (cout & 15, k >> 3), element k & 7 of block hi / mid / lo
    halves = np.stack([got & 0xFFFF, got >> 16], axis=-1).reshape(cout // 16, 3, 64, 8)
    seen = np.zeros(halves.shape, bool)
    want = [sm.bf16_bits(p) for p in sm.split_rne3(wf)]
    for co in range(cout):
        for k in range(32):
            lane, el = (co & 15) + 16 * (k >> 3), k & 7
            src = sm.k_source(k)
            for q in range(3):
                assert halves[co >> 4, q, lane, el] == (want[q][src, co] if src >= 0 else 0), (co, k, q)
                seen[co >> 4, q, lane, el] = True
    assert seen.all()                                                  # every half-word of the image is one (channel, K, piece)
    assert sorted(sm.k_source(k) for k in range(27)) == list(range(27)) and all(sm.k_source(k) < 0 for k in range(27, 32))
    assert fa.lib().fh_debug_stem_pack(wf.ctypes.data, 24, got.ctypes.data) != 0 and "cout % 16" in _lib.last_error()


def test_fold_is_exact_on_the_bitwise_classes():
    """class I: wf = k, bf = b - 127.5 sum(k), both exact; class P: wf = K, bf = 0"""
    k, b, _ = sc.i_stem(64, 1, "relu", False)
    wf, bf = sm.fold(128.0 * k, b)
    assert np.array_equal(wf.reshape(3, 9, -1).transpose(2, 0, 1), sm.window_weights(k))
    assert np.array_equal(bf.astype(np.float64), b - 127.5 * k.sum(axis=(1, 2, 3)))
    K, _ = sc.p_stem(64, 1)
    wf, bf = sm.fold(sm.onnx_from_window(K), np.zeros(64))
    assert np.array_equal(wf.reshape(3, 9, -1).transpose(2, 0, 1), K) and not bf.any()


# ---------------------------------------------------------------------------------------------------------------- class I: preconditions
def test_class_I_every_partial_sum_is_a_half_integer_below_2_23():
    stem_bound = 27 * 7 * 127.5 + 8
    front_bound = ((27 * 3 * 127.5 + 8) * 9 + 8) * 16 + 8
    assert stem_bound < 2 ** 15 and front_bound < 2 ** 21 < 2 ** 23
    for case in sc.I_STEMS:
        k, b, t2 = sc.i_stem(*case)
        w = (128.0 * k).astype(np.float32)
        assert np.array_equal(w / np.float32(128), k) and np.abs(k).max() <= 7 and np.abs(b).max() <= 8      # integers, as f32 ONNX weights
        assert (np.abs(k).sum(axis=(1, 2, 3)) * 127.5 + np.abs(b)).max() <= stem_bound
        hi, mid, lo = sm.split_rne3(k.astype(np.float32))
        assert np.array_equal(hi, k) and not mid.any() and not lo.any()                                       # one piece carries the weight
        if t2 is not None:
            assert np.abs(t2).max() <= 8
    # PReLU 1/4 and s2 = 1/2: multiples of 1/16 below 2^15 + 8 — 20 bits
    assert (stem_bound + 8) * sm.UNIT < 2 ** 24
    for case in sc.I_FRONTS:
        k, b, dw, dwb, pw, pwb = sc.i_front(*case)
        assert np.abs(k).max() <= 3 and max(np.abs(v).max() for v in (dw, pw)) <= 1 and max(np.abs(v).max() for v in (b, dwb, pwb)) <= 8
        s = np.abs(k).sum(axis=(1, 2, 3)) * 127.5 + np.abs(b)
        d = np.abs(dw).sum(axis=(1, 2)) * s + np.abs(dwb)
        assert (np.abs(pw) @ d + np.abs(pwb)).max() <= front_bound
    # the bf16 MFMA's addition (mfma_acc_step, tests/wino_x3_model.py): addends aligned at the largest exponent, 25 bits kept.  A multiple
    # of 1/2 below 2^23 has its last bit 24 places under the leading one at most: nothing is dropped, whatever the order.
    for bound in (stem_bound, front_bound):
        assert x3._floor_log2(np.float64(bound)) - 24 <= -1
    acc = x3.mfma_acc_step(np.float32(-stem_bound), np.float32(7.0), np.float32(127.5))
    assert float(acc) == -stem_bound + 7 * 127.5


# ---------------------------------------------------------------------------------------------------------------- class P: preconditions
def _p_all():
    """every class P weight draw: (tag, K, pieces)"""
    for c, s in sc.P_STEMS:
        yield (c, s), *sc.p_stem(c, s)
    for ss, mode in sc.P_FRONTS:
        for rnd in range(sc.P_ROUNDS[mode]):
            K, P = sc.p_front(ss, mode, rnd)[:2]
            yield (ss, mode, rnd), K, P


def test_class_P_weights_have_three_untouched_pieces_and_products_of_24_bits():
    for tag, K, P in _p_all():
        taps = K != 0
        assert (taps.sum(axis=(1, 2)) == 2).all() and not K.sum(axis=(1, 2)).any(), tag      # +w, -w
        got = sm.split_rne3(K)
        for q in range(3):
            assert np.array_equal(got[q], P[q]) and (P[q][taps] != 0).all(), (tag, q)
        # no tie: neither w nor w - hi lies halfway between two bf16
        r1 = (K - got[0]).astype(np.float32)
        for v in (K, r1):
            assert not ((v.view(np.uint32) & 0xFFFF) == 0x8000)[taps].any(), tag
        # w (x1 - x2) and every partial sum of its six piece products, for bytes 0..P_BYTES-1: a multiple of lo's last bit below 2^24 of them
        xmax = sm.P_BYTES - 1
        for c, g, j in zip(*np.nonzero(taps)):
            lsb = F(float(abs(P[2][c, g, j])))
            top = sum(F(float(abs(p[c, g, j]))) for p in P) * xmax       # all pieces of one tap against the largest byte
            assert (top / lsb).denominator == 1 and top / lsb < 2 ** 24, (tag, c)
            assert F(float(abs(K[c, g, j]))) * xmax / lsb < 2 ** 24
    for hw, frames in sc.INPUTS + sc.BIG_INPUTS:
        for i, (rows, cols, _) in enumerate(frames):
            assert sc.frames("P", hw, i, rows, cols).max() == sm.P_BYTES - 1


def test_class_P_uses_every_K_position_with_both_signs():
    for name, draws in (("stem 48", [sc.p_stem(48, 1)[0]]), ("stem 64", [sc.p_stem(64, 2)[0]]),
                        *[(f"front {m}", [sc.p_front(1, m, r)[0] for r in range(sc.P_ROUNDS[m])]) for m in ("pm", "pm-relu", "dup")]):
        K = np.concatenate(draws).reshape(-1, 27)
        assert (K > 0).any(axis=0).all() and (K < 0).any(axis=0).all(), name


def test_class_P_exempts_the_border_ring_and_nothing_else():
    for (H, W), _ in sc.INPUTS + sc.BIG_INPUTS:
        for s in (1, 2):
            Ho, Wo = sm.out_hw(H, W, s)
            r = sm.ring(H, W, s)
            bottom, right = (Ho - 1) * s + 1 >= H, (Wo - 1) * s + 1 >= W
            assert r.sum() == Ho * Wo - (Ho - 1 - bottom) * (Wo - 1 - right)
            assert (bottom, right) == ((s == 1), (s == 1))              # even sides: stride 2 never reaches the far padding
            # the ring IS where the padding value matters
            fr = np.zeros((1, H, W, 3), np.uint8)
            diff = (sm.windows2(fr, H, W, s) != sm.windows2(fr, H, W, s, pad2=254)).any(axis=(0, 3, 4))
            assert np.array_equal(diff, r)


# ---------------------------------------------------------------------------------------------------------------- class D
def test_class_D_plain_f32_evaluation_stays_inside_the_derived_bar():
    worst = 0.0
    draws = [(s, sc.d_stem(c, s, act), sc.inputs()) for c, s, act in sc.D_STEMS]
    draws += [(ss, sc.d_front(ss, mode)[:2], sc.inputs(True, ss, True)) for ss, mode in sc.D_FRONTS]
    for s, (w, b), inputs in draws:
        wf, bf = sm.fold(w, b)
        for (H, W), frames in inputs:
            for i, (rows, cols, _) in enumerate(frames):
                fr = sc.frames("D", (H, W), i, rows, cols)
                ref = sm.stem_fp64(fr, H, W, s, w, b)
                ratio = np.abs(sm.stem_f32(fr, H, W, s, wf, bf) - ref) / sm.d_bound(fr, H, W, s, wf, bf)
                worst = max(worst, ratio.max())
    print(f"class D, plain f32 chain: worst |f32 - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- power
def _swap(K, a, b):
    K = K.copy()
    K[(slice(None),) + a], K[(slice(None),) + b] = K[(slice(None),) + b].copy(), K[(slice(None),) + a].copy()
    return K


def _bgr(K):
    return np.ascontiguousarray(K.reshape(K.shape[0], 3, 3, 3)[..., ::-1].reshape(K.shape[0], 3, 9))


I_VARIANTS = {                                                         # name -> (model arguments, change of the window weights, channels it needs)
    "padding 127 instead of 127.5": (dict(pad2=254), None, 0),
    "canvas treated as padding": (dict(canvas2=255), None, 0),
    "byte 8 of rows 0 and 1 exchanged": ({}, lambda K: _swap(K, (0, 8), (1, 8)), 0),
    "B and R exchanged": ({}, _bgr, 0),
    "window row 1 shifted by one byte": (dict(shift=(0, 1, 0)), None, 0),
    "fragment of channel block cb + 1 for block cb": ({}, lambda K: np.roll(K, -16, axis=0), 32),
}


def _frames_of(cls, front=False, ss=1, fused_only=False):
    for (H, W), frames in sc.inputs(front, ss, fused_only):
        for i, (rows, cols, _) in enumerate(frames):
            yield H, W, rows, cols, sc.frames(cls, (H, W), i, rows, cols)


def _tally(counts, name, good, bad):
    c = counts.setdefault(name, [0, 0])
    c[0] += int((good != bad).sum()); c[1] += good.size


def _settle(shares, counts, case, names):
    """every named variant changed an output of this case; keep each variant's smallest share over the cases"""
    for name in names:
        changed, total = counts[name]
        assert changed > 0, (name, case)
        shares[name] = min(shares.get(name, 1.0), changed / total)


def test_power_class_I_catches_every_wrong_byte():
    stems, fronts = {}, {}
    for c, s, act, bn in sc.I_STEMS:
        k, b, t2 = sc.i_stem(c, s, act, bn)
        K = sm.window_weights(k)
        names = [n for n, v in I_VARIANTS.items() if c >= v[2]]
        counts = {}
        for H, W, rows, cols, fr in _frames_of("I"):
            good = sm.epilogue_int(sm.stem_int(fr, rows, cols, H, W, s, k, b), act, t2)
            for name in names:
                kw, change, _ = I_VARIANTS[name]
                bad = sm.epilogue_int(sm.stem_int(fr, rows, cols, H, W, s, k, b, K=change(K) if change else K, **kw), act, t2)
                for a, x in zip(good, bad):
                    if a is not None:
                        _tally(counts, name, a, x)
        _settle(stems, counts, (c, s, act, bn), names)
    names = [n for n, v in I_VARIANTS.items() if v[2] == 0]             # (the front kernel holds one 16-channel fragment: no neighbouring block)
    for ss, relus, ds, co in sc.I_FRONTS:
        k, b, dw, dwb, pw, pwb = sc.i_front(ss, relus, ds, co)
        K = sm.window_weights(k)
        counts = {}
        for H, W, rows, cols, fr in _frames_of("I", True, ss):
            args = (fr, rows, cols, H, W, ss, k, b, relus[0], dw, dwb, ds, relus[1], pw, pwb, relus[2])
            good = sm.front_int(*args)
            for name in names:
                kw, change, _ = I_VARIANTS[name]
                _tally(counts, name, good, sm.front_int(*args, K=change(K) if change else K, **kw))
        _settle(fronts, counts, (ss, relus, ds, co), names)
    assert len(stems) == 6 and len(fronts) == 5
    for name in I_VARIANTS:
        print(f"class I power, {name}: smallest share of a case's outputs changed, stems {stems[name]:.4f}" +
              (f", blocks {fronts[name]:.4f}" if name in fronts else ""))


P_VARIANTS = {
    "lo dropped": lambda h, m, l: h + m,
    "mid dropped": lambda h, m, l: h + l,
    "mid twice in place of lo": lambda h, m, l: h + m + m,
}


def test_power_class_P_catches_every_lost_piece():
    stems, fronts = {}, {}
    for c, s in sc.P_STEMS:
        K, P = sc.p_stem(c, s)
        wrong = {name: f(*(p.astype(np.float64) for p in P)) for name, f in P_VARIANTS.items()}
        counts = {}
        for H, W, rows, cols, fr in _frames_of("P"):
            keep = ~sm.ring(H, W, s)
            good = sm.stem_exact(fr, H, W, s, K)[:, keep]
            assert np.array_equal(good, good.astype(np.float32))         # the expected value IS an f32
            for name, Kw in wrong.items():
                _tally(counts, name, good, sm.stem_exact(fr, H, W, s, Kw)[:, keep].astype(np.float32))
        _settle(stems, counts, (c, s), P_VARIANTS)
    for ss, mode in sc.P_FRONTS:
        for rnd in range(sc.P_ROUNDS[mode]):
            K, P, relus, dw, pw = sc.p_front(ss, mode, rnd)
            wrong = {name: f(*(p.astype(np.float64) for p in P)) for name, f in P_VARIANTS.items()}
            counts = {}
            for H, W, rows, cols, fr in _frames_of("P", True, ss, True):
                keep = ~sm.ring(H, W, ss)
                good = sc.front_exact(sm.stem_exact(fr, H, W, ss, K), relus, pw)[:, keep]
                assert np.array_equal(good, good.astype(np.float32))
                for name, Kw in wrong.items():
                    _tally(counts, name, good, sc.front_exact(sm.stem_exact(fr, H, W, ss, Kw), relus, pw)[:, keep].astype(np.float32))
            _settle(fronts, counts, (ss, mode, rnd), P_VARIANTS)
    for name in P_VARIANTS:
        print(f"class P power, {name}: smallest share of a case's checked outputs changed, stems {stems[name]:.4f}, front_kernel {fronts[name]:.4f}")


def test_model_agrees_with_itself():
    """stem_int against the fp64 ONNX form and a literal loop on one small case; front_int's depthwise against a literal loop"""
    rng = np.random.default_rng(5)
    k, b = sm.draw_int(rng, 8, 7)
    fr = rng.integers(0, 256, (2, 5, 4, 3), dtype=np.uint8)
    H, W = 7, 6
    for s in (1, 2):
        y2 = sm.stem_int(fr, 5, 4, H, W, s, k, b)
        assert np.array_equal(y2 / 2, sm.stem_fp64(fr, H, W, s, 128.0 * k, b))
        Ho, Wo = sm.out_hw(H, W, s)
        for n, oy, ox, co in ((0, 0, 0, 0), (1, Ho - 1, Wo - 1, 7), (1, 1, 1, 3), (0, 2, Wo - 1, 5)):
            acc = F(int(b[co]))
            for ci in range(3):
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = oy * s - 1 + ky, ox * s - 1 + kx
                        if 0 <= iy < H and 0 <= ix < W:
                            x = int(fr[n, iy, ix, 2 - ci]) if iy < 5 and ix < 4 else 0
                            acc += int(k[co, ci, ky, kx]) * (F(x) - F(255, 2))
            assert F(int(y2[n, oy, ox, co]), 2) == acc
    m = rng.integers(-9, 10, (1, 5, 6, 2))
    taps = rng.integers(-1, 2, (2, 3, 3))
    for s in (1, 2):
        out = sm.dw_int(m, taps, [2, -4], s)
        p = np.pad(m, ((0, 0), (1, 1), (1, 1), (0, 0)))
        for oy in range(out.shape[1]):
            for ox in range(out.shape[2]):
                for c in range(2):
                    assert out[0, oy, ox, c] == (p[0, oy * s:oy * s + 3, ox * s:ox * s + 3, c] * taps[c]).sum() + (2, -4)[c]
    assert sm.epilogue_int(np.array([-8, 3]), "prelu", [1, -2])[0].tolist() == [-16, 24]
    assert sm.epilogue_int(np.array([-8, 3]), "prelu", [1, -2])[1].tolist() == [8, -20]
