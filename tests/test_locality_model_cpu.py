"""CPU model of the locality property (tests/locality.py): where the radii of tests/test_gpu_locality.py come from.

(1) numpy emulations of Winograd F(4x4,3x3) (uniform and the mixed F(4) / F(2) tiling) and F(2x2,3x3), written from the transform
    matrices (Lavin & Gray 2016), contaminate at most Chebyshev radius 4 / 2 around a NaN input pixel — exactly 4 / 2 in the worst case
    when the transforms are plain matrix products, one less when their structural zeros are skipped — and always the pixel's direct
    3x3 neighbourhood;
(2) torch conv2d in fp64 and fp32 contaminates exactly the geometric receptive field (stride 1 and 2, 3x3 and 1x1, corners, borders,
    interior);
(3) oracle/torch_graph.py in fp64 on the small direct-form graphs of the GPU test contaminates exactly the set that
    locality.propagate_graph_mask derives (one receptive-field step per convolution);
plus the helpers' own contracts (exemption cap, guard layout, plant list, the comparison catching a leak).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import onnx_min                    # noqa: E402
from oracle import torch_graph                 # noqa: E402
from tests import locality as loc              # noqa: E402
from tests import util                         # noqa: E402

# Lavin & Gray 2016: F(4x4,3x3) on points 0, +-1, +-2, inf; F(2x2,3x3) on 0, +-1, inf
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
MATS = {4: (BT4, G4, AT4), 2: (BT2, G2, AT2)}


def _apply(M, v, dense):
    """M @ v along axis 0.  dense: a plain matrix product, 0 * NaN = NaN included — the widest reach an implementation of the algorithm
    can have (a whole patch poisons its whole tile), which is what the radii are taken from.  Not dense: the structural zeros of M are
    skipped, as hand-written transforms do (a zero coefficient is no term at all); its reach must lie inside the dense one."""
    if dense:
        return M @ v
    out = np.zeros((M.shape[0],) + v.shape[1:])
    for i in range(M.shape[0]):
        for j in range(M.shape[1]):
            if M[i, j] != 0:
                out[i] = out[i] + M[i, j] * v[j]
    return out


def _wino_conv(x, w, spans_y, spans_x, dense=True):
    """Single-channel 3x3 'same' convolution of x [H, W] by tiles: spans_* = [(start, m)], m = 4 or 2 outputs per tile and direction."""
    H, W = x.shape
    xp = np.zeros((H + 8, W + 8)); xp[1:1 + H, 1:1 + W] = x                  # zero padding; index = coordinate + 1
    out = np.zeros((H + 4, W + 4))
    for y0, my in spans_y:
        for x0, mx in spans_x:
            BTy, Gy, ATy = MATS[my]; BTx, Gx, ATx = MATS[mx]
            d = xp[y0:y0 + my + 2, x0:x0 + mx + 2]
            V = _apply(BTx, _apply(BTy, d, dense).T, dense).T
            U = Gy @ w @ Gx.T
            M = U * V
            out[y0:y0 + my, x0:x0 + mx] = _apply(ATx, _apply(ATy, M, dense).T, dense).T
    return out[:H, :W]


def _spans(n, m, mixed=False):
    """Tile starts along one direction: uniform tiles of m outputs (hanging over the border), or the mixed tiling — F(4) tiles and one F(2)
    tile at the end where n = 4 k + 2 (what the 14 x 14 maps take)."""
    if mixed and n % 4 == 2:
        return [(s, 4) for s in range(0, n - 2, 4)] + [(n - 2, 2)]
    return [(s, m) for s in range(0, n, m)]


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("m,mixed,R", [(4, False, loc.R_WINO4), (4, True, loc.R_WINO4), (2, False, loc.R_WINO2)])
def test_winograd_emulation_contaminates_radius_4_and_2(m, mixed, R, dense):
    H, W = 14, 13
    rng = np.random.default_rng(m)
    x = rng.standard_normal((H, W)); w = rng.standard_normal((3, 3))
    sy, sx = _spans(H, m, mixed), _spans(W, m, mixed)
    clean = _wino_conv(x, w, sy, sx, dense)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x)[None, None], torch.from_numpy(w)[None, None], padding=1)[0, 0].numpy()
    np.testing.assert_allclose(clean, ref, rtol=0, atol=1e-12)            # the emulation IS a convolution
    worst = 0
    for y in range(H):
        for xx in range(W):
            d = x.copy(); d[y, xx] = np.nan
            bad = ~np.isfinite(_wino_conv(d, w, sy, sx, dense))
            ys, xs = np.nonzero(bad)
            r = max(np.abs(ys - y).max(), np.abs(xs - xx).max())
            worst = max(worst, int(r))
            assert bad[max(0, y - 1):y + 2, max(0, xx - 1):xx + 2].all(), (y, xx)          # the 3x3 neighbourhood is always included
            allowed = loc.allowed_mask((1, H, W), [(0, y, xx)], 1, R)[0]
            assert not (bad & ~allowed).any(), (y, xx)
    assert worst == R if dense else R - 1 <= worst <= R, worst   # (zero-skipping transforms reach one pixel less: measured 3 and 1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_torch_conv_contaminates_exactly_the_receptive_field(dtype, k, stride):
    B, C, H, W = 3, 5, 11, 10
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, C, H, W)); w = rng.standard_normal((6, C, k, k))
    for _, b, y, xx in loc.plant_positions(B, H, W):
        for bits in (loc.NAN_BITS, loc.PINF_BITS):
            d = x.copy(); d[b, C - 1, y, xx] = loc.bits_to_f32(bits)
            out = torch.nn.functional.conv2d(torch.from_numpy(d).to(dtype), torch.from_numpy(w).to(dtype), stride=stride, padding=k // 2).numpy()
            bad = ~np.isfinite(out)
            assert (bad.all(axis=1) == bad.any(axis=1)).all()                # a poisoned pixel is poisoned in every output channel
            m = np.zeros((B, H, W), bool); m[b, y, xx] = True
            want = loc.propagate_conv_mask(m, k, stride)
            assert np.array_equal(bad.any(axis=1), want), (b, y, xx, k, stride)
            R = loc.R_DIRECT3 if k == 3 else loc.R_1X1
            assert not (want & ~loc.allowed_mask(want.shape, [(b, y, xx)], stride, R)).any()   # the radius form is a superset of the exact set


GRAPHS = [
    ("dwpw", lambda p: util.dwpw_graph(p, 21, 18, 16, 24, 1), 21, 18),
    ("dwpw_s2", lambda p: util.dwpw_graph(p, 21, 18, 16, 24, 2), 21, 18),
    ("dw_s1", lambda p: util.dw_graph(p, 13, 11, 8, 1, "prelu", 5), 13, 11),
    ("dw_s2", lambda p: util.dw_graph(p, 13, 11, 8, 2, "none", 6), 13, 11),
    ("halo", lambda p: util.halo_graph(p, 15, 19, 16, 12, False), 15, 19),
    ("halo_res", lambda p: util.halo_graph(p, 15, 19, 16, 8, True), 15, 19),
]


@pytest.mark.parametrize("name,build,H,W", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_torch_graph_contamination_equals_mask_propagation(tmp_path, name, build, H, W):
    g = onnx_min.load(build(str(tmp_path / f"{name}.onnx")))
    tg = torch_graph.TorchGraph(g)
    B = 3
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, 3, H, W)) * 0.5
    iname = g.inputs[0][0]
    for _, b, y, xx in loc.plant_positions(B, H, W):
        for c in (0, 2):
            d = x.copy(); d[b, c, y, xx] = np.nan
            m = np.zeros((B, H, W), bool); m[b, y, xx] = True
            want = loc.propagate_graph_mask(g, m)
            out = tg.run({iname: d})
            for oname, v in out.items():
                bad = ~np.isfinite(v).reshape(want[oname].shape + (-1,))
                assert np.array_equal(bad.any(axis=-1), want[oname]) and np.array_equal(bad.all(axis=-1), want[oname]), (name, b, y, xx, c)
    clean = tg.run({iname: x})
    assert all(np.isfinite(v).all() for v in clean.values())


def test_helpers_hold_their_own_contracts():
    # exemption cap and clipping
    m = loc.allowed_mask((2, 7, 5), [(0, 0, 0), (1, 6, 4)], 1, 1)
    assert m.sum() == 8 and m[0, :2, :2].all() and m[1, 5:, 3:].all()
    assert loc.allowed_mask((1, 5, 5), [(0, 9, 9)], 2, 0).sum() == 1
    with pytest.raises(AssertionError):
        loc.allowed_mask((1, 4, 4), [(1, 0, 0)], 1, 1)
    # guards: >= 64 KiB, multiples of 256 B, pattern phase continues behind a tensor of whole dwords
    for nbytes in (4, 12, 1000, 65536, 3 * 7 * 5):
        off, total = loc.guard_layout(nbytes)
        assert off >= 65536 and off % 256 == 0 and total - off - nbytes >= 65536 and total % 256 == 0
    gb = loc.GuardedBuffer(np.arange(6, dtype=np.float32), loc.NAN_BITS)
    assert np.isnan(gb.host[:gb.off].view(np.float32)).all() and np.isnan(gb.host[gb.off + 24:gb.off + 24 + 1024].view(np.float32)).all()
    assert np.array_equal(gb.tensor_host(), np.arange(6, dtype=np.float32))
    # the plant list is fixed and holds what it promises
    for B, H, W, C in ((1, 4, 4, 128), (2, 14, 14, 64), (66, 40, 52, 32), (3, 7, 7, 3)):
        pl = loc.plant_list(B, H, W, C)
        assert pl == loc.plant_list(B, H, W, C)
        pos = {(b, y, x) for _, b, y, x, *_ in pl}
        assert {(0, 0, 0), (B // 2, 0, 0), (B - 1, H - 1, W - 1)} <= pos
        if B > 1:
            assert any((b, H - 1, W - 1) in pos and (b + 1, 0, 0) in pos for b in range(B - 1))
        assert {c for *_, c, _, _ in pl} == {0, C - 1}
        assert {p[5] for p in pl} == {"nan", "+inf", "-inf"}
        assert sum(len(g) for g in loc.plant_groups(B, H, W, C)) == len(pl)
        x = np.zeros((B, H, W, C), np.float32)
        assert (~np.isfinite(loc.apply_plants(x, pl))).sum() == len(pl)
    for B in (2, 3, 5, 64, 70):
        sets = loc.aggressor_victim_sets(B)
        assert len(sets) == (2 if B == 2 else 1)
        for v in sets:
            assert 3 * len(v) >= B and 0 < len(v) < B                      # at least a third are victims, and there IS an aggressor
        assert {0, B - 1} <= set().union(*sets)
    # hostile aggressor images: behind conv3x3 + ReLU (NaN -> 0, as the GPU's `v > 0 ? v : 0`) something non-finite AND something large is left,
    # while an all-NaN image is left as all zeros
    h = loc.hostile_images((2, 9, 11, 4), 3, seed=1)
    assert (h[..., 3] == 0).all() and np.isinf(h[:, ::5, ::5, 0]).all() and np.isfinite(h[..., 1:]).all()
    w = np.random.default_rng(2).standard_normal((8, 3, 3, 3))
    with np.errstate(invalid="ignore"):
        y = torch.nn.functional.conv2d(torch.from_numpy(h[..., :3].transpose(0, 3, 1, 2).astype(np.float64)), torch.from_numpy(w), padding=1).numpy()
        relu = np.where(y > 0, y, 0.0)
        ynan = torch.nn.functional.conv2d(torch.full((1, 3, 9, 11), float("nan"), dtype=torch.float64), torch.from_numpy(w), padding=1).numpy()
    assert np.isposinf(relu).any() and not np.isnan(relu).any() and (relu[np.isfinite(relu)] > 10).any()
    assert (np.where(ynan > 0, ynan, 0.0) == 0).all()
    a = np.zeros((3, 4), np.float32); b = a.copy(); b[1, 2] = 1
    loc.assert_images_changed(b, a, [False, True, False])
    with pytest.raises(AssertionError):
        loc.assert_images_changed(b, a, [True, True, False])
    with pytest.raises(AssertionError):
        loc.assert_images_changed(b, a, [False, True, False], need_nonfinite=True)
    # the comparison is bitwise (-0.0 != +0.0, NaN == the same NaN) and sees a leak outside the allowed set
    a = np.zeros((1, 3, 3, 2), np.float32); b = a.copy()
    allowed = np.zeros((1, 3, 3), bool); allowed[0, 1, 1] = True
    b[0, 1, 1, 0] = np.nan
    assert loc.assert_bitwise_outside(b, a, allowed) == (2, 16)
    b[0, 0, 2, 1] = -0.0
    with pytest.raises(AssertionError):
        loc.assert_bitwise_outside(b, a, allowed)
    a[0, 0, 2, 1] = -0.0; a[0, 2, 2, 0] = b[0, 2, 2, 0] = np.nan
    loc.assert_bitwise_outside(b, a, allowed)
