"""Long tile walks of the persistent detector and stem kernels.

front_kernel, dwpw_reg_kernel, dwpw_reg2_kernel (csrc/dwpw_mfma.hip over csrc/dwpw_tile.h), stem_mfma_kernel and stem_conv_u8_kernel
(csrc/stem.hip) keep
their workgroups alive: a workgroup computes tile t while tile t + wgs is already on its way into registers, and it reuses one LDS halo /
stage buffer from tile to tile.  Their launchers give every tile a workgroup of its own as long as there are at most 2 .. 4 tiles per
compute unit, which is every single-layer case of the other test files — the loop-carried part of the kernels (the prefetch one tile ahead,
the barrier that protects the halo from the previous tile's readers, the double stage, the division-free advance(), the per-image buffer
descriptor and the border-column select that change in mid-walk) then never runs.

`fh_det_set_cus` shrinks the persistent grids: at cus = 1 every launcher ends at `max(8, ...)` = 8 workgroups, one per XCD, and each walks
its XCD's whole contiguous run of tiles.  A tile's arithmetic depends neither on the workgroup that computes it nor on what that workgroup
computed before, so the output must not change in a single bit — and the one-tile-per-workgroup form is held to the oracle on every image.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from oracle import oracle                     # noqa: E402
from tests import util                        # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)
    oracle.set_threads(8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _det_outputs(det, n):
    outs = []
    for i in range(fa.lib().fh_det_num_outputs(det.handle)):
        r, c = C.c_int(), C.c_int()
        p = fa.lib().fh_det_output_dev(det.handle, i, C.byref(r), C.byref(c))
        out = np.empty((n, r.value, c.value), np.float32)
        assert fa.lib().fh_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0, _lib.last_error()
        outs.append(out)
    return outs


B = 7                                                # frames; 45 x 41 maps: 7 x 18 = 126 tiles of 8 x 16, 126 & 7 = 6 (XCD runs of 16 and 15 tiles)
CUS = (1, 8, 12)                                     # workgroups per XCD: 1, 2 .. 4, 3 .. 6 across the kernels' 2 .. 4 workgroups per CU

FRONT, REG, REG2 = "front_kernel", "dwpw_reg_kernel", "dwpw_reg2_kernel"
STEM_MFMA, STEM_U8 = "stem_mfma_kernel", "stem_conv_u8_kernel"

# Smallest maps with a first, an interior and a last tile in both directions, ragged, above the planner's fusion thresholds (plan.cpp:
# Ho * Wo >= 1600 outputs behind a stride-1 depthwise convolution, >= 6400 behind a stride-2 one):
#   stride-1 blocks: 45 x 41 map = 6 x 3 tiles of 8 x 16;  stride-2 blocks: 137 x 185 -> 69 x 93 = 6417 outputs, 9 x 6 tiles, odd sides
#   (right / bottom padding inside the halo), 7 x 54 = 378 tiles, 378 & 7 = 2;  stride-2 stems: frame 89 x 81 -> 45 x 41;  stems' own
#   16 x 16 tiles: 3 x 3 per 45 x 41 map.
# One row per instantiation the launchers can pick (launch_dwpw_reg, dwpw_mfma.hip; launch_stem, stem.hip).  `walkers`: the
# persistent kernels of the row, restated from the launchers.  The stem of the other rows runs in a kernel without a tile loop: the
# thread-per-pixel stem (16 channels), or — 72 channels, more than the u8 stems take — the float preprocess + conv_igemm_kernel.  That
# convolution goes through launch_conv, whose stream-K cut and tall split follow `cus`, but neither can touch it: K = 36 is two 32-deep
# chunks, conv_streamk_plan (csrc/conv_plan.h) never cuts below min(chunks, 8) chunks per segment, and the tall form needs Cin % 32 == 0.  Every tile is
# computed whole by one workgroup whatever `cus` is, so the bitwise leg holds for those rows too.
#   id                H   W  Cc Cout ds ss pad4 front  walkers
CASES = [
    # dwpw_reg_kernel<CQ, TN, OCC>, stride 1: CQ = C / 4, TN = ceil(Cout / 32)
    ("reg-16-24",     45, 41, 16, 24, 1, 1, False, False, (REG,)),                 # <4, 1, 4>; the fused front switched off
    ("reg-16-64",     45, 41, 16, 64, 1, 1, False, False, (REG,)),                 # <4, 2, 4>
    ("reg-16-96",     45, 41, 16, 96, 1, 1, False, False, (REG,)),                 # <4, 3, 3>
    ("reg-40-24",     45, 41, 40, 24, 1, 1, False, False, (STEM_U8, REG)),         # <10, 1, 3>; stem_conv_u8_kernel<1>: 63 tiles, 8 blocks at cus = 1
    ("reg-40-40",     45, 41, 40, 40, 1, 1, False, False, (STEM_U8, REG)),         # <10, 2, 3>
    ("reg-40-72",     45, 41, 40, 72, 1, 1, False, False, (STEM_U8, REG)),         # <10, 3, 3>
    ("reg-64-32",     45, 41, 64, 32, 1, 1, False, False, (STEM_MFMA, REG)),       # <16, 1, 2>; stem_mfma_kernel<1, 4>
    ("reg-64-64",     45, 41, 64, 64, 1, 1, False, False, (STEM_MFMA, REG)),       # <16, 2, 2>
    ("reg-64-96",     45, 41, 64, 96, 1, 1, False, False, (STEM_MFMA, REG)),       # <16, 3, 2>
    ("reg-72-32",     45, 41, 72, 32, 1, 1, False, False, (REG,)),                 # <18, 1, 2>
    ("reg-72-64",     45, 41, 72, 64, 1, 1, False, False, (REG,)),                 # <18, 2, 2>
    ("reg-72-96",     45, 41, 72, 96, 1, 1, False, False, (REG,)),                 # <18, 3, 2>
    # dwpw_reg_kernel<4, TN, 3, 2>: the stride-2 block of 16 channels
    ("reg-s2-16-24", 137, 185, 16, 24, 2, 1, False, False, (REG,)),
    ("reg-s2-16-40", 137, 185, 16, 40, 2, 1, False, False, (REG,)),
    # dwpw_reg2_kernel<6, 4, 3, 2>: 40 channels through one halo buffer in two parts
    ("reg2-40-72",   137, 185, 40, 72, 2, 1, False, False, (STEM_U8, REG2)),
    # front_kernel<STEP4>: stem stride 1 | 2, 16 -> 16 | 32, row pitch cols * 3 (123 / 243 bytes: <false>) and padded to a multiple of 4 (<true>)
    ("front-s1-16",   45, 41, 16, 16, 1, 1, False, True, (FRONT,)),
    ("front-s1-16-p", 45, 41, 16, 16, 1, 1, True, True, (FRONT,)),
    ("front-s1-32",   45, 41, 16, 32, 1, 1, False, True, (FRONT,)),
    ("front-s1-32-p", 45, 41, 16, 32, 1, 1, True, True, (FRONT,)),
    ("front-s2-16",   89, 81, 16, 16, 1, 2, False, True, (FRONT,)),
    ("front-s2-16-p", 89, 81, 16, 16, 1, 2, True, True, (FRONT,)),
    ("front-s2-32",   89, 81, 16, 32, 1, 2, False, True, (FRONT,)),
    ("front-s2-32-p", 89, 81, 16, 32, 1, 2, True, True, (FRONT,)),
    # stem_mfma_kernel<STRIDE, CB>: <1, 4> runs in the reg-64 rows; the 48-channel block behind it is the LDS dwpw_kernel (one tile per workgroup)
    ("stem-s2-64",    89, 81, 64, 32, 1, 2, False, False, (STEM_MFMA, REG)),       # <2, 4>
    ("stem-s1-48",    45, 41, 48, 24, 1, 1, False, False, (STEM_MFMA,)),           # <1, 3>
    ("stem-s2-48",    89, 81, 48, 24, 1, 2, False, False, (STEM_MFMA,)),           # <2, 3>
    # stem_conv_u8_kernel<2> (<1> runs in the reg-40 rows)
    ("stemu8-s2-40",  89, 81, 40, 24, 1, 2, False, False, (STEM_U8, REG)),
]


def _cdiv(a, b):
    return (a + b - 1) // b


def _walkers(Cc, Cout, ds, front):
    """Which persistent kernels a row launches: launch_dwpw_reg / front_fused_ok (dwpw_mfma.hip), Net::run_u8 and the stem_ok_ rule
    (engine.cpp), launch_stem (stem.hip)."""
    if front:
        assert Cc == 16 and ds == 1 and Cout <= 32 and Cout % 4 == 0
        return (FRONT,)
    out = []
    if Cc in (48, 64):
        out.append(STEM_MFMA)
    elif Cc not in (16, 32) and Cc <= 64 and Cc % 4 == 0:
        out.append(STEM_U8)
    tn = _cdiv(Cout, 32)
    if Cout % 4 == 0 and Cout <= 96:
        if ds == 2 and Cc == 40 and tn == 3:
            out.append(REG2)
        elif (ds == 2 and Cc == 16 and tn <= 2) or (ds == 1 and Cc in (16, 40, 64, 72)):
            out.append(REG)
    return tuple(out)


def _tiles_differing(a, b, Ho, Wo):
    """(image, tile row, tile column) of the 8 x 16 tiles in which two outputs [B, Ho * Wo, C] differ, for the failure message."""
    bad = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2).reshape(a.shape[0], Ho, Wo)
    n, y, x = np.nonzero(bad)
    return sorted(set(zip(n.tolist(), (y // 8).tolist(), (x // 16).tolist())))


@pytest.mark.parametrize("name,H,W,Cc,Cout,ds,ss,pad4,front,walkers", CASES, ids=[c[0] for c in CASES])
def test_long_tile_walks_are_bitwise_the_one_tile_per_workgroup_form(tmp_path, name, H, W, Cc, Cout, ds, ss, pad4, front, walkers):
    """u8 frames -> stem 3x3 + ReLU -> depthwise 3x3 + ReLU -> 1x1 + ReLU at cus = 0 (one tile per workgroup: all 7 images against the
    oracle at the block bar), then at cus = 1 / 8 / 12 and again at 0: bit for bit the first run."""
    Hs, Ws = (H - 1) // ss + 1, (W - 1) // ss + 1                     # the stem's map (3x3, pad 1)
    Ho, Wo = (Hs - 1) // ds + 1, (Ws - 1) // ds + 1
    path = util.dwpw_graph(str(tmp_path / "walk.onnx"), H, W, Cc, Cout, ds, stem_stride=ss)
    # the plan is the stem convolution and the fused block, nothing else: no further launch_conv whose stream-K / tall split could follow cus
    desc = fa.plan_describe(path, H, W)
    ops = [ln for ln in desc.splitlines() if ln[:1].isdigit()]
    assert len(ops) == 2, desc
    assert ops[0].startswith(f"0 CONV k3s{ss} {H}x{W}x4 -> {Hs}x{Ws}x{Cc}+relu "), desc
    assert ops[1].startswith(f"1 DW+PW k1s1 {Hs}x{Ws}x{Cc} -> {Ho}x{Wo}x{Cout}+relu "), desc
    assert ("(depthwise s2)" in ops[1]) == (ds == 2), desc
    assert _walkers(Cc, Cout, ds, front) == walkers

    # tiles of the persistent kernels: 8 x 16 outputs for the block kernels, 16 x 16 (STEM_TILE) for the stems
    tiles = {k: B * (_cdiv(Hs, 16) * _cdiv(Ws, 16) if k in (STEM_MFMA, STEM_U8) else _cdiv(Ho, 8) * _cdiv(Wo, 16)) for k in walkers}
    cus_dev = torch.cuda.get_device_properties(0).multi_processor_count
    for k, t in tiles.items():
        # cus = 0: grid = max(8, floor8(min(ceil8(tiles), CUs * OCC))) with OCC >= 2 (launch_dwpw_reg_cfg, launch_dwpw_reg2_cfg, launch_front:
        # dwpw_mfma.hip; launch_stem_mfma: stem.hip), min(tiles, 256 * 8) blocks for stem_conv_u8_kernel: a workgroup per tile
        if k == STEM_U8:
            assert t <= 256 * 8, (k, t)
        else:
            assert _cdiv(t, 8) * 8 <= 2 * cus_dev // 8 * 8, (k, t, cus_dev)
        # cus = 1: cus * OCC <= 4 and cus * 8 = 8, so the grid is 8 — one workgroup per XCD walks its whole run of tiles / 8 (+ 1) tiles
        assert t // 8 >= 7, (k, t)

    det = fa.FaceDetector(); odet = oracle.OracleDetector()
    assert det.loadModel(path) and odet.loadModel(path)
    L = fa.lib()
    if Cc == 16 and ds == 1 and Cout <= 32:
        assert L.fh_det_set_fused_front(det.handle, 1 if front else 0) == 0
    pitch = (W * 3 + 3) // 4 * 4 if pad4 else W * 3
    assert (pitch % 4 == 0) == pad4                                   # front_kernel<true> only with the padded rows

    def staged(seed):
        frames = util.frames_u8(B, H, W, seed=seed)
        img = np.full((B, H, pitch), 255, np.uint8)                   # (padding bytes that are no pixel of any frame)
        img[:, :, :W * 3] = frames.reshape(B, H, W * 3)
        return frames, dev(img)

    frames, d = staged(Cout + 7 * Cc)
    _, scrub = staged(Cout + 7 * Cc + 1)

    def run(cus):
        # different frames first, one tile per workgroup: every tensor of the arena then holds values of ANOTHER input, so a tile that a walk
        # skipped could not pass as "unchanged" on what the previous run left there
        assert L.fh_det_set_cus(det.handle, 0) == 0
        assert L.fh_det_run_network_dev(det.handle, scrub.data_ptr(), B, H, W, pitch, H * pitch, 0) == B
        assert L.fh_det_set_cus(det.handle, cus) == 0
        assert L.fh_det_run_network_dev(det.handle, d.data_ptr(), B, H, W, pitch, H * pitch, 0) == B, _lib.last_error()
        torch.cuda.synchronize()
        (out,) = _det_outputs(det, B)
        assert out.shape == (B, Ho * Wo, Cout)
        return out

    try:
        base = run(0)
        for i in range(B):
            inp, _ = oracle.det_preprocess(frames[i], W, H)
            ref = odet.run_network(inp)[0]
            # the block bar of test_depthwise_pointwise_block_matches_oracle (docs/tolerances.md)
            np.testing.assert_allclose(base[i], ref.reshape(base[i].shape), rtol=1e-5, atol=2e-5, err_msg=f"{name} image {i}")
        for cus in CUS + (0,):
            got = run(cus)
            diff = _tiles_differing(got, base, Ho, Wo)
            assert not diff, f"{name} cus={cus}: {len(diff)} of {B * _cdiv(Ho, 8) * _cdiv(Wo, 16)} tiles differ, (image, ty, tx) = {diff[:24]}"
    finally:
        L.fh_det_set_cus(det.handle, 0)


def _records(t, n, per):
    return t.cpu().numpy().view(np.uint8).reshape(n, per, 60).copy().view(fa.FACE_DTYPE).reshape(n, per)


def test_det500m_heads_and_records_under_every_cu_count():
    """`fh_det_set_cus` on a full plan: det_500m at B = 3 and 640 x 640 with cus = 0 / 1 / 8 / 100 — front_kernel walks 300 tiles per
    workgroup at cus = 1, the register-fed blocks 75.  All 9 heads of all 3 slots against the oracle at the network bar for every cus (no
    bitwise claim: the direct convolutions' stream-K cut points and tall / igemm split follow cus), and the records of the post-processing
    bit-exact on the GPU's own heads, as test_det500m_batch8_heads_and_records holds them."""
    from facerecognizeonnx_amd.synth import models
    path = models.cached("det_500m_seed100.onnx", models.make_det_500m)
    det = fa.FaceDetector(); odet = oracle.OracleDetector()
    assert det.loadModel(path) and odet.loadModel(path)
    L = fa.lib()
    n = 3
    frames = np.concatenate([util.frames_u8(2, 640, 640, seed=71), util.frames_u8(1, 640, 640, seed=72, smooth=True)])
    d = dev(frames)
    refs = [odet.run_network(oracle.det_preprocess(frames[b], 640, 640)[0]) for b in range(n)]
    max_pf = 1024
    faces = torch.zeros((n, max_pf, 15), device="cuda"); counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    try:
        for cus in (0, 1, 8, 100):
            assert L.fh_det_set_cus(det.handle, cus) == 0
            assert L.fh_det_run_network_dev(det.handle, d.data_ptr(), n, 640, 640, 640 * 3, 640 * 640 * 3, 0) == n, _lib.last_error()
            torch.cuda.synchronize()
            got = _det_outputs(det, n)
            assert len(got) == 9
            for b in range(n):
                for i in range(9):
                    # fp32 through ~50 layers; heads: sigmoid scores in [0,1], distances O(1..10) in stride units
                    np.testing.assert_allclose(got[i][b], refs[b][i], rtol=1e-4, atol=1e-4, err_msg=f"cus {cus} slot {b} output {i}")
            for thr, nms in ((0.5, 0.4), (0.02, 0.4)):
                assert L.fh_det_postprocess_dev(det.handle, n, thr, nms, faces.data_ptr(), max_pf, counts.data_ptr(), 0) == n
                torch.cuda.synchronize()
                cnt = counts.cpu().numpy(); rec = _records(faces, n, max_pf)
                for b in range(n):
                    rows = oracle.scrfd_decode([g[b] for g in got], 640, 640)
                    ref = oracle.postprocess_rows(rows, 1.0, thr, nms)
                    assert cnt[b] == len(ref), (cus, thr, b, cnt[b], len(ref))
                    k = min(len(ref), max_pf)
                    assert rec[b, :k].tobytes() == ref[:k].tobytes(), (cus, thr, b)
    finally:
        L.fh_det_set_cus(det.handle, 0)
