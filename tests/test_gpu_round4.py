"""GPU parity tests added in round 4: batch-1 graph replay beside batched calls and setters on one handle, config C5's per-rank
workload at its own size, equal-count consensus ties of the 5-point similarity, the fused F(2x2,3x3) Winograd kernel.

Same bars as tests/test_gpu_parity.py: integer / byte / index work bit-exact, fp32 network outputs within the tolerance written
beside each assert, embeddings within 1e-3 cosine of the oracle (north star).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402
from oracle import oracle                     # noqa: E402
from tests import util                        # noqa: E402
from tests.test_gpu_parity import dev         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)
    oracle.set_threads(min(16, os.cpu_count() or 8))


def test_graph_replay_survives_batched_calls_and_setters_on_the_same_handle(models_dir):
    """A captured batch-1 graph (fh_det_detect / fh_rec_extract, face_detector.cpp:170, face_recognizer.cpp:270) holds the addresses of
    the handle's INTERNAL buffers (arena, Winograd workspaces, candidate / key / crop buffers).  A batched call on the same handle
    grows and moves them; a setter changes which kernels run.  Neither may be answered by a replay of the old launch sequence:
    batch-1 calls interleaved with batched calls and setters must equal the eager path bitwise."""
    L = fa.lib()
    imgs = util.frames_u8(5, 128, 128, seed=150, smooth=True)
    batch = dev(util.frames_u8(24, 128, 128, seed=151, smooth=True))
    crops = dev(util.frames_u8(40, 112, 112, seed=152))
    max_pf = 64
    out = torch.zeros(24 * max_pf * 60, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(24, dtype=torch.int32, device="cuda")
    emb = torch.zeros(40, 512, device="cuda")

    def sequence():
        # fresh handles per pass: the batched calls below must GROW this pass's buffers (the bug: graphs captured before the growth
        # kept replaying into the freed arena)
        det = fa.FaceDetector(); rec = fa.FaceRecognizer()
        assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
        res = []
        for im in imgs[:3]:                                                   # eager, capture, replay
            f = det.detect_records(im, 0.5, 0.4); res.append(f.tobytes())
            res.append(rec.extractFeature(im, f[0]).tobytes())
        det.detect_batch_dev(batch.data_ptr(), 24, 128, 128, out.data_ptr(), max_pf, cnt.data_ptr())   # moves arena / cand / keys
        rec.embed_aligned_dev(crops.data_ptr(), 40, emb.data_ptr())                                    # moves arena / crops
        torch.cuda.synchronize()
        res.append(cnt.cpu().numpy().tobytes())
        for im in imgs[2:]:
            f = det.detect_records(im, 0.5, 0.4); res.append(f.tobytes())
            res.append(rec.extractFeature(im, f[0]).tobytes())
            res.append(rec.extractFeatureSimple(im).tobytes())
        assert L.fh_rec_set_shortcut_fold(rec.handle, 0) == 0 and L.fh_det_set_fused_front(det.handle, 0) == 0   # setters between calls
        assert L.fh_det_set_halo_conv(det.handle, 0) == 0
        for im in imgs[3:]:
            f = det.detect_records(im, 0.5, 0.4); res.append(f.tobytes())
            res.append(rec.extractFeature(im, f[0]).tobytes())
        assert L.fh_rec_set_shortcut_fold(rec.handle, 1) == 0 and L.fh_det_set_fused_front(det.handle, 1) == 0
        assert L.fh_det_set_halo_conv(det.handle, 1) == 0
        for im in imgs[3:]:
            f = det.detect_records(im, 0.5, 0.4); res.append(f.tobytes())
            res.append(rec.extractFeature(im, f[0]).tobytes())
        n = C.c_longlong(0)
        nodes = L.fh_det_graph_stats(det.handle, C.byref(n))
        return res, nodes, n.value

    try:
        assert L.fh_set_graph_replay(0) == 0
        eager, _, replays0 = sequence()
        assert L.fh_set_graph_replay(1) == 0
        graph, nodes, replays = sequence()
    finally:
        L.fh_set_graph_replay(1)
    assert replays0 == 0 and nodes > 10 and replays >= 2, (replays0, nodes, replays)
    assert len(eager) == len(graph) and all(a == b for a, b in zip(eager, graph)), \
        [i for i, (a, b) in enumerate(zip(eager, graph)) if a != b]


_C5_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
# the process group comes first (nothing has touched the GPU yet), as bench.py does for N > 1
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
torch.cuda.set_device(0)
import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd.distributed import allgather_queries, allgather_topk, gallery_shard_base
from oracle import oracle
fa._lib.check(fa.lib().fh_init(0), "fh_init")
oracle.set_threads(min(16, os.cpu_count() or 8))
TOTAL, WORLD, RANK8 = 10_000_000, 8, 7                    # this process plays the LAST of 8 ranks of config C5
b, e = gallery_shard_base(TOTAL, RANK8, WORLD)
assert (b, e) == (8_750_000, 10_000_000)
G, Q, k = e - b, 64, 16
rng = np.random.default_rng(5)
gal = np.empty((G, 512), np.float32)
for s in range(0, G, 125_000):                            # generated in slices: one 2.56 GB standard_normal call doubles the peak
    blk = rng.standard_normal((min(125_000, G - s), 512), dtype=np.float32)
    blk /= np.linalg.norm(blk, axis=1, keepdims=True)
    gal[s:s + len(blk)] = blk
q = rng.standard_normal((Q, 512)).astype(np.float32); q /= np.linalg.norm(q, axis=1, keepdims=True)
S = 1 << 20
gal[3] = q[0]; gal[S - 1] = q[0]; gal[S] = q[0]; gal[G - 1] = q[0]      # exact duplicates on both sides of what used to be the slab boundary
gal[S - 2] = q[1]; gal[S + 1] = q[1]
for j in range(2, 10):                                                 # near matches: a noisy copy of the query somewhere in the shard
    row = q[j] + 0.05 * rng.standard_normal(512).astype(np.float32)
    gal[int(rng.integers(0, G))] = row / np.linalg.norm(row)
# the 64 queries are what 8 ranks x 8 frames contribute: this rank holds 8 of them, the gather returns them (world 1) and the other
# 56 come from the peers in a real run — here they are appended so that the scan runs at C5's Q = 64
mine = torch.from_numpy(q[:8].copy()).cuda()
got = allgather_queries(mine)                                          # RCCL all_gather, device tensors
assert got.is_cuda and torch.equal(got, mine)
allq = torch.cat([got, torch.from_numpy(q[8:].copy()).cuda()], 0).contiguous()
g = fa.Gallery(512)
gd = torch.from_numpy(gal).cuda(); g.upload(gd.data_ptr(), G, True, b); del gd
ls = torch.zeros((Q, k), device="cuda"); li = torch.zeros((Q, k), dtype=torch.int32, device="cuda")
g.topk_dev(allq.data_ptr(), Q, k, ls.data_ptr(), li.data_ptr()); torch.cuda.synchronize()
s, i = allgather_topk(ls, li, k, comm_device=torch.device("cuda", 0))   # RCCL all_gather_into_tensor + topk_merge_kernel
torch.cuda.synchronize()
gs, gi = s.cpu().numpy(), i.cpu().numpy().astype(np.int64)
assert gi.min() >= b and gi.max() < e, (gi.min(), gi.max())             # GLOBAL indices of the last shard
rs, ri = oracle.gallery_topk(q, gal, k)
np.testing.assert_allclose(gs, rs, atol=2e-6)
li_ = gi - b
exact = lambda idx: (np.einsum("qkd,qd->qk", gal[idx].astype(np.float64), q.astype(np.float64)) + 1.0) / 2.0
eg, er = exact(li_), exact(ri)
diff = li_ != ri
# identical indices, except that two DIFFERENT rows whose exact scores differ by less than fp32 summation-order noise may swap ranks
assert np.abs(eg - er)[diff].max(initial=0.0) < 1e-6 and diff.mean() < 0.01, (int(diff.sum()), float(np.abs(eg - er)[diff].max(initial=0.0)))
assert np.all(np.diff(eg, axis=1) <= 1e-6)
assert gi[0, :4].tolist() == [b + 3, b + S - 1, b + S, b + G - 1]       # exact ties ordered by global index across the boundary
assert gi[1, :2].tolist() == [b + S - 2, b + S + 1]
assert "librccl" in open("/proc/self/maps").read()
print("c5 shard rows", G, "base", b, "max |score - oracle|", float(np.abs(gs - rs).max()), "rank swaps", int(diff.sum()))
dist.barrier(); dist.destroy_process_group()
print("c5 rank ok")
"""


@pytest.mark.timeout(900)
def test_c5_per_rank_shard_at_full_size_with_global_index_base_over_rccl(tmp_path):
    """Config C5 (BASELINE.json configs[4]; reference shape main.cpp:221-238 + face_recognizer.cpp:320-334 generalised to 1:N): the
    workload ONE of the 8 ranks runs, at its own size — a 1 250 000 x 512 gallery shard uploaded with index base 8 750 000 (the last
    rank's), 64 queries that arrive through `allgather_queries`, `topk_dev`, then `allgather_topk(comm_device=cuda)` (RCCL, world 1:
    one GPU per box) — against `oracle.gallery_topk` on the same shard, with duplicates planted across the 2^20-row boundary the
    round-1 slabs had.  What stays unmeasured is the 8-rank exchange itself (no 8-GPU node is available to this build)."""
    script = tmp_path / "c5_worker.py"
    script.write_text(_C5_WORKER)
    port = 31500 + os.getpid() % 2000
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=850)
    assert p.returncode == 0 and "c5 rank ok" in p.stdout, p.stdout[-3000:]
    print(p.stdout[-400:])


def test_align_equal_count_consensus_ties_match_oracle_bit_exact(models_dir):
    """estimateAffinePartial2D's restatement on the committed tie fixtures (tests/golden/consensus_ties.npz: the best inlier count, 3 or
    4 of 5, is reached by two or more pair models with DIFFERENT inlier sets; face_recognizer.cpp:110-113): `align_kernel` must pick
    the same model as the oracle ("most inliers, then the first pair") — the warped crops are compared bytewise, plain and under a
    3e-5 px landmark perturbation (what a GPU-vs-oracle network difference amounts to)."""
    from tests.test_gpu_parity import _align_gpu
    rec = fa.FaceRecognizer()
    assert rec.loadModel(util.tiny_iresnet(models_dir))
    z = np.load(os.path.join(util.GOLDEN, "consensus_ties.npz"))
    lms = z["landmarks"]
    rng = np.random.default_rng(9)
    lms = np.concatenate([lms, lms + rng.uniform(-3e-5, 3e-5, lms.shape).astype(np.float32)])
    n = len(lms)
    frames = util.frames_u8(2, 480, 640, seed=21, smooth=True)
    faces = np.zeros(n, fa.FACE_DTYPE)
    faces["lm"] = lms.reshape(n, 10)
    faces["x"], faces["y"], faces["w"], faces["h"] = 30, 40, 90, 100
    frame_of = np.arange(n) % 2
    crops, ok = _align_gpu(rec, frames, faces, frame_of)
    for i in range(n):
        ref = oracle.align_face(frames[frame_of[i]], faces[i])
        assert ref is not None and ok[i] == 1, i
        assert np.array_equal(crops[i], ref), f"case {i}: {np.abs(crops[i].astype(int) - ref).max()}"
    half = n // 2
    same = sum(np.array_equal(crops[i], crops[half + i]) or np.abs(crops[i].astype(int) - crops[half + i]).max() <= 1 for i in range(half))
    assert same == half, same                       # the tiny perturbation never flips the chosen model


WINO2_CASES = [
    # B, H,   W,   Cin, Cout, act (0 none / 1 relu / 2 prelu), residual, 9 bias classes
    (2, 56, 56, 64, 64, 2, True, True),        # IResNet stage 1 shape: 7 x 7 tile groups, PReLU + residual, folded BatchNorm
    (1, 112, 112, 64, 64, 2, False, True),     # the first block's conv
    (3, 56, 56, 64, 128, 0, False, False),     # two column tiles
    (5, 13, 17, 64, 64, 1, True, False),       # odd map: ragged tile groups in x and y (half-empty groups, a last pixel row / column)
    (2, 30, 22, 64, 192, 2, True, True),       # three column tiles; map sides off the 8-pixel grid
    (1, 2, 2, 64, 64, 0, False, True),         # a single tile
    (4, 80, 80, 64, 64, 1, False, False),      # SCRFD's head map size
]


def check_wino2_case(B, H, W, Cin, Cout, act, with_res, cls):
    """One WINO2_CASES row through fh_conv_wino2_dev against the oracle's direct fp32 convolution, 5e-5 absolute."""
    rng = np.random.default_rng(B * 1000 + H * 10 + Cin + Cout)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    ref = oracle.conv2d(x, w, None, 1, 1, 1)                               # NCHW, no bias
    if cls:
        b9 = rng.standard_normal((9, Cout)).astype(np.float32)
        ys = np.ones(H, int); ys[0] = 0; ys[-1] = 2 if H > 1 else 0
        xs = np.ones(W, int); xs[0] = 0; xs[-1] = 2 if W > 1 else 0
        ref = ref + b9[3 * ys[:, None] + xs[None, :]].transpose(2, 0, 1)[None]
        bias = b9
    else:
        bias = rng.standard_normal(Cout).astype(np.float32)
        ref = ref + bias[None, :, None, None]
    slope = (0.25 * rng.uniform(0.5, 1.5, Cout)).astype(np.float32)
    if act == 1:
        ref = np.maximum(ref, 0)
    elif act == 2:
        ref = np.where(ref >= 0, ref, ref * slope[None, :, None, None])
    res = rng.standard_normal((B, H, W, Cout)).astype(np.float32) if with_res else None
    if with_res:
        ref = ref + res.transpose(0, 3, 1, 2)
    xd, bd, sd = dev(x.transpose(0, 2, 3, 1)), dev(bias), dev(slope)
    rd = dev(res) if with_res else None
    w_ohwi = np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(Cout, 9, Cin))
    out = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    rc = fa.lib().fh_conv_wino2_dev(xd.data_ptr(), w_ohwi.ctypes.data, bd.data_ptr(), sd.data_ptr(), rd.data_ptr() if with_res else 0,
                                    out.data_ptr(), B, H, W, Cin, Cout, act, 1 if cls else 0, 0)
    assert rc == 0, fa._lib.last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().transpose(0, 3, 1, 2)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, ref.astype(np.float32), rtol=0, atol=5e-5)


@pytest.mark.parametrize("B,H,W,Cin,Cout,act,with_res,cls", WINO2_CASES)
def test_wino2_fused_conv_layer_matches_oracle(B, H, W, Cin, Cout, act, with_res, cls):
    """The fused Winograd F(2x2,3x3) kernel (conv_wino2.hip) that takes the 3x3 stride-1 convolutions of w600k_r50's 64-channel stages
    (and, through the network tests, SCRFD's merged 64 -> 30 head convolutions)
    (Conv nodes inside session_->Run, face_recognizer.cpp:279-283) against the oracle's direct fp32 convolution: bias per border class
    (the block's BatchNorm folded in), PReLU / ReLU, residual.  5e-5 absolute on O(1) outputs: F(2x2) rounds ~3x coarser than the direct
    form's 2e-5 bar (points 0, +-1, inf), far inside F(4x4)'s 2e-4."""
    check_wino2_case(B, H, W, Cin, Cout, act, with_res, cls)


WINO2_NW1_CASES = [(1, 2, 2, 64, 64, 0, False, True), (5, 13, 17, 64, 64, 1, True, False), (2, 30, 22, 64, 192, 2, True, True)]

_WINO2_NW1_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import facerecognizeonnx_amd as fa
from oracle import oracle
from tests.test_gpu_round4 import WINO2_NW1_CASES, check_wino2_case
assert os.environ.get("FACEHIP_WINO2_NW") == "1"
fa._lib.check(fa.lib().fh_init(0), "fh_init")
oracle.set_threads(min(16, os.cpu_count() or 8))
for case in WINO2_NW1_CASES:
    check_wino2_case(*case)
    print("wino2 nw1 case", case, "ok", flush=True)
print("wino2 nw1 ok")
"""


@pytest.mark.timeout(150)
def test_wino2_one_wave_form_matches_oracle_in_a_child_process(tmp_path):
    """`wino2_kernel<4, 1, false>` — one wave per workgroup, all 64 channels of the column tile — is reached only through
    FACEHIP_WINO2_NW=1, which the library reads once per process: a fresh child process with the variable set runs three WINO2_CASES rows
    (a single tile; ragged tile groups with ReLU + residual; three column tiles with PReLU, residual and the 9 bias classes) against the
    same oracle at the same 5e-5 bar as the two-wave form above."""
    script = tmp_path / "wino2_nw1_worker.py"
    script.write_text(_WINO2_NW1_WORKER)
    p = subprocess.run([sys.executable, str(script), ROOT], env=dict(os.environ, FACEHIP_WINO2_NW="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "wino2 nw1 ok" in p.stdout, p.stdout[-3000:]


_dw_graph = util.dw_graph                            # (shared with tests/test_gpu_locality.py)


@pytest.mark.parametrize("H,W,CH,stride,act", [
    (20, 20, 288, 1, "relu"),        # SCRFD's 20x20x288 blocks (row run 1440 float4s: six workgroups per row strip, the last one ragged)
    (40, 40, 152, 2, "relu"),        # ... and the stride-2 entry of that stage (C / 4 = 38: not a power of two)
    (7, 9, 8, 1, "none"),            # smallest channel count of the lean form, odd map, fewer rows than two strips
    (9, 7, 8, 2, "prelu"),           # odd W at stride 2: the right tap of the last column is out of the map
    (13, 31, 20, 1, "prelu"),        # H not a multiple of the strip
    (33, 17, 64, 2, "none"),         # odd H at stride 2: the bottom tap row of the last output row is out of the map
    (5, 5, 4, 1, "relu"),            # C = 4: the generic kernel (no lean form below 8 channels)
])
def test_depthwise_lean_kernel_matches_oracle(tmp_path, H, W, CH, stride, act):
    """dwconv3x3_lean_kernel (ops_misc.hip): buffer-load taps (rows outside the image read as zero in hardware, edge columns pushed out of
    range by one select), the multiply-high channel index, both strides, all three activations, two images (per-image descriptors) —
    against the oracle's graph runner on the same preprocessed input."""
    from oracle import onnx_min
    path = _dw_graph(str(tmp_path / "dw.onnx"), H, W, CH, stride, act, seed=H * 100 + W + CH)
    det = fa.FaceDetector()
    assert det.loadModel(path)
    assert det.input_size() == (W, H)
    n = 2
    img = util.frames_u8(n, H, W, seed=7 + CH, smooth=False)
    d = torch.from_numpy(img).cuda()
    assert fa.lib().fh_det_run_network_dev(det.handle, d.data_ptr(), n, H, W, W * 3, H * W * 3, None) == n
    torch.cuda.synchronize()
    r, c = C.c_int(), C.c_int()
    p = fa.lib().fh_det_output_dev(det.handle, 0, C.byref(r), C.byref(c))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert (r.value, c.value) == (Ho * Wo, CH), (r.value, c.value)
    got = np.empty((n, Ho * Wo, CH), np.float32)
    assert fa.lib().fh_memcpy_d2h(got.ctypes.data, p, got.nbytes) == 0
    g = onnx_min.load(path)
    for i in range(n):
        inp, _ = oracle.det_preprocess(img[i], W, H)
        ref = oracle.run_graph(g, {"input.1": inp[None]})["out"]
        np.testing.assert_allclose(got[i], np.asarray(ref).reshape(Ho * Wo, CH), rtol=1e-5, atol=1e-5, err_msg=f"image {i}")


def test_handle_sync_entry_points():
    """fh_det_sync / fh_rec_sync: wait for a stream and report a handle's deferred errors — FH_OK on a healthy handle (also right after an
    asynchronous call on that stream), FH_ERR_ARG on a null handle."""
    L = fa.lib()
    det = fa.FaceDetector(); rec = fa.FaceRecognizer()
    assert det.loadModel(models.cached("det_500m_seed100.onnx", models.make_det_500m))
    assert rec.loadModel(models.cached("w600k_r50_seed200.onnx", models.make_w600k_r50))
    assert L.fh_det_sync(det.handle, None) == 0 and L.fh_rec_sync(rec._h, None) == 0
    s = torch.cuda.Stream()
    crops = dev(util.frames_u8(5, 112, 112, seed=4))
    out = torch.zeros((5, 512), device="cuda")
    torch.cuda.synchronize()
    assert rec.embed_aligned_dev(crops.data_ptr(), 5, out.data_ptr(), 0, s.cuda_stream) == 5
    rec.sync(s.cuda_stream)                                               # returns only once the embeddings are complete
    host = np.empty((5, 512), np.float32)
    assert L.fh_memcpy_d2h(host.ctypes.data, out.data_ptr(), host.nbytes) == 0
    assert np.allclose(np.linalg.norm(host, axis=1), 1.0, atol=1e-5)
    det.sync()
    assert L.fh_det_sync(None, None) == -1 and L.fh_rec_sync(None, None) == -1
