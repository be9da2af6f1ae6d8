"""Every fused u8 stem kernel (csrc/stem.hip over csrc/stem_tile.h) on frames pasted without a resize.

launch_stem picks the kernel from the stem's channel count: 8 / 24 -> stem_conv_u8_kernel (LDS tile), 16 / 32 -> stem_conv_px_kernel for
the interior plus stem_conv_border_kernel for the frame around it, 48 / 64 -> stem_mfma_kernel (matrix cores).  Each runs at stride 1 and
2 on a static 64 x 64 net input (4 x 4 / 2 x 2 tiles of 16 x 16 per image, batch 3), with frames whose longer side is exactly 64 — letterbox
scale 1, so the bytes reach the stem as they are and the rest of the net input is canvas:
  64 x 41, pitch 41 * 3 + 1   canvas on the right; the pitch is 124, a multiple of 4: every row is misaligned alike
  64 x 41, pitch 41 * 3 + 2   the same frame with a different misalignment in every row
  41 x 64, pitch 192          canvas below, every row aligned
  64 x 3 and 64 x 1           no interior pixel at all, rows shorter than one 12-byte window
with ReLU, PReLU and no activation, and (bn) a BatchNormalization behind the stem whose plain map stays in use: out1, out2, s2 / t2 and
the slope all live.  Held as test_matrix_core_stem_stride2_letterbox_and_odd_pitch holds its two shapes (docs/tolerances.md): against the
separate preprocess + convolution form at 1e-5 and against the oracle at 1e-4; the long walks of cus = 1 repeat cus = 0 bit for bit.
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


B, HW = 3, 64
#         rows cols pitch
FRAMES = [(64, 41, 41 * 3 + 1), (64, 41, 41 * 3 + 2), (41, 64, 192), (64, 3, 3 * 3 + 1), (64, 1, 5)]
CHANNELS = (8, 24, 16, 32, 48, 64)
# every kernel family sees every activation, each with and without the second output
CASES = [(c, s, act, (i + j + s) % 2 == 1) for i, c in enumerate(CHANNELS) for s in (1, 2) for j, act in enumerate(("relu", "prelu", "none"))]


def _outputs(det, n):
    (r, c) = (C.c_int(), C.c_int())
    assert fa.lib().fh_det_num_outputs(det.handle) == 1
    p = fa.lib().fh_det_output_dev(det.handle, 0, C.byref(r), C.byref(c))
    out = np.empty((n, r.value, c.value), np.float32)
    assert fa.lib().fh_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0, _lib.last_error()
    return out


def run_case(tmp, c, stride, act, bn):
    """-> (path, [(frames, fused cus 0, fused cus 1, separate) per FRAMES row])"""
    path = util.stem_graph(str(tmp / f"stem_{c}_{stride}_{act}_{int(bn)}.onnx"), HW, HW, c, stride, act, bn, seed=1000 * c + 10 * stride + len(act))
    desc = fa.plan_describe(path, HW, HW)
    ho = (HW - 1) // stride + 1
    tail = {"relu": "+relu", "prelu": "+prelu", "none": ""}[act] + (" +bn2nd" if bn else "") + " "
    assert f"0 CONV k3s{stride} {HW}x{HW}x4 -> {ho}x{ho}x{c}{tail}" in desc and "DW+PW" not in desc, desc      # (nothing the front kernel could take)
    det = fa.FaceDetector()
    assert det.loadModel(path), _lib.last_error()
    L = fa.lib()
    runs = []
    try:
        for k, (rows, cols, pitch) in enumerate(FRAMES):
            frames = util.frames_u8(B, rows, cols, seed=7 * c + k)
            img = np.full((B, rows, pitch), 255, np.uint8)                # (pitch bytes that are no pixel of any frame)
            img[:, :, :cols * 3] = frames.reshape(B, rows, cols * 3)
            d = torch.from_numpy(img).cuda()
            outs = []
            for fused, cus in ((1, 0), (1, 1), (0, 0)):
                assert L.fh_det_set_fused_stem(det.handle, fused) == 0 and L.fh_det_set_cus(det.handle, cus) == 0
                assert L.fh_det_run_network_dev(det.handle, d.data_ptr(), B, rows, cols, pitch, rows * pitch, 0) == B, _lib.last_error()
                torch.cuda.synchronize()
                outs.append(_outputs(det, B))
            runs.append((frames, *outs))
    finally:
        L.fh_det_set_cus(det.handle, 0)
    return path, runs


@pytest.mark.parametrize("c,stride,act,bn", CASES, ids=[f"c{c}-s{s}-{a}{'-bn' if b else ''}" for c, s, a, b in CASES])
def test_fused_stem_on_pasted_frames_matches_separate_form_and_oracle(tmp_path, c, stride, act, bn):
    path, runs = run_case(tmp_path, c, stride, act, bn)
    odet = oracle.OracleDetector()
    assert odet.loadModel(path)
    for (rows, cols, pitch), (frames, fused, walked, separate) in zip(FRAMES, runs):
        tag = f"{rows}x{cols} pitch {pitch}"
        assert np.array_equal(fused.view(np.uint32), walked.view(np.uint32)), tag
        np.testing.assert_allclose(fused, separate, rtol=1e-5, atol=1e-5, err_msg=tag)
        for i in range(B):
            inp, scale = oracle.det_preprocess(frames[i], HW, HW)
            assert scale == 1.0
            (ref,) = odet.run_network(inp)
            np.testing.assert_allclose(fused[i].reshape(-1), np.asarray(ref).reshape(-1), rtol=1e-4, atol=1e-4, err_msg=f"{tag} image {i}")
