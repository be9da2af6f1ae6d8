"""Mixed-size frame batches on the GPU (include/facehip.h: fh_*_ragged_dev, fh_pipeline_run_images): one call detects, aligns and
embeds frames that each have their own size.  The letterbox canvas, the network heads, the per-frame un-scaled records, the align
and the pipeline are held bit for bit to the uniform entry points and the oracle wherever the same bytes go through the same kernels;
the two comparisons against a batch of ONE (other batch size, fp32 summation order) carry the bounds the existing suite holds there.

Base set S: a same-size frame (copy branch), an exact 2x one (INTER_AREA branch), down- and up-scaled ones, a frame with a padded row
pitch, a 1 x 1 one, a frame whose plan is dead (new_h == 0) and an empty descriptor — all at odd byte offsets of ONE device buffer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from oracle import oracle                     # noqa: E402
from tests import util                        # noqa: E402

IN = 128                                                       # tiny_scrfd(hw=128)
# (rows, cols, row pitch; 0 = cols * 3); None = an empty descriptor
S = [(128, 128, 0), (256, 256, 0), (100, 180, 0), (300, 200, 0), (64, 50, 0), (96, 128, 0), (37, 128, 128 * 3 + 5), (1, 1, 0), (1, 2000, 0), None]
DEAD = (8, 9)                                                  # (1, 2000): new_h == 0; the empty descriptor
MAX_PF = 672                                                   # every anchor of a 128 x 128 input: nothing is truncated


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)
    oracle.set_threads(8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Frames:
    """Images packed at ODD byte offsets into one device buffer; descs(order) = the (ptr, rows, cols, step) list of a call."""

    def __init__(self, shapes, seed=None):
        self.shapes = shapes
        self.imgs, self.offs = [], []
        off = 1
        for i, sh in enumerate(shapes):
            if sh is None:
                self.imgs.append(None); self.offs.append(0)
                continue
            rows, cols, step = sh
            step = step or cols * 3
            # (frames_u8's smooth pattern needs 16 pixels a side: a smaller frame is the corner of a 16-pixel one)
            big = util.frames_u8(1, max(rows, 16), max(cols, 16), seed=cols if seed is None else seed + i, smooth=True)[0]
            self.imgs.append(np.ascontiguousarray(big[:rows, :cols]))
            self.offs.append(off)
            off = (off + rows * step) | 1
        host = np.full(off + 8, 0xA5, np.uint8)                # (pitch padding holds a pattern, not zeros)
        for img, o, sh in zip(self.imgs, self.offs, shapes):
            if img is None:
                continue
            rows, cols, step = sh
            step = step or cols * 3
            for y in range(rows):
                host[o + y * step:o + y * step + cols * 3] = img[y].reshape(-1)
        self.buf = dev(host)
        assert all(o % 2 == 1 for o, sh in zip(self.offs, shapes) if sh is not None)

    def desc(self, i):
        sh = self.shapes[i]
        if sh is None:
            return None
        return (self.buf.data_ptr() + self.offs[i], sh[0], sh[1], sh[2] or sh[1] * 3)

    def descs(self, order=None):
        return [self.desc(i) for i in (range(len(self.shapes)) if order is None else order)]

    def plan(self, i):
        sh = self.shapes[i]
        return fa.letterbox_plan(sh[0], sh[1], IN, IN) if sh is not None else (False, 0, 0, 0.0)


@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    assert det.input_size() == (IN, IN)
    return det, rec


@pytest.fixture(scope="module")
def base():
    """S on the device and the canvases the TEST builds: fh_resize_u8c3_dev to each live frame's plan, pasted top-left into zeros."""
    fr = Frames(S)
    canv = np.zeros((len(S), IN, IN, 3), np.uint8)
    for i in range(len(S)):
        live, nw, nh, _ = fr.plan(i)
        assert live == (i not in DEAD)
        if not live:
            continue
        ptr, rows, cols, step = fr.desc(i)
        d = torch.zeros((nh, nw, 3), dtype=torch.uint8, device="cuda")
        assert fa.lib().fh_resize_u8c3_dev(ptr, rows, cols, step, d.data_ptr(), nh, nw, nw * 3, 0) == 0, _lib.last_error()
        torch.cuda.synchronize()
        canv[i, :nh, :nw] = d.cpu().numpy()
    canv.setflags(write=False)
    return fr, canv


def _det_outputs(det, n):
    outs = []
    for i in range(fa.lib().fh_det_num_outputs(det.handle)):
        r, c = C.c_int(), C.c_int()
        p = fa.lib().fh_det_output_dev(det.handle, i, C.byref(r), C.byref(c))
        out = np.empty((n, r.value, c.value), np.float32)
        assert fa.lib().fh_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0, _lib.last_error()
        outs.append(out)
    return outs


def _records(t, n, per):
    return t.cpu().numpy().view(np.uint8).reshape(n, per, 60).copy().view(fa.FACE_DTYPE).reshape(n, per)


def _detect_ragged(det, descs, thr=0.5, nms=0.4, sync=True):
    n = len(descs)
    out = torch.zeros((n, MAX_PF, 15), device="cuda"); cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    assert det.detect_ragged_dev(descs, out.data_ptr(), MAX_PF, cnt.data_ptr(), thr, nms) == n
    if sync:
        torch.cuda.synchronize()
    return out, cnt


def _canvas_ragged(det, descs):
    n = len(descs)
    arr = fa.frame_array(descs)
    c = torch.full((n, IN, IN, 3), 0x5A, dtype=torch.uint8, device="cuda")          # (every byte must be written, the zeros included)
    assert fa.lib().fh_det_letterbox_ragged_dev(det.handle, arr, n, c.data_ptr(), 0) == n, _lib.last_error()
    torch.cuda.synchronize()
    return c.cpu().numpy()


def test_canvas_bitwise(models_, base):
    det, _ = models_
    fr, canv = base
    got = _canvas_ragged(det, fr.descs())
    for i in range(len(S)):
        assert got[i].tobytes() == canv[i].tobytes(), (i, S[i], int((got[i] != canv[i]).sum()))
    for i in DEAD:
        assert not got[i].any()
    for i in (2, 4):                                           # tie to the CPU restatement: a down-scaled and an up-scaled frame
        _, nw, nh, _ = fr.plan(i)
        ref = np.zeros((IN, IN, 3), np.uint8)
        ref[:nh, :nw] = oracle.resize_bilinear(fr.imgs[i], nw, nh)
        assert np.array_equal(got[i], ref), i
    order = list(range(len(S)))[::-1]
    rev = _canvas_ragged(det, fr.descs(order))
    assert rev.tobytes() == got[::-1].tobytes()                # a frame's canvas does not depend on its slot


def test_heads_bitwise_against_the_uniform_batch_on_the_same_canvases(models_, base):
    det, _ = models_
    fr, canv = base
    n = len(S)
    arr = fa.frame_array(fr.descs())
    assert fa.lib().fh_det_run_network_ragged_dev(det.handle, arr, n, 0) == n, _lib.last_error()
    torch.cuda.synchronize()
    got = _det_outputs(det, n)
    cd = dev(canv.copy())                                      # (the shared reference stays read-only)
    assert fa.lib().fh_det_run_network_dev(det.handle, cd.data_ptr(), n, IN, IN, IN * 3, IN * IN * 3, 0) == n, _lib.last_error()
    torch.cuda.synchronize()
    ref = _det_outputs(det, n)
    assert len(got) == 9
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.tobytes() == b.tobytes(), (i, float(np.abs(a - b).max()))       # same bytes in, same batch, same kernels


def test_records_bitwise_given_the_heads(models_, base):
    det, _ = models_
    fr, _ = base
    n = len(S)
    for thr, nms in ((0.5, 0.4), (0.3, 0.2)):
        out, cnt = _detect_ragged(det, fr.descs(), thr, nms)
        heads = _det_outputs(det, n)                           # the heads these records were decoded from
        rec, cnt = _records(out, n, MAX_PF), cnt.cpu().numpy()
        scales_with_faces = set()
        for b in range(n):
            live, _, _, scale = fr.plan(b)
            if not live:
                assert cnt[b] == 0 and b in DEAD, b
                continue
            ref = oracle.postprocess_rows(oracle.scrfd_decode([h[b] for h in heads], IN, IN), scale, thr, nms)
            assert cnt[b] == len(ref), (thr, nms, b, cnt[b], len(ref))
            assert rec[b, :len(ref)].tobytes() == ref.tobytes(), (thr, nms, b)
            if len(ref) > 0:
                scales_with_faces.add(scale)
        assert len(scales_with_faces) >= 4, scales_with_faces   # >= 4 frames with faces whose scales all differ


def test_ragged_frames_match_the_batch_one_host_path(models_, base):
    """Frame b of ONE ragged call against det.detect_records(img_b): other batch size, so tolerant — with the pairing rule and
    max_unexplained = 0 that test_detect_host_api_matches_oracle_end_to_end holds for these shapes and seeds (seed = cols)."""
    det, _ = models_
    fr, _ = base
    out, cnt = _detect_ragged(det, fr.descs(), 0.5, 0.4)
    rec, cnt = _records(out, len(S), MAX_PF), cnt.cpu().numpy()
    for b in (0, 2, 3):
        assert S[b][:2] in ((128, 128), (100, 180), (300, 200))
        ref = det.detect_records(fr.imgs[b], 0.5, 0.4)
        assert len(ref) > 0
        util.assert_records_equivalent(rec[b, :cnt[b]], ref, 0.5, 0.4, max_unexplained=0)


def _pipeline_bufs(n, F, dim=512):
    faces = torch.full((n * F, 15), 7.0, device="cuda"); fo = torch.full((n * F,), -7, dtype=torch.int32, device="cuda")
    emb = torch.full((n * F, dim), 7.0, device="cuda")
    return faces, fo, emb


def test_uniform_special_case_is_bitwise_the_uniform_pipeline(models_):
    det, rec = models_
    n, F = 6, 2
    frames = util.frames_u8(n, IN, IN, seed=41, smooth=True)
    fd = dev(frames)
    descs = [(fd.data_ptr() + i * IN * IN * 3, IN, IN) for i in range(n)]
    a, b = _pipeline_bufs(n, F), _pipeline_bufs(n, F)
    ta = fa.pipeline_run_ragged_dev(det, rec, descs, F, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), 0.5, 0.4)
    torch.cuda.synchronize()
    tb = fa.pipeline_run_dev(det, rec, fd.data_ptr(), n, IN, IN, F, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), 0.5, 0.4)
    torch.cuda.synchronize()
    assert ta == tb and ta > 0
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()       # the live entries AND the untouched tail


def test_align_bitwise_against_the_uniform_align_per_frame(models_):
    _, rec = models_
    shapes = [(240, 320, 0), (100, 180, 180 * 3 + 7), (300, 200, 0), None]
    fr = Frames(shapes, seed=500)
    per = 6
    n = 3 * per + 1
    faces = np.zeros(n, fa.FACE_DTYPE)
    frame_of = np.zeros(n, np.int32)
    for f in range(3):
        rows, cols = shapes[f][:2]
        sl = slice(f * per, (f + 1) * per)
        faces["lm"][sl] = util.random_landmarks(per, rows, cols, seed=60 + f).reshape(per, 10)
        faces["x"][sl], faces["y"][sl], faces["w"][sl], faces["h"][sl] = 10, 12, cols // 2, rows // 2
        frame_of[sl] = f
    faces["lm"][1] = np.tile(faces["lm"][1][:2], 5)             # coincident landmarks: no transform -> the crop-resize fallback
    faces["lm"][per + 2] = np.tile(faces["lm"][per + 2][:2], 5)  # ... and with a box outside the frame: the empty result
    faces["x"][per + 2] = 5000
    faces["lm"][n - 1] = faces["lm"][0]; frame_of[n - 1] = 3    # a face on the empty frame
    perm = np.random.default_rng(9).permutation(n)              # faces of different frames interleaved
    faces, frame_of = faces[perm], frame_of[perm]
    facd, fod = dev(faces.view(np.uint8).reshape(n, 60)), dev(frame_of)
    crops = torch.full((n, 112, 112, 3), 9, dtype=torch.uint8, device="cuda"); ok = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    arr = fa.frame_array(fr.descs())
    assert fa.lib().fh_rec_align_ragged_dev(rec.handle, arr, len(shapes), facd.data_ptr(), fod.data_ptr(), n, crops.data_ptr(), ok.data_ptr(), 0) == n, _lib.last_error()
    torch.cuda.synchronize()
    crops, ok = crops.cpu().numpy(), ok.cpu().numpy()
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    for f in range(3):
        idx = np.where(frame_of == f)[0]
        ptr, rows, cols, step = fr.desc(f)
        sub = dev(faces[idx].view(np.uint8).reshape(len(idx), 60))
        c1 = torch.zeros((len(idx), 112, 112, 3), dtype=torch.uint8, device="cuda"); o1 = torch.zeros(len(idx), dtype=torch.int32, device="cuda")
        assert fa.lib().fh_rec_align_dev(rec.handle, ptr, rows, cols, step, rows * step, sub.data_ptr(), zero.data_ptr(), len(idx),
                                         c1.data_ptr(), o1.data_ptr(), 0) == len(idx), _lib.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(ok[idx], o1.cpu().numpy()), f
        assert crops[idx].tobytes() == c1.cpu().numpy().tobytes(), f
    modes = {int(frame_of[i]): [] for i in range(n)}
    for i in range(n):
        modes[int(frame_of[i])].append(int(ok[i]))
    assert 2 in modes[0] and 0 in modes[1] and modes[2] == [1] * per and modes[3] == [0]      # fallback, empty box, warps, empty frame
    assert not crops[frame_of == 3].any()


def test_mixed_pipeline(models_, base):
    det, rec = models_
    fr, _ = base
    n, F = len(S), 2
    _, cnt = _detect_ragged(det, fr.descs(), 0.5, 0.4)
    want = np.minimum(cnt.cpu().numpy(), F)
    assert all(want[i] == 0 for i in DEAD) and (want > 0).sum() >= 4
    faces, fo, emb = _pipeline_bufs(n, F)
    total = fa.pipeline_run_ragged_dev(det, rec, fr.descs(), F, faces.data_ptr(), fo.data_ptr(), emb.data_ptr(), 0.5, 0.4)
    torch.cuda.synchronize()
    assert total == int(want.sum())
    got_fo = fo.cpu().numpy()
    assert np.array_equal(got_fo[:total], np.repeat(np.arange(n), want))         # compacted, frame order; dead frames contribute nothing
    # every embedding against the uniform per-face call on that one face and frame
    ser = torch.zeros((total, 512), device="cuda")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    for i in range(total):
        ptr, rows, cols, step = fr.desc(int(got_fo[i]))
        one = faces[i:i + 1].contiguous()
        assert fa.lib().fh_rec_embed_faces_dev(rec.handle, ptr, rows, cols, step, rows * step, one.data_ptr(), zero.data_ptr(), 1,
                                               ser[i:i + 1].data_ptr(), 0, 0) == 1, _lib.last_error()
    torch.cuda.synchronize()
    a, b = emb[:total].cpu().numpy().astype(np.float64), ser.cpu().numpy().astype(np.float64)
    worst = float((1.0 - (a * b).sum(1)).max())
    print("mixed pipeline: total", total, "max 1 - cos vs batch of one", worst)
    assert worst < 1e-6                                          # batch of `total` vs batch of 1: the bound test_pipeline_embeds_live_faces_only holds
    assert torch.all(emb[total:] == 7.0) and torch.all(faces[total:] == 7.0) and torch.all(fo[total:] == -7)   # slots beyond total: not written


def test_back_to_back_calls_with_different_tables(models_, base):
    det, _ = models_
    fr, _ = base
    first, second = fr.descs(), fr.descs([3, 9, 1, 4])           # different tables, the second one shorter
    alone = []
    for d in (first, second):
        out, cnt = _detect_ragged(det, d)
        alone.append((out.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes()))
    torch.cuda.synchronize()
    o1, c1 = _detect_ragged(det, first, sync=False)              # no synchronise between the two calls
    o2, c2 = _detect_ragged(det, second, sync=False)
    torch.cuda.synchronize()
    assert (o1.cpu().numpy().tobytes(), c1.cpu().numpy().tobytes()) == alone[0]
    assert (o2.cpu().numpy().tobytes(), c2.cpu().numpy().tobytes()) == alone[1]
    assert c2.cpu().numpy()[1] == 0 and c2.cpu().numpy()[0] > 0


def test_host_images_entry_equals_the_device_pipeline(models_, base):
    det, rec = models_
    fr, _ = base
    n, F = len(S), 2
    images = list(fr.imgs)
    i = 6                                                        # (37, 128): handed over as a strided view with a padded pitch
    rows, cols = S[i][:2]
    padded = np.full((rows, cols * 3 + 64), 0xEE, np.uint8); padded[:, :cols * 3] = fr.imgs[i].reshape(rows, -1)
    images[i] = np.lib.stride_tricks.as_strided(padded, shape=(rows, cols, 3), strides=(padded.strides[0], 3, 1))
    hf, hfo, hemb = fa.pipeline_images(det, rec, images, faces_per_frame=F, scoreThreshold=0.5, nmsThreshold=0.4)
    faces, fo, emb = _pipeline_bufs(n, F)
    total = fa.pipeline_run_ragged_dev(det, rec, fr.descs(), F, faces.data_ptr(), fo.data_ptr(), emb.data_ptr(), 0.5, 0.4)
    torch.cuda.synchronize()
    assert total == len(hf) == len(hfo) == len(hemb) and total >= 4
    assert hf.tobytes() == _records(faces, 1, n * F)[0, :total].tobytes()
    assert hfo.tobytes() == fo.cpu().numpy()[:total].tobytes()
    assert hemb.tobytes() == emb.cpu().numpy()[:total].tobytes()
    # cap < total truncates and still returns total; untouched entries stay
    cap = total - 1
    f2 = np.zeros(total, fa.FACE_DTYPE); fo2 = np.full(total, -5, np.int32); e2 = np.full((total, 512), 5.0, np.float32)
    arr = fa.frame_array([None if a is None else (a.ctypes.data, a.shape[0], a.shape[1], a.strides[0]) for a in images])
    assert fa.lib().fh_pipeline_run_images(det.handle, rec.handle, arr, n, 0.5, 0.4, F, f2.ctypes.data, fo2.ctypes.data, e2.ctypes.data, cap) == total
    assert f2[:cap].tobytes() == hf[:cap].tobytes() and fo2[:cap].tobytes() == hfo[:cap].tobytes() and e2[:cap].tobytes() == hemb[:cap].tobytes()
    assert fo2[cap] == -5 and np.all(e2[cap] == 5.0)
    assert fa.lib().fh_pipeline_run_images(det.handle, rec.handle, arr, n, 0.5, 0.4, F, None, None, None, 0) == total   # any output may be NULL
    assert len(fa.pipeline_images(det, rec, images, faces_per_frame=F, cap=cap)[0]) == cap
    # only dead frames: 0
    df, dfo, demb = fa.pipeline_images(det, rec, [None, np.zeros((0, 0, 3), np.uint8)], faces_per_frame=F)
    assert len(df) == 0 and len(dfo) == 0 and demb.shape == (0, 512)
    dead = fa.frame_array([None, (0, 5, 5)])
    assert fa.lib().fh_pipeline_run_images(det.handle, rec.handle, dead, 2, 0.5, 0.4, F, f2.ctypes.data, fo2.ctypes.data, e2.ctypes.data, total) == 0
