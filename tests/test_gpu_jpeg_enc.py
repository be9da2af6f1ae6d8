"""The forward path of the JPEG encoder on the device (csrc/jpeg_enc.hip behind fh_jpeg_forward_batch_dev / fh_jpeg_encode_batch) held to
the host's fh_jpeg_forward / fh_jpeg_write, bit for bit and byte for byte: one mixed batch of every size, layout and quality at odd frame
addresses and padded pitches, the pixel extremes, the files, the round trip through the device decoder, the validator in front of the
launches, and the face chips of the detect -> align path."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import jpeg_enc_model as m         # noqa: E402
from tests import jpeg_split as js            # noqa: E402
from tests import util                        # noqa: E402

FH_ERR_ARG = -1
GUARD = 96                                                     # int16 elements of fill pattern in front of, between and behind the images


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


@pytest.fixture(scope="module")
def enc():
    return fa.JpegEncoder()


def host_forward(d, bgr):
    rc, coef = m.c_forward(d, bgr)
    assert rc == 0, _lib.last_error()
    return coef[: int(d.coef_count)]


def place_frames(pictures, pads):
    """The pictures in ONE device buffer full of 0xEE, picture i at an address that is odd for every second one, at pitch cols * 3 +
    pads[i]: (tensor, [(ptr, rows, cols, step)])."""
    offs, size = [], 1
    for i, (p, pad) in enumerate(zip(pictures, pads)):
        size += int(size % 2 != (i + 1) % 2)                                  # odd and even base addresses alternate
        offs.append(size)
        size += p.shape[0] * (p.shape[1] * 3 + pad) + 3
    host = np.full(size, 0xEE, np.uint8)
    for p, pad, off in zip(pictures, pads, offs):
        step = p.shape[1] * 3 + pad
        host[off: off + p.shape[0] * step].reshape(p.shape[0], step)[:, : p.shape[1] * 3] = p.reshape(p.shape[0], -1)
    buf = torch.from_numpy(host).cuda()
    return buf, [(buf.data_ptr() + off, p.shape[0], p.shape[1], p.shape[1] * 3 + pad) for p, pad, off in zip(pictures, pads, offs)]


def run_forward(enc, descs, frames, skip=(), odd_base=(), expect_rc=None):
    """ONE fh_jpeg_forward_batch_dev into a device array full of 0x5A5A with GUARD elements around every image (images in `odd_base` start
    at an odd element: the kernel's unaligned stores): (the array copied back, the images' bases)."""
    n = len(descs)
    base, off = np.zeros(n, np.int64), GUARD
    for i, d in enumerate(descs):
        off += (-off) % 64 + (1 if i in odd_base else 0)
        base[i] = off
        off += int(d.coef_count) + GUARD
    d_coef = torch.full((off,), 0x5A5A, dtype=torch.int16, device="cuda")
    arr = (_lib.FhJpegDesc * n)(*descs)
    fr = fa.frame_array([None if i in skip else f for i, f in enumerate(frames)])
    rc = fa.lib().fh_jpeg_forward_batch_dev(enc.handle, arr, n, fr, d_coef.data_ptr(), base.ctypes.data, 0)
    torch.cuda.synchronize()
    if expect_rc is None:
        assert rc == n, _lib.last_error()
    else:
        assert rc == expect_rc
    return d_coef.cpu().numpy(), base


def check_forward(enc, cases, pictures, descs, skip=(), odd_base=()):
    """The device's coefficients equal fh_jpeg_forward's in every image; every element outside the live images still holds 0x5A5A."""
    pads = [(0, 1, 5)[i % 3] for i in range(len(pictures))]
    keep, frames = place_frames(pictures, pads)
    got, base = run_forward(enc, descs, frames, skip, odd_base)
    exp = np.full_like(got, 0x5A5A)
    for i, (d, p) in enumerate(zip(descs, pictures)):
        if i not in skip:
            exp[base[i]: base[i] + int(d.coef_count)] = host_forward(d, p)
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        i = int(np.searchsorted(base, at, side="right")) - 1
        pytest.fail(f"image {i} {cases[i]}: element {at - base[i]} (block {(at - base[i]) // 64}, position {(at - base[i]) % 64}) is {got[at]}, "
                    f"host {exp[at]}; {np.count_nonzero(got != exp)} elements differ in the batch")
    del keep


def mixed_batch():
    cases = [(("noise", "ramp")[(si + li + qi) % 2], w, h, layout, q)
             for si, (w, h) in enumerate(m.SIZES) for li, layout in enumerate(m.LAYOUTS) for qi, q in enumerate((30, 75, 100))]
    cases.append(("noise", 640, 640, "420", 90))
    cases += [("noise", 200, 200, layout, 75) for layout in m.LAYOUTS]         # several workgroups per component; a boundary inside a block row
    return cases


def test_mixed_batch_equals_the_host_forward(enc):
    cases = mixed_batch()
    pictures = [m.picture(k, w, h, grey=layout == "grey") for (k, w, h, layout, q) in cases]
    descs = [m.enc_desc(w, h, layout, q) for (k, w, h, layout, q) in cases]
    assert len(cases) == 11 * 4 * 3 + 5
    for d in descs[-4:]:                                                       # 25 or 26 luma blocks per row: workgroups of 64 end inside a block row
        assert d.comp[0].wblocks * d.comp[0].hblocks > 64 and (64 % d.comp[0].wblocks) != 0
    skip = (len(cases) // 2,)                                                  # a NULL slot in the middle keeps its fill pattern
    check_forward(enc, cases, pictures, descs, skip=skip, odd_base=set(range(1, len(cases), 4)))


def test_pixel_extremes(enc):
    cases, pictures, descs = [], [], []
    for layout in m.LAYOUTS:
        for name in ("zeros", "ones", "checker", "checker2", "stripes"):
            w, h = 50, 37
            yy, xx = np.mgrid[0:h, 0:w]
            if name == "zeros":
                g = np.zeros((h, w), np.uint8)
            elif name == "ones":
                g = np.full((h, w), 255, np.uint8)
            elif name == "checker":
                g = (((xx + yy) & 1) * 255).astype(np.uint8)
            elif name == "checker2":                                            # survives 2 x 2 down-sampling
                g = ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)
            else:
                g = ((xx & 1) * 255).astype(np.uint8)
            p = np.repeat(g[:, :, None], 3, axis=2)
            if layout != "grey" and name in ("checker", "checker2"):           # saturated colours: the chroma planes swing too
                p = p.copy(); p[:, :, 0] = 255 - p[:, :, 0]
            cases.append((name, w, h, layout, 100)); pictures.append(np.ascontiguousarray(p)); descs.append(m.enc_desc(w, h, layout, 100))
    check_forward(enc, cases, pictures, descs)
    top = max(int(np.abs(host_forward(d, p)).max()) for d, p in zip(descs, pictures))
    assert top >= 1000                                                         # the extremes are extreme: coefficients at the top of the range


def host_file(bgr, layout, quality):
    return m.encode_host(bgr, layout, quality)[2]


def test_encode_batch_equals_the_host_writer(enc):
    shapes = [(640, 640), (112, 112), (17, 23), (1, 1), (200, 200), (40, 9), (100, 75)]
    pictures = [m.picture(("noise", "ramp")[i % 2], w, h) for i, (w, h) in enumerate(shapes)]
    keep, frames = place_frames(pictures, [(0, 1, 5)[i % 3] for i in range(len(pictures))])
    frames = frames[:3] + [None, (frames[3][0], 0, 5, 15)] + frames[3:]        # an empty slot and a frame of no rows
    pictures = pictures[:3] + [None, None] + pictures[3:]
    for layout, q in (("420", 90), ("422", 30), ("444", 100)):
        outs = [enc.encode_dev(frames, quality=q, subsampling=layout, threads=t) for t in (1, 16, 1, 0)]
        for i, p in enumerate(pictures):
            if p is None:
                assert all(o[i] is None for o in outs)
                continue
            exp = host_file(p, layout, q)
            for o in outs:                                                     # threads 1 and 16, and a second call: identical bytes
                assert o[i] == exp, (layout, q, i)
    L = fa.lib()
    blobs = (_lib.FhBlob * 2)()
    assert L.fh_jpeg_encode_batch(enc.handle, fa.frame_array([None, None]), 2, 90, 2, 0, blobs, 0) == 0     # only empty frames: no files
    assert not blobs[0].bytes and blobs[0].n == 0
    short = fa.frame_array([frames[0], (frames[1][0], 112, 112, 112 * 3 - 1)])
    assert L.fh_jpeg_encode_batch(enc.handle, short, 2, 90, 2, 0, blobs, 0) == FH_ERR_ARG
    del keep


def test_round_trip_through_the_device_decoder(enc):
    dec = fa.JpegDecoder()
    shapes = [(100, 75), (33, 16), (112, 112), (9, 40)]
    for layout in ("420", "422", "444"):
        pictures = [m.picture("ramp" if i % 2 else "noise", w, h) for i, (w, h) in enumerate(shapes)]
        files = enc.encode(pictures, quality=90, subsampling=layout, threads=2)
        imgs, status = dec.decode(files)
        assert status.tolist() == [0] * len(files)
        for p, im, (w, h) in zip(pictures, imgs, shapes):
            d = m.enc_desc(w, h, layout, 90)
            assert np.array_equal(im, js.picture(d, host_forward(d, p)))       # fh_jpeg_reconstruct of the host's coefficients


def test_one_invalid_descriptor_stops_the_call(enc):
    cases = [("noise", 33, 16, "420", 75), ("ramp", 17, 23, "422", 75), ("noise", 24, 8, "grey", 75)]
    pictures = [m.picture(k, w, h, grey=layout == "grey") for (k, w, h, layout, q) in cases]
    descs = [m.enc_desc(w, h, layout, q) for (k, w, h, layout, q) in cases]
    check_forward(enc, cases, pictures, descs)                                 # valid as they are
    keep, frames = place_frames(pictures, [0, 1, 5])

    def rows_differ(d):
        d.height = d.rows = 24; d.comp[0].dh = 24; d.comp[1].dh = d.comp[2].dh = 24         # a consistent descriptor of another picture

    for breakit in (lambda d: setattr(d, "orientation", 3), lambda d: setattr(d, "color", 2), lambda d: d.comp[0].quant.__setitem__(5, 0),
                    lambda d: d.comp[2].quant.__setitem__(63, 300), lambda d: setattr(d.comp[1], "wblocks", 40),
                    lambda d: setattr(d.comp[2], "coef_off", 1 << 33), lambda d: setattr(d, "cols", d.cols + 1)):
        bad = [js.clone(d) for d in descs]
        breakit(bad[1])
        got, _ = run_forward(enc, bad, frames, expect_rc=FH_ERR_ARG)
        assert np.all(got.view(np.uint16) == 0x5A5A)                           # nothing was launched: no coefficient was written
    short = list(frames)
    short[0] = (frames[0][0], frames[0][1], frames[0][2], frames[0][2] * 3 - 1)
    got, _ = run_forward(enc, descs, short, expect_rc=FH_ERR_ARG)
    assert np.all(got.view(np.uint16) == 0x5A5A)
    other = list(frames)
    other[2] = (frames[2][0], frames[2][1] + 1, frames[2][2], frames[2][3])    # rows that are not the descriptor's
    got, _ = run_forward(enc, descs, other, expect_rc=FH_ERR_ARG)
    assert np.all(got.view(np.uint16) == 0x5A5A)
    bad = [js.clone(d) for d in descs]                                         # a bad descriptor in a slot that is skipped is not looked at
    bad[1].ncomp = 2
    got, base = run_forward(enc, bad, frames, skip=(1,))
    assert np.array_equal(got[base[0]: base[0] + int(descs[0].coef_count)], host_forward(descs[0], pictures[0]))
    assert np.all(got[base[1] - GUARD: base[1] + int(descs[1].coef_count)].view(np.uint16) == 0x5A5A)
    del keep


@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    return det, rec


def test_face_chips_equal_the_host_path(models_, enc, models_dir, tmp_path, capsys):
    det, rec = models_
    path = os.path.join(js.IMAGES, "c1_640x640.jpg")
    img = fa.imread(path)
    faces = det.detect_records(img, 0.5, 0.4)
    assert len(faces) >= 1
    files, crops = fa.face_chips(rec, img, faces, quality=90, subsampling="4:2:0", encoder=enc)
    assert len(files) == len(faces) and crops.shape[1:] == (112, 112, 3)
    for data, crop in zip(files, crops):
        assert data is not None and data == host_file(crop, "420", 90)         # the host path on the crop read back
    from facerecognizeonnx_amd import cli
    out_dir = str(tmp_path / "chips")
    dpath, rpath = util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0), util.tiny_iresnet(models_dir)
    assert cli.main(["detect", path, "--det", dpath, "--rec", rpath, "--chips", out_dir, "--chip-quality", "90"]) == 0
    assert "Chip 0:" in capsys.readouterr().out
    with open(os.path.join(out_dir, "c1_640x640_0.jpg"), "rb") as f:
        assert f.read() == files[0]
    assert cli.main(["compare", path, path, "--det", dpath, "--rec", rpath, "--chips", out_dir]) == -1     # the flag belongs to detect
