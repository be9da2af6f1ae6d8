"""JPEG reconstruction on the device (csrc/jpeg_dev.hip behind fh_jpeg_reconstruct_batch_dev / fh_jpeg_decode_batch /
fh_pipeline_run_files) held to the host's fh_jpeg_reconstruct, byte for byte: every fixture, hand-made descriptors that reach the
up-sampling branches no fixture has, coefficient / quantiser extremes that need the IDCT's 64-bit column pass, the validator in front of
the launches, and the file pipeline against imread + pipeline_images."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import jpeg_split as js            # noqa: E402
from tests import util                        # noqa: E402

PAD = 5                                                        # bytes between the rows of a test frame
FH_ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


@pytest.fixture(scope="module")
def dec():
    return fa.JpegDecoder()


def run_batch(dec, descs, coefs, skip=(), expect_rc=None):
    """descs[i] / coefs[i] through ONE fh_jpeg_reconstruct_batch_dev: the coefficients packed into one device array (every third image at
    an odd element offset: the kernel's unaligned loads), the frames at pitch cols * 3 + PAD in one device buffer full of 0xA5.  Returns
    (rc, the buffer copied back, the frames' offsets)."""
    n = len(descs)
    base, parts, off = np.zeros(n, np.int64), [], 0
    for i, c in enumerate(coefs):
        lead = 1 if i % 3 == 1 else (-off) % 64
        parts.append(np.zeros(lead, np.int16)); parts.append(np.ascontiguousarray(c, np.int16))
        base[i] = off + lead
        off += lead + len(c)
    d_coef = torch.from_numpy(np.concatenate(parts)).cuda()
    offs, size = [], 3
    for d in descs:
        offs.append(size)
        size += d.rows * (d.cols * 3 + PAD) + 7
    d_out = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    frames = fa.frame_array([None if i in skip else (d_out.data_ptr() + offs[i], d.rows, d.cols, d.cols * 3 + PAD) for i, d in enumerate(descs)])
    arr = (_lib.FhJpegDesc * n)(*descs)
    rc = fa.lib().fh_jpeg_reconstruct_batch_dev(dec.handle, arr, n, d_coef.data_ptr(), base.ctypes.data, frames, 0)
    torch.cuda.synchronize()
    if expect_rc is None:
        assert rc == n, _lib.last_error()
    else:
        assert rc == expect_rc
    return rc, d_out.cpu().numpy(), offs


def check_batch(dec, descs, coefs, skip=(), names=None):
    """The device's bytes equal fh_jpeg_reconstruct's in every frame; every byte outside the pixel rows still holds 0xA5."""
    _, got, offs = run_batch(dec, descs, coefs, skip)
    exp = np.full_like(got, 0xA5)
    for i, (d, c) in enumerate(zip(descs, coefs)):
        if i in skip:
            continue
        rc, ref = js.reconstruct(d, c, pad=PAD)
        assert rc == 0, _lib.last_error()
        step = d.cols * 3 + PAD
        exp[offs[i]: offs[i] + d.rows * step].reshape(d.rows, step)[:, : d.cols * 3] = ref[:, : d.cols * 3]
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        i = int(np.searchsorted(offs, at, side="right")) - 1
        d = descs[i]
        pytest.fail(f"image {i} ({names[i] if names else ''} {d.width}x{d.height} ncomp {d.ncomp} h{d.hmax} v{d.vmax} color {d.color} "
                    f"orientation {d.orientation}): byte {at - offs[i]} of its frame is {got[at]}, host {exp[at]}; "
                    f"{np.count_nonzero(got != exp)} bytes differ in the batch")


def test_every_fixture_in_one_batch(dec):
    """4:2:0, 4:2:2, 4:4:4, grey, progressive, restart intervals, EXIF 2..8 on non-square pictures, the dw <= 2 fallbacks (j420_1x1,
    j420_w3, j422_w4, j420_w5h2) and the 640 x 640 photograph: one call, one slot with a NULL output, padded pitches full of sentinels."""
    descs, coefs = [], []
    for name in js.JPEGS:
        rc, d, coef = js.entropy(js.read(name))
        assert rc == 0, _lib.last_error()
        descs.append(d); coefs.append(coef[: int(d.coef_count)])
    assert {"j420_1x1.jpg", "j420_w3.jpg", "j422_w4.jpg", "j420_w5h2.jpg", "c1_640x640.jpg", "j411.jpg", "jprog_rst.jpg"} <= set(js.JPEGS)
    check_batch(dec, descs, coefs, skip=(4,), names=js.JPEGS)


def test_decode_batch_from_file_bytes(dec):
    """fh_jpeg_decode_batch on every fixture plus a PNG (status 1: host pixels, same copy), a corrupt header and an empty blob (status
    < 0: the empty frame): every picture equals fh_image_decode's; a second call reuses the arenas."""
    names = list(js.JPEGS) + ["p_rgb.png"]
    files = [js.read(n) for n in names] + [js.read("j420_q75_odd.jpg")[:20], b"", os.path.join(js.IMAGES, "n_rgb.ppm")]
    for threads in (0, 1, 3):
        imgs, status = dec.decode(files, threads=threads)
        assert status[: len(js.JPEGS)].tolist() == [0] * len(js.JPEGS)
        assert status[len(js.JPEGS)] == 1 and status[-3] < 0 and status[-2] < 0 and status[-1] == 1
        assert imgs[-3] is None and imgs[-2] is None
        for n, im in zip(names + ["", "", "n_rgb.ppm"], imgs):
            if n:
                ref = fa.imread(os.path.join(js.IMAGES, n))
                assert im.shape == ref.shape and np.array_equal(im, ref), n
    imgs, status = dec.decode([b"junk", b""])
    assert imgs == [None, None] and np.all(status < 0)


SIZES = [(1, 1), (3, 2), (9, 17), (17, 9), (40, 24)]


def test_crafted_descriptors_reach_every_branch(dec):
    """Seeded coefficients under hand-made descriptors: every (h, v) chroma ratio in {1, 2, 4}^2 — h1v2 and the box replications no
    fixture has, fancy h2v1 / h2v2 on both sides of dw > 2 — grey / YCbCr / RGB, all eight orientations.  One call."""
    rng = np.random.default_rng(11)
    scale = 1 + np.arange(64) // 4
    descs, coefs = [], []
    for w, h in SIZES:
        for hs in (1, 2, 4):
            for vs in (1, 2, 4):
                for color in (0, 1, 2):
                    for o in range(1, 9):
                        factors = [(hs, vs)] if color == 0 else [(hs, vs), (1, 1), (1, 1)]
                        d = js.make_desc(w, h, factors, color, o, quant=rng.integers(1, 40, (len(factors), 64)))
                        c = (rng.integers(-60, 61, (int(d.coef_count) // 64, 64)) // scale).astype(np.int16)
                        c[:, 0] = rng.integers(-400, 401, len(c))
                        descs.append(d); coefs.append(c.reshape(-1))
    assert len(descs) == 5 * 9 * 3 * 8
    check_batch(dec, descs, coefs)


def test_extreme_coefficients_and_quantisers(dec):
    """What only the 64-bit column pass gets right: blocks of +-32767 / -32768, quantisers 1 / 255 / 65535, one non-zero coefficient at
    each of the 64 positions, all-equal blocks, full-range noise."""
    rng = np.random.default_rng(12)
    descs, coefs = [], []
    for q in (1, 255, 65535):
        single = np.zeros((4, 64, 64), np.int16)                              # [value][position] -> block
        for vi, v in enumerate((32767, -32768, 1, -1)):
            single[vi, np.arange(64), np.arange(64)] = v
        equal = np.repeat(np.array([32767, -32767, -32768, 1, -1, 128, -129, 0], np.int16)[:, None], 64, axis=1)
        mixed = rng.choice(np.array([32767, -32767, -32768], np.int16), (56, 64))
        blocks = np.concatenate([single.reshape(256, 64), equal, mixed])      # 320 blocks = 20 x 16
        d = js.make_desc(160, 128, [(1, 1)], 0, quant=q)
        assert int(d.coef_count) == blocks.size
        descs.append(d); coefs.append(blocks.reshape(-1))
        d = js.make_desc(40, 24, [(2, 2), (1, 1), (1, 1)], 1, 7, quant=q)      # the same extremes through up-sampling and the colour tables
        descs.append(d); coefs.append(rng.choice(np.array([32767, -32768, 0, 1], np.int16), int(d.coef_count)))
    d = js.make_desc(64, 64, [(2, 1), (1, 1), (1, 1)], 2, 3, quant=rng.integers(0, 65536, (3, 64)))
    descs.append(d); coefs.append(rng.integers(-32768, 32768, int(d.coef_count)).astype(np.int16))
    d = js.make_desc(64, 64, [(1, 1)], 0, quant=rng.integers(0, 65536, (1, 64)))
    descs.append(d); coefs.append(rng.integers(-32768, 32768, int(d.coef_count)).astype(np.int16))
    check_batch(dec, descs, coefs)


def test_one_invalid_descriptor_stops_the_call(dec):
    rng = np.random.default_rng(13)
    descs = [js.make_desc(17, 9, [(2, 2), (1, 1), (1, 1)], 1, o, quant=2) for o in (1, 6, 3)]
    coefs = [rng.integers(-50, 51, int(d.coef_count)).astype(np.int16) for d in descs]
    check_batch(dec, descs, coefs)                                            # valid as they are
    for breakit in (lambda d: setattr(d.comp[1], "wblocks", 40), lambda d: setattr(d, "orientation", 0),
                    lambda d: setattr(d.comp[2], "coef_off", 1 << 33), lambda d: setattr(d, "cols", d.cols + 1)):
        bad = [js.clone(d) for d in descs]
        breakit(bad[1])
        _, got, _ = run_batch(dec, bad, coefs, expect_rc=FH_ERR_ARG)
        assert np.all(got == 0xA5)                                            # nothing was launched: no frame was touched
    # a bad descriptor in a slot that is skipped is not looked at
    bad = [js.clone(d) for d in descs]
    bad[1].ncomp = 2
    check_batch(dec, bad, coefs, skip=(1,))


@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    return det, rec


def test_pipeline_files_equals_imread_then_pipeline_images(models_, dec):
    det, rec = models_
    names = ["c1_640x640.jpg", "j420_160x120.jpg", "jexif6.jpg", "p_rgb.png", None, "jprog420.jpg"]
    files = [js.read("j420_q75_odd.jpg")[:20] if n is None else os.path.join(js.IMAGES, n) for n in names]
    images = [None if n is None else fa.imread(os.path.join(js.IMAGES, n)) for n in names]
    assert all((im is None) == (n is None) for im, n in zip(images, names))
    F = 3
    ef, efo, eemb = fa.pipeline_images(det, rec, images, faces_per_frame=F)
    print("pipeline_files: faces", len(ef), "frame_of", efo.tolist())
    assert len(ef) >= 1
    for threads in (1, 4):
        f, fo, emb, status = fa.pipeline_files(det, rec, files, faces_per_frame=F, threads=threads, decoder=dec)
        assert status[:4].tolist() == [0, 0, 0, 1] and status[4] < 0 and status[5] == 0
        assert f.tobytes() == ef.tobytes() and fo.tobytes() == efo.tobytes() and emb.tobytes() == eemb.tobytes()
    f, fo, emb, status = fa.pipeline_files(det, rec, [b"", b"junk"], faces_per_frame=F, decoder=dec)
    assert len(f) == 0 and emb.shape == (0, rec.feature_dim()) and np.all(status < 0)
    f, _, _, _ = fa.pipeline_files(det, rec, files, faces_per_frame=F, cap=1)  # a decoder of its own; cap truncates
    assert f.tobytes() == ef[:1].tobytes()


def test_cli_compare_with_device_jpeg(models_dir, capsys):
    from facerecognizeonnx_amd import cli
    dpath, rpath = util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0), util.tiny_iresnet(models_dir)
    c1 = os.path.join(js.IMAGES, "c1_640x640.jpg")
    assert cli.main(["compare", c1, c1, "--device-jpeg", "--det", dpath, "--rec", rpath]) == 0
    out = capsys.readouterr().out
    assert "Image 1: 1 faces, Image 2: 1 faces" in out and "Similarity: 1.000000" in out and "Same person" in out
    assert cli.main(["compare", c1, os.path.join(js.IMAGES, "missing.jpg"), "--device-jpeg", "--det", dpath, "--rec", rpath]) == -1
    assert cli.main(["detect", c1, "--device-jpeg", "--det", dpath]) == -1       # the flag belongs to compare
