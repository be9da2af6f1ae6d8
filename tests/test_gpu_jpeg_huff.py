"""The Huffman coder of the JPEG encoder on the device (csrc/jpeg_huff.hip behind fh_jpeg_code_batch_dev / fh_jpeg_encode_batch_gpu) held to
the host's fh_jpeg_write / fh_jpeg_scan_bits on the same coefficients, byte for byte: the mixed batch of every size, layout and quality,
crafted coefficient planes for the code paths a picture rarely reaches, the limits of the baseline tables, workgroup and scan boundaries,
what else is written (nothing), determinism, and the validator in front of the launches."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import jpeg_enc_model as m         # noqa: E402
from tests import jpeg_huff_model as hm       # noqa: E402
from tests import jpeg_split as js            # noqa: E402
from tests import util                        # noqa: E402

FH_ERR_ARG = -1
GUARD = 96                                                     # int16 elements of fill pattern in front of, between and behind the images
FILL = 0x5A5A


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


@pytest.fixture(scope="module")
def enc():
    return fa.JpegEncoder()


def host_file(d, coef):
    rc, n, out = m.c_write(d, coef)
    return out[:n].tobytes() if rc == 0 else None


def host_bits(d, coef):
    rc, bits = hm.c_scan_bits(d, coef)
    assert rc == 0
    return bits[: hm.blocks_of(d)]


def arena(enc, fill=-1):
    """The device byte arena of the coder: (base address, its bytes copied to the host); fill in 0..255 sets every byte first."""
    dev, size = C.c_void_p(0), C.c_size_t(0)
    assert fa.lib().fh_debug_jpeg_arena(enc.handle, fill, C.byref(dev), C.byref(size)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    host = np.zeros(max(size.value, 1), np.uint8)
    if size.value:
        assert fa.lib().fh_memcpy_d2h(host.ctypes.data, dev, size.value) == 0
    return dev.value or 0, host[: size.value]


def code_batch(enc, items, skip=(), expect_rc=None):
    """ONE fh_jpeg_code_batch_dev on (descriptor, coefficients) pairs laid into a device array full of 0x5A5A with GUARD elements around every
    image; slots in `skip` get coef_base = -1.  Returns (files as bytes or None, status, sizes and arena offsets of the files, the
    coefficient array before and after the call, the whole arena)."""
    n = len(items)
    base, off = np.zeros(n, np.int64), GUARD
    for i, (d, coef) in enumerate(items):
        off += (-off) % 64
        base[i] = off
        off += int(d.coef_count) + GUARD
    host = np.full(off, FILL, np.uint16).view(np.int16)
    for i, (d, coef) in enumerate(items):
        host[base[i]: base[i] + int(d.coef_count)] = coef[: int(d.coef_count)]
    d_coef = torch.from_numpy(host).cuda()
    arr = (_lib.FhJpegDesc * n)(*[d for d, _ in items])
    cb = base.copy()
    cb[list(skip)] = -1
    blobs = (_lib.FhBlob * n)()
    status = np.full(n, 77, np.int32)
    rc = fa.lib().fh_jpeg_code_batch_dev(enc.handle, arr, n, d_coef.data_ptr(), cb.ctypes.data, blobs, status.ctypes.data, 0)
    torch.cuda.synchronize()
    if expect_rc is not None:
        assert rc == expect_rc, (rc, _lib.last_error())
        return None, status, None, (host, d_coef.cpu().numpy()), None
    assert rc >= 0, _lib.last_error()
    a0, whole = arena(enc)
    where = [((b.bytes or 0) - a0 if b.bytes else None, b.n) for b in blobs]
    files = [None if at is None else whole[at: at + size].tobytes() for at, size in where]
    assert rc == sum(f is not None for f in files)
    return files, status, where, (host, d_coef.cpu().numpy()), whole


def check_batch(enc, names, items, skip=()):
    """Every live image's file equals fh_jpeg_write's; skipped slots are {NULL, 0} with status 1; the files lie back to back in slot order
    from the arena's first byte; the coefficients are untouched; the size pass equals fh_jpeg_scan_bits."""
    files, status, where, (before, after), whole = code_batch(enc, items, skip)
    assert np.array_equal(before, after)
    at = 0
    for i, (d, coef) in enumerate(items):
        if i in skip:
            assert files[i] is None and where[i] == (None, 0) and status[i] == 1, names[i]
            continue
        exp = host_file(d, coef)
        assert status[i] == 0 and where[i] == (at, len(exp)), (names[i], where[i], at, len(exp))
        if files[i] != exp:
            first = next(k for k, (a, b) in enumerate(zip(files[i], exp)) if a != b)
            pytest.fail(f"image {i} {names[i]}: byte {first} of {len(exp)} is {files[i][first]:#x}, host {exp[first]:#x}")
        at += len(exp)
    exp_bits = np.concatenate([host_bits(d, coef) for i, (d, coef) in enumerate(items) if i not in skip])
    got = np.zeros(len(exp_bits), np.uint32)
    assert fa.lib().fh_debug_jpeg_scan_bits(enc.handle, got.ctypes.data, len(got)) == len(got), _lib.last_error()
    assert np.array_equal(got, exp_bits)
    return files


def place_frames(pictures, pads):
    """The pictures in ONE device buffer full of 0xEE, picture i at an address that is odd for every second one, at pitch cols * 3 +
    pads[i]: (tensor, [(ptr, rows, cols, step)])."""
    offs, size = [], 1
    for i, (p, pad) in enumerate(zip(pictures, pads)):
        size += int(size % 2 != (i + 1) % 2)
        offs.append(size)
        size += p.shape[0] * (p.shape[1] * 3 + pad) + 3
    host = np.full(size, 0xEE, np.uint8)
    for p, pad, off in zip(pictures, pads, offs):
        step = p.shape[1] * 3 + pad
        host[off: off + p.shape[0] * step].reshape(p.shape[0], step)[:, : p.shape[1] * 3] = p.reshape(p.shape[0], -1)
    buf = torch.from_numpy(host).cuda()
    return buf, [(buf.data_ptr() + off, p.shape[0], p.shape[1], p.shape[1] * 3 + pad) for p, pad, off in zip(pictures, pads, offs)]


def mixed_cases():
    """The encoder test's mixed batch, restated: 11 sizes x 4 layouts x 3 qualities, 640 x 640 4:2:0 q90, 200 x 200 in every layout."""
    cases = [(("noise", "ramp")[(si + li + qi) % 2], w, h, layout, q)
             for si, (w, h) in enumerate(m.SIZES) for li, layout in enumerate(m.LAYOUTS) for qi, q in enumerate((30, 75, 100))]
    cases.append(("noise", 640, 640, "420", 90))
    cases += [("noise", 200, 200, layout, 75) for layout in m.LAYOUTS]
    assert len(cases) == 137
    return cases


@pytest.fixture(scope="module")
def mixed():
    """(cases, pictures, [(descriptor, host coefficients)]): computed once, shared, never changed."""
    cases = mixed_cases()
    pictures = [m.picture(k, w, h, grey=layout == "grey") for (k, w, h, layout, q) in cases]
    items = []
    for (k, w, h, layout, q), p in zip(cases, pictures):
        d = m.enc_desc(w, h, layout, q)
        rc, coef = m.c_forward(d, p)
        assert rc == 0
        items.append((d, coef[: int(d.coef_count)]))
    return cases, pictures, items


def test_mixed_batch_through_the_whole_call(enc, mixed):
    """fh_jpeg_encode_batch_gpu takes one quality and one (colour) layout per call: every colour case goes through it in the group of its
    layout and quality, at odd frame addresses and padded pitches, with a None slot in the middle."""
    cases, pictures, items = mixed
    groups = {}
    for i, (k, w, h, layout, q) in enumerate(cases):
        if layout != "grey":
            groups.setdefault((layout, q), []).append(i)
    assert sum(len(g) for g in groups.values()) == 137 - 34
    for (layout, q), idx in groups.items():
        keep, frames = place_frames([pictures[i] for i in idx], [(0, 1, 5)[j % 3] for j in range(len(idx))])
        mid = len(idx) // 2
        frames = frames[:mid] + [None] + frames[mid:]
        got = enc.encode_dev(frames, quality=q, subsampling=layout, coder="device")
        assert got[mid] is None
        del got[mid]
        for i, data in zip(idx, got):
            assert data == host_file(*items[i]), cases[i]
        del keep
    keep, frames = place_frames([pictures[5]], [1])                            # n = 1
    k, w, h, layout, q = cases[5]
    assert layout != "grey"
    assert enc.encode_dev(frames, quality=q, subsampling=layout, coder="device") == [host_file(*items[5])]
    L = fa.lib()
    blobs = (_lib.FhBlob * 2)()
    assert L.fh_jpeg_encode_batch_gpu(enc.handle, fa.frame_array([None, None]), 2, 90, 2, blobs, 0) == 0       # only empty frames: no files
    assert not blobs[0].bytes and blobs[0].n == 0 and not blobs[1].bytes
    short = fa.frame_array([frames[0], (frames[0][0], 8, 8, 8 * 3 - 1)])
    assert L.fh_jpeg_encode_batch_gpu(enc.handle, short, 2, 90, 2, blobs, 0) == FH_ERR_ARG
    del keep


def test_mixed_batch_in_one_coder_call(enc, mixed):
    """All 137 cases — grey and the three colour layouts, three qualities, 1 x 1 to 640 x 640 — in ONE fh_jpeg_code_batch_dev, two slots
    skipped; and the device's own coefficients (fh_jpeg_forward_batch_dev) give the same files."""
    cases, pictures, items = mixed
    check_batch(enc, cases, items, skip=(0, len(cases) // 2))
    check_batch(enc, cases[:1], items[:1])                                     # n = 1


def craft_items():
    names, items = [], []
    for name, d, coef in hm.crafted():
        names.append(name); items.append((d, coef))
    return names, items


def entropy(data):
    at = data.index(b"\xff\xda")
    return data[at + 2 + int.from_bytes(data[at + 2: at + 4], "big"): -2]


def test_crafted_planes(enc):
    names, items = craft_items()
    files = check_batch(enc, names, items)
    # the batch is built as meant: asserted on the HOST writer's output
    host = [host_file(d, coef) for d, coef in items]
    assert files == host
    ecs = [entropy(f) for f in host]
    assert any(b"\xff\x00\xff\x00" in e for e in ecs)                          # two adjacent 0xFF bytes
    assert any(e.endswith(b"\xff\x00") for e in ecs)                           # a last stream byte of 0xFF
    assert any(int(host_bits(d, coef).sum()) % 8 == 0 for d, coef in items)    # a bit total that needs no pad
    assert any(int(host_bits(d, coef).sum()) % 8 != 0 for d, coef in items)    # and one that does
    chunk = fa.lib().fh_jpeg_stuff_chunk()
    assert chunk == 1024
    straddle = False
    for e in ecs:                                                              # stuffed bytes on either side of a chunk boundary of one image
        raw = np.frombuffer(e.replace(b"\xff\x00", b"\xff"), np.uint8)
        ff = np.flatnonzero(raw == 0xFF)
        straddle |= len(raw) > chunk and bool(np.any(ff < chunk)) and bool(np.any(ff >= chunk))
    assert straddle
    assert any(len(e.replace(b"\xff\x00", b"\xff")) > 2 * chunk for e in ecs)  # more than two chunks in one image


def test_limits_of_the_baseline_tables(enc):
    """+-2047 / +-1023 are coded (the extreme planes); one step beyond marks that image alone, and its neighbours equal the host's files."""
    good = {name: (d, coef) for name, d, coef in hm.crafted()}
    names, items = [], []
    for k, (name, d, coef) in enumerate(hm.uncodable()):
        g = ("extreme_grey", "extreme_420", "ramp_grey", "single_420")[k % 4]
        names += [g, name]; items += [good[g], (d, coef)]
    names.append("extreme_grey"); items.append(good["extreme_grey"])
    files, status, where, (before, after), whole = code_batch(enc, items)
    assert np.array_equal(before, after)
    at = 0
    for i, (name, (d, coef)) in enumerate(zip(names, items)):
        exp = host_file(d, coef)
        if i % 2 == 1:
            assert exp is None and status[i] == FH_ERR_ARG and files[i] is None and where[i] == (None, 0), name
        else:
            assert status[i] == 0 and files[i] == exp and where[i] == (at, len(exp)), name
            at += len(exp)
    files, status, _, _, _ = code_batch(enc, [items[1]])                       # alone: no file, the call still succeeds
    assert files == [None] and status.tolist() == [FH_ERR_ARG]


def test_workgroup_and_scan_boundaries(enc, mixed):
    """2049 x 8 grey: 257 blocks, more than a workgroup's four and no multiple of it; behind 640 x 640 4:2:0 (9600 blocks) the image
    boundary falls inside a scan chunk of 1024 blocks, as do the boundaries of the small images in front of it."""
    cases, pictures, items = mixed
    big = items[cases.index(("noise", 640, 640, "420", 90))]
    p = m.picture("noise", 2049, 8, grey=True)
    d = m.enc_desc(2049, 8, "grey", 75)
    rc, coef = m.c_forward(d, p)
    assert rc == 0 and hm.blocks_of(d) == 257
    small = items[40]
    batch = [small, big, (d, coef), items[41], (d, coef), big]
    firsts = np.cumsum([0] + [hm.blocks_of(x[0]) for x in batch])
    assert any(f % 1024 and f % 4 for f in firsts[1:-1]) and firsts[-1] > 2 * 1024 and firsts[-1] % 1024
    check_batch(enc, ["small", "640", "2049x8", "small2", "2049x8", "640"], batch)


def test_nothing_else_is_written(enc):
    names, items = craft_items()
    files, _, where, _, whole = code_batch(enc, items)                         # sizes the arena
    total = sum(size for _, size in where)
    a0, filled = arena(enc, fill=0xA5)
    assert len(filled) >= total and np.all(filled == 0xA5)
    again, _, where2, (before, after), whole = code_batch(enc, items)
    assert where2 == where and again == files and np.array_equal(before, after)
    assert len(whole) == len(filled) and np.all(whole[total:] == 0xA5)         # the files, back to back from the first byte, and nothing behind
    assert whole[:total].tobytes() == b"".join(files)
    fewer, _, where3, _, whole = code_batch(enc, items[:3])                    # a smaller batch leaves the rest of the arena alone
    used = sum(size for _, size in where3)
    assert np.array_equal(whole[used:total], np.frombuffer(b"".join(files), np.uint8)[used:total]) and np.all(whole[total:] == 0xA5)


def test_determinism(enc, mixed):
    cases, pictures, items = mixed
    names, crafted = craft_items()
    batch = crafted + items[100:110]
    a = code_batch(enc, batch)[0]
    b = code_batch(enc, batch)[0]
    assert a == b and None not in a
    for i in (0, 4, len(crafted) + 3):                                         # coded alone: the same bytes as inside the batch
        assert code_batch(enc, [batch[i]])[0] == [a[i]]
    pics = [pictures[i] for i in (5, 50, 101)] + [None]
    assert enc.encode(pics, quality=90, subsampling="4:2:0", coder="device") == enc.encode(pics, quality=90, subsampling="4:2:0", coder="host")
    with pytest.raises(ValueError):
        enc.encode(pics, coder="gpu")


def test_one_invalid_descriptor_stops_the_call(enc):
    names, items = craft_items()
    items = items[:4]
    code_batch(enc, items)
    a0, filled = arena(enc, fill=0xC3)
    for breakit in (lambda d: setattr(d, "orientation", 3), lambda d: setattr(d, "color", 2), lambda d: d.comp[0].quant.__setitem__(5, 0),
                    lambda d: setattr(d.comp[0], "wblocks", 40), lambda d: setattr(d.comp[0], "coef_off", 1 << 33)):
        bad = [(js.clone(d), coef) for d, coef in items]
        breakit(bad[2][0])
        _, status, _, (before, after), _ = code_batch(enc, bad, expect_rc=FH_ERR_ARG)
        assert np.array_equal(before, after) and np.all(status == 77)          # refused before anything was launched or written
        assert np.all(arena(enc)[1] == 0xC3)
    bad = [(js.clone(d), coef) for d, coef in items]                           # a bad descriptor in a skipped slot is not looked at
    bad[2][0].ncomp = 2
    files, status, _, _, _ = code_batch(enc, bad, skip=(2,))
    assert status.tolist() == [0, 0, 1, 0] and files[3] == host_file(*items[3])
    L = fa.lib()
    blobs = (_lib.FhBlob * 1)()
    d = items[0][0]
    t = torch.zeros(int(d.coef_count), dtype=torch.int16, device="cuda")
    base = np.zeros(1, np.int64)
    assert L.fh_jpeg_code_batch_dev(enc.handle, C.byref(d), 0, t.data_ptr(), base.ctypes.data, blobs, None, 0) == FH_ERR_ARG
    assert L.fh_jpeg_code_batch_dev(enc.handle, C.byref(d), 1, t.data_ptr() + 1, base.ctypes.data, blobs, None, 0) == FH_ERR_ARG
    assert L.fh_jpeg_code_batch_dev(enc.handle, C.byref(d), 1, t.data_ptr(), base.ctypes.data, blobs, None, 0) == 1    # status may be NULL


@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    return det, rec


def test_face_chips_with_the_device_coder(models_, enc, models_dir, tmp_path, capsys):
    det, rec = models_
    path = os.path.join(js.IMAGES, "c1_640x640.jpg")
    img = fa.imread(path)
    faces = det.detect_records(img, 0.5, 0.4)
    assert len(faces) >= 1
    files, crops = fa.face_chips(rec, img, faces, quality=90, subsampling="4:2:0", encoder=enc)
    dev_files, dev_crops = fa.face_chips(rec, img, faces, quality=90, subsampling="4:2:0", encoder=enc, coder="device")
    assert dev_files == files and None not in files and np.array_equal(crops, dev_crops)
    from facerecognizeonnx_amd import cli
    out_dir = str(tmp_path / "chips")
    dpath, rpath = util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0), util.tiny_iresnet(models_dir)
    assert cli.main(["detect", path, "--det", dpath, "--rec", rpath, "--chips", out_dir, "--chip-quality", "90", "--coder", "device"]) == 0
    assert "Chip 0:" in capsys.readouterr().out
    with open(os.path.join(out_dir, "c1_640x640_0.jpg"), "rb") as f:
        assert f.read() == files[0]
