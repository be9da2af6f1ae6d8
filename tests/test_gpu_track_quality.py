"""Face quality, best-shot re-embedding and the quality-weighted pool on the GPU (include/facehip.h, "face quality"; face_quality.hip and
the extended track.hip / track_ident.hip) held to their CPU model (tests/track_quality_model.py).  Every comparison is bit equality,
except the normalised pooled queries, which today's identity tests (tests/test_gpu_track_ident.py) hold to
gallery_fuse_model.unit_tolerance — a float64 unit form of the exact float32 sum against the device's float32 one; the same here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_fuse_model as gm    # noqa: E402
from tests import track_cases as tc           # noqa: E402
from tests import track_ident_model as im     # noqa: E402
from tests import track_quality_model as qm   # noqa: E402
from tests import util                        # noqa: E402

FH_ERR_ARG = -1
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
THRESHOLD = 0.6
IN = 128
DET_SEED, VIDEO_SEED, THR = 6, 7, (0.3, 0.4)                       # a seeded tiny detector whose landmarks give P > 0 on this video
LADDER = (256, 320, 400, 500, 625)                                 # neighbours are exactly 5 / 4 apart: ties at the ratio


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def dev_records(det):
    return dev(np.ascontiguousarray(det).view(np.uint8).reshape(-1, 60))


def records(t, n):
    return t.cpu().numpy().view(np.uint8).reshape(n, 60).copy().view(fa.FACE_DTYPE).reshape(n)


def from_device(ptr, shape, dtype=np.float32):
    out = np.empty(shape, dtype)
    if out.size:
        assert ptr and fa.lib().fh_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0, _lib.last_error()
    return out


def i32(shape, v=77):
    return torch.full(shape, v, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def cases():
    return {name: tc.Case(name) for name in tc.CASES}


# ---------------------------------------------------------------------------------------------- 1. the score
F1 = 24
FRONTAL = (30.0, 40.0, 50.0, 40.0, 40.0, 50.0, 32.0, 60.0, 48.0, 60.0)


def padded_frames(rng, n, rows, cols, pad):
    """n frames of random bytes with a row pitch of cols * 3 + pad (the padding is random too): (buffer [n][rows][step], images)."""
    buf = rng.integers(0, 256, (n, rows, cols * 3 + pad), dtype=np.uint8)
    return buf, [buf[f, :, :cols * 3].reshape(rows, cols, 3) for f in range(n)]


def planted_records(rng, rows, cols):
    """F1 records for a rows x cols frame: every hazard of the contract, then live-looking filler."""
    det = np.zeros(F1, fa.FACE_DTYPE)
    lm = np.array(FRONTAL, np.float32)
    bw, bh = min(50, cols - 12), min(60, rows - 12)                # a box that fits inside
    boxes = [(6, 5, bw, bh),                                        # inside
             (-10, 5, 30, bh), (6, -9, bw, 30), (cols - 15, 5, 40, bh), (6, rows - 14, bw, 40),     # across each edge
             (cols + 50, rows + 50, 40, 40), (-100, -100, 40, 40), (cols - 1, 3, 40, 40),           # wholly outside / one column left
             (20, 10, -12, 20), (20, 10, 20, -12),                  # negative w, negative h
             (10, 10, 8, 8), (10, 10, 7, 9), (10, 10, 9, 7),        # at and just below the floor
             (0, 0, cols, rows), (-7, -7, cols + 30, rows + 30),    # the whole frame
             (5, 5, INT_MAX - 5, bh), (INT_MAX - 10, 5, INT_MAX, bh), (INT_MIN, INT_MIN, INT_MAX, INT_MAX), (3, INT_MAX, 20, INT_MAX),
             (6, 5, bw, bh), (6, 5, bw, bh), (6, 5, bw, bh)]        # the landmark cases below
    for j in range(F1):
        b = boxes[j] if j < len(boxes) else (int(rng.integers(0, cols // 2)), int(rng.integers(0, rows // 2)), int(rng.integers(8, cols)),
                                             int(rng.integers(8, rows)))
        det[j]["x"], det[j]["y"], det[j]["w"], det[j]["h"] = b
        det[j]["lm"] = lm + rng.uniform(-3, 3, 10).astype(np.float32)
        det[j]["score"] = 0.9
    k = len(boxes) - 3
    det[k]["lm"][2] = det[k]["lm"][0]                               # the eyes coincide
    det[k]["lm"][4] = det[k]["lm"][0] + np.float32(0.25)
    det[k + 1]["lm"][4] = det[k + 1]["lm"][2] + np.float32(4.0)     # the nose beyond the right eye: P = 0
    det[k + 2]["lm"][0] = np.nan
    det[0]["lm"] = lm                                               # a frontal face: P = 256
    return det


SIZES = {"160x200": (160, 200, 8), "40x48": (40, 48, 5)}           # rows, cols, row padding (an odd pitch for the small one)


@pytest.fixture(scope="module")
def score_cases():
    out = {}
    for name, (rows, cols, pad) in SIZES.items():
        rng = np.random.default_rng(rows)
        buf, imgs = padded_frames(rng, 4, rows, cols, pad)
        det = np.stack([planted_records(rng, rows, cols) for _ in range(4)])
        counts = np.array([F1, F1 + 7, 0, 5], np.int32)
        events = set()
        want = qm.quality_batch(imgs, det, counts, F1, events)
        want.setflags(write=False)
        out[name] = dict(rows=rows, cols=cols, step=cols * 3 + pad, buf=buf, imgs=imgs, det=det, counts=counts, want=want, events=events)
    return out


@pytest.mark.parametrize("name", list(SIZES))
def test_score_equals_the_model(score_cases, name):
    c = score_cases[name]
    want = c["want"]
    # the premises: the hazards score what the contract says, the live ones score something
    assert want[0, 0] > 0 and (want[0, 5:10] == 0).all() and want[0, 10] > 0 and want[0, 11] == 0 and want[0, 12] == 0
    assert want[0, 13] > 0 and want[0, 15] > 0 and (want[0, 16:19] == 0).all() and want[0, 19] > 0 and want[0, 20] == 0 and want[0, 21] == 0
    assert (want[2] == 0).all() and (want[3, 5:] == 0).all() and (want[1] == qm.quality_batch(c["imgs"][1:2], c["det"][1:2], [F1], F1)).all()
    assert ("strided" in c["events"]) == (name == "160x200")       # the whole-frame box of the large frame reaches d = 2
    fd, d, cnt, q = dev(c["buf"]), dev_records(c["det"]), dev(c["counts"]), i32((4, F1))
    assert fa.face_quality_dev(fd.data_ptr(), d.data_ptr(), cnt.data_ptr(), F1, q.data_ptr(), n=4, rows=c["rows"], cols=c["cols"],
                               step=c["step"]) == 4
    torch.cuda.synchronize()
    got = q.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_score_through_the_ragged_twin(score_cases):
    """Frames of different sizes and an empty one, each with its own pitch, in one call."""
    big, small = score_cases["160x200"], score_cases["40x48"]
    rng = np.random.default_rng(5)
    mid_buf, mid_imgs = padded_frames(rng, 1, 64, 72, 0)
    bufs = [dev(big["buf"][0]), None, dev(small["buf"][1]), dev(mid_buf[0]), dev(small["buf"][0])]
    imgs = [big["imgs"][0], None, small["imgs"][1], mid_imgs[0], small["imgs"][0]]
    det = np.stack([big["det"][0], big["det"][1], small["det"][1], planted_records(rng, 64, 72), small["det"][0]])
    counts = np.array([F1, F1, F1 + 3, 9, 0], np.int32)
    shapes = [(160, 200, big["step"]), (0, 0, 0), (40, 48, small["step"]), (64, 72, 72 * 3), (40, 48, small["step"])]
    frames = [(b.data_ptr() if b is not None else 0, r, c, s) for b, (r, c, s) in zip(bufs, shapes)]
    want = qm.quality_batch(imgs, det, counts, F1)
    assert (want[1] == 0).all() and (want[4] == 0).all() and (want[3, 9:] == 0).all() and want[0, 0] > 0 and want[2, 0] > 0 and want[3, 0] > 0
    assert np.array_equal(want[0], big["want"][0])
    d, cnt, q = dev_records(det), dev(counts), i32((5, F1))
    assert fa.face_quality_dev(frames, d.data_ptr(), cnt.data_ptr(), F1, q.data_ptr()) == 5
    torch.cuda.synchronize()
    got = q.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


# ---------------------------------------------------------------------------------------------- 2. the update
class Walk:
    """Seeded random walks in the style of tests/track_cases.py — a population of drifting boxes per stream with births and deaths, the
    streams interleaved — with a quality per entry drawn from LADDER (whose neighbours tie exactly at 5 / 4), 0 and two outliers."""

    def __init__(self, seed, stream_of, per_frame, cap, grid=False):
        rng = np.random.default_rng(seed)
        self.stream_of = np.asarray(stream_of, np.int32)
        self.n, self.per_frame, self.streams = len(stream_of), per_frame, int(max(stream_of)) + 1
        self.det = np.zeros((self.n, per_frame), fa.FACE_DTYPE)
        self.counts = np.zeros(self.n, np.int32)
        walkers = [[] for _ in range(self.streams)]
        for f in range(self.n):
            if grid:                                                # more faces than lanes: jittered cells, a random subset per frame
                count = int(rng.choice([per_frame, per_frame + 9, per_frame - 4, 66, 3]))
                cells = [(45 * (i % 10) + int(rng.integers(-2, 3)), 45 * (i // 10) + int(rng.integers(-2, 3)), 30, 30) for i in range(90)]
                boxes = [cells[i] for i in rng.permutation(90)[:count]]
            else:
                w = walkers[int(self.stream_of[f])]
                w[:] = [b for b in w if rng.random() > 0.1]
                for b in w:
                    b[0] += int(rng.integers(-3, 4)); b[1] += int(rng.integers(-3, 4))
                while len(w) < cap and rng.random() < 0.5:
                    w.append([int(rng.integers(0, 400)), int(rng.integers(0, 400)), int(rng.integers(20, 60)), int(rng.integers(20, 60))])
                boxes = [tuple(w[i]) for i in rng.permutation(len(w))]
                count = len(boxes)
            self.counts[f] = count
            boxes = boxes[:per_frame]
            while len(boxes) < per_frame:                           # garbage behind the count: boxes that WOULD match
                boxes.append(boxes[int(rng.integers(len(boxes)))] if boxes else (10, 10, 30, 30))
            for j, b in enumerate(boxes):
                self.det[f, j]["x"], self.det[f, j]["y"], self.det[f, j]["w"], self.det[f, j]["h"] = b
        self.quality = rng.choice(LADDER + LADDER + (0, 1000, 99999), (self.n, per_frame)).astype(np.int32)


def interleaved(seed, sizes):
    rng = np.random.default_rng(seed)
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


WALKS = {     # name -> (max_tracks, max_missed, walk): more than 64 frames of stream 0 in a call / more than 64 detections in a frame
    "three_slots": (3, 1, lambda: Walk(11, interleaved(1, [150, 30, 30]), 5, 5)),
    "one_slot": (1, 0, lambda: Walk(12, interleaved(2, [140, 20]), 2, 2)),
    "64_slots": (64, 1, lambda: Walk(13, interleaved(3, [8, 4]), 70, 0, grid=True)),
}


@pytest.fixture(scope="module")
def walks():
    return {name: make() for name, (_, _, make) in WALKS.items()}


def state_bytes(trk, streams):
    parts = []
    for s in range(streams):
        st, fno, nid = trk.state(s, counters=True)
        parts.append(st.tobytes() + bytes([fno % 256, nid % 256]))
    return b"".join(parts)


def check_state(trk, model, streams):
    for s in range(streams):
        got, fno, nid = trk.state(s, counters=True)
        want, wf, wn = model.state(s)
        assert [tuple(int(v) for v in r) for r in got] == want and (fno, nid) == (wf, wn), s
        assert np.array_equal(trk.best_quality(s), model.best_quality(s)), s


def update_q(trk, w, first, last, quality, slot=True, sync=True):
    n, per = last - first, w.per_frame
    d, cnt = dev_records(w.det[first:last]), dev(w.counts[first:last])
    q = dev(quality[first:last]) if quality is not None else None
    t3 = [i32((n, per)) for _ in range(3)]
    assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, t3[0].data_ptr(), t3[1].data_ptr(), stream_of=w.stream_of[first:last],
                          slot_ptr=t3[2].data_ptr() if slot else None, quality_ptr=q.data_ptr() if q is not None else None) == n
    if sync:
        torch.cuda.synchronize()
    return t3


@pytest.mark.parametrize("refresh,min_gap", [(0, 1), (0, 4), (3, 1), (3, 4)])
@pytest.mark.parametrize("name", list(WALKS))
def test_update_equals_the_model(walks, name, refresh, min_gap):
    w = walks[name]
    max_tracks, max_missed, _ = WALKS[name]
    kw = dict(streams=w.streams, max_tracks=max_tracks, iou_thr=0.3, max_missed=max_missed, refresh=refresh)
    trk, model = fa.Tracker(**kw), qm.IdentTracker(64, bestshot=(5, 4, min_gap), **kw)
    trk.set_bestshot(5, 4, min_gap)
    cut = w.n * 2 // 3                                              # two calls: best_q survives in the state
    if name != "64_slots":
        assert (w.stream_of[:cut] == 0).sum() > 64                  # the frame loop of stream 0 turns over in the first call
    else:
        assert w.counts.max() > 64 and w.per_frame > 64             # the detection loop turns over
    for a, b in ((0, cut), (cut, w.n)):
        want = model.update(w.det[a:b], w.counts[a:b], w.per_frame, w.stream_of[a:b], w.quality[a:b])
        got = update_q(trk, w, a, b, w.quality)
        for key, g, x in zip(("track", "embed", "slot"), got, want):
            g = g.cpu().numpy()
            assert np.array_equal(g, x), (key, a, np.argwhere(g != x)[:5])
        check_state(trk, model.trk, w.streams)
    ev = model.trk.events
    assert "exact_ratio" in ev, ev                                  # a face sat exactly at the ratio
    # the rule fired on its own — unless the timer always comes first: it resets last_embed every `refresh` <= min_gap frames
    assert ("bestshot" in ev) == (not 0 < refresh <= min_gap), ev
    if min_gap > 1:
        assert "held_back" in ev, ev
    if refresh:
        assert "refresh" in ev
    assert any(model.trk.best_quality(s).size and model.trk.best_quality(s).max() > 0 for s in range(w.streams))


def test_reset_and_a_second_set_bestshot_clear_the_best_qualities(walks):
    w = walks["three_slots"]
    kw = dict(streams=w.streams, max_tracks=3, iou_thr=0.3, max_missed=1, refresh=0)
    trk, model = fa.Tracker(**kw), qm.Tracker((5, 4, 1), **kw)
    trk.set_bestshot(5, 4, 1)
    model.update(w.det, w.counts, w.per_frame, w.stream_of, w.quality)
    update_q(trk, w, 0, w.n, w.quality)
    check_state(trk, model, w.streams)
    assert all(model.best_quality(s).max() > 0 for s in range(w.streams))
    trk.reset(1)
    model.reset(1)
    check_state(trk, model, w.streams)
    before = state_bytes(trk, w.streams)
    trk.set_bestshot(2, 1, 3)                                       # again: clears every stream's, leaves the tracks
    assert state_bytes(trk, w.streams) == before
    assert all((trk.best_quality(s) == 0).all() and len(trk.best_quality(s)) == len(trk.state(s)) for s in range(w.streams))


# ---------------------------------------------------------------------------------------------- 3. nothing changes when unused
@pytest.mark.parametrize("name", list(tc.CASES))
def test_nothing_changes_when_unused(cases, name):
    case = cases[name]
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    rng = np.random.default_rng(3)
    equal = np.full((case.n, case.per_frame), 4321, np.int32)
    noise = rng.integers(0, 100000, (case.n, case.per_frame)).astype(np.int32)
    plain, on_equal, off_noise, cleared = (fa.Tracker(**kw) for _ in range(4))
    on_equal.set_bestshot(5, 4, 1)
    cleared.set_bestshot(1, 1, 1)
    cleared.clear_bestshot()
    want = update_q(plain, case, 0, case.n, None)                                  # fh_track_update_slots_dev
    for trk, quality, what in ((on_equal, equal, "on, equal"), (off_noise, noise, "off, noise"), (cleared, noise, "cleared, noise")):
        got = update_q(trk, case, 0, case.n, quality)
        for g, x in zip(got, want):
            assert g.cpu().numpy().tobytes() == x.cpu().numpy().tobytes(), what
        assert state_bytes(trk, case.streams) == state_bytes(plain, case.streams), what
    assert (cleared.best_quality(0) == 0).all()                                    # the policy off: best_q is not touched
    no_slot = fa.Tracker(**kw)                                                      # ... and fh_track_update_dev is what it was
    got = update_q(no_slot, case, 0, case.n, None, slot=False)
    assert got[0].cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes() and got[1].cpu().numpy().tobytes() == want[1].cpu().numpy().tobytes()
    assert torch.all(got[2] == 77)


# ---------------------------------------------------------------------------------------------- 4. the weighted pool
class Gal:
    def __init__(self, dim, rows=None):
        rng = np.random.default_rng(900 + dim)
        self.dim = dim
        self.rows = gm.unit_rows(rng, 300, dim) if rows is None else rows
        self.g = fa.Gallery(dim)
        self.g.enroll(self.rows, None)

    def label(self, q_ptr, total):
        lab, sc = i32((max(total, 1),), 55), torch.full((max(total, 1),), 5.5, device="cuda")
        for c0 in range(0, total, 256):
            self.g.label_dev(q_ptr + c0 * self.dim * 4, min(256, total - c0), THRESHOLD, lab.data_ptr() + c0 * 4, sc.data_ptr() + c0 * 4)
        torch.cuda.synchronize()
        return lab.cpu().numpy()[:total], sc.cpu().numpy()[:total]


def identity_bytes(trk, streams):
    return b"".join(a.tobytes() for s in range(streams) for a in trk.identity(s, sums=True)) + state_bytes(trk, streams)


def pool_case(case, dim):
    """Qualities (a fifth of them 0: weight 1) and one unit embedding per entry of a tc case."""
    rng = np.random.default_rng(dim + sum(case.name.encode()))
    quality = rng.choice(LADDER + (0, 0, 7, 1000, 114240), (case.n, case.per_frame)).astype(np.int32)
    return quality, gm.unit_rows(rng, case.n * case.per_frame, dim).astype(np.float32)


def identify(trk, case, gal, out, rows, quality, total=None):
    n, per = case.n, case.per_frame
    total = len(rows) if total is None else total
    label, score = i32((n, per)), torch.full((n, per), 7.0, device="cuda")
    d_emb = dev(rows)
    q = dev(quality) if quality is not None else None
    assert trk.identify_dev(gal.g, THRESHOLD, out[0].data_ptr(), out[2].data_ptr(), out[1].data_ptr(), d_emb.data_ptr(), total, n, per,
                            label.data_ptr(), score.data_ptr(), stream_of=case.stream_of,
                            quality_ptr=q.data_ptr() if q is not None else None) == n
    torch.cuda.synchronize()
    return label.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("dim", [64, 512])
def test_weighted_pool_equals_the_model(cases, dim):
    case, gal = cases["three_streams_exhausted"], Gal(dim)
    quality, entry_emb = pool_case(case, dim)
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    trk, model = fa.Tracker(**kw), qm.IdentTracker(dim, qm.POOL_WEIGHTED, bestshot=(5, 4, 1), **kw)
    trk.set_bestshot(5, 4, 1)
    trk.enable_identity(dim, fa.TRACK_POOL_WEIGHTED)
    wt, we, ws = model.update(case.det, case.counts, case.per_frame, case.stream_of, quality)
    out = update_q(trk, case, 0, case.n, quality)
    assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(out, (wt, we, ws)))
    rows = np.ascontiguousarray(entry_emb[np.flatnonzero(we.reshape(-1) != 0)])
    total = len(rows)
    # NULL qualities: FH_ERR_ARG before anything is launched, the state untouched
    before = identity_bytes(trk, case.streams)
    label, score = i32((case.n, case.per_frame)), torch.full((case.n, case.per_frame), 7.0, device="cuda")
    d_emb = dev(rows)
    for call in ("fh_track_identify_dev", "fh_track_identify_q_dev"):
        args = [trk.handle, gal.g._h, THRESHOLD, out[0].data_ptr(), out[2].data_ptr(), out[1].data_ptr()] + \
            ([None] if call.endswith("_q_dev") else []) + \
            [d_emb.data_ptr(), total, case.n, case.per_frame, case.stream_of.ctypes.data, label.data_ptr(), score.data_ptr(), 0]
        assert getattr(fa.lib(), call)(*args) == FH_ERR_ARG and "weighted pool" in _lib.last_error(), call
    torch.cuda.synchronize()
    assert identity_bytes(trk, case.streams) == before and torch.all(label == 77) and torch.all(score == 7.0)
    assert all((sums == 0).all() for s in range(case.streams) for sums in [trk.identity(s, sums=True)[1]])
    # the real call
    got_l, got_s = identify(trk, case, gal, out, rows, quality)
    q_dev = from_device(trk.queries_ptr(), (total, dim))
    q64, verbatim = model.pool_queries(wt, ws, we, rows, total, case.stream_of, quality=quality)
    assert q_dev[verbatim].tobytes() == rows[verbatim].tobytes()
    ok = gm.within_unit_tolerance(q_dev[~verbatim], q64[~verbatim], dim)           # (test_gpu_track_ident.py's tolerance for normalize)
    assert ok.all(), np.argwhere(~ok)[:5]
    labs, scs = gal.label(trk.queries_ptr(), total)
    want_l, want_s = model.carry(wt, ws, we, labs, scs, total, case.stream_of)
    assert np.array_equal(got_l, want_l) and got_s.tobytes() == want_s.tobytes()
    for s in range(case.streams):                                                  # the sums, bit for bit
        recs, sums = trk.identity(s, sums=True)
        want, want_sums = model.identity(s)
        assert [(int(r["id"]), int(r["n_emb"])) for r in recs] == [x[:2] for x in want], s
        assert sums.tobytes() == want_sums.tobytes(), (s, np.argwhere(sums != want_sums)[:5])
    assert {"reopened", "pooled", "untracked", "weight_one"} <= model.events, model.events
    assert not verbatim.all() and verbatim.any()


@pytest.mark.parametrize("pool", [im.POOL_SUM, im.POOL_LAST])
def test_the_other_pools_ignore_the_qualities(cases, pool):
    case, gal = cases["three_streams_exhausted"], Gal(64)
    quality, entry_emb = pool_case(case, 64)
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    results = []
    for with_q in (False, True):
        trk = fa.Tracker(**kw)
        trk.enable_identity(64, pool)
        out = update_q(trk, case, 0, case.n, None)
        flags = out[1].cpu().numpy()
        rows = np.ascontiguousarray(entry_emb[np.flatnonzero(flags.reshape(-1) != 0)])
        got = identify(trk, case, gal, out, rows, quality if with_q else None)
        results.append((got[0].tobytes(), got[1].tobytes(), from_device(trk.queries_ptr(), (len(rows), 64)).tobytes(),
                        identity_bytes(trk, case.streams)))
    assert results[0] == results[1]


# ---------------------------------------------------------------------------------------------- 5. the pipeline
@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, seed=DET_SEED, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    assert det.input_size() == (IN, IN)
    return det, rec


def pipeline_bufs(n, F, dim=512):
    return dict(all=torch.full((n * F, 15), 5.0, device="cuda"), cnt=i32((n,), -5), track=i32((n, F)), faces=torch.full((n * F, 15), 7.0, device="cuda"),
                fo=i32((n * F,), -7), to=i32((n * F,), -7), emb=torch.full((n * F, dim), 7.0, device="cuda"), label=i32((n, F)),
                score=torch.full((n, F), 7.0, device="cuda"))


def blurred(img):
    """A 3 x 3 box filter: the same picture, less sharp."""
    p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    rows, cols = img.shape[:2]
    return ((sum(p[dy:dy + rows, dx:dx + cols] for dy in range(3) for dx in range(3)) + 4) // 9).astype(np.uint8)


@pytest.mark.parametrize("policy,refresh,pool", [(True, 2, qm.POOL_WEIGHTED), (True, 0, im.POOL_SUM), (False, 2, im.POOL_SUM)])
def test_pipeline_equals_its_stages(models_, policy, refresh, pool):
    """a A A B B A on one stream, `a` being A blurred: the tracks open on the blurred frame, and the sharp one that follows is the better
    shot.  (The landmarks of a seeded detector are noise; DET_SEED and VIDEO_SEED were chosen so that every face of this video has P > 0
    — the premise is asserted below.)"""
    det, rec = models_
    F = 4
    two = util.frames_u8(2, IN, IN, seed=VIDEO_SEED, smooth=True)
    frames = np.ascontiguousarray(np.stack([blurred(two[0]), two[0], two[0], two[1], two[1], two[0]]))
    n, fd = len(frames), dev(frames)
    kw = dict(streams=1, max_tracks=8, iou_thr=0.3, max_missed=0, refresh=refresh)

    def tracker():
        t = fa.Tracker(**kw)
        if policy:
            t.set_bestshot(1, 1, 1)                                               # any improvement embeds again
        t.enable_identity(512, pool)
        return t
    # the stages by hand: detect, quality, update, select, embed, identify
    hand, h = tracker(), pipeline_bufs(n, F)
    assert det.detect_batch_dev(fd.data_ptr(), n, IN, IN, h["all"].data_ptr(), F, h["cnt"].data_ptr(), *THR) == n
    quality = i32((n, F))
    if policy:
        assert fa.face_quality_dev(fd.data_ptr(), h["all"].data_ptr(), h["cnt"].data_ptr(), F, quality.data_ptr(), n=n, rows=IN, cols=IN) == n
    qp = quality.data_ptr() if policy else None
    embed, slot, d_total = i32((n, F)), i32((n, F)), i32((1,))
    assert hand.update_dev(h["all"].data_ptr(), h["cnt"].data_ptr(), n, F, h["track"].data_ptr(), embed.data_ptr(), slot_ptr=slot.data_ptr(),
                           quality_ptr=qp) == n
    assert fa.Tracker.select_dev(h["all"].data_ptr(), embed.data_ptr(), n, F, h["faces"].data_ptr(), h["fo"].data_ptr(), h["track"].data_ptr(),
                                 h["to"].data_ptr(), d_total.data_ptr()) == n
    torch.cuda.synchronize()
    total = int(d_total.cpu().numpy()[0])
    counts = h["cnt"].cpu().numpy()
    assert counts[0] >= 2 and counts[3] >= 2 and total >= 2, counts               # premise: A and B each yield at least 2 faces
    assert fa.lib().fh_rec_embed_faces_dev(rec.handle, fd.data_ptr(), IN, IN, IN * 3, IN * IN * 3, h["faces"].data_ptr(), h["fo"].data_ptr(),
                                           total, h["emb"].data_ptr(), 0, 0) == total, _lib.last_error()
    torch.cuda.synchronize()
    gal = Gal(512, rows=h["emb"][:2].cpu().numpy())                               # the first two faces of frame A are the gallery
    assert hand.identify_dev(gal.g, THRESHOLD, h["track"].data_ptr(), slot.data_ptr(), embed.data_ptr(), h["emb"].data_ptr(), total, n, F,
                             h["label"].data_ptr(), h["score"].data_ptr(), quality_ptr=qp) == n
    torch.cuda.synchronize()
    hand_queries = from_device(hand.queries_ptr(), (total, 512))
    # the pipeline
    trk, b = tracker(), pipeline_bufs(n, F)
    got_total = fa.pipeline_run_identified_dev(det, rec, trk, gal.g, THRESHOLD, fd.data_ptr(), n, IN, IN, F, b["all"].data_ptr(), b["cnt"].data_ptr(),
                                               b["track"].data_ptr(), b["faces"].data_ptr(), b["fo"].data_ptr(), b["to"].data_ptr(),
                                               b["emb"].data_ptr(), b["label"].data_ptr(), b["score"].data_ptr(), scoreThreshold=THR[0],
                                               nmsThreshold=THR[1])
    torch.cuda.synchronize()
    assert got_total == total
    for key in b:
        assert b[key].cpu().numpy().tobytes() == h[key].cpu().numpy().tobytes(), key
    assert from_device(trk.queries_ptr(), (total, 512)).tobytes() == hand_queries.tobytes()
    assert identity_bytes(trk, 1) == identity_bytes(hand, 1)
    q_host = quality.cpu().numpy()
    if policy:
        assert from_device(trk.quality_ptr(), (n, F), np.int32).tobytes() == q_host.tobytes()
        assert np.array_equal(trk.best_quality(0), hand.best_quality(0))
        frames_list = [frames[f] for f in range(n)]
        recs = records(h["all"], n * F).reshape(n, F)
        assert np.array_equal(q_host, qm.quality_batch(frames_list, recs, counts, F))        # the detector's records, the model's score
        model = qm.IdentTracker(512, pool, bestshot=(1, 1, 1), **kw)
        wt, we, ws = model.update(recs, counts, F, None, q_host)
        assert np.array_equal(embed.cpu().numpy(), we) and np.array_equal(slot.cpu().numpy(), ws)
        assert np.array_equal(hand.best_quality(0), model.trk.best_quality(0))
        assert (q_host[:, :2] > 0).all() and "bestshot" in model.trk.events       # premises: real scores, and the rule fired on its own
        assert we[1].sum() >= 2                                                   # ... on the first sharp frame
        print(f"best-shot pipeline, refresh {refresh}: {total} faces embedded, events {sorted(model.trk.events)}")
    else:
        assert trk.quality_ptr() == 0                                             # the policy off: no buffer, nothing launched


# ---------------------------------------------------------------------------------------------- 6. arguments
def test_argument_errors_launch_nothing(walks, score_cases):
    L, w = fa.lib(), walks["three_slots"]
    kw = dict(streams=w.streams, max_tracks=3, iou_thr=0.3, max_missed=1, refresh=0)
    trk, model = fa.Tracker(**kw), qm.Tracker((5, 4, 2), **kw)
    assert L.fh_tracker_get_quality(trk.handle, 0, np.zeros(3, np.int32).ctypes.data) == FH_ERR_ARG       # never set
    assert "fh_tracker_get_quality" in _lib.last_error()
    trk.set_bestshot(5, 4, 2)
    half = w.n // 2
    model.update(w.det[:half], w.counts[:half], w.per_frame, w.stream_of[:half], w.quality[:half])
    update_q(trk, w, 0, half, w.quality)
    for what, (on, num, den, gap) in [("den < 1", (1, 5, 0, 1)), ("num < den", (1, 3, 4, 1)), ("num > 32768", (1, 32769, 4, 1)),
                                      ("min_gap < 1", (1, 5, 4, 0)), ("negative", (1, -5, -4, 1)), ("off, bad limits", (0, 3, 4, 1))]:
        assert L.fh_tracker_set_bestshot(trk.handle, on, num, den, gap) == FH_ERR_ARG and "fh_tracker_set_bestshot" in _lib.last_error(), what
    assert L.fh_tracker_set_bestshot(None, 1, 5, 4, 1) == FH_ERR_ARG
    assert L.fh_tracker_get_quality(trk.handle, w.streams, np.zeros(3, np.int32).ctypes.data) == FH_ERR_ARG
    assert L.fh_tracker_get_quality(trk.handle, 0, None) == FH_ERR_ARG
    check_state(trk, model, w.streams)                              # nothing was cleared; the policy (5, 4, 2) still holds:
    want = model.update(w.det[half:], w.counts[half:], w.per_frame, w.stream_of[half:], w.quality[half:])
    got = update_q(trk, w, half, w.n, w.quality)
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    check_state(trk, model, w.streams)
    assert fa.Tracker(**kw).set_bestshot(32768, 32768, 1) is None and fa.Tracker(**kw).set_bestshot(32768, 1, 10 ** 6) is None
    # the score
    c = score_cases["40x48"]
    fd, d, cnt, q = dev(c["buf"]), dev_records(c["det"]), dev(c["counts"]), i32((4, F1))
    P = dict(frames=fd.data_ptr(), n=4, rows=c["rows"], cols=c["cols"], step=c["step"], det=d.data_ptr(), cnt=cnt.data_ptr(), per=F1,
             q=q.data_ptr())

    def score(**kv):
        a = dict(P, **kv)
        return L.fh_face_quality_dev(a["frames"], a["n"], a["rows"], a["cols"], a["step"], a["rows"] * a["step"], a["det"], a["cnt"], a["per"],
                                     a["q"], 0)
    for what, kv in [("null output", dict(q=None)), ("null frames", dict(frames=None)), ("null records", dict(det=None)),
                     ("null counts", dict(cnt=None)), ("n = 0", dict(n=0)), ("n > 4096", dict(n=4097)), ("per_frame = 0", dict(per=0)),
                     ("rows = 0", dict(rows=0)), ("cols = 0", dict(cols=0)), ("a pitch below the row", dict(step=c["cols"] * 3 - 1))]:
        assert score(**kv) == FH_ERR_ARG and "fh_face_quality_dev" in _lib.last_error(), what
    frames = fa.frame_array([(fd.data_ptr(), c["rows"], c["cols"], c["step"])] * 4)
    assert L.fh_face_quality_ragged_dev(frames, 4, d.data_ptr(), cnt.data_ptr(), F1, None, 0) == FH_ERR_ARG
    assert "fh_face_quality_ragged_dev" in _lib.last_error()
    assert L.fh_face_quality_ragged_dev(None, 4, d.data_ptr(), cnt.data_ptr(), F1, q.data_ptr(), 0) == FH_ERR_ARG
    short = fa.frame_array([(fd.data_ptr(), c["rows"], c["cols"], c["cols"] * 3 - 1)])
    assert L.fh_face_quality_ragged_dev(short, 1, d.data_ptr(), cnt.data_ptr(), F1, q.data_ptr(), 0) == FH_ERR_ARG
    # the update and the pool mode
    t3 = [i32((4, F1)) for _ in range(3)]
    assert L.fh_track_update_q_dev(trk.handle, d.data_ptr(), cnt.data_ptr(), 4, F1, None, None, t3[1].data_ptr(), t3[2].data_ptr(), q.data_ptr(),
                                   0) == FH_ERR_ARG and "fh_track_update_q_dev" in _lib.last_error()
    assert L.fh_tracker_enable_identity(trk.handle, 64, 3) == FH_ERR_ARG
    fresh = fa.Tracker(**kw)                                        # the weighted pool needs the opt-in of fh_tracker_set_bestshot
    assert L.fh_tracker_enable_identity(fresh.handle, 64, fa.TRACK_POOL_WEIGHTED) == FH_ERR_ARG
    assert "fh_tracker_enable_identity" in _lib.last_error() and L.fh_tracker_get_identity(fresh.handle, 0, None, None) == FH_ERR_ARG
    fresh.clear_bestshot()                                          # on = 0 opts in as well
    assert L.fh_tracker_enable_identity(fresh.handle, 64, fa.TRACK_POOL_WEIGHTED) == 0
    torch.cuda.synchronize()
    assert torch.all(q == 77) and all(torch.all(t == 77) for t in t3)              # nothing was launched
    check_state(trk, model, w.streams)
