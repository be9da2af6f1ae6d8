"""Per-track identity on the GPU (include/facehip.h, "track identity"; track_ident.hip) held to its CPU model
(tests/track_ident_model.py): the slots the update reports, the pooled sums BIT FOR BIT, the queries (verbatim rows to the bit, pooled
rows to gallery_fuse_model.unit_tolerance), and — given the device's own queries, labelled by the test through the gallery's existing
calls — every label and score of the call and of the state, on the record streams of tests/track_cases.py, across truncated, split and
back-to-back calls, and through fh_pipeline_run_identified_dev with the tiny detector and recogniser."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_fuse_model as gm    # noqa: E402
from tests import track_cases as tc           # noqa: E402
from tests import track_ident_model as im     # noqa: E402
from tests import util                        # noqa: E402

FH_ERR_ARG = -1
THRESHOLD = 0.6
G_ROWS = 300
IN = 128
VIDEO_SEED, THR = 42, (0.3, 0.4)                                   # the A A A B B A video of tests/test_gpu_track.py


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


@pytest.fixture(scope="module")
def cases():
    return {name: tc.Case(name) for name in tc.CASES}


class Gal:
    """A gallery of G_ROWS unit rows (labelled: sparse ids with several rows per identity), on the host and on the device."""

    def __init__(self, dim, labelled, rows=None, empty=False):
        rng = np.random.default_rng(900 + dim)
        self.dim, self.labelled = dim, labelled
        self.rows = gm.unit_rows(rng, G_ROWS, dim) if rows is None else rows
        self.ids = (rng.integers(0, 90, len(self.rows)) * 5 + 2).astype(np.int32) if labelled else None
        self.g = fa.Gallery(dim)
        if not empty:
            self.g.enroll(self.rows, self.ids)

    def label(self, q_ptr, total, thr=THRESHOLD):
        """The test's own stage B on a device query buffer: chunks of at most 256 through the gallery's existing calls."""
        lab = torch.full((max(total, 1),), 55, dtype=torch.int32, device="cuda")
        sc = torch.full((max(total, 1),), 5.5, device="cuda")
        for c0 in range(0, total, 256):
            q = min(256, total - c0)
            call = self.g.label_ids_dev if self.labelled else self.g.label_dev
            call(q_ptr + c0 * self.dim * 4, q, thr, lab.data_ptr() + c0 * 4, sc.data_ptr() + c0 * 4)
        torch.cuda.synchronize()
        return lab.cpu().numpy()[:total], sc.cpu().numpy()[:total]


@pytest.fixture(scope="module")
def gals():
    made = {}

    def get(dim, labelled=False):
        if (dim, labelled) not in made:
            made[dim, labelled] = Gal(dim, labelled)
        return made[dim, labelled]
    return get


def entry_embeddings(case, gal):
    """One unit row per ENTRY [n * per_frame] of the case (so that a face has the same embedding however the batch is cut): a gallery
    row plus noise for three in five, random for the rest."""
    rng = np.random.default_rng(sum(case.name.encode()) + gal.dim)
    m = case.n * case.per_frame
    x = gm.unit_rows(rng, m, gal.dim)
    near = rng.random(m) < 0.6
    x[near] = gal.rows[rng.integers(0, len(gal.rows), int(near.sum()))] + np.float32(0.6) * x[near]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def make(case, dim, pool=im.POOL_SUM, iou_thr=0.3, refresh=None):
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=iou_thr, max_missed=case.max_missed,
              refresh=case.refresh if refresh is None else refresh)
    trk = fa.Tracker(**kw)
    trk.enable_identity(dim, pool)
    return trk, im.IdentTracker(dim, pool, **kw)


def gpu_call(trk, case, gal, entry_emb, want_embed, first=0, last=None, total=None, sync=True, with_stream_of=True, thr=THRESHOLD):
    """fh_track_update_slots_dev + fh_track_identify_dev on frames [first, last).  The embeddings are those of the flagged entries of
    want_embed (the model's flags: the device's are compared with them by the caller), cut to `total`."""
    last = case.n if last is None else last
    n, per = last - first, case.per_frame
    flat = np.flatnonzero(np.asarray(want_embed).reshape(-1) != 0)
    total = len(flat) if total is None else total
    rows = np.ascontiguousarray(entry_emb[first * per + flat][:total])
    d = dev_records(case.det[first:last])
    cnt = dev(case.counts[first:last])
    i32 = lambda v: torch.full((n, per), v, dtype=torch.int32, device="cuda")          # noqa: E731
    track, embed, slot, label = i32(77), i32(77), i32(77), i32(77)
    score = torch.full((n, per), 7.0, device="cuda")
    d_emb = dev(rows) if total > 0 else None
    so = case.stream_of[first:last] if with_stream_of else None
    assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, track.data_ptr(), embed.data_ptr(), stream_of=so,
                          slot_ptr=slot.data_ptr()) == n
    assert trk.identify_dev(gal.g, thr, track.data_ptr(), slot.data_ptr(), embed.data_ptr(), d_emb.data_ptr() if total > 0 else None,
                            total, n, per, label.data_ptr(), score.data_ptr(), stream_of=so) == n
    if sync:
        torch.cuda.synchronize()
    return dict(d=d, cnt=cnt, track=track, embed=embed, slot=slot, label=label, score=score, d_emb=d_emb, rows=rows, total=total, so=so,
                n=n, per=per)


def run_and_check(trk, model, case, gal, entry_emb, first=0, last=None, total=None, with_stream_of=True, thr=THRESHOLD):
    """One call on the device and in the model, compared: slots (check 1), queries (3), labels and scores given the device's own
    queries (4).  Returns the device's outputs plus what the model says."""
    last = case.n if last is None else last
    so = case.stream_of[first:last]
    wt, we, ws = model.update(case.det[first:last], case.counts[first:last], case.per_frame, so)
    out = gpu_call(trk, case, gal, entry_emb, we, first, last, total, with_stream_of=with_stream_of, thr=thr)
    for key, want in (("track", wt), ("embed", we), ("slot", ws)):
        got = out[key].cpu().numpy()
        assert np.array_equal(got, want), (key, np.argwhere(got != want)[:5])
    tot, dim = out["total"], gal.dim
    q_dev = from_device(trk.queries_ptr(), (tot, dim))
    labs, scs = gal.label(trk.queries_ptr(), tot, thr)
    q64, verbatim = model.pool_queries(wt, ws, we, out["rows"], tot, so)
    assert q_dev[verbatim].tobytes() == out["rows"][verbatim].tobytes()
    ok = gm.within_unit_tolerance(q_dev[~verbatim], q64[~verbatim], dim)
    assert ok.all(), np.argwhere(~ok)[:5]
    want_l, want_s = model.carry(wt, ws, we, labs, scs, tot, so)
    got_l, got_s = out["label"].cpu().numpy(), out["score"].cpu().numpy()
    assert np.array_equal(got_l, want_l), np.argwhere(got_l != want_l)[:5]
    assert got_s.tobytes() == want_s.tobytes(), np.argwhere(got_s != want_s)[:5]
    out.update(want_embed=we, labs=labs, verbatim=verbatim, got_l=got_l, got_s=got_s)
    return out


def check_identity(trk, model, streams):
    """fh_tracker_get_identity against the model: ids, n_emb, labels, scores and the sums, bit for bit (check 2)."""
    for s in streams:
        recs, sums = trk.identity(s, sums=True)
        want, want_sums = model.identity(s)
        assert [(int(r["id"]), int(r["n_emb"]), int(r["label"])) for r in recs] == [w[:3] for w in want], s
        assert recs["score"].tobytes() == np.array([w[3] for w in want], np.float32).tobytes(), s
        assert sums.tobytes() == want_sums.tobytes(), (s, np.argwhere(sums != want_sums)[:5])


def identity_bytes(trk, streams):
    return b"".join(a.tobytes() for s in streams for a in trk.identity(s, sums=True)) + \
        b"".join(trk.state(s, counters=True)[0].tobytes() for s in streams)


# ---------------------------------------------------------------------------------------------- 1. slots
@pytest.mark.parametrize("name", list(tc.CASES))
def test_slots_equal_the_model_and_nothing_else_changes(cases, name):
    case = cases[name]
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    plain, slotted, model = fa.Tracker(**kw), fa.Tracker(**kw), im.IdentTracker(64, **kw)
    _, _, want_slot = model.update(case.det, case.counts, case.per_frame, case.stream_of)
    n, per = case.n, case.per_frame
    d, cnt = dev_records(case.det), dev(case.counts)
    outs = []
    for trk, with_slot in ((plain, False), (slotted, True)):
        t3 = [torch.full((n, per), 77, dtype=torch.int32, device="cuda") for _ in range(3)]
        assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, t3[0].data_ptr(), t3[1].data_ptr(), stream_of=case.stream_of,
                              slot_ptr=t3[2].data_ptr() if with_slot else None) == n
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in t3])
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    assert (outs[0][2] == 77).all()                                               # without the pointer nothing is written
    assert np.array_equal(outs[1][2], want_slot), np.argwhere(outs[1][2] != want_slot)[:5]
    assert (want_slot >= 0).any() and (want_slot == -1).any() and want_slot.max() < case.max_tracks
    for s in range(case.streams):
        a, b = plain.state(s, counters=True), slotted.state(s, counters=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:], s


# ---------------------------------------------------------------------------------------------- 2-4. sums, queries, labels
@pytest.mark.parametrize("name,dim,pool,labelled", [
    ("one_stream", 64, im.POOL_SUM, False), ("one_stream", 192, im.POOL_SUM, True), ("one_stream", 512, im.POOL_SUM, False),
    ("one_stream", 512, im.POOL_LAST, True),
    ("three_streams_exhausted", 64, im.POOL_SUM, True), ("three_streams_exhausted", 192, im.POOL_SUM, False),
    ("three_streams_exhausted", 512, im.POOL_SUM, True), ("three_streams_exhausted", 512, im.POOL_LAST, False)])
def test_identify_equals_the_model(cases, gals, name, dim, pool, labelled):
    case, gal = cases[name], gals(dim, labelled)
    trk, model = make(case, dim, pool)
    out = run_and_check(trk, model, case, gal, entry_embeddings(case, gal), with_stream_of=case.streams > 1)
    check_identity(trk, model, range(case.streams))
    if pool == im.POOL_LAST:
        assert out["verbatim"].all()
    assert (out["got_l"] >= 0).any() and (out["got_l"] == -1).any()
    if labelled:
        assert set(out["labs"][out["labs"] >= 0]) <= set(gal.ids.tolist())      # identity ids, not row indices


def test_every_case_and_the_hazards_it_plants(cases, gals):
    """Dim 512 on all four record streams (max_tracks 1 and 64, per_frame 70, 64 streams); together they must show every hazard."""
    gal, events, labels = gals(512, True), set(), []
    for name in tc.CASES:
        case = cases[name]
        trk, model = make(case, 512)
        out = run_and_check(trk, model, case, gal, entry_embeddings(case, gal))
        check_identity(trk, model, range(case.streams))
        events |= model.events
        labels.append(out["got_l"].reshape(-1))
    labels = np.concatenate(labels)
    assert {"reopened", "pooled", "carried", "untracked"} <= events, events
    assert (labels == -1).any() and (labels >= 0).any()
    assert cases["64_streams_one_slot"].max_tracks == 1 and cases["more_faces_than_lanes"].max_tracks == 64
    assert cases["more_faces_than_lanes"].per_frame == 70


# ---------------------------------------------------------------------------------------------- 5. end to end against the pure model
PLANT_FRAMES, PLANT_PER = 12, 4
PLANT_BOXES = [(20, 20, 40, 40), (120, 20, 40, 40), (220, 20, 40, 40), (320, 20, 40, 40)]


def planted(pool):
    """Four still faces, refresh every 2 frames: faces 0 and 1 are people of the gallery, face 2 is nobody (random embeddings), face 3
    appears from frame 4 on.  POOL_LAST: face 1 becomes another person at its second refresh (label_changed) — under POOL_SUM a template
    that has switched scores against BOTH rows, which the margins below forbid, so there face 1 stays who it is.  The premise is
    asserted here, on the CPU in float64, before anything runs on the device."""
    dim, noise = 512, 0.35
    rng = np.random.default_rng(2024)
    q, _ = np.linalg.qr(rng.standard_normal((dim, G_ROWS)))
    rows = np.ascontiguousarray(q.T, np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    person = {0: 17, 1: 101, 3: 250}
    det = np.zeros((PLANT_FRAMES, PLANT_PER), fa.FACE_DTYPE)
    counts = np.zeros(PLANT_FRAMES, np.int32)
    for f in range(PLANT_FRAMES):
        boxes = PLANT_BOXES[:3] + (PLANT_BOXES[3:] if f >= 4 else [])
        counts[f] = len(boxes)
        for j, b in enumerate(boxes):
            det[f, j]["x"], det[f, j]["y"], det[f, j]["w"], det[f, j]["h"] = b
    kw = dict(streams=1, max_tracks=8, iou_thr=0.3, max_missed=0, refresh=2)
    model = im.IdentTracker(dim, pool, **kw)
    wt, we, ws = model.update(det, counts, PLANT_PER)
    flat = np.flatnonzero(we.reshape(-1) != 0)
    emb, intended = np.zeros((len(flat), dim), np.float32), np.full(len(flat), -1)
    for e, i in enumerate(flat):
        f, j = divmod(int(i), PLANT_PER)
        g = gm.unit_rows(rng, 1, dim)[0]
        if j in person:
            who = 200 if (pool == im.POOL_LAST and j == 1 and f >= 4) else person[j]
            g = rows[who] + np.float32(noise) * g
            intended[e] = who
        emb[e] = g / np.linalg.norm(g)
    want_l, want_s, q64, verbatim = model.identify(wt, ws, we, emb, im.gallery_labels(rows, THRESHOLD))
    sc = (q64 @ rows.astype(np.float64).T + 1.0) / 2.0
    known = intended >= 0
    assert known.sum() >= 10 and (~known).sum() >= 3
    assert (sc[known, intended[known]] > THRESHOLD + 0.02).all()              # every intended match is well above the threshold
    others = sc.copy()
    others[known, intended[known]] = 0.0
    assert (others < THRESHOLD - 0.02).all(), others.max()                    # every other (query, row) pair well below it
    top2 = np.sort(sc[known], axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] > 0.02).all()                             # and the winner is clear
    assert {"carried", "pooled"} <= model.events and ("label_changed" in model.events) == (pool == im.POOL_LAST)
    assert (pool == im.POOL_LAST) == bool(verbatim.all())
    return dict(dim=dim, kw=kw, rows=rows, det=det, counts=counts, we=we, ws=ws, emb=emb, flat=flat, want_l=want_l, want_s=want_s)


@pytest.mark.parametrize("pool", [im.POOL_LAST, im.POOL_SUM])
def test_planted_video_gives_the_float64_models_labels(pool):
    p = planted(pool)
    dim, rows, det, counts, we, ws, emb, flat, want_l, want_s = (p[k] for k in ("dim", "rows", "det", "counts", "we", "ws", "emb", "flat",
                                                                                  "want_l", "want_s"))
    trk = fa.Tracker(**p["kw"])
    trk.enable_identity(dim, pool)
    # the device
    gal = Gal(dim, False, rows=rows)
    n = PLANT_FRAMES
    t4 = [torch.full((n, PLANT_PER), 77, dtype=torch.int32, device="cuda") for _ in range(4)]
    score = torch.full((n, PLANT_PER), 7.0, device="cuda")
    d, cnt, d_emb = dev_records(det), dev(counts), dev(emb)
    assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, PLANT_PER, t4[0].data_ptr(), t4[1].data_ptr(), slot_ptr=t4[2].data_ptr()) == n
    assert trk.identify_dev(gal.g, THRESHOLD, t4[0].data_ptr(), t4[2].data_ptr(), t4[1].data_ptr(), d_emb.data_ptr(), len(flat), n, PLANT_PER,
                            t4[3].data_ptr(), score.data_ptr()) == n
    torch.cuda.synchronize()
    assert np.array_equal(t4[1].cpu().numpy(), we) and np.array_equal(t4[2].cpu().numpy(), ws)
    got = t4[3].cpu().numpy()
    assert np.array_equal(got, want_l), np.argwhere(got != want_l)[:5]
    assert np.abs(score.cpu().numpy().astype(np.float64) - want_s).max() < 1e-5
    assert (got[:, 2] == -1).all() and (got[:, 0] == 17).all() and (got[4:, 3] == 250).all() and (got[:4, 3] == -1).all()
    assert (got[-1, 1] == 200) == (pool == im.POOL_LAST)


# ---------------------------------------------------------------------------------------------- 6. chunking and edges
@pytest.mark.parametrize("total", [None, 257, 100])
def test_more_than_256_queries_and_a_total_that_cuts_the_flags(cases, gals, total):
    case, gal = cases["more_faces_than_lanes"], gals(512, False)
    trk, model = make(case, 512, refresh=1)                                       # every matched face is embedded again
    flags = int(im.IdentTracker(512, **dict(streams=1, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=1))
                .update(case.det, case.counts, case.per_frame)[1].sum())
    assert flags > 2 * 256 + 1                                                    # the premise: three chunks, the last one short
    out = run_and_check(trk, model, case, gal, entry_embeddings(case, gal), total=total)
    assert out["total"] == (flags if total is None else total)
    check_identity(trk, model, [0])
    if total is not None:                                                         # the surplus entries answer (-1, -1.0f)
        rank = im.IdentTracker.ranks(out["want_embed"])
        surplus = (out["want_embed"] != 0) & (rank >= total)
        assert surplus.sum() == flags - total
        assert (out["got_l"][surplus] == -1).all() and (out["got_s"][surplus] == -1.0).all()
        assert any(r[1] == 0 for r in model.identity(0)[0])                       # a live track that was never identified


def test_total_zero_with_null_embeddings_and_an_empty_gallery(cases, gals):
    case = cases["three_streams_exhausted"]
    trk, model = make(case, 512)
    gal = gals(512, False)
    emb = entry_embeddings(case, gal)
    a, b = case.slices([30, 30])
    out = run_and_check(trk, model, case, gal, emb, *a, total=0)                   # d_emb = NULL
    assert out["d_emb"] is None and (out["got_l"] == -1).all() and (out["got_s"] == -1.0).all()
    check_identity(trk, model, range(3))
    assert all(r[1] == 0 for s in range(3) for r in model.identity(s)[0])
    out = run_and_check(trk, model, case, gal, emb, *b)                            # ... and the stream goes on
    check_identity(trk, model, range(3))
    assert (out["got_l"] >= 0).any()

    empty = Gal(512, False, empty=True)
    trk, model = make(case, 512)
    out = run_and_check(trk, model, case, empty, emb)
    assert out["total"] > 0 and (out["got_l"] == -1).all() and (out["got_s"] == -1.0).all()
    check_identity(trk, model, range(3))
    assert any(r[1] >= 2 for s in range(3) for r in model.identity(s)[0])          # the sums were pooled all the same


# ---------------------------------------------------------------------------------------------- 7. continuation, reset
def test_split_calls_continue_the_stream(cases, gals):
    case, gal = cases["one_stream"], gals(512, True)
    emb = entry_embeddings(case, gal)
    trk, model = make(case, 512)
    whole = run_and_check(trk, model, case, gal, emb)
    check_identity(trk, model, [0])
    want = identity_bytes(trk, [0])
    pieces_trk, pieces_model = make(case, 512)
    sizes = [1, 7, 32, case.n - 40]
    assert sizes[-1] == 0                                                          # (the case has 40 frames: three pieces are all of it)
    for a, b in case.slices(sizes[:3]):
        out = run_and_check(pieces_trk, pieces_model, case, gal, emb, a, b)
        for key in ("track", "embed", "slot", "label", "score"):
            assert out[key].cpu().numpy().tobytes() == whole[key][a:b].cpu().numpy().tobytes(), (key, a, b)
    assert identity_bytes(pieces_trk, [0]) == want


def test_back_to_back_calls_with_different_stream_tables(cases, gals):
    """Six update + identify pairs on one tracker, each with its own stream_of and no synchronise between them (more calls than the
    staging ring has slots), against the same six calls made one at a time."""
    case, gal = cases["three_streams_exhausted"], gals(512, False)
    emb = entry_embeddings(case, gal)
    pieces = case.slices([10] * 6)
    assert len({case.stream_of[a:b].tobytes() for a, b in pieces}) == 6
    slow, model = make(case, 512)
    ref = [run_and_check(slow, model, case, gal, emb, a, b) for a, b in pieces]
    check_identity(slow, model, range(3))
    fast, _ = make(case, 512)
    outs = [gpu_call(fast, case, gal, emb, r["want_embed"], a, b, sync=False) for r, (a, b) in zip(ref, pieces)]
    torch.cuda.synchronize()
    for out, r in zip(outs, ref):
        for key in ("track", "embed", "slot", "label", "score"):
            assert out[key].cpu().numpy().tobytes() == r[key].cpu().numpy().tobytes(), key
    assert identity_bytes(fast, range(3)) == identity_bytes(slow, range(3))


def test_reset_and_enable_again_clear_the_identity(cases, gals):
    case, gal = cases["three_streams_exhausted"], gals(512, False)
    trk, model = make(case, 512)
    run_and_check(trk, model, case, gal, entry_embeddings(case, gal))
    assert all(len(model.identity(s)[0]) > 0 for s in range(3))
    trk.reset(0)
    model.reset(0)
    assert len(trk.identity(0)) == 0
    check_identity(trk, model, range(3))                                          # streams 1 and 2 are what they were
    # stream 0 starts again with track id 0 in slot 0: the old owner 0 of that slot must be gone, so its first row is kept verbatim
    a, b = 0, 10
    out = run_and_check(trk, model, case, gal, entry_embeddings(case, gal), a, b)
    check_identity(trk, model, range(3))
    trk.enable_identity(512, im.POOL_SUM)                                         # again: clears all
    for s in range(3):
        recs, sums = trk.identity(s, sums=True)
        assert len(recs) == len(trk.state(s)) and (recs["n_emb"] == 0).all() and (recs["label"] == -1).all() and not sums.any()
        assert (recs["score"] == -1.0).all()


# ---------------------------------------------------------------------------------------------- 8. arguments
def test_argument_errors_change_nothing(cases, gals):
    case, gal = cases["three_streams_exhausted"], gals(512, False)
    trk, model = make(case, 512)
    out = run_and_check(trk, model, case, gal, entry_embeddings(case, gal))
    before = identity_bytes(trk, range(3))
    n, per, L = case.n, case.per_frame, fa.lib()
    label = torch.full((n, per), 77, dtype=torch.int32, device="cuda")
    score = torch.full((n, per), 7.0, device="cuda")
    bad = case.stream_of.copy(); bad[n // 2] = 3
    other_dim, plain = fa.Gallery(64), fa.Tracker(streams=3, max_tracks=4)
    P = dict(t=trk.handle, g=gal.g._h, track=out["track"].data_ptr(), slot=out["slot"].data_ptr(), embed=out["embed"].data_ptr(),
             emb=out["d_emb"].data_ptr(), total=out["total"], n=n, per=per, so=case.stream_of.ctypes.data, label=label.data_ptr(),
             score=score.data_ptr())

    def ident(**kw):
        a = dict(P, **kw)
        return L.fh_track_identify_dev(a["t"], a["g"], THRESHOLD, a["track"], a["slot"], a["embed"], a["emb"], a["total"], a["n"], a["per"],
                                       a["so"], a["label"], a["score"], 0)
    for what, kw in [("null tracker", dict(t=None)), ("null gallery", dict(g=None)), ("null track", dict(track=None)),
                     ("null slot", dict(slot=None)), ("null embed", dict(embed=None)), ("null label", dict(label=None)),
                     ("null score", dict(score=None)), ("null emb with total > 0", dict(emb=None)),
                     ("identity not enabled", dict(t=plain.handle)), ("gallery of another dim", dict(g=other_dim._h)),
                     ("total < 0", dict(total=-1)), ("total > n * per_frame", dict(total=n * per + 1)), ("n = 0", dict(n=0)),
                     ("per_frame = 0", dict(per=0)), ("stream out of range", dict(so=bad.ctypes.data))]:
        assert ident(**kw) == FH_ERR_ARG, what
        assert "fh_track_identify_dev" in _lib.last_error(), what
    for dim, pool in ((0, 1), (32, 1), (100, 1), (4160, 1), (512, 2), (512, -1)):
        assert L.fh_tracker_enable_identity(trk.handle, dim, pool) == FH_ERR_ARG and "fh_tracker_enable_identity" in _lib.last_error()
    assert L.fh_tracker_enable_identity(None, 512, 1) == FH_ERR_ARG
    assert L.fh_tracker_get_identity(plain.handle, 0, None, None) == FH_ERR_ARG and "fh_tracker_get_identity" in _lib.last_error()
    assert L.fh_tracker_get_identity(trk.handle, 3, None, None) == FH_ERR_ARG
    assert L.fh_track_update_slots_dev(None, out["d"].data_ptr(), out["cnt"].data_ptr(), n, per, None, out["track"].data_ptr(),
                                       out["embed"].data_ptr(), out["slot"].data_ptr(), 0) == FH_ERR_ARG
    assert "fh_track_update_slots_dev" in _lib.last_error()
    torch.cuda.synchronize()
    assert identity_bytes(trk, range(3)) == before                                # the state is what the one good call left
    assert torch.all(label == 77) and torch.all(score == 7.0)                     # nothing was launched
    with pytest.raises(fa.FaceHipError):
        trk.identify_dev(other_dim, THRESHOLD, P["track"], P["slot"], P["embed"], P["emb"], P["total"], n, per, P["label"], P["score"],
                         stream_of=case.stream_of)


# ---------------------------------------------------------------------------------------------- 9. the pipeline
@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    assert det.input_size() == (IN, IN)
    return det, rec


def pipeline_bufs(n, F, dim=512):
    return dict(all=torch.full((n * F, 15), 5.0, device="cuda"), cnt=torch.full((n,), -5, dtype=torch.int32, device="cuda"),
                track=torch.full((n, F), 77, dtype=torch.int32, device="cuda"), faces=torch.full((n * F, 15), 7.0, device="cuda"),
                fo=torch.full((n * F,), -7, dtype=torch.int32, device="cuda"), to=torch.full((n * F,), -7, dtype=torch.int32, device="cuda"),
                emb=torch.full((n * F, dim), 7.0, device="cuda"), label=torch.full((n, F), 77, dtype=torch.int32, device="cuda"),
                score=torch.full((n, F), 7.0, device="cuda"))


TRACKED = ("all", "cnt", "track", "faces", "fo", "to", "emb")


@pytest.mark.parametrize("refresh", [0, 2])
def test_pipeline_names_every_face(models_, refresh):
    det, rec = models_
    F = 4
    two = util.frames_u8(2, IN, IN, seed=VIDEO_SEED, smooth=True)
    frames = np.ascontiguousarray(two[[0, 0, 0, 1, 1, 0]])                        # A A A B B A
    n, fd = len(frames), dev(frames)
    kw = dict(streams=1, max_tracks=8, iou_thr=0.3, max_missed=0, refresh=refresh)
    # the parent path: the tracked pipeline on a fresh tracker — also the source of frame A's embeddings, which are enrolled
    plain, b0 = fa.Tracker(**kw), pipeline_bufs(n, F)
    args = lambda b: (fd.data_ptr(), n, IN, IN, F, b["all"].data_ptr(), b["cnt"].data_ptr(), b["track"].data_ptr(),  # noqa: E731
                      b["faces"].data_ptr(), b["fo"].data_ptr(), b["to"].data_ptr(), b["emb"].data_ptr())
    total0 = fa.pipeline_run_tracked_dev(det, rec, plain, *args(b0), scoreThreshold=THR[0], nmsThreshold=THR[1])
    torch.cuda.synchronize()
    counts = b0["cnt"].cpu().numpy()
    c0 = int(min(counts[0], F))
    assert c0 >= 2 and counts[3] >= 2, counts                                     # premise: A and B each yield at least 2 faces
    fo = b0["fo"].cpu().numpy()[:total0]
    assert (fo[:c0] == 0).all() and (fo[c0:] > 0).all()                           # frame 0 opens c0 tracks: its faces lead the list
    gal = Gal(512, False, rows=b0["emb"][:c0].cpu().numpy())
    # the identified pipeline on a fresh tracker
    trk, model, b = fa.Tracker(**kw), im.IdentTracker(512, im.POOL_SUM, **kw), pipeline_bufs(n, F)
    trk.enable_identity(512, im.POOL_SUM)
    total = fa.pipeline_run_identified_dev(det, rec, trk, gal.g, THRESHOLD, *args(b), b["label"].data_ptr(), b["score"].data_ptr(),
                                           scoreThreshold=THR[0], nmsThreshold=THR[1])
    torch.cuda.synchronize()
    assert total == total0
    for key in TRACKED:
        assert b[key].cpu().numpy().tobytes() == b0[key].cpu().numpy().tobytes(), key
    assert trk.state(0, counters=True)[0].tobytes() == plain.state(0, counters=True)[0].tobytes()
    # labels and scores: check 4's construction on the pipeline's own outputs
    recs = records(b["all"], n * F).reshape(n, F)
    wt, we, ws = model.update(recs, counts, F)
    assert np.array_equal(b["track"].cpu().numpy(), wt) and int(we.sum()) == total
    emb = b["emb"][:total].cpu().numpy()
    q_dev = from_device(trk.queries_ptr(), (total, 512))
    labs, scs = gal.label(trk.queries_ptr(), total)
    q64, verbatim = model.pool_queries(wt, ws, we, emb, total)
    assert q_dev[verbatim].tobytes() == emb[verbatim].tobytes()
    assert gm.within_unit_tolerance(q_dev[~verbatim], q64[~verbatim], 512).all()
    want_l, want_s = model.carry(wt, ws, we, labs, scs, total)
    got_l, got_s = b["label"].cpu().numpy(), b["score"].cpu().numpy()
    assert np.array_equal(got_l, want_l) and got_s.tobytes() == want_s.tobytes()
    check_identity(trk, model, [0])
    assert (got_l[0, :c0] >= 0).all() and (got_s[0, :c0] > 0.99).all()            # frame A's faces find themselves in the gallery
    if refresh == 0:
        assert we[1].sum() == 0 and we[2].sum() == 0                              # the second and third A were never embedded ...
        for f in (1, 2):                                                          # ... and carry their track's label from the first
            for j in range(c0):
                src = int(np.flatnonzero(wt[0] == wt[f, j])[0])
                assert got_l[f, j] == got_l[0, src] and got_s[f, j] == got_s[0, src]
        assert "carried" in model.events
    else:
        assert we[2].sum() > 0 and not verbatim.all()                             # the refresh embeds again and pools


def test_pipeline_argument_errors(models_, gals):
    det, rec = models_
    n, F = 4, 4
    frames = dev(util.frames_u8(n, IN, IN, seed=41, smooth=True))
    b = pipeline_bufs(n, F)
    gal = gals(512, False)
    good, plain, dim64 = fa.Tracker(streams=1, max_tracks=4), fa.Tracker(streams=1, max_tracks=4), fa.Tracker(streams=1, max_tracks=4)
    good.enable_identity(512)
    dim64.enable_identity(64)
    gal64 = fa.Gallery(64)
    bad4 = np.array([0, 0, 1, 0], np.int32)

    def run(t, g, n_=n, so=None, label=b["label"].data_ptr()):
        return fa.lib().fh_pipeline_run_identified_dev(det.handle, rec.handle, t, g, THRESHOLD, frames.data_ptr(), n_, IN, IN, IN * 3,
                                                       IN * IN * 3, so, THR[0], THR[1], F, b["all"].data_ptr(), b["cnt"].data_ptr(),
                                                       b["track"].data_ptr(), b["faces"].data_ptr(), b["fo"].data_ptr(), b["to"].data_ptr(),
                                                       b["emb"].data_ptr(), label, b["score"].data_ptr(), 0)
    for what, call in [("null tracker", lambda: run(None, gal.g._h)), ("null gallery", lambda: run(good.handle, None)),
                       ("null label", lambda: run(good.handle, gal.g._h, label=None)),
                       ("identity not enabled", lambda: run(plain.handle, gal.g._h)),
                       ("identity dim is not the recogniser's", lambda: run(dim64.handle, gal64._h)),
                       ("gallery of another dim", lambda: run(good.handle, gal64._h)),
                       ("n = 0", lambda: run(good.handle, gal.g._h, n_=0)),
                       ("stream out of range", lambda: run(good.handle, gal.g._h, so=bad4.ctypes.data))]:
        assert call() == FH_ERR_ARG, what
        assert "fh_pipeline_run_identified_dev" in _lib.last_error(), what
    torch.cuda.synchronize()
    assert torch.all(b["cnt"] == -5) and torch.all(b["track"] == 77) and torch.all(b["label"] == 77) and torch.all(b["emb"] == 7.0)
    assert good.state(0, counters=True)[1:] == (0, 0)
