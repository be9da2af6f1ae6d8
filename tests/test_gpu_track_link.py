"""Track re-linking on the GPU (include/facehip.h, "track re-linking"; track_link_kernel) held to its CPU model
(tests/track_link_model.py) BIT FOR BIT: the table (fh_tracker_get_links), the sums, d_root, labels and scores; pooled queries to
gallery_fuse_model's unit tolerance.  The tracker is driven with the hand-made records of tests/track_link_cases.py and the identify
step with designed embeddings (exact ones, whose decisions cannot depend on the reduction order, and seeded random ones, whose score
bits do), then once through fh_pipeline_run_identified_dev with the tiny detector and recogniser."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import gallery_fuse_model as gm    # noqa: E402
from tests import track_cases as tc           # noqa: E402
from tests import track_link_cases as lc      # noqa: E402
from tests import track_link_model as lm      # noqa: E402
from tests import util                        # noqa: E402

FH_ERR_ARG, FH_ERR_STATE = -1, -4
THRESHOLD = 0.6
IN = 128
VIDEO_SEED, THR = 42, (0.3, 0.4)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def dev_records(det):
    return dev(np.ascontiguousarray(det).view(np.uint8).reshape(-1, 60))


def from_device(ptr, shape, dtype=np.float32):
    out = np.empty(shape, dtype)
    if out.size:
        assert ptr and fa.lib().fh_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0, _lib.last_error()
    return out


class Gal:
    """A small gallery: the exact rows of persons 1 .. 4, then seeded unit rows."""

    def __init__(self, dim):
        self.dim = dim
        self.rows = np.concatenate([lc.exact_rows([1, 2, 3, 4], dim), gm.unit_rows(np.random.default_rng(dim), 20, dim)])
        self.g = fa.Gallery(dim)
        self.g.enroll(self.rows, None)

    def label(self, q_ptr, total):
        lab = torch.full((max(total, 1),), 55, dtype=torch.int32, device="cuda")
        sc = torch.full((max(total, 1),), 5.5, device="cuda")
        if total:
            self.g.label_dev(q_ptr, total, THRESHOLD, lab.data_ptr(), sc.data_ptr())
        torch.cuda.synchronize()
        return lab.cpu().numpy()[:total], sc.cpu().numpy()[:total]


@pytest.fixture(scope="module")
def gals():
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = Gal(dim)
        return made[dim]
    return get


def make(dim, pool, max_tracks, memory, max_age, thr=0.6, streams=1, relink=True):
    kw = dict(streams=streams, max_tracks=max_tracks, iou_thr=0.3, max_missed=lc.MAX_MISSED, refresh=0)
    trk, model = fa.Tracker(**kw), lm.LinkTracker(dim, pool, **kw)
    if pool == lm.POOL_WEIGHTED:
        trk.clear_bestshot()                                                      # opts the tracker into the quality feature
    trk.enable_identity(dim, pool)
    if relink:
        trk.enable_relink(memory, thr, max_age)
        model.enable_relink(memory, thr, max_age)
    return trk, model


def qualities(clip):
    """Small integer weights (0 included: it weighs 1), exact in any sum."""
    return np.random.default_rng(clip.n).integers(0, 6, (clip.n, clip.per_frame)).astype(np.int32)


def call(trk, model, clip, gal, rows_of, total=None, qual=None):
    """One update + identify_link call on the device and in the model, compared: the update's outputs, the roots, the queries, and —
    given the device's own queries, labelled here through the gallery — every label and score."""
    n, per, so = clip.n, clip.per_frame, clip.stream_of
    wt, we, ws = model.update(clip.det, clip.counts, per, so)
    flat = np.flatnonzero(we.reshape(-1) != 0)
    total = len(flat) if total is None else total
    rows = np.ascontiguousarray(rows_of(clip.person.reshape(-1)[flat])[:total], np.float32)
    qual = qualities(clip) if qual is None else np.ascontiguousarray(qual)
    i32 = lambda v: torch.full((n, per), v, dtype=torch.int32, device="cuda")      # noqa: E731
    track, embed, slot, label, root = i32(77), i32(77), i32(77), i32(77), i32(77)
    score = torch.full((n, per), 7.0, device="cuda")
    d, cnt, d_emb, d_q = dev_records(clip.det), dev(clip.counts), dev(rows) if total else None, dev(qual)
    assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, track.data_ptr(), embed.data_ptr(), stream_of=so, slot_ptr=slot.data_ptr()) == n
    assert trk.identify_dev(gal.g, THRESHOLD, track.data_ptr(), slot.data_ptr(), embed.data_ptr(), d_emb.data_ptr() if total else None, total,
                            n, per, label.data_ptr(), score.data_ptr(), stream_of=so, quality_ptr=d_q.data_ptr(),
                            root_ptr=root.data_ptr()) == n
    torch.cuda.synchronize()
    for got, want, key in ((track, wt, "track"), (embed, we, "embed"), (slot, ws, "slot")):
        assert np.array_equal(got.cpu().numpy(), want), key
    q64, verbatim = model.pool_queries(wt, ws, we, rows, total, so, qual)
    got_root = root.cpu().numpy()
    assert np.array_equal(got_root, model.roots), np.argwhere(got_root != model.roots)[:5]
    q_dev = from_device(trk.queries_ptr(), (total, gal.dim))
    assert q_dev[verbatim].tobytes() == rows[verbatim].tobytes()
    ok = gm.within_unit_tolerance(q_dev[~verbatim], q64[~verbatim], gal.dim)
    assert ok.all(), np.argwhere(~ok)[:5]
    labs, scs = gal.label(trk.queries_ptr(), total)
    want_l, want_s = model.carry(wt, ws, we, labs, scs, total, so)
    got_l, got_s = label.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(got_l, want_l), np.argwhere(got_l != want_l)[:5]
    assert got_s.tobytes() == want_s.tobytes()
    return dict(track=wt, embed=we, slot=ws, roots=got_root, label=got_l, verbatim=verbatim, total=total)


def check_table(trk, model, streams=(0,)):
    """fh_tracker_get_links against the model: every field of every row and the sums, bit for bit."""
    for s in streams:
        recs, sums = trk.links(s, sums=True)
        want, want_sums = model.links(s)
        assert len(recs) == len(want)
        got = [tuple(r[k] for k in ("owner", "root", "n_emb", "label", "score", "last_seen", "links", "pad")) for r in recs]
        for i, (g, w) in enumerate(zip(got, want)):
            assert g[:4] == tuple(w[:4]) and g[5:] == tuple(w[5:]) and np.float32(g[4]).tobytes() == np.float32(w[4]).tobytes(), (s, i, g, w)
        assert sums.tobytes() == want_sums.tobytes(), (s, np.argwhere(sums != want_sums)[:5])


def table_bytes(trk, streams=(0,)):
    return b"".join(a.tobytes() for s in streams for a in trk.links(s, sums=True))


def exact(dim):
    return lambda persons: lc.exact_rows(persons, dim)


def roots_of(clip, roots, who):
    return [int(roots[f, j]) for f in range(clip.n) for j in range(clip.per_frame) if clip.person[f, j] == who]


DIMS, POOLS = (64, 192, 512), (lm.POOL_SUM, lm.POOL_LAST, lm.POOL_WEIGHTED)


# ---------------------------------------------------------------------------------------------- 1. the clips, one call each
@pytest.mark.parametrize("i,name", list(enumerate(lc.CLIPS)))
def test_clips_equal_the_model(gals, i, name):
    """Every scenario of the clips in one call (so every death and return happens inside one call), dims and pools in rotation."""
    clip, kw, events = lc.clip(name)
    dim, pool = DIMS[i % 3], POOLS[(i // 3) % 3]
    trk, model = make(dim, pool, **kw)
    out = call(trk, model, clip, gals(dim), exact(dim))
    check_table(trk, model)
    assert events <= model.events, (name, model.events)
    forgotten = name in ("no_memory", "age_beyond", "evict")                      # A comes back and is NOT recognised
    assert (model.links_made > 0) == (not forgotten)
    if name not in ("competition", "twins"):                                      # (two faces of A at once there)
        assert (len(set(roots_of(clip, out["roots"], lc.A))) == 1) == (not forgotten), name
    if name == "chain":
        assert trk.links(0)[0]["links"] == 2 and trk.links(0)[0]["root"] == 0
    if name == "competition":
        assert list(out["roots"][5][:2]) == [0, 2]                                # the first in j order resumed track 0
    if name == "twins":
        assert out["roots"][5, 0] == 0 and trk.links(0)[1]["owner"] == 1          # the smaller owner won, the other one waits


@pytest.mark.parametrize("name,pool", [("same_slot", lm.POOL_SUM), ("from_memory", lm.POOL_WEIGHTED), ("other_slot", lm.POOL_LAST)])
def test_across_calls_equals_one_call(gals, name, pool):
    """A track dies in one call and returns in a later one: the pieces leave the table of the whole."""
    clip, kw, events = lc.clip(name)
    dim = 512
    whole_trk, whole_model = make(dim, pool, **kw)
    whole = call(whole_trk, whole_model, clip, gals(dim), exact(dim))
    trk, model = make(dim, pool, **kw)
    roots = []
    for a, b in ((0, 4), (4, 8), (8, clip.n)):                                    # the returns are at frame 7 (same call as nothing before them)
        roots.append(call(trk, model, clip.sub(a, b), gals(dim), exact(dim), qual=qualities(clip)[a:b])["roots"])   # the whole call's weights
        check_table(trk, model)
    assert np.array_equal(np.concatenate(roots), whole["roots"])
    # the same table however the clip is cut — but for the (label, score) of a MEMORY row, which by the contract are what the slot held
    # when the retiring call began: in one call that is before the track was ever named
    (recs, sums), (w_recs, w_sums) = trk.links(0, sums=True), whole_trk.links(0, sums=True)
    mem = np.arange(len(recs)) >= kw["max_tracks"]
    for key in ("owner", "root", "n_emb", "last_seen", "links"):
        assert np.array_equal(recs[key], w_recs[key]), key
    assert recs["label"][~mem].tobytes() == w_recs["label"][~mem].tobytes() and recs["score"][~mem].tobytes() == w_recs["score"][~mem].tobytes()
    assert sums.tobytes() == w_sums.tobytes()
    assert events <= model.events and model.links_made == 1


@pytest.mark.parametrize("name,cut,events", lc.CUTS)
def test_a_record_opened_or_resumed_and_retired_inside_one_call(gals, name, cut, events):
    """Two calls; the first one NAMES the slot (the gallery holds the people).  In the second a record is opened or resumed and retired
    again: it takes to the memory no name (opened) or the winner's (resumed), not what the slot was called when the call began."""
    clip, kw, _ = lc.clip(name)
    dim = 192
    trk, model = make(dim, lm.POOL_SUM, **kw)
    for a, b in ((0, cut), (cut, clip.n)):
        call(trk, model, clip.sub(a, b), gals(dim), exact(dim))
        check_table(trk, model)
        if a == 0:
            assert trk.links(0)[0]["label"] >= 0                                  # named by the first call
    assert events <= model.events, model.events
    recs = trk.links(0)
    if name == "evict":
        assert recs[1]["owner"] == 2 and recs[1]["label"] == -1 and recs[1]["score"] == -1.0
    if name == "resume_retire":
        assert recs[1]["owner"] == 1 and recs[1]["label"] == -1                           # B: opened and retired in this call
        assert recs[2]["owner"] == 2 and recs[2]["root"] == 0 and recs[2]["label"] == lc.A - 1 and recs[2]["score"] == 1.0


# ---------------------------------------------------------------------------------------------- 2. the threshold, `total`
def test_a_score_equal_to_the_threshold_does_not_link(gals):
    clip, kw, _ = lc.clip("same_slot")
    dim = 64
    tmpl = np.zeros(dim, np.float32)
    tmpl[[1, 2]] = 3.0, 4.0                                                       # |tmpl| = 5: every term is exact in fp32
    face = lc.exact_rows([1], dim)[0]
    s0 = lm.score(face, tmpl)
    for thr, linked in ((s0, False), (np.nextafter(s0, np.float32(0.0)), True)):
        trk, model = make(dim, lm.POOL_SUM, thr=float(thr), **kw)
        out = call(trk, model, clip, gals(dim), lambda persons: np.stack([tmpl, face]))
        check_table(trk, model)
        assert (roots_of(clip, out["roots"], lc.A)[-1] == 0) == linked and model.links_made == int(linked)
        assert ("score_equals_threshold" in model.events) == (not linked)


def test_total_cuts_the_open_event(gals):
    clip, kw, _ = lc.clip("same_slot")
    trk, model = make(192, lm.POOL_SUM, **kw)
    out = call(trk, model, clip, gals(192), exact(192), total=1)
    check_table(trk, model)
    assert int(out["embed"].sum()) == 2 and roots_of(clip, out["roots"], lc.A) == [0, 0, 0, -1, -1, -1] and model.links_made == 0


# ---------------------------------------------------------------------------------------------- 3. streams, the long walk
def test_three_streams_interleaved(gals):
    clip = lc.three_streams()
    trk, model = make(512, lm.POOL_SUM, max_tracks=3, memory=1, max_age=150, streams=3)
    out = call(trk, model, clip, gals(512), exact(512))
    check_table(trk, model, range(3))
    assert model.links_made == 6
    for s in range(3):
        assert len(set(roots_of(clip, out["roots"], 10 * s + lc.A))) == 1
    trk.reset(1)
    model.reset(1)
    check_table(trk, model, range(3))                                             # stream 1's table is clear, the others are what they were
    assert (trk.links(1)["owner"] == -1).all() and (trk.links(0)["owner"] >= 0).any()


@pytest.mark.parametrize("per_frame,people", [(70, 66), (64, 64)])
def test_full_frames_and_a_memory_that_overflows(gals, per_frame, people):
    """64 slots, a frame of exactly 64 entries and one of 70 (the walk in pieces): everybody hides and comes back somewhere else."""
    crowd = lc.crowd(per_frame, people)
    trk, model = make(192, lm.POOL_SUM, max_tracks=64, memory=8, max_age=150)
    out = call(trk, model, crowd, gals(192), exact(192))
    check_table(trk, model)
    assert crowd.per_frame == per_frame and (out["track"][0] == -1).sum() == per_frame - 64
    assert 8 < model.links_made < 64 and {"other_slot", "evicted", "from_memory"} <= model.events


# ---------------------------------------------------------------------------------------------- 4. random rows: the score's bits
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("pool", POOLS)
def test_random_rows_follow_the_stated_order(gals, dim, pool):
    for clip, kw in ((lc.clip("from_memory")[0], lc.clip("from_memory")[1]), (lc.three_streams(), dict(max_tracks=3, memory=8, max_age=150))):
        streams = 1 if clip.stream_of is None else 3
        trk, model = make(dim, pool, streams=streams, **kw)
        call(trk, model, clip, gals(dim), lambda p: lc.random_rows(p, dim, seed=dim))
        check_table(trk, model, range(streams))
        assert model.links_made >= 1 and "refused" in model.events                # (the premise; also held without a GPU)


# ---------------------------------------------------------------------------------------------- 4b. one pooling step
def run_steady(trk, clip, cuts, gal, rows, qual, weighted):
    """The clip through update + identify_link in calls of `cuts` frames: the queries, labels, scores and roots of all calls, in order."""
    out = dict(queries=[], label=[], score=[], root=[], track=[])
    per, a, at = clip.per_frame, 0, 0
    for frames in cuts:
        part, n = clip.sub(a, a + frames), frames
        i32 = lambda v: torch.full((n, per), v, dtype=torch.int32, device="cuda")      # noqa: E731
        track, embed, slot, label, root = i32(77), i32(77), i32(77), i32(77), i32(77)
        score = torch.full((n, per), 7.0, device="cuda")
        d, cnt, d_q = dev_records(part.det), dev(part.counts), dev(qual[a:a + n])
        assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, track.data_ptr(), embed.data_ptr(), slot_ptr=slot.data_ptr(),
                              quality_ptr=d_q.data_ptr() if weighted else None) == n
        torch.cuda.synchronize()
        total = int(embed.cpu().numpy().sum())
        assert total == 2 * n                                                     # refresh 1: both faces of every frame are pooled
        d_emb = dev(rows[at:at + total])
        assert trk.identify_dev(gal.g, THRESHOLD, track.data_ptr(), slot.data_ptr(), embed.data_ptr(), d_emb.data_ptr(), total, n, per,
                                label.data_ptr(), score.data_ptr(), quality_ptr=d_q.data_ptr(), root_ptr=root.data_ptr()) == n
        torch.cuda.synchronize()
        out["queries"].append(from_device(trk.queries_ptr(), (total, gal.dim)))
        for key, t in (("label", label), ("score", score), ("root", root), ("track", track)):
            out[key].append(t.cpu().numpy())
        a, at = a + n, at + total
    return {k: np.concatenate(v) for k, v in out.items()}


@pytest.mark.parametrize("cuts", [(6,), (2, 4)])
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("dim", (64, 192))
def test_continued_tracks_pool_alike_with_relinking_off_and_on(gals, dim, pool, cuts):
    """Two faces that never leave, pooled in every frame (refresh 1): the first frame opens both tracks, the other five continue them.
    Nothing is ever lost, so re-linking has nothing to link, and the pool kernel (re-linking off) and the link kernel (on) must write
    the same queries, labels, scores and sums, bit for bit: both take the one pooling step of track_dev.h."""
    clip = lc.Clip([[(0, lc.A), (1, lc.B)]] * 6, 3)
    kw = dict(streams=1, max_tracks=4, iou_thr=0.3, max_missed=1, refresh=1)
    rows = lc.random_rows(clip.person.reshape(-1)[clip.person.reshape(-1) >= 0], dim, seed=dim)
    qual = qualities(clip)
    runs = {}
    for on in (False, True):
        trk = fa.Tracker(**kw)
        if pool == lm.POOL_WEIGHTED:
            trk.clear_bestshot()                                                  # opts the tracker into the quality feature
        trk.enable_identity(dim, pool)
        if on:
            trk.enable_relink(4, 0.6, 8)
        runs[on] = (trk, run_steady(trk, clip, cuts, gals(dim), rows, qual, pool == lm.POOL_WEIGHTED))
    (off_trk, off), (on_trk, on) = runs[False], runs[True]
    assert set(off["track"].reshape(-1)) == {-1, 0, 1}                            # (the premise: two tracks, opened once)
    for key in ("track", "queries", "label", "score"):
        assert off[key].tobytes() == on[key].tobytes(), key
    assert np.array_equal(on["root"], on["track"]) and np.array_equal(off["root"], off["track"])    # every root is the entry's own track id
    (recs, sums), (on_recs, on_sums), (link_recs, link_sums) = (off_trk.identity(0, sums=True), on_trk.identity(0, sums=True),
                                                                on_trk.links(0, sums=True))
    assert len(recs) == 2 and recs.tobytes() == on_recs.tobytes() and sums.tobytes() == on_sums.tobytes()
    assert list(recs["id"]) == [0, 1] and list(recs["n_emb"]) == [6, 6]
    assert sums.tobytes() == link_sums[:2].tobytes() and not link_sums[2:4].any() and sums.any()    # the slots' rows; free rows report zero
    assert list(link_recs["owner"][:4]) == [0, 1, -1, -1] and list(link_recs["n_emb"][:2]) == [6, 6]


# ---------------------------------------------------------------------------------------------- 5. off, errors, state
def test_relink_off_is_the_old_call_plus_own_roots(gals):
    case, dim = tc.Case("three_streams_exhausted"), 192
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    old, new, model = fa.Tracker(**kw), fa.Tracker(**kw), lm.LinkTracker(dim, lm.POOL_SUM, **kw)
    wt, we, ws = model.update(case.det, case.counts, case.per_frame, case.stream_of)
    rows = gm.unit_rows(np.random.default_rng(8), int(we.sum()), dim)
    n, per = case.n, case.per_frame
    d, cnt, d_emb = dev_records(case.det), dev(case.counts), dev(rows)
    outs = []
    for trk, link in ((old, False), (new, True)):
        trk.enable_identity(dim)
        t5 = [torch.full((n, per), 77, dtype=torch.int32, device="cuda") for _ in range(5)]
        score = torch.full((n, per), 7.0, device="cuda")
        trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, t5[0].data_ptr(), t5[1].data_ptr(), stream_of=case.stream_of, slot_ptr=t5[2].data_ptr())
        trk.identify_dev(gals(dim).g, THRESHOLD, t5[0].data_ptr(), t5[2].data_ptr(), t5[1].data_ptr(), d_emb.data_ptr(), len(rows), n, per,
                         t5[3].data_ptr(), score.data_ptr(), stream_of=case.stream_of, root_ptr=t5[4].data_ptr() if link else None)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in t5] + [score.cpu().numpy(), from_device(trk.queries_ptr(), (len(rows), dim))])
    for a, b in zip(outs[0][:4] + outs[0][5:], outs[1][:4] + outs[1][5:]):
        assert a.tobytes() == b.tobytes()
    assert (outs[0][4] == 77).all() and np.array_equal(outs[1][4], model.own_roots(wt, ws))
    for s in range(case.streams):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(old.identity(s, sums=True), new.identity(s, sums=True)))
    assert fa.lib().fh_tracker_get_links(new.handle, 0, np.zeros(64, fa.TRACK_LINK_DTYPE).ctypes.data, None) == FH_ERR_STATE


def test_errors_leave_the_state_untouched(gals):
    clip, kw, _ = lc.clip("from_memory")
    dim, L = 64, fa.lib()
    plain = fa.Tracker(streams=1, max_tracks=3, max_missed=lc.MAX_MISSED)
    assert L.fh_tracker_enable_relink(plain.handle, 8, 0.6, 150) == FH_ERR_STATE and "fh_tracker_enable_relink" in _lib.last_error()
    assert L.fh_tracker_enable_relink(None, 8, 0.6, 150) == FH_ERR_ARG
    trk, model = make(dim, lm.POOL_SUM, **kw)
    out = call(trk, model, clip, gals(dim), exact(dim))
    before = table_bytes(trk)
    for memory, thr, age in ((-1, 0.6, 150), (257, 0.6, 150), (8, float("nan"), 150), (8, float("inf"), 150), (8, 0.6, lc.MAX_MISSED)):
        assert L.fh_tracker_enable_relink(trk.handle, memory, thr, age) == FH_ERR_ARG, (memory, thr, age)
    n, per = clip.n, clip.per_frame
    t3 = [dev(out[k]) for k in ("track", "slot", "embed")]
    label = torch.full((n, per), 77, dtype=torch.int32, device="cuda")
    score = torch.full((n, per), 7.0, device="cuda")
    emb = dev(np.zeros((out["total"], dim), np.float32))
    args = (t3[0].data_ptr(), t3[1].data_ptr(), t3[2].data_ptr(), emb.data_ptr(), out["total"], n, per, None, label.data_ptr(), score.data_ptr())
    assert L.fh_track_identify_dev(trk.handle, gals(dim).g._h, THRESHOLD, *args, 0) == FH_ERR_STATE        # the old calls refuse
    assert "fh_track_identify_dev" in _lib.last_error()
    assert L.fh_track_identify_q_dev(trk.handle, gals(dim).g._h, THRESHOLD, *args[:3], t3[0].data_ptr(), *args[3:], 0) == FH_ERR_STATE
    assert L.fh_track_identify_link_dev(trk.handle, gals(dim).g._h, THRESHOLD, *args[:3], None, *args[3:], None, 0) == FH_ERR_ARG   # no d_root
    assert L.fh_tracker_get_links(trk.handle, 1, np.zeros(4, fa.TRACK_LINK_DTYPE).ctypes.data, None) == FH_ERR_ARG
    torch.cuda.synchronize()
    assert table_bytes(trk) == before and torch.all(label == 77) and torch.all(score == 7.0)
    check_table(trk, model)
    trk.reset(0)
    assert (trk.links(0)["owner"] == -1).all() and not trk.links(0, sums=True)[1].any()
    trk.enable_identity(dim)                                                      # a second enable_identity switches re-linking off
    assert L.fh_tracker_get_links(trk.handle, 0, np.zeros(4, fa.TRACK_LINK_DTYPE).ctypes.data, None) == FH_ERR_STATE


# ---------------------------------------------------------------------------------------------- 6. the pipeline
@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    return det, rec


def pipeline_bufs(n, F, dim=512):
    return dict(all=torch.full((n * F, 15), 5.0, device="cuda"), cnt=torch.full((n,), -5, dtype=torch.int32, device="cuda"),
                track=torch.full((n, F), 77, dtype=torch.int32, device="cuda"), faces=torch.full((n * F, 15), 7.0, device="cuda"),
                fo=torch.full((n * F,), -7, dtype=torch.int32, device="cuda"), to=torch.full((n * F,), -7, dtype=torch.int32, device="cuda"),
                emb=torch.full((n * F, dim), 7.0, device="cuda"), label=torch.full((n, F), 77, dtype=torch.int32, device="cuda"),
                score=torch.full((n, F), 7.0, device="cuda"))


BESTSHOT = (5, 4, 1)


@pytest.mark.parametrize("pool,bestshot", [(lm.POOL_SUM, None), (lm.POOL_WEIGHTED, BESTSHOT)])
def test_pipeline_resumes_the_faces_that_come_back(models_, pool, bestshot):
    """The A A A B B A video: with max_missed = 0 the faces of A lose their tracks during B B and come back in the last frame.  Once
    plain, once with the best-shot policy on and the weighted pool, where the pipeline hands its quality buffer to the identify step.
    Both runs — re-linking off and on — are held to the model, given the device's own records, qualities, embeddings and queries."""
    det, rec = models_
    F = 4
    two = util.frames_u8(2, IN, IN, seed=VIDEO_SEED, smooth=True)
    frames = np.ascontiguousarray(two[[0, 0, 0, 1, 1, 0]])
    n, fd = len(frames), dev(frames)
    kw = dict(streams=1, max_tracks=8, iou_thr=0.3, max_missed=0, refresh=0)
    gal = Gal(512)
    runs = {}
    for on in (False, True):
        trk, b = fa.Tracker(**kw), pipeline_bufs(n, F)
        model = lm.LinkTracker(512, pool, bestshot, **kw)
        if bestshot:
            trk.set_bestshot(*bestshot)
        trk.enable_identity(512, pool)
        if on:
            trk.enable_relink(8, 0.6, 150)
            model.enable_relink(8, 0.6, 150)
        total = fa.pipeline_run_identified_dev(det, rec, trk, gal.g, THRESHOLD, fd.data_ptr(), n, IN, IN, F, b["all"].data_ptr(),
                                               b["cnt"].data_ptr(), b["track"].data_ptr(), b["faces"].data_ptr(), b["fo"].data_ptr(),
                                               b["to"].data_ptr(), b["emb"].data_ptr(), b["label"].data_ptr(), b["score"].data_ptr(),
                                               scoreThreshold=THR[0], nmsThreshold=THR[1])
        torch.cuda.synchronize()
        counts = b["cnt"].cpu().numpy()
        recs = b["all"].cpu().numpy().view(np.uint8).reshape(n * F, 60).copy().view(fa.FACE_DTYPE).reshape(n, F)
        qual = from_device(trk.quality_ptr(), (n, F), np.int32) if bestshot else None
        wt, we, ws = model.update(recs, counts, F, quality=qual)
        assert np.array_equal(b["track"].cpu().numpy(), wt) and int(we.sum()) == total
        emb = b["emb"][:total].cpu().numpy()
        q64, verbatim = model.pool_queries(wt, ws, we, emb, total, None, qual)
        q_dev = from_device(trk.queries_ptr(), (total, 512))
        assert q_dev[verbatim].tobytes() == emb[verbatim].tobytes()
        assert gm.within_unit_tolerance(q_dev[~verbatim], q64[~verbatim], 512).all()
        labs, scs = gal.label(trk.queries_ptr(), total)
        want_l, want_s = model.carry(wt, ws, we, labs, scs, total)
        assert np.array_equal(b["label"].cpu().numpy(), want_l) and b["score"].cpu().numpy().tobytes() == want_s.tobytes(), on
        runs[on] = (trk, b, total, model, wt)
    (off_trk, b0, total0, _, _), (trk, b, total, model, wt) = runs[False], runs[True]
    assert total == total0 and off_trk.roots_ptr() == 0                           # off: nothing new is allocated
    for key in ("all", "cnt", "track", "faces", "fo", "to", "emb"):
        assert b[key].cpu().numpy().tobytes() == b0[key].cpu().numpy().tobytes(), key
    roots = from_device(trk.roots_ptr(), (n, F), np.int32)
    assert np.array_equal(roots, model.roots)
    check_table(trk, model)
    assert not verbatim.all()                                                     # a resumed face was pooled into the older template
    assert model.links_made >= 1 and (roots[5][roots[5] >= 0] < wt[5][roots[5] >= 0]).any()    # a face of the last frame continues an older track
