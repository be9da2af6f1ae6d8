"""The re-linking model (tests/track_link_model.py) without a GPU: with re-linking never enabled it IS the identity model on every
record stream of tests/track_cases.py, and on the hand-made clips of tests/track_link_cases.py it gives the answers a reader works out
by hand — resume after an occlusion, chains, competition, ties, the max_age boundary, eviction."""
import numpy as np
import pytest

from tests import gallery_fuse_model as gm
from tests import track_cases as tc
from tests import track_ident_model as im
from tests import track_link_cases as lc
from tests import track_link_model as lm

DIM = 64


def no_gallery(q):
    return np.full(len(q), -1, np.int32), np.full(len(q), -1.0, np.float32)


def run(model, clip, rows_of, total=None):
    """update + identify of one clip (one call); rows_of(persons of the flagged entries) -> embeddings."""
    wt, we, ws = model.update(clip.det, clip.counts, clip.per_frame, clip.stream_of)
    flat = np.flatnonzero(we.reshape(-1) != 0)
    emb = rows_of(clip.person.reshape(-1)[flat])
    out = model.identify(wt, ws, we, emb, no_gallery, total, clip.stream_of)
    return wt, we, ws, out


def make(max_tracks, memory, max_age, pool=lm.POOL_SUM, thr=0.6, streams=1, dim=DIM):
    m = lm.LinkTracker(dim, pool, streams=streams, max_tracks=max_tracks, iou_thr=0.3, max_missed=lc.MAX_MISSED, refresh=0)
    m.enable_relink(memory, thr, max_age)
    return m


# ---------------------------------------------------------------------------------------------- 1. off = the identity model
@pytest.mark.parametrize("name", list(tc.CASES))
@pytest.mark.parametrize("pool", [im.POOL_SUM, im.POOL_LAST])
def test_without_relink_it_is_the_identity_model(name, pool):
    case = tc.Case(name)
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    a, b = im.IdentTracker(DIM, pool, **kw), lm.LinkTracker(DIM, pool, **kw)
    rng = np.random.default_rng(3)
    rows = gm.unit_rows(rng, 40, DIM)
    label_fn = im.gallery_labels(rows, 0.55)
    for first, last in case.slices([case.n // 2, case.n - case.n // 2]):
        so = case.stream_of[first:last]
        ta = a.update(case.det[first:last], case.counts[first:last], case.per_frame, so)
        tb = b.update(case.det[first:last], case.counts[first:last], case.per_frame, so)
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
        emb = gm.unit_rows(rng, int(ta[1].sum()), DIM)
        la, sa, qa, va = a.identify(ta[0], ta[2], ta[1], emb, label_fn, stream_of=so)
        lb, sb, qb, vb, roots = b.identify(tb[0], tb[2], tb[1], emb, label_fn, stream_of=so)
        assert np.array_equal(la, lb) and sa.tobytes() == sb.tobytes() and qa.tobytes() == qb.tobytes() and np.array_equal(va, vb)
        assert np.array_equal(roots, np.where(ta[2] >= 0, ta[0], -1))
    for s in range(case.streams):
        (ra, sa), (rb, sb) = a.identity(s), b.identity(s)
        assert ra == rb and sa.tobytes() == sb.tobytes()


# ---------------------------------------------------------------------------------------------- 2. the score
def test_score_of_exact_rows_and_its_order():
    e = lc.exact_rows([1, 2], DIM)
    assert lm.score(e[0], 3 * e[0]) == np.float32(1.0) and lm.score(e[0], 7 * e[1]) == np.float32(0.5)
    assert lm.score(e[0], np.zeros(DIM, np.float32)) == np.float32(0.5)                     # a zero template: c = d = 0
    assert not lm.score(e[0], np.full(DIM, np.nan, np.float32)) > np.float32(0.0)          # a NaN exceeds nothing
    rng = np.random.default_rng(1)
    for dim in (64, 192, 512):
        x, y = gm.unit_rows(rng, 2, dim)
        got, want = lm.lane_dot(x, y), float(np.dot(x.astype(np.float64), y.astype(np.float64)))
        assert got.dtype == np.float32 and abs(float(got) - want) < 1e-6
    # the order matters for random rows: the plain left-to-right float32 sum differs from the lane order somewhere
    differs = 0
    for _ in range(50):
        x, y = gm.unit_rows(rng, 2, 512)
        serial = np.float32(0.0)
        for p in x * y:
            serial = np.float32(serial + p)
        differs += serial != lm.lane_dot(x, y)
    assert differs > 0


# ---------------------------------------------------------------------------------------------- 3. the clips
def roots_of(clip, roots, who):
    return [int(roots[f, j]) for f in range(clip.n) for j in range(clip.per_frame) if clip.person[f, j] == who]


@pytest.mark.parametrize("name", list(lc.CLIPS))
def test_clips_show_their_events(name):
    clip, kw, events = lc.clip(name)
    model = make(**kw)
    run(model, clip, lambda p: lc.exact_rows(p, DIM))
    assert events <= model.events, (name, model.events)


def test_occlusion_resumes_the_track_with_its_template():
    clip, kw, _ = lc.clip("same_slot")
    model = make(**kw)
    wt, we, ws, (_, _, q, verbatim, roots) = run(model, clip, lambda p: lc.exact_rows(p, DIM))
    assert sorted(set(wt[wt >= 0])) == [0, 1]                                               # the tracker gave the returning face a new id
    assert roots_of(clip, roots, lc.A) == [0] * 6                                           # ... and the chain says it is track 0
    recs, sums = model.links(0)
    assert recs == [(1, 0, 2, -1, np.float32(-1.0), 9, 1, 0)]                               # owner 1, root 0, two embeddings, one link
    assert sums[0, lc.A] == 2.0 and not verbatim[1] and q[1, lc.A] == 1.0
    assert model.opens == 2 and model.links_made == 1


def test_without_relink_the_same_clip_starts_again():
    clip, kw, _ = lc.clip("same_slot")
    model = lm.LinkTracker(DIM, streams=1, max_tracks=1, iou_thr=0.3, max_missed=lc.MAX_MISSED, refresh=0)
    _, _, _, (_, _, _, verbatim, roots) = run(model, clip, lambda p: lc.exact_rows(p, DIM))
    assert roots_of(clip, roots, lc.A) == [0, 0, 0, 1, 1, 1] and verbatim.all()


def test_split_calls_give_the_same_table():
    clip, kw, _ = lc.clip("from_memory")
    whole, pieces = make(**kw), make(**kw)
    run(whole, clip, lambda p: lc.exact_rows(p, DIM))
    roots = []
    for a, b in ((0, 4), (4, 8), (8, clip.n)):
        roots.append(run(pieces, clip.sub(a, b), lambda p: lc.exact_rows(p, DIM))[3][4])
    assert whole.links(0)[0] == pieces.links(0)[0] and whole.links(0)[1].tobytes() == pieces.links(0)[1].tobytes()
    assert np.array_equal(np.concatenate(roots), whole.roots)
    recs = whole.links(0)[0]
    assert recs[1][:3] == (2, 0, 2) and recs[1][6] == 1 and recs[0][:2] == (1, 1) and recs[3] == lm.FREE     # A back in slot 1; the memory row freed


def test_chain_competition_twins():
    clip, kw, _ = lc.clip("chain")
    model = make(**kw)
    roots = run(model, clip, lambda p: lc.exact_rows(p, DIM))[3][4]
    assert roots_of(clip, roots, lc.A) == [0] * 6 and model.links(0)[0][0][:3] == (2, 0, 3) and model.links(0)[0][0][6] == 2

    clip, kw, _ = lc.clip("competition")
    model = make(**kw)
    wt, _, _, out = run(model, clip, lambda p: lc.exact_rows(p, DIM))
    assert list(out[4][5][:2]) == [0, int(wt[5, 1])] and wt[5, 1] == 2                      # the first in j order resumes 0; the second is new

    clip, kw, _ = lc.clip("twins")
    model = make(**kw)
    roots = run(model, clip, lambda p: lc.exact_rows(p, DIM))[3][4]
    assert roots[5, 0] == 0 and model.links(0)[0][1][0] == 1                                # owner 0 won; owner 1's record is still there


def test_age_boundary_eviction_and_no_memory():
    for name, linked in (("age_in_reach", True), ("age_beyond", False), ("evict", False), ("keep", True), ("no_memory", False),
                         ("from_memory", True)):
        clip, kw, _ = lc.clip(name)
        model = make(**kw)
        roots = run(model, clip, lambda p: lc.exact_rows(p, DIM))[3][4]
        got = roots_of(clip, roots, lc.A)
        assert (len(set(got)) == 1) == linked, (name, got)


@pytest.mark.parametrize("name,cut,events", lc.CUTS)
def test_a_record_opened_or_resumed_and_retired_inside_one_call(name, cut, events):
    """The (label, score) a record takes to the memory: a record opened in the call is unnamed, a resumed one keeps the winner's — not
    what an earlier call's stage C left in the slot."""
    clip, kw, _ = lc.clip(name)
    model = make(**kw)
    names = im.gallery_labels(lc.exact_rows([lc.A, lc.B, lc.C, lc.D], DIM), 0.6)        # person p is labelled p - 1, score 1.0
    for a, b in ((0, cut), (cut, clip.n)):
        part = clip.sub(a, b)
        wt, we, ws = model.update(part.det, part.counts, part.per_frame)
        flat = np.flatnonzero(we.reshape(-1) != 0)
        model.identify(wt, ws, we, lc.exact_rows(part.person.reshape(-1)[flat], DIM), names)
        if a == 0:
            assert model.links(0)[0][0][3] >= 0                                          # the first call named the slot
    assert events <= model.events, model.events
    recs = model.links(0)[0]
    if name == "evict":
        assert recs[1][0] == 2 and recs[1][3:5] == (-1, np.float32(-1.0))                # C, opened and retired in the second call: unnamed
    if name == "resume_retire":
        assert recs[1][0] == 1 and recs[1][3] == -1                                      # B, opened and retired in the second call: unnamed
        assert recs[2][:2] == (2, 0) and recs[2][3:5] == (lc.A - 1, np.float32(1.0))     # A, resumed in B's slot, kept the winner's name


def test_threshold_is_strict():
    clip, kw, _ = lc.clip("same_slot")
    tmpl = np.zeros(DIM, np.float32)
    tmpl[[1, 2]] = 3.0, 4.0                                                                 # |tmpl| = 5 exactly
    face = lc.exact_rows([1], DIM)[0]
    s0 = lm.score(face, tmpl)                                                               # (3 / 5 + 1) / 2 in float32

    for thr, linked in ((s0, False), (np.nextafter(s0, np.float32(0.0)), True)):
        model = make(thr=thr, **kw)
        roots = run(model, clip, lambda persons: np.stack([tmpl, face]))[3][4]                 # the clip's two embedded faces
        assert (roots_of(clip, roots, lc.A)[-1] == 0) == linked
        assert ("score_equals_threshold" in model.events) == (not linked)


def test_total_cuts_the_open_event_and_reset_clears():
    clip, kw, _ = lc.clip("same_slot")
    model = make(**kw)
    _, we, _, out = run(model, clip, lambda p: lc.exact_rows(p, DIM)[:1], total=1)          # the returning face is behind `total`
    assert int(we.sum()) == 2 and roots_of(clip, out[4], lc.A) == [0, 0, 0, -1, -1, -1] and model.links_made == 0
    assert model.links(0)[0][0][:3] == (0, 0, 1)
    model.reset(0)
    assert model.links(0)[0] == [lm.FREE]


def test_three_streams_crowd_and_random_rows():
    clip = lc.three_streams()
    model = make(max_tracks=3, memory=1, max_age=150, streams=3)
    roots = run(model, clip, lambda p: lc.exact_rows(p, DIM))[3][4]
    for s in range(3):
        for who in (lc.A, lc.B):
            assert len(set(roots_of(clip, roots, 10 * s + who))) == 1, (s, who)
    assert model.links_made == 6

    crowd = lc.crowd()
    model = make(max_tracks=64, memory=8, max_age=150, dim=192)
    wt, _, _, out = run(model, crowd, lambda p: lc.exact_rows(p, 192))
    # every returning face displaces another slot's record into a memory of 8 rows, which overflows: some links, some people forgotten
    assert (wt[0] == -1).sum() == 6 and 8 < model.links_made < 64 and {"other_slot", "evicted", "from_memory"} <= model.events

    # random rows: the decisions hang on the score's bits; the premise of the GPU test is a link AND a refusal
    for dim in (64, 192, 512):
        clip, kw, _ = lc.clip("from_memory")
        model = make(dim=dim, **kw)
        run(model, clip, lambda p: lc.random_rows(p, dim, seed=dim))
        assert model.links_made >= 1 and "refused" in model.events, dim
