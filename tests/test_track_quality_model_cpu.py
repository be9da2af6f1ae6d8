"""The CPU model of face quality and best-shot re-embedding (tests/track_quality_model.py) held to hand-worked cases and to the models
it extends — no GPU.  The GPU tests (tests/test_gpu_track_quality.py) then hold the kernels to this model bit for bit.  (The argument
limits of fh_tracker_set_bestshot need a tracker handle, which lives on the device: they are checked in the GPU file.)"""
import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from tests import track_cases as tc
from tests import track_ident_model as im
from tests import track_model as tm
from tests import track_quality_model as qm

FRONTAL = (30.0, 40.0, 50.0, 40.0, 40.0, 50.0, 32.0, 60.0, 48.0, 60.0)      # eyes at x = 30 and 50, the nose at 40: P = 256


def rec(x, y, w, h, lm=FRONTAL):
    r = np.zeros((), fa.FACE_DTYPE)
    r["x"], r["y"], r["w"], r["h"], r["lm"] = x, y, w, h, lm
    return r


@pytest.fixture(scope="module")
def cases():
    return {name: tc.Case(name) for name in tc.CASES}


# ---------------------------------------------------------------------------------------------- the score
def test_a_flat_image_has_no_sharpness():
    img = np.full((64, 64, 3), 93, np.uint8)
    assert qm.sharpness(img, 10, 10, 40, 40) == 0 and qm.quality(img, rec(10, 10, 40, 40)) == 0


def test_a_checkerboard_has_the_closed_form_value():
    """White has luma (256 * 255 + 128) >> 8 = 255 and black 128 >> 8 = 0; every pixel's 4 neighbours are of the other colour, so L =
    |4 C - 4 (255 - C)| = 1020 everywhere: S = 1020, the largest value there is, and q = (1020 * 40 * 256) >> 8 = 40800."""
    yy, xx = np.mgrid[0:64, 0:64]
    img = np.repeat((((xx + yy) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    assert qm.luma(img).max() == 255 and qm.luma(img).min() == 0
    assert qm.sharpness(img, 10, 10, 40, 40) == 1020
    assert qm.quality(img, rec(10, 10, 40, 40)) == 40800
    assert qm.quality(img, rec(-5, -5, 500, 500)) == (1020 * 112 * 256) >> 8       # clipped to the frame; Z capped at 112


def test_stripes_under_a_stride_keep_their_distance_one_neighbours():
    """Columns alternate black and white: left and right are of the other colour, up and down of the same, L = |4 C - 2 (255 - C) -
    2 C| = 510 whatever the column.  A 200-wide window has d = 3; the neighbours stay at distance 1, so S stays 510."""
    yy, xx = np.mgrid[0:220, 0:220]
    img = np.repeat(((xx % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    events = set()
    assert qm.window(5, 5, 200, 210, 220, 220)[4] == 3
    assert qm.sharpness(img, 5, 5, 200, 210, events) == 510 and "strided" in events
    assert qm.sharpness(img, 5, 5, 40, 40) == 510


def test_a_box_of_seven_pixels_scores_nothing():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    assert qm.sharpness(img, 10, 10, 8, 8) > 0
    for box in ((10, 10, 7, 9), (10, 10, 9, 7), (10, 10, -20, 20), (58, 10, 40, 40), (0, 0, 8, 8), (500, 500, 40, 40)):
        assert qm.sharpness(img, *box) == 0 and qm.quality(img, rec(*box)) == 0, box
    assert qm.sharpness(img, 2 ** 31 - 40, 10, 2 ** 31 - 1, 40) == 0               # x + w beyond int32: clipped in wide integers
    assert qm.sharpness(img, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1) == 0
    assert qm.sharpness(img, -2 ** 31 + 8, 3, 2 ** 31 - 1, 30) == 0                # ends at x = 7: 6 columns
    assert qm.sharpness(None, 10, 10, 40, 40) == 0                                 # an empty frame


def test_the_sample_grid_and_the_integer_mean():
    """One bright pixel on black: its own L is 4 * 255, each of its 4 neighbours' is 255, so a stride-1 window around it sums to
    8 * 255 = 2040; a 10 x 9 window has 90 samples: S = 2040 // 90 = 22."""
    img = np.zeros((40, 40, 3), np.uint8)
    img[20, 20] = 255
    assert qm.sharpness(img, 15, 16, 10, 9) == 2040 // 90 == 22
    assert qm.sharpness(img, 21, 16, 10, 9) == 255 // 90                            # only the right-hand neighbour is inside


def test_size_and_pose():
    assert [qm.size(w, h) for w, h in ((40, 50), (50, 40), (300, 200), (112, 113), (-4, 50), (0, 9))] == [40, 40, 112, 112, 0, 0]
    lm = np.array(FRONTAL, np.float32)
    assert qm.pose(lm) == 256
    for nose, want in ((45.0, 128), (35.0, 128), (50.0, 0), (55.0, 0), (42.5, 192), (np.nan, 0), (np.inf, 0)):
        lm[4] = nose
        assert qm.pose(lm) == want, nose
    lm = np.array(FRONTAL, np.float32)
    lm[2] = lm[0]                                                                   # the eyes coincide: e = 1
    lm[4] = lm[0] + np.float32(0.25)
    assert qm.pose(lm) == 128
    for k in (0, 2):
        lm = np.array(FRONTAL, np.float32)
        lm[k] = np.nan
        assert qm.pose(lm) == 0
    lm = np.array(FRONTAL, np.float32)
    lm[1] = lm[3] = lm[5] = np.nan                                                  # the y coordinates play no part
    assert qm.pose(lm) == 256


# ---------------------------------------------------------------------------------------------- the update
@pytest.mark.parametrize("name", list(tc.CASES))
def test_equal_qualities_or_no_policy_reproduce_the_tracker_model(cases, name):
    case = cases[name]
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh)
    base = tm.Tracker(**kw)
    want = base.update(case.det, case.counts, case.per_frame, case.stream_of)
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 100000, (case.n, case.per_frame)).astype(np.int32)
    equal = np.full((case.n, case.per_frame), 4321, np.int32)
    for bestshot, quality in (((5, 4, 1), equal), ((1, 1, 1), equal), (None, noise), ((5, 4, 1), None), (None, None)):
        model = qm.Tracker(bestshot, **kw)
        got = model.update(case.det, case.counts, case.per_frame, case.stream_of, quality)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (bestshot, quality is None)
        for s in range(case.streams):
            assert model.state(s) == base.state(s)
    ident, ident_q = im.IdentTracker(64, **kw), qm.IdentTracker(64, bestshot=(5, 4, 1), **kw)
    a = ident.update(case.det, case.counts, case.per_frame, case.stream_of)
    b = ident_q.update(case.det, case.counts, case.per_frame, case.stream_of, equal)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert case.events <= base.events


BOX = (10, 10, 40, 40)


def run(model, quals, stream=0):
    return [model.frame(stream, [BOX], [q])[0] for q in quals]


def test_the_better_rule_is_strict_at_the_exact_ratio():
    model = qm.Tracker((5, 4, 1), max_tracks=2)
    out = run(model, [400, 500, 499, 501, 501, 626, 627])
    # opened with 400; 500 * 4 == 400 * 5: no; 499: no; 501: yes (best 501); 501 again: no; 626 * 4 = 2504 < 2505: no; 627: yes
    assert [flag for _, flag in out] == [1, 0, 0, 1, 0, 0, 1]
    assert {"exact_ratio", "bestshot"} <= model.events
    assert list(model.best_quality()) == [627] and model.state()[0][0][6] == 6     # last_embed


def test_falling_quality_never_embeds_and_the_timer_still_does():
    model = qm.Tracker((5, 4, 1), max_tracks=2, refresh=3)
    out = run(model, [900, 800, 700, 600, 500, 2000, 100, 100, 100])
    # the timer fires at t = 3 (quality 600: best stays 900), the jump to 2000 at t = 5, the timer again at t = 8
    assert [flag for _, flag in out] == [1, 0, 0, 1, 0, 1, 0, 0, 1]
    assert list(model.best_quality()) == [2000]


def test_min_gap_holds_an_improvement_back_and_releases_it():
    model = qm.Tracker((2, 1, 4), max_tracks=2)
    out = run(model, [100, 300, 300, 300, 300, 900, 900, 900, 900, 900])
    # 300 > 2 * 100 from t = 1 on, but only t = 4 is 4 frames after the opening; 900 > 2 * 300 from t = 5, released at t = 8
    assert [flag for _, flag in out] == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0]
    assert {"held_back", "bestshot"} <= model.events and list(model.best_quality()) == [900]


def test_a_reopened_slot_starts_its_best_quality_again_and_reset_clears_it():
    model = qm.Tracker((5, 4, 1), streams=2, max_tracks=1)
    assert run(model, [1000]) == [(0, 1)]
    assert model.frame(0, [], []) == [] and model.frame(0, [], []) == []           # the track expires (max_missed = 0)
    assert run(model, [10, 13]) == [(1, 1), (1, 1)] and list(model.best_quality()) == [13]
    assert model.frame(0, [BOX, (300, 300, 40, 40)], [5, 99999]) == [(1, 0), (-1, 1)]     # the untracked face changes nothing
    assert list(model.best_quality()) == [13]
    run(model, [77], stream=1)
    model.reset(0)
    assert model.best == [[0], [77]]


# ---------------------------------------------------------------------------------------------- the weighted pool
def test_the_weighted_pool_by_hand():
    dim = 64
    model = qm.IdentTracker(dim, qm.POOL_WEIGHTED, bestshot=(5, 4, 1), max_tracks=2)
    det = np.zeros((3, 1), fa.FACE_DTYPE)
    det["x"], det["y"], det["w"], det["h"] = BOX
    quality = np.array([[0], [3], [7]], np.int32)                                   # 0 weighs 1
    track, embed, slot = model.update(det, np.ones(3, np.int32), 1, None, quality)
    assert embed.reshape(-1).tolist() == [1, 1, 1] and slot.reshape(-1).tolist() == [0, 0, 0]
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((3, dim)).astype(np.float32)
    q, verbatim = model.pool_queries(track, slot, embed, emb, quality=quality)
    assert verbatim.tolist() == [True, False, False] and np.array_equal(q[0], emb[0])
    f = np.float32
    want = (emb[0] * f(1.0) + emb[1] * f(3.0)).astype(np.float32)
    want = (want + emb[2] * f(7.0)).astype(np.float32)
    assert model.ident[0][0].sum.tobytes() == want.tobytes() and model.ident[0][0].n_emb == 3
    assert np.allclose(q[2], want.astype(np.float64) / np.linalg.norm(want.astype(np.float64)), rtol=0, atol=1e-12)
    assert "weight_one" in model.events
    # the other pool modes do not look at the array
    for pool in (im.POOL_SUM, im.POOL_LAST):
        a, b = qm.IdentTracker(dim, pool, max_tracks=2), im.IdentTracker(dim, pool, max_tracks=2)
        ta = a.update(det, np.ones(3, np.int32), 1)
        tb = b.update(det, np.ones(3, np.int32), 1)
        qa = a.pool_queries(ta[0], ta[2], ta[1], emb, quality=quality)
        qb = b.pool_queries(tb[0], tb[2], tb[1], emb)
        assert np.array_equal(qa[0], qb[0]) and a.ident[0][0].sum.tobytes() == b.ident[0][0].sum.tobytes()
