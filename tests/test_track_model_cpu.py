"""The face tracker's contract on the host (include/facehip.h, "face tracker").  No GPU needed: the model (tests/track_model.py) is
held to hand-written scenarios whose expected ids are written out, fh_track_plan is host code, and fh_tracker_create checks its
arguments before it touches a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import track_cases as tc
from tests import track_model as tm

FH_ERR_ARG = -1
NEW = ("fh_tracker_create", "fh_tracker_destroy", "fh_tracker_reset", "fh_tracker_get_state", "fh_track_plan", "fh_track_update_dev",
       "fh_track_select_dev", "fh_pipeline_run_tracked_dev")


def test_tracker_symbols_resolve():
    L = fa.lib()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    assert C.sizeof(_lib.FhTrackState) == 32 and fa.TRACK_DTYPE.itemsize == 32 and _lib.TRACK_MAX == 64
    assert callable(fa.track_plan) and callable(fa.pipeline_run_tracked_dev)
    for name in ("update_dev", "select_dev", "reset", "state"):
        assert callable(getattr(fa.Tracker, name)), name


# ---------------------------------------------------------------------------------------------- the model, by hand
def ids(out):
    return [t for t, _ in out]


def flags(out):
    return [e for _, e in out]


def test_iou_is_the_reference_arithmetic():
    assert tm.iou((0, 0, 10, 10), (0, 0, 10, 10)) == np.float32(1.0)
    assert tm.iou((0, 0, 10, 10), (5, 0, 10, 10)) == np.float32(50) / np.float32(150)
    assert tm.iou((0, 0, 10, 10), (10, 0, 10, 10)) == np.float32(0.0)                 # touching: empty intersection
    assert np.isnan(tm.iou((3, 3, 0, 5), (3, 3, 0, 7)))                               # 0 / 0


def test_a_drifting_box_keeps_its_id():
    t = tm.Tracker(max_tracks=4, iou_thr=0.3, max_missed=0)
    for k in range(12):
        out = t.frame(0, [(10 + k, 20 + k, 40, 40)])
        assert out == [(0, 1 if k == 0 else 0)], k
    live, frame_no, next_id = t.state()
    assert live == [(0, 21, 31, 40, 40, 11, 0, 12)] and frame_no == 12 and next_id == 1


def test_two_boxes_swapping_score_order_keep_their_ids():
    t = tm.Tracker(max_tracks=4, iou_thr=0.3)
    a, b = (0, 0, 30, 30), (100, 0, 30, 30)
    assert ids(t.frame(0, [a, b])) == [0, 1]
    assert ids(t.frame(0, [b, a])) == [1, 0]                                          # b now scores higher: listed first, still id 1
    assert ids(t.frame(0, [a, b])) == [0, 1]
    assert t.state()[2] == 2 and "tie" not in t.events


@pytest.mark.parametrize("max_missed", [0, 1, 3])
def test_expiry_after_exactly_max_missed_plus_one_absent_frames(max_missed):
    box = (5, 5, 20, 20)
    # absent for max_missed frames: the track is still there
    t = tm.Tracker(max_tracks=2, iou_thr=0.3, max_missed=max_missed)
    assert ids(t.frame(0, [box])) == [0]
    for _ in range(max_missed):
        assert t.frame(0, []) == []
    assert t.frame(0, [box]) == [(0, 0)]
    assert "expired" not in t.events
    # absent for max_missed + 1 frames: gone, the face opens track 1 (in the slot that was freed: the lowest)
    t = tm.Tracker(max_tracks=2, iou_thr=0.3, max_missed=max_missed)
    assert ids(t.frame(0, [box])) == [0]
    for _ in range(max_missed + 1):
        assert t.frame(0, []) == []
    assert t.frame(0, [box]) == [(1, 1)]
    assert "expired" in t.events
    live, frame_no, next_id = t.state()
    assert [s[0] for s in live] == [1] and frame_no == max_missed + 3 and next_id == 2


def test_refresh_fires_at_exactly_t_minus_last_embed_equal_refresh():
    box = (0, 0, 16, 16)
    t = tm.Tracker(max_tracks=2, refresh=3)
    got = [t.frame(0, [box])[0] for _ in range(8)]
    assert got == [(0, 1), (0, 0), (0, 0), (0, 1), (0, 0), (0, 0), (0, 1), (0, 0)]    # embedded at t = 0, 3, 6
    assert t.state()[0] == [(0, 0, 0, 16, 16, 7, 6, 8)]
    t = tm.Tracker(max_tracks=2, refresh=0)                                           # 0: once, when the track opens
    assert [t.frame(0, [box])[0] for _ in range(5)] == [(0, 1)] + [(0, 0)] * 4
    t = tm.Tracker(max_tracks=2, refresh=1)                                           # 1: every frame
    assert [t.frame(0, [box])[0] for _ in range(3)] == [(0, 1)] * 3


def test_an_equal_iou_tie_goes_to_the_smaller_id():
    t = tm.Tracker(max_tracks=4, iou_thr=0.1, max_missed=5)
    left, right, mid = (0, 0, 20, 10), (20, 0, 20, 10), (10, 0, 20, 10)
    assert ids(t.frame(0, [right, left])) == [0, 1]                                   # the RIGHT box is id 0, in slot 0
    assert tm.iou(left, mid) == tm.iou(right, mid) == np.float32(100) / np.float32(300)
    assert ids(t.frame(0, [mid])) == [0] and "tie" in t.events
    # the same with the smaller id in the HIGHER slot: ids decide, not slots
    t = tm.Tracker(max_tracks=4, iou_thr=0.1, max_missed=5)
    far = (500, 500, 8, 8)
    assert ids(t.frame(0, [far])) == [0]                                              # slot 0, id 0
    for _ in range(7):
        t.frame(0, [])                                                                # ... expires
    assert ids(t.frame(0, [far, left])) == [1, 2]                                     # slot 0 = id 1, slot 1 = id 2
    for _ in range(7):
        t.frame(0, [left])                                                            # id 1 (far) expires, id 2 stays in slot 1
    assert ids(t.frame(0, [left, right])) == [2, 3]                                   # right opens id 3 in slot 0
    assert [s[0] for s in t.state()[0]] == [3, 2]
    assert ids(t.frame(0, [mid])) == [2]


def test_a_zero_area_box_never_matches():
    t = tm.Tracker(max_tracks=8, iou_thr=0.0, max_missed=9)
    flat, thin = (4, 4, 0, 9), (4, 4, 9, 0)
    assert ids(t.frame(0, [flat])) == [0]
    assert ids(t.frame(0, [flat])) == [1] and "nan" in t.events                       # 0 / 0 = NaN fails the strict comparison
    assert ids(t.frame(0, [thin, (0, 0, 20, 20)])) == [2, 3]                          # nor does a real box match a zero-area track
    assert ids(t.frame(0, [(0, 0, 20, 20)])) == [3]
    assert flags(t.frame(0, [flat])) == [1]


def test_the_65th_simultaneous_face_is_untracked_and_flagged():
    t = tm.Tracker(max_tracks=64, iou_thr=0.3)
    boxes = [(40 * (k % 10), 40 * (k // 10), 30, 30) for k in range(65)]
    assert t.frame(0, boxes) == [(k, 1) for k in range(64)] + [(-1, 1)]
    assert t.frame(0, boxes) == [(k, 0) for k in range(64)] + [(-1, 1)] and "exhausted" in t.events
    live, frame_no, next_id = t.state()
    assert len(live) == 64 and next_id == 64 and frame_no == 2


def test_model_update_walks_streams_in_batch_order_and_closes_frames():
    t = tm.Tracker(streams=2, max_tracks=2)
    det = np.zeros((4, 3, 4), np.int64)
    det[:, 0] = (0, 0, 10, 10)
    det[:, 1] = (50, 0, 10, 10)
    track, embed = t.update(det, [2, 1, -3, 7], 3, stream_of=[1, 0, 1, 0])
    assert track.tolist() == [[0, 1, -1], [0, -1, -1], [-1, -1, -1], [0, 1, -1]]      # frame 3: count 7 > per_frame = 3 slots, 2 tracks
    assert embed.tolist() == [[1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 1]]
    assert {"negative", "overfull", "exhausted"} <= t.events
    flat, frame_of, track_of = tm.select(embed, track)
    assert flat.tolist() == [0, 1, 3, 10, 11] and frame_of.tolist() == [0, 0, 1, 3, 3] and track_of.tolist() == [0, 1, 0, 1, -1]
    assert t.state(1)[1:] == (2, 2) and t.state(0)[1:] == (2, 2)


@pytest.mark.parametrize("iou_thr", tc.IOU_THRS)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_every_planted_hazard_of_the_gpu_cases_occurs_in_the_model(name, iou_thr):
    """The seeds of tests/track_cases.py are chosen here, without a GPU: the GPU tests assert the same before they compare."""
    case = tc.Case(name)
    assert (case.streams, case.n, case.per_frame) == tc.CASES[name][:3] and case.det.shape == (case.n, case.per_frame)
    model = tm.Tracker(streams=case.streams, max_tracks=case.max_tracks, iou_thr=iou_thr, max_missed=case.max_missed, refresh=case.refresh)
    track, embed = model.update(case.det, case.counts, case.per_frame, case.stream_of)
    assert case.events <= model.events, case.events - model.events
    assert (track[embed == 0] >= -1).all() and ((track == -1) <= ((embed == 1) | (embed == 0))).all()
    c = np.clip(case.counts, 0, case.per_frame)
    for f in range(case.n):
        assert (track[f, c[f]:] == -1).all() and (embed[f, c[f]:] == 0).all() and (embed[f, :c[f]][track[f, :c[f]] == -1] == 1).all()
    assert 0 < embed.sum() <= c.sum()
    assert (embed.sum() == c.sum()) == (case.refresh == 1)        # refresh 1 embeds every face; otherwise the tracker saves some


# ---------------------------------------------------------------------------------------------- fh_track_plan
@pytest.mark.parametrize("stream_of,streams", [
    ([0], 1),                                                       # n = 1
    ([0] * 9, 1),                                                   # all one stream
    ([2, 0, 1, 2, 0, 1, 2, 0, 1, 1, 1, 0], 3),                      # interleaved
    ([3, 0, 3, 0, 0], 5),                                           # streams 1, 2 and 4 have no frames
    (list(np.random.default_rng(5).integers(0, 4096, 4096)), 4096),  # the limits
])
def test_track_plan_against_a_stable_argsort(stream_of, streams):
    order, starts = fa.track_plan(stream_of, streams)
    a = np.asarray(stream_of)
    assert order.dtype == np.int32 and starts.dtype == np.int32 and len(starts) == streams + 1
    assert np.array_equal(order, np.argsort(a, kind="stable"))
    assert np.array_equal(starts, np.concatenate([[0], np.cumsum(np.bincount(a, minlength=streams))]))
    mo, ms = tm.plan(stream_of, streams)
    assert np.array_equal(order, mo) and np.array_equal(starts, ms)


def test_track_plan_null_stream_of_is_stream_zero():
    order, starts = np.full(5, -1, np.int32), np.full(3, -1, np.int32)
    assert fa.lib().fh_track_plan(None, 5, 2, order.ctypes.data, starts.ctypes.data) == 0
    assert order.tolist() == [0, 1, 2, 3, 4] and starts.tolist() == [0, 5, 5]


@pytest.mark.parametrize("stream_of,n,streams", [
    ([0, 3, 1], 3, 3),                                              # a stream index out of range
    ([0, -1, 1], 3, 3),
    ([0], 0, 1),                                                    # n = 0
    ([0], 1, 0),                                                    # streams = 0
    ([0] * 4097, 4097, 1),
    ([0], 1, 4097),
])
def test_track_plan_rejects(stream_of, n, streams):
    a = np.asarray(stream_of, np.int32)
    order, starts = np.full(len(a) + 1, -7, np.int32), np.full(max(streams, 0) + 2, -7, np.int32)
    assert fa.lib().fh_track_plan(a.ctypes.data, n, streams, order.ctypes.data, starts.ctypes.data) == FH_ERR_ARG
    assert "fh_track_plan" in _lib.last_error()
    assert (order == -7).all() and (starts == -7).all()             # nothing written
    with pytest.raises(fa.FaceHipError):
        fa.track_plan(stream_of[:n], streams)


def test_track_plan_under_asan_ubsan(tmp_path):
    """csrc/track_plan.h as a stand-alone CPU program with exactly sized arrays: tests/native/track_plan_sanitize.cpp."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "track_plan_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(root, "tests", "native", "track_plan_sanitize.cpp")]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
    assert b.returncode == 0, b.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------- fh_tracker_create
@pytest.mark.parametrize("args", [
    (1, 0, 0.3, 0, 0), (1, 65, 0.3, 0, 0),                          # max_tracks 0 and 65
    (1, 8, 0.3, -1, 0), (1, 8, 0.3, 0, -1),                         # negative max_missed / refresh
    (0, 8, 0.3, 0, 0), (4097, 8, 0.3, 0, 0),                        # streams
])
def test_tracker_create_checks_its_arguments_before_any_device_work(args):
    assert fa.lib().fh_tracker_create(*args) is None
    assert "fh_tracker_create" in _lib.last_error()
    with pytest.raises(fa.FaceHipError):
        fa.Tracker(*args)


def test_null_tracker_is_an_argument_error():
    L = fa.lib()
    assert L.fh_tracker_reset(None, 0) == FH_ERR_ARG and L.fh_tracker_get_state(None, 0, None, None, None) == FH_ERR_ARG
    assert L.fh_track_update_dev(None, 1, 1, 1, 1, None, 1, 1, None) == FH_ERR_ARG and "fh_track_update_dev" in _lib.last_error()
    L.fh_tracker_destroy(None)
