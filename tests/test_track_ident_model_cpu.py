"""The per-track identity model (tests/track_ident_model.py) held to the contract of include/facehip.h ("track identity") on hand-written
scenarios of a few frames each — no GPU — and the one check that needs the built library: every new entry point is exported and bound."""
import ctypes

import numpy as np

import facerecognizeonnx_amd as fa
from facerecognizeonnx_amd import _lib
from tests import track_ident_model as im

A, B, FAR = (10, 10, 40, 40), (12, 11, 40, 40), (300, 300, 40, 40)      # B overlaps A (one track), FAR does not
DIM = 4
E = np.eye(DIM, dtype=np.float32)


def axis_labels(q):
    """A stand-in for the gallery: the label is the query's largest component when that is > 0.6, the score is that component."""
    q = np.asarray(q, np.float64)
    best = q.argmax(1)
    top = q[np.arange(len(q)), best]
    return np.where(top > 0.6, best, -1).astype(np.int32), top.astype(np.float32)


def run(model, frames, emb, per_frame=2, total=None):
    """frames = [[box, ...]] on stream 0.  Returns (track, embed, slot, label, score, queries, verbatim)."""
    det = np.zeros((len(frames), per_frame, 4), np.int64)
    counts = np.array([len(f) for f in frames], np.int32)
    for i, f in enumerate(frames):
        for j, b in enumerate(f):
            det[i, j] = b
    track, embed, slot = model.update(det, counts, per_frame)
    label, score, q, verbatim = model.identify(track, slot, embed, emb, axis_labels, total=total)
    return track, embed, slot, label, score, q, verbatim


def test_slots_are_the_lanes_of_the_tracks():
    m = im.IdentTracker(DIM, streams=1, max_tracks=2, iou_thr=0.3, max_missed=0, refresh=0)
    track, embed, slot, *_ = run(m, [[A, FAR], [FAR, B], [A, FAR, ]], np.tile(E[0], (2, 1)), per_frame=3)
    assert track.tolist() == [[0, 1, -1], [1, 0, -1], [0, 1, -1]]
    assert slot.tolist() == [[0, 1, -1], [1, 0, -1], [0, 1, -1]]             # the slot follows the track, not the position
    assert embed.tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 0]]


def test_a_single_embedding_track_keeps_its_row_and_its_label_is_carried():
    m = im.IdentTracker(DIM, streams=1, max_tracks=2, iou_thr=0.3, max_missed=0, refresh=0)
    row = np.array([0.1, 0.9, 0.3, 0.2], np.float32)                          # not a unit vector: it must NOT be re-normalised
    _, embed, _, label, score, q, verbatim = run(m, [[A], [B], [A]], row[None])
    assert embed.tolist() == [[1, 0], [0, 0], [0, 0]]
    assert verbatim.all() and q[0].astype(np.float32).tobytes() == row.tobytes()
    assert label.tolist() == [[1, -1], [1, -1], [1, -1]]                      # frames 1 and 2 were never embedded
    assert score[:, 0].tolist() == [np.float32(0.9)] * 3 and (score[:, 1] == -1.0).all()
    assert "carried" in m.events and "pooled" not in m.events
    recs, sums = m.identity(0)
    assert recs == [(0, 1, 1, np.float32(0.9))] and sums[0].tobytes() == row.tobytes()


def test_pool_sum_adds_in_time_order_and_pool_last_keeps_the_latest():
    rows = np.array([[1, 0, 0, 0], [0.6, 0.8, 0, 0], [0, 1, 0, 0]], np.float32)
    m = im.IdentTracker(DIM, pool=im.POOL_SUM, streams=1, max_tracks=1, iou_thr=0.3, max_missed=0, refresh=1)
    _, embed, _, label, _, q, verbatim = run(m, [[A], [B], [A]], rows, per_frame=1)
    assert embed.tolist() == [[1], [1], [1]] and verbatim.tolist() == [True, False, False]
    s2 = rows[0] + rows[1]
    s3 = s2 + rows[2]
    assert np.allclose(q[1], s2.astype(np.float64) / np.linalg.norm(s2.astype(np.float64)), rtol=0, atol=1e-15)
    assert np.allclose(q[2], s3.astype(np.float64) / np.linalg.norm(s3.astype(np.float64)), rtol=0, atol=1e-15)
    assert label.tolist() == [[0], [0], [1]] and {"pooled", "label_changed"} <= m.events          # the template drifted to axis 1
    recs, sums = m.identity(0)
    assert recs[0][:3] == (0, 3, 1) and sums[0].tobytes() == s3.tobytes()

    last = im.IdentTracker(DIM, pool=im.POOL_LAST, streams=1, max_tracks=1, iou_thr=0.3, max_missed=0, refresh=1)
    _, _, _, label, _, q, verbatim = run(last, [[A], [B], [A]], rows, per_frame=1)
    assert verbatim.all() and q.astype(np.float32).tobytes() == rows.tobytes()
    recs, sums = last.identity(0)
    assert recs[0][:3] == (0, 3, 1) and sums[0].tobytes() == rows[2].tobytes()


def test_reopen_resets_the_sum_and_propagation_stops_at_expiry():
    m = im.IdentTracker(DIM, streams=1, max_tracks=1, iou_thr=0.3, max_missed=0, refresh=0)
    rows = np.array([[0, 0, 1, 0], [0.5, 0.5, 0.5, 0.5]], np.float32)         # the second face is unknown (no component > 0.6)
    track, embed, slot, label, score, q, _ = run(m, [[A], [B], [], [FAR], [FAR]], rows, per_frame=1)
    assert track.tolist() == [[0], [0], [-1], [1], [1]] and slot.tolist() == [[0], [0], [-1], [0], [0]]
    assert label.tolist() == [[2], [2], [-1], [-1], [-1]]                     # track 1 sits in track 0's slot and does not inherit its name
    assert score[3:, 0].tolist() == [np.float32(0.5)] * 2
    assert "reopened" in m.events
    recs, sums = m.identity(0)
    assert recs == [(1, 1, -1, np.float32(0.5))] and sums[0].tobytes() == rows[1].tobytes()


def test_an_untracked_face_leaves_the_state_alone():
    m = im.IdentTracker(DIM, streams=1, max_tracks=1, iou_thr=0.3, max_missed=0, refresh=0)
    rows = np.array([[1, 0, 0, 0], [0, 0, 0, 1]], np.float32)
    track, embed, slot, label, _, q, verbatim = run(m, [[A, FAR], [B, FAR]], np.concatenate([rows, rows[1:]]))
    assert track.tolist() == [[0, -1], [0, -1]] and slot.tolist() == [[0, -1], [0, -1]] and embed.tolist() == [[1, 1], [0, 1]]
    assert verbatim.all() and q.astype(np.float32).tobytes() == np.concatenate([rows, rows[1:]]).tobytes()
    assert label.tolist() == [[0, 3], [0, 3]] and "untracked" in m.events     # the untracked face is named, every time it is embedded
    recs, sums = m.identity(0)
    assert recs == [(0, 1, 0, np.float32(1.0))] and sums[0].tobytes() == rows[0].tobytes()


def test_a_flag_behind_total_answers_nothing_and_changes_nothing():
    m = im.IdentTracker(DIM, streams=1, max_tracks=2, iou_thr=0.3, max_missed=0, refresh=0)
    _, embed, _, label, score, q, _ = run(m, [[A, FAR]], E[:1], total=1)
    assert embed.tolist() == [[1, 1]] and len(q) == 1
    assert label.tolist() == [[0, -1]] and score.tolist() == [[1.0, -1.0]]
    recs, _ = m.identity(0)
    assert recs == [(0, 1, 0, np.float32(1.0)), (1, 0, -1, np.float32(-1.0))]      # track 1 is live but was never identified


def test_reset_clears_the_identity():
    m = im.IdentTracker(DIM, streams=2, max_tracks=1, iou_thr=0.3, max_missed=0, refresh=0)
    det = np.zeros((2, 1, 4), np.int64)
    det[:, 0] = A
    track, embed, slot = m.update(det, np.array([1, 1], np.int32), 1, stream_of=[0, 1])
    m.identify(track, slot, embed, E[:2], axis_labels, stream_of=[0, 1])
    assert m.identity(0)[0] == [(0, 1, 0, np.float32(1.0))] and m.identity(1)[0] == [(0, 1, 1, np.float32(1.0))]
    m.reset(0)
    assert m.identity(0)[0] == [] and m.ident[0][0].owner == -1 and m.identity(1)[0] == [(0, 1, 1, np.float32(1.0))]
    track, embed, slot = m.update(det[:1], np.array([1], np.int32), 1, stream_of=[0])          # track ids restart at 0 on stream 0
    label, _, q, verbatim = m.identify(track, slot, embed, E[2:3], axis_labels, stream_of=[0])
    assert track.tolist() == [[0]] and verbatim.all() and label.tolist() == [[2]] and m.identity(0)[0] == [(0, 1, 2, np.float32(1.0))]


NEW_SYMBOLS = ("fh_track_update_slots_dev", "fh_tracker_enable_identity", "fh_track_identify_dev", "fh_tracker_queries_dev",
               "fh_tracker_get_identity", "fh_pipeline_run_identified_dev")


def test_new_entry_points_are_exported_and_declared():
    raw = ctypes.CDLL(_lib.build())                                          # the library itself, not the bound handle
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name
        assert getattr(raw, name) is not None, name                         # AttributeError: not exported
        assert getattr(fa.lib(), name).argtypes == _lib.PROTOTYPES[name][1], name
    for name in ("enable_identity", "identify_dev", "identity"):
        assert callable(getattr(fa.Tracker, name)), name
    assert callable(fa.pipeline_run_identified_dev)
    assert _lib.TRACK_IDENT_DTYPE.itemsize == 16 and (fa.TRACK_POOL_LAST, fa.TRACK_POOL_SUM) == (0, 1)
