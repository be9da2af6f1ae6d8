"""The face tracker on the GPU (include/facehip.h, "face tracker"; track.hip) held BIT FOR BIT to its CPU model (tests/track_model.py):
track ids, embed flags, the selected list, its total and the device state, on synthetic record streams (tests/track_cases.py: random
walks with births and deaths plus planted ties, zero-area boxes, empty and negative counts), across split and back-to-back calls, and
through fh_pipeline_run_tracked_dev with the tiny detector and recogniser."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import facerecognizeonnx_amd as fa            # noqa: E402
from facerecognizeonnx_amd import _lib        # noqa: E402
from tests import track_cases as tc           # noqa: E402
from tests import track_model as tm           # noqa: E402
from tests import util                        # noqa: E402

FH_ERR_ARG = -1
IN = 128                                                       # tiny_scrfd(hw=128): the frame size of test_gpu_ragged.py's pipeline tests
# the pipeline test's two frames and thresholds: with these the CPU oracle finds 6 and 4 faces, of which frame B shares three with A
VIDEO_SEED, THR = 42, (0.3, 0.4)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real device: the product path has no CPU fallback")
    fa.lib().fh_init(0)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the cases are read-only)


def dev_records(det):
    return dev(np.ascontiguousarray(det).view(np.uint8).reshape(-1, 60))


def records(t, n):
    return t.cpu().numpy().view(np.uint8).reshape(n, 60).copy().view(fa.FACE_DTYPE).reshape(n)


@pytest.fixture(scope="module")
def cases():
    return {name: tc.Case(name) for name in tc.CASES}


def make(case, iou_thr):
    kw = dict(streams=case.streams, max_tracks=case.max_tracks, iou_thr=iou_thr, max_missed=case.max_missed, refresh=case.refresh)
    return fa.Tracker(**kw), tm.Tracker(**kw)


def gpu_update(trk, case, first=0, last=None, sync=True, with_stream_of=True):
    """One fh_track_update_dev + fh_track_select_dev on frames [first, last) of the case; every output buffer starts as a pattern."""
    last = case.n if last is None else last
    n, per = last - first, case.per_frame
    d = dev_records(case.det[first:last])
    cnt = dev(case.counts[first:last])
    track = torch.full((n, per), 77, dtype=torch.int32, device="cuda"); embed = torch.full((n, per), 77, dtype=torch.int32, device="cuda")
    faces = torch.full((n * per, 15), 7.0, device="cuda"); fo = torch.full((n * per,), -7, dtype=torch.int32, device="cuda")
    to = torch.full((n * per,), -7, dtype=torch.int32, device="cuda"); total = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    so = case.stream_of[first:last] if with_stream_of else None
    assert trk.update_dev(d.data_ptr(), cnt.data_ptr(), n, per, track.data_ptr(), embed.data_ptr(), stream_of=so) == n
    assert fa.Tracker.select_dev(d.data_ptr(), embed.data_ptr(), n, per, faces.data_ptr(), fo.data_ptr(), track.data_ptr(), to.data_ptr(),
                                 total.data_ptr()) == n
    if sync:
        torch.cuda.synchronize()
    return dict(d=d, cnt=cnt, track=track, embed=embed, faces=faces, fo=fo, to=to, total=total, first=first, last=last)


def check_against_model(out, case, want_track, want_embed):
    """want_* = the model's outputs for the frames of this call."""
    n, per = out["last"] - out["first"], case.per_frame
    track, embed = out["track"].cpu().numpy(), out["embed"].cpu().numpy()
    assert np.array_equal(track, want_track), np.argwhere(track != want_track)[:5]
    assert np.array_equal(embed, want_embed), np.argwhere(embed != want_embed)[:5]
    flat, frame_of, track_of = tm.select(want_embed, want_track)
    total = int(out["total"].cpu().numpy()[0])
    assert total == len(flat)
    got = records(out["faces"], n * per)
    assert got[:total].tobytes() == np.ascontiguousarray(case.det[out["first"]:out["last"]]).reshape(-1)[flat].tobytes()
    assert np.array_equal(out["fo"].cpu().numpy()[:total], frame_of) and np.array_equal(out["to"].cpu().numpy()[:total], track_of)
    assert torch.all(out["faces"][total:] == 7.0) and torch.all(out["fo"][total:] == -7) and torch.all(out["to"][total:] == -7)


def check_state(trk, model, streams):
    for s in streams:
        live, frame_no, next_id = trk.state(s, counters=True)
        assert ([tuple(int(v) for v in r) for r in live], frame_no, next_id) == model.state(s), s


# ---------------------------------------------------------------------------------------------- synthetic records, no detector
@pytest.mark.parametrize("iou_thr", tc.IOU_THRS)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_synthetic_records_equal_the_model(cases, name, iou_thr):
    case = cases[name]
    trk, model = make(case, iou_thr)
    want_track, want_embed = model.update(case.det, case.counts, case.per_frame, case.stream_of)
    assert case.events <= model.events, case.events - model.events               # every planted hazard occurred
    if name == "more_faces_than_lanes":
        assert case.per_frame > _lib.TRACK_MAX and case.counts.max() > case.per_frame and (case.counts == 70).any()
    if name == "64_streams_one_slot":
        assert tc.UNUSED_STREAM not in case.stream_of and model.state(tc.UNUSED_STREAM) == ([], 0, 0)
    out = gpu_update(trk, case, with_stream_of=case.streams > 1)                  # (one stream: the NULL stream_of form)
    check_against_model(out, case, want_track, want_embed)
    check_state(trk, model, range(case.streams))


# ---------------------------------------------------------------------------------------------- continuation, reset
def test_split_calls_continue_the_stream_and_reset_starts_again(cases):
    case = cases["one_stream"]
    trk, model = make(case, 0.3)
    want_track, want_embed = model.update(case.det, case.counts, case.per_frame, case.stream_of)
    whole = gpu_update(trk, case)
    check_against_model(whole, case, want_track, want_embed)
    state_whole = trk.state(0, counters=True)
    assert state_whole[2] > 3

    def in_pieces(t):
        for a, b in case.slices([1, 7, 32]):
            check_against_model(gpu_update(t, case, a, b), case, want_track[a:b], want_embed[a:b])
        got = t.state(0, counters=True)
        assert got[0].tobytes() == state_whole[0].tobytes() and got[1:] == state_whole[1:]

    in_pieces(fa.Tracker(streams=1, max_tracks=case.max_tracks, iou_thr=0.3, max_missed=case.max_missed, refresh=case.refresh))
    trk.reset(0)                                                                  # the used tracker, reset: ids start from 0 again
    live, frame_no, next_id = trk.state(0, counters=True)
    assert len(live) == 0 and (frame_no, next_id) == (0, 0)
    in_pieces(trk)


def test_reset_of_one_stream_leaves_the_others(cases):
    case = cases["three_streams_exhausted"]
    trk, model = make(case, 0.3)
    model.update(case.det, case.counts, case.per_frame, case.stream_of)
    gpu_update(trk, case)
    check_state(trk, model, range(3))
    assert all(len(model.state(s)[0]) > 0 for s in (1, 2))
    trk.reset(0)
    model.reset(0)
    assert model.state(0) == ([], 0, 0)
    check_state(trk, model, range(3))
    trk.reset()                                                                   # -1: all
    for s in range(3):
        live, frame_no, next_id = trk.state(s, counters=True)
        assert len(live) == 0 and (frame_no, next_id) == (0, 0)


# ---------------------------------------------------------------------------------------------- the staging ring
def test_back_to_back_calls_with_different_stream_tables(cases):
    """Six calls on one tracker, each with its own stream_of, without a synchronise between them: more calls than the staging ring has
    slots, so a stale or overwritten table would walk the wrong frames."""
    case = cases["three_streams_exhausted"]
    trk, model = make(case, 0.3)
    want_track, want_embed = model.update(case.det, case.counts, case.per_frame, case.stream_of)
    pieces = case.slices([10] * 6)
    assert len({case.stream_of[a:b].tobytes() for a, b in pieces}) == 6           # the tables differ
    outs = [gpu_update(trk, case, a, b, sync=False) for a, b in pieces]
    torch.cuda.synchronize()
    for out, (a, b) in zip(outs, pieces):
        check_against_model(out, case, want_track[a:b], want_embed[a:b])
    check_state(trk, model, range(3))


# ---------------------------------------------------------------------------------------------- arguments
@pytest.fixture(scope="module")
def models_(models_dir):
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    assert det.loadModel(util.tiny_scrfd(models_dir, hw=128, cls_bias=-2.0)) and rec.loadModel(util.tiny_iresnet(models_dir))
    assert det.input_size() == (IN, IN)
    return det, rec


def pipeline_bufs(n, F, dim=512):
    b = dict(all=torch.full((n * F, 15), 5.0, device="cuda"), cnt=torch.full((n,), -5, dtype=torch.int32, device="cuda"),
             track=torch.full((n, F), 77, dtype=torch.int32, device="cuda"), faces=torch.full((n * F, 15), 7.0, device="cuda"),
             fo=torch.full((n * F,), -7, dtype=torch.int32, device="cuda"), to=torch.full((n * F,), -7, dtype=torch.int32, device="cuda"),
             emb=torch.full((n * F, dim), 7.0, device="cuda"))
    return b


def run_pipeline_raw(det, rec, trk_handle, frames, n, F, b, stream_of_ptr):
    return fa.lib().fh_pipeline_run_tracked_dev(det.handle, rec.handle, trk_handle, frames.data_ptr(), n, IN, IN, IN * 3, IN * IN * 3,
                                                stream_of_ptr, THR[0], THR[1], F, b["all"].data_ptr(), b["cnt"].data_ptr(), b["track"].data_ptr(),
                                                b["faces"].data_ptr(), b["fo"].data_ptr(), b["to"].data_ptr(), b["emb"].data_ptr(), 0)


def test_argument_errors_change_nothing(cases, models_):
    det, rec = models_
    case = cases["three_streams_exhausted"]
    trk, model = make(case, 0.3)
    model.update(case.det, case.counts, case.per_frame, case.stream_of)
    out = gpu_update(trk, case)
    n, per = case.n, case.per_frame
    L = fa.lib()
    bad = case.stream_of.copy(); bad[n // 2] = 3
    neg = case.stream_of.copy(); neg[0] = -1
    bad4 = np.array([0, 1, 3, 2], np.int32)                                       # for the pipeline's four frames
    upd = lambda t, n_, so: L.fh_track_update_dev(t, out["d"].data_ptr(), out["cnt"].data_ptr(), n_, per, so, out["track"].data_ptr(),  # noqa: E731
                                                  out["embed"].data_ptr(), 0)
    frames = dev(util.frames_u8(4, IN, IN, seed=41, smooth=True))
    b = pipeline_bufs(4, per)
    so = case.stream_of.ctypes.data
    for what, call in [("null tracker", lambda: upd(None, n, so)),
                       ("n = 0", lambda: upd(trk.handle, 0, so)),
                       ("stream out of range", lambda: upd(trk.handle, n, bad.ctypes.data)),
                       ("negative stream", lambda: upd(trk.handle, n, neg.ctypes.data)),
                       ("pipeline: null tracker", lambda: run_pipeline_raw(det, rec, None, frames, 4, per, b, None)),
                       ("pipeline: n = 0", lambda: run_pipeline_raw(det, rec, trk.handle, frames, 0, per, b, None)),
                       ("pipeline: stream out of range", lambda: run_pipeline_raw(det, rec, trk.handle, frames, 4, per, b, bad4.ctypes.data))]:
        rc = call()
        assert rc == FH_ERR_ARG, what
        assert ("fh_pipeline_run_tracked_dev" if what.startswith("pipeline") else "fh_track_update_dev") in _lib.last_error(), what
        torch.cuda.synchronize()
        check_state(trk, model, range(3))                                         # the state is what the one good call left
    assert torch.all(b["cnt"] == -5) and torch.all(b["track"] == 77) and torch.all(b["emb"] == 7.0)   # nothing was launched
    with pytest.raises(fa.FaceHipError):
        trk.update_dev(out["d"].data_ptr(), out["cnt"].data_ptr(), n, per, out["track"].data_ptr(), out["embed"].data_ptr(), stream_of=bad)


# ---------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def video(models_):
    """A A A B B A on one stream, and what fh_det_detect_batch_dev says about it (the reference the pipeline's d_all / d_counts must
    equal bitwise, and the records the model runs on)."""
    det, _ = models_
    F = 4
    two = util.frames_u8(2, IN, IN, seed=VIDEO_SEED, smooth=True)
    assert two[0].tobytes() != two[1].tobytes()
    frames = np.ascontiguousarray(two[[0, 0, 0, 1, 1, 0]])
    n = len(frames)
    fd = dev(frames)
    ref_all = torch.full((n * F, 15), 5.0, device="cuda"); ref_cnt = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    assert det.detect_batch_dev(fd.data_ptr(), n, IN, IN, ref_all.data_ptr(), F, ref_cnt.data_ptr(), *THR) == n
    torch.cuda.synchronize()
    counts = ref_cnt.cpu().numpy()
    assert counts[0] >= 2 and counts[3] >= 2, counts                              # premise: A and B each yield at least 2 faces
    return dict(fd=fd, n=n, F=F, ref_all=ref_all.cpu().numpy(), counts=counts, recs=records(ref_all, n * F).reshape(n, F))


@pytest.mark.parametrize("refresh", [0, 2])
def test_pipeline_embeds_a_track_once(models_, video, refresh):
    det, rec = models_
    n, F, fd = video["n"], video["F"], video["fd"]
    kw = dict(streams=1, max_tracks=8, iou_thr=0.3, max_missed=0, refresh=refresh)
    trk, model = fa.Tracker(**kw), tm.Tracker(**kw)
    want_track, want_embed = model.update(video["recs"], video["counts"], F)
    flat, frame_of, track_of = tm.select(want_embed, want_track)
    b = pipeline_bufs(n, F)
    total = fa.pipeline_run_tracked_dev(det, rec, trk, fd.data_ptr(), n, IN, IN, F, b["all"].data_ptr(), b["cnt"].data_ptr(),
                                        b["track"].data_ptr(), b["faces"].data_ptr(), b["fo"].data_ptr(), b["to"].data_ptr(),
                                        b["emb"].data_ptr(), scoreThreshold=THR[0], nmsThreshold=THR[1])
    torch.cuda.synchronize()
    # the detector's part is fh_det_detect_batch_dev's output, bit for bit
    assert b["all"].cpu().numpy().tobytes() == video["ref_all"].tobytes() and np.array_equal(b["cnt"].cpu().numpy(), video["counts"])
    # the tracker's part is the model's
    assert total == len(flat) and np.array_equal(b["track"].cpu().numpy(), want_track)
    assert records(b["faces"], n * F)[:total].tobytes() == video["recs"].reshape(-1)[flat].tobytes()
    assert np.array_equal(b["fo"].cpu().numpy()[:total], frame_of) and np.array_equal(b["to"].cpu().numpy()[:total], track_of)
    assert torch.all(b["faces"][total:] == 7.0) and torch.all(b["fo"][total:] == -7) and torch.all(b["emb"][total:] == 7.0)
    check_state(trk, model, [0])
    # the recogniser ran on exactly the model's list: the same call on that list gives the same bits
    sel = dev_records(video["recs"].reshape(-1)[flat]); sel_fo = dev(frame_of)
    ref_emb = torch.zeros((total, 512), device="cuda")
    assert fa.lib().fh_rec_embed_faces_dev(rec.handle, fd.data_ptr(), IN, IN, IN * 3, IN * IN * 3, sel.data_ptr(), sel_fo.data_ptr(), total,
                                           ref_emb.data_ptr(), 0, 0) == total, _lib.last_error()
    torch.cuda.synchronize()
    assert b["emb"][:total].cpu().numpy().tobytes() == ref_emb.cpu().numpy().tobytes()
    every_face = int(np.minimum(video["counts"], F).sum())
    per_frame = want_embed.sum(1)
    print(f"tracked pipeline, refresh {refresh}: {total} of {every_face} faces embedded, per frame {per_frame.tolist()}")
    if refresh == 0:
        assert per_frame[0] == min(video["counts"][0], F) and per_frame[1] == 0 and per_frame[2] == 0   # premise: the second A embeds nothing
        assert total < every_face
    else:
        once = tm.Tracker(**dict(kw, refresh=0))
        assert per_frame[2] > 0 and total > int(once.update(video["recs"], video["counts"], F)[1].sum())   # the refresh embeds more
