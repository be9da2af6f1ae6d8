"""Interleaved A/B of the tracked pipeline (fh_pipeline_run_tracked_dev) on one MI355X, one process, full-size seeded models (det_500m +
w600k_r50), 128 frames of 640x640 per step, F = 8 faces per frame, HIP events around every block of steps, the legs alternated round
by round after a warm-up.

  (a) fh_pipeline_run_dev (unchanged code) on 128 distinct frames: every face embedded.  Against the parent commit's figure for the same
      call this is the regression check of the untracked path.
  (b) video: every stream repeats ONE frame, so every track survives.  128 frames as 1 stream x 128 and as 16 streams x 8 ([t][camera]
      order), each through fh_pipeline_run_dev (every face embedded) and through fh_pipeline_run_tracked_dev with refresh 0 and 8.  The
      tracker is NOT reset between steps: a step is the next 128 frames of the same cameras (steady state); the faces of the first
      step, on a fresh tracker, are reported beside it.
  (c) the update call alone (plan copy + track_update_kernel) on the detector's records of the (a) frames, as 1, 16 and 128 streams,
      beside fh_det_detect_batch_dev on the same frames in the same run.

  (d) identity: the video of (b) and a gallery of 10 000 rows; fh_pipeline_run_tracked_dev (the parent commit's path, unchanged) beside
      fh_pipeline_run_identified_dev with refresh 0 and 8, and — the serial chain at its worst — the update with slots alone beside
      update + fh_track_identify_dev on one stream with refresh 1, where every face of every frame is pooled into its track's sum.

  (e) best shot: the identified pipeline of (d) with the best-shot policy on (the quality kernel between the detector and the update,
      the update and the identify reading the qualities), beside the same pipeline with the policy off in the same run; and the
      quality kernel alone on the detector's records of the (a) frames.  Every camera of the video repeats one frame, so no face ever
      gets better: the step pays for the score and embeds nothing more.

  (f) re-linking: one camera shows a frame for 12 frames and a blank one for 4, over and over, with max_missed 0: every face loses its
      track in each pause and comes back as a new one.  fh_pipeline_run_identified_dev with re-linking off and on (memory 64, link_thr
      0.6, max_age 150) in the same run; the open events and links of a step are counted from the roots of the last step.

Writes --md (default profiles/track_ab.md) and prints one JSON line per case.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=128)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--steps", type=int, default=100, help="timed steps per leg (at least)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--block", type=int, default=5, help="steps per HIP-event sample")
ap.add_argument("--cases", nargs="+", default=["a", "b", "c", "d", "e", "f"])
ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "track_ab.md"))
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import facerecognizeonnx_amd as fa  # noqa: E402
from facerecognizeonnx_amd.synth import models  # noqa: E402

THR, NMS, F, HW = 0.5, 0.4, 8, 640
IOU_THR, MAX_TRACKS = 0.3, 64
GALLERY_ROWS, ID_THRESHOLD = 10000, 0.6
BESTSHOT = (5, 4, 1)                                               # num, den, min_gap
RELINK = (64, 0.6, 150)                                            # memory, link_thr, max_age


def samples(step, steps, block):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per, faces = [], 0
    for _ in range((steps + block - 1) // block):
        e0.record()
        for _ in range(block):
            faces = step()
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) / block)
    return per, faces


def stats(v):
    q = statistics.quantiles(v, n=10) if len(v) >= 10 else [min(v)] * 9
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4), "samples": len(v)}


def ab(legs, warmup, steps, rounds, block):
    """legs: name -> step.  The faces of every leg's FIRST step, a warm-up of every leg, then the legs alternated round by round."""
    res, faces, first = {k: [] for k in legs}, {}, {}
    for name, step in legs.items():
        first[name] = step()
        samples(step, warmup, block)
    for _ in range(rounds):
        for name, step in legs.items():
            per, faces[name] = samples(step, (steps + rounds - 1) // rounds, block)
            res[name] += per
    return {k: stats(v) for k, v in res.items()}, faces, first


def main():
    if not torch.cuda.is_available():
        raise SystemExit("track_ab.py measures on a GPU; none found")
    torch.cuda.set_device(0)
    fa._lib.check(fa.lib().fh_init(0), "fh_init")
    det, rec = fa.FaceDetector(), fa.FaceRecognizer()
    if not det.loadModel(models.cached("det_500m_seed100.onnx", models.make_det_500m)) or \
            not rec.loadModel(models.cached("w600k_r50_seed200.onnx", models.make_w600k_r50)):
        raise SystemExit("model load failed: " + fa._lib.last_error())
    B = a.frames
    stream = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    faces = torch.zeros((B * F, 15), device="cuda"); frame_of = torch.zeros(B * F, **i32); track_of = torch.zeros(B * F, **i32)
    emb = torch.zeros((B * F, 512), device="cuda")
    all_ = torch.zeros((B * F, 15), device="cuda"); counts = torch.zeros(B, **i32); track = torch.zeros((B, F), **i32)
    rng = np.random.default_rng(0)
    distinct = torch.from_numpy(rng.integers(0, 256, (B, HW, HW, 3), dtype=np.uint8)).cuda()
    out = {}

    def untracked(data):
        return lambda: fa.pipeline_run_dev(det, rec, data.data_ptr(), B, HW, HW, F, faces.data_ptr(), frame_of.data_ptr(), emb.data_ptr(),
                                           THR, NMS, stream)

    def tracked(data, trk, stream_of):
        return lambda: fa.pipeline_run_tracked_dev(det, rec, trk, data.data_ptr(), B, HW, HW, F, all_.data_ptr(), counts.data_ptr(),
                                                   track.data_ptr(), faces.data_ptr(), frame_of.data_ptr(), track_of.data_ptr(),
                                                   emb.data_ptr(), stream_of, THR, NMS, stream)

    if "a" in a.cases:
        st, fc, _ = ab({"untracked": untracked(distinct)}, a.warmup, a.steps, a.rounds, a.block)
        out["a"] = {"frames": B, "faces_per_step": fc["untracked"], **st}
        print(json.dumps({"case": "a", **out["a"]}), flush=True)

    if "b" in a.cases:
        out["b"] = {}
        for streams in (1, 16):
            if B % streams:
                continue
            stream_of = np.tile(np.arange(streams, dtype=np.int32), B // streams)                  # [t][camera]
            data = distinct[torch.from_numpy(stream_of.astype(np.int64)).cuda()].contiguous()      # camera s shows frame s, always
            trk = {r: fa.Tracker(streams, MAX_TRACKS, IOU_THR, 0, r) for r in (0, 8)}
            legs = {"untracked": untracked(data), "tracked_refresh0": tracked(data, trk[0], stream_of),
                    "tracked_refresh8": tracked(data, trk[8], stream_of)}
            st, fc, first = ab(legs, a.warmup, a.steps, a.rounds, a.block)
            out["b"][f"{streams}x{B // streams}"] = {"faces_per_step": fc, "faces_first_step": first, **st}
            del data
        print(json.dumps({"case": "b", **out["b"]}), flush=True)

    if "c" in a.cases:
        det.detect_batch_dev(distinct.data_ptr(), B, HW, HW, all_.data_ptr(), F, counts.data_ptr(), THR, NMS, stream=stream)
        torch.cuda.synchronize()
        embed = torch.zeros((B, F), **i32)
        legs, so = {}, {}
        for streams in (1, 16, B):
            so[streams] = np.tile(np.arange(streams, dtype=np.int32), B // streams)
            trk = fa.Tracker(streams, MAX_TRACKS, IOU_THR, 0, 8)
            legs[f"update_{streams}_streams"] = (lambda t, s: lambda: t.update_dev(all_.data_ptr(), counts.data_ptr(), B, F, track.data_ptr(),
                                                                                   embed.data_ptr(), stream_of=s, stream=stream))(trk, so[streams])
        legs["detector"] = lambda: det.detect_batch_dev(distinct.data_ptr(), B, HW, HW, faces.data_ptr(), F, frame_of.data_ptr(), THR, NMS,
                                                        stream=stream)
        st, _, _ = ab(legs, a.warmup, a.steps, a.rounds, a.block)
        out["c"] = {"frames": B, "faces_in_records": int(torch.clamp(counts, 0, F).sum().item()), **st}
        print(json.dumps({"case": "c", **out["c"]}), flush=True)

    if "d" in a.cases or "e" in a.cases or "f" in a.cases:
        gal = fa.Gallery(512)
        g = rng.standard_normal((GALLERY_ROWS, 512), dtype=np.float32)
        gal.enroll(g / np.linalg.norm(g, axis=1, keepdims=True))
        label = torch.zeros((B, F), **i32); score = torch.zeros((B, F), device="cuda")

        def identified(data, trk, stream_of):
            return lambda: fa.pipeline_run_identified_dev(det, rec, trk, gal, ID_THRESHOLD, data.data_ptr(), B, HW, HW, F, all_.data_ptr(),
                                                          counts.data_ptr(), track.data_ptr(), faces.data_ptr(), frame_of.data_ptr(),
                                                          track_of.data_ptr(), emb.data_ptr(), label.data_ptr(), score.data_ptr(), stream_of,
                                                          THR, NMS, stream)

    if "d" in a.cases:
        out["d"] = {"pipeline": {}}
        for streams in (1, 16):
            if B % streams:
                continue
            stream_of = np.tile(np.arange(streams, dtype=np.int32), B // streams)
            data = distinct[torch.from_numpy(stream_of.astype(np.int64)).cuda()].contiguous()
            legs = {}
            for r in (0, 8):
                legs[f"tracked_refresh{r}"] = tracked(data, fa.Tracker(streams, MAX_TRACKS, IOU_THR, 0, r), stream_of)
                t = fa.Tracker(streams, MAX_TRACKS, IOU_THR, 0, r)
                t.enable_identity(512)
                legs[f"identified_refresh{r}"] = identified(data, t, stream_of)
            st, fc, first = ab(legs, a.warmup, a.steps, a.rounds, a.block)
            out["d"]["pipeline"][f"{streams}x{B // streams}"] = {"faces_per_step": fc, "faces_first_step": first, **st}
            del data
        # the serial chain: one camera shows one frame, refresh 1 -> every face is flagged and pooled, 128 adds deep per slot and call
        one = distinct[:1].expand(B, HW, HW, 3).contiguous()
        det.detect_batch_dev(one.data_ptr(), B, HW, HW, all_.data_ptr(), F, counts.data_ptr(), THR, NMS, stream=stream)
        torch.cuda.synchronize()
        flagged = int(torch.clamp(counts, 0, F).sum().item())
        embed = torch.zeros((B, F), **i32); slot = torch.zeros((B, F), **i32)
        rows = torch.nn.functional.normalize(torch.randn((max(flagged, 1), 512), device="cuda"), dim=1)
        t_upd, t_id = fa.Tracker(1, MAX_TRACKS, IOU_THR, 0, 1), fa.Tracker(1, MAX_TRACKS, IOU_THR, 0, 1)
        t_id.enable_identity(512)

        def update(t):
            return t.update_dev(all_.data_ptr(), counts.data_ptr(), B, F, track.data_ptr(), embed.data_ptr(), stream=stream,
                                slot_ptr=slot.data_ptr())

        def update_identify():
            update(t_id)
            return t_id.identify_dev(gal, ID_THRESHOLD, track.data_ptr(), slot.data_ptr(), embed.data_ptr(), rows.data_ptr(), flagged, B, F,
                                     label.data_ptr(), score.data_ptr(), stream=stream)
        st, _, _ = ab({"update_slots": lambda: update(t_upd), "update_slots_identify": update_identify}, a.warmup, a.steps, a.rounds, a.block)
        out["d"]["chain"] = {"frames": B, "faces_pooled_per_call": flagged, **st}
        print(json.dumps({"case": "d", **out["d"]}), flush=True)

    if "e" in a.cases:
        out["e"] = {"pipeline": {}}
        for streams in (1, 16):
            if B % streams:
                continue
            stream_of = np.tile(np.arange(streams, dtype=np.int32), B // streams)
            data = distinct[torch.from_numpy(stream_of.astype(np.int64)).cuda()].contiguous()
            legs = {}
            for r in (0, 8):
                for policy in ("off", "bestshot"):
                    t = fa.Tracker(streams, MAX_TRACKS, IOU_THR, 0, r)
                    t.enable_identity(512)
                    if policy == "bestshot":
                        t.set_bestshot(*BESTSHOT)
                    legs[f"identified_{policy}_refresh{r}"] = identified(data, t, stream_of)
            st, fc, first = ab(legs, a.warmup, a.steps, a.rounds, a.block)
            out["e"]["pipeline"][f"{streams}x{B // streams}"] = {"faces_per_step": fc, "faces_first_step": first, **st}
            del data
        det.detect_batch_dev(distinct.data_ptr(), B, HW, HW, all_.data_ptr(), F, counts.data_ptr(), THR, NMS, stream=stream)
        torch.cuda.synchronize()
        quality = torch.zeros((B, F), **i32)
        st, _, _ = ab({"quality": lambda: fa.face_quality_dev(distinct.data_ptr(), all_.data_ptr(), counts.data_ptr(), F, quality.data_ptr(),
                                                              n=B, rows=HW, cols=HW, stream=stream)}, a.warmup, a.steps, a.rounds, a.block)
        q = quality.cpu().numpy()
        out["e"]["kernel"] = {"frames": B, "faces_in_records": int(torch.clamp(counts, 0, F).sum().item()),
                              "quality_min_median_max": [int(q.min()), int(np.median(q)), int(q.max())], **st}
        print(json.dumps({"case": "e", **out["e"]}), flush=True)

    if "f" in a.cases:
        shown = (np.arange(B) % 16) < 12                                                           # 12 frames of the face, 4 blank ones
        data = distinct[:1].expand(B, HW, HW, 3).contiguous()
        data[torch.from_numpy(~shown).cuda()] = 0
        legs, trks = {}, {}
        for mode in ("off", "on"):
            t = fa.Tracker(1, MAX_TRACKS, IOU_THR, 0, 0)
            t.enable_identity(512)
            if mode == "on":
                t.enable_relink(*RELINK)
            trks[mode] = t
            legs[f"identified_relink_{mode}"] = identified(data, t, None)
        st, fc, first = ab(legs, a.warmup, a.steps, a.rounds, a.block)
        torch.cuda.synchronize()
        roots = np.empty((B, F), np.int32)
        fa._lib.check(fa.lib().fh_memcpy_d2h(roots.ctypes.data, trks["on"].roots_ptr(), roots.nbytes), "fh_memcpy_d2h")
        tr = track.cpu().numpy()
        per_frame = torch.clamp(counts, 0, F).cpu().numpy()
        out["f"] = {"frames": B, "faces_per_step": fc, "faces_first_step": first, "open_events_per_step": fc["identified_relink_on"],
                    "faces_in_shown_frames": int(per_frame[shown].sum()), "faces_in_blank_frames": int(per_frame[~shown].sum()),
                    "links_per_step": int(len({int(t_) for t_, r in zip(tr.reshape(-1), roots.reshape(-1)) if r >= 0 and r != t_})),
                    "relink_cost_ms": round(st["identified_relink_on"]["median_ms"] - st["identified_relink_off"]["median_ms"], 4), **st}
        print(json.dumps({"case": "f", **out["f"]}), flush=True)

    if a.md and out:
        write_md(out)


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['min_ms']:.3f}-{s['max_ms']:.3f}; p10-p90 {s['p10_ms']:.3f}-{s['p90_ms']:.3f}; {s['samples']} samples)"


def write_md(out):
    L = ["# Tracked pipeline: interleaved A/B", "",
         f"`scripts/track_ab.py` on one MI355X, one process: det_500m + w600k_r50 (seeded), {a.frames} frames of {HW}x{HW} per step, up to "
         f"{F} faces per frame, thresholds {THR} / {NMS}, tracker iou_thr {IOU_THR}, max_missed 0, {MAX_TRACKS} slots; {a.warmup} warm-up "
         f"steps per leg, then the legs alternated for {a.rounds} rounds, >= {a.steps} timed steps per leg, HIP events around blocks of "
         f"{a.block} steps (ms per step: median, min-max, p10-p90 over the block samples).", ""]
    if "a" in out:
        d = out["a"]
        L += ["## (a) the untracked path, on the parent's terms", "",
              "| leg | ms per step | faces embedded per step |", "|---|---|---|",
              f"| `fh_pipeline_run_dev`, {d['frames']} distinct frames | {fmt(d['untracked'])} | {d['faces_per_step']} |", ""]
    if "b" in out:
        L += ["## (b) video: every camera shows one frame, the tracker carries on from step to step", "",
              "| streams x frames | leg | ms per step | faces embedded per step | ... on the first step |", "|---|---|---|---|---|"]
        names = {"untracked": "`fh_pipeline_run_dev` (every face)", "tracked_refresh0": "`fh_pipeline_run_tracked_dev`, refresh 0",
                 "tracked_refresh8": "`fh_pipeline_run_tracked_dev`, refresh 8"}
        for shape, d in out["b"].items():
            for k, label in names.items():
                L.append(f"| {shape} | {label} | {fmt(d[k])} | {d['faces_per_step'][k]} | {d['faces_first_step'][k]} |")
        L += [""]
    if "c" in out:
        d = out["c"]
        det_ms = d["detector"]["median_ms"]
        L += [f"## (c) the update call alone ({d['frames']} frames, {d['faces_in_records']} faces in the records)", "",
              "One `fh_track_update_dev` = the copy of the walk plan plus `track_update_kernel` (one wave per stream).", "",
              "| leg | ms per call | share of the detector's time |", "|---|---|---|"]
        for k, s in d.items():
            if k.startswith("update_"):
                L.append(f"| {k.replace('_', ' ')} | {fmt(s)} | {100 * s['median_ms'] / det_ms:.1f} % |")
        L += [f"| `fh_det_detect_batch_dev`, same frames, same run | {fmt(d['detector'])} | |", ""]
    if "d" in out:
        L += [f"## (d) identity: a label for every face, against a gallery of {GALLERY_ROWS} rows", "",
              "The video of (b); `fh_pipeline_run_tracked_dev` is the parent commit's path, `fh_pipeline_run_identified_dev` adds the slots, "
              "the pooling, the 1:N label and the carry.", "",
              "| streams x frames | leg | ms per step | faces embedded per step | ... on the first step |", "|---|---|---|---|---|"]
        for shape, d in out["d"]["pipeline"].items():
            for k in d["faces_per_step"]:
                L.append(f"| {shape} | `fh_pipeline_run_{k.split('_')[0]}_dev`, refresh {k[-1]} | {fmt(d[k])} | {d['faces_per_step'][k]} | "
                         f"{d['faces_first_step'][k]} |")
        c = out["d"]["chain"]
        L += ["", f"The serial chain at its worst: one camera, {c['frames']} frames, refresh 1, so all {c['faces_pooled_per_call']} faces of a "
              "call are pooled (each slot's sum takes one 2 KB read-add-write per frame) and labelled.", "",
              "| leg | ms per call |", "|---|---|",
              f"| `fh_track_update_slots_dev` | {fmt(c['update_slots'])} |",
              f"| `fh_track_update_slots_dev` + `fh_track_identify_dev` | {fmt(c['update_slots_identify'])} |", ""]
    if "e" in out:
        L += [f"## (e) best shot: the identified pipeline with the policy {BESTSHOT[0]} / {BESTSHOT[1]}, min_gap {BESTSHOT[2]}", "",
              "The video of (b) and the gallery of (d).  Every camera repeats one frame, so no face ever gets better: the policy pays for "
              "`fh_face_quality_dev` and the extended update and embeds nothing more.", "",
              "| streams x frames | leg | ms per step | faces embedded per step | ... on the first step |", "|---|---|---|---|---|"]
        for shape, d in out["e"]["pipeline"].items():
            for k in d["faces_per_step"]:
                L.append(f"| {shape} | `fh_pipeline_run_identified_dev`, policy {k.split('_')[1]}, refresh {k[-1]} | {fmt(d[k])} | "
                         f"{d['faces_per_step'][k]} | {d['faces_first_step'][k]} |")
        c = out["e"]["kernel"]
        L += ["", f"The quality kernel alone: {c['frames']} frames of {HW}x{HW}, {c['faces_in_records']} faces in the records (up to {F} per "
              f"frame), scores min / median / max {c['quality_min_median_max']}.", "",
              "| leg | ms per call |", "|---|---|", f"| `fh_face_quality_dev` | {fmt(c['quality'])} |", ""]
    if "f" in out:
        d = out["f"]
        L += [f"## (f) re-linking: memory {RELINK[0]}, link_thr {RELINK[1]}, max_age {RELINK[2]}", "",
              f"One camera, {d['frames']} frames per step: 12 frames of one picture, 4 blank ones, repeated; max_missed 0, refresh 0, so every "
              "face loses its track in each pause and opens a new one when it is back.  The gallery of (d).  The detector's records hold "
              f"{d['faces_in_shown_frames']} faces in the {int(d['frames'] * 12 / 16)} frames of the picture and {d['faces_in_blank_frames']} in the blank ones.", "",
              "| leg | ms per step | faces embedded per step | ... on the first step |", "|---|---|---|---|"]
        for k in ("identified_relink_off", "identified_relink_on"):
            L.append(f"| `fh_pipeline_run_identified_dev`, re-linking {k.split('_')[-1]} | {fmt(d[k])} | {d['faces_per_step'][k]} | "
                     f"{d['faces_first_step'][k]} |")
        L += ["", f"Re-linking on minus off: {d['relink_cost_ms']:+.3f} ms per step, for {d['open_events_per_step']} open events and "
              f"{d['links_per_step']} resumed tracks per step.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as f:
        f.write("\n".join(L))


if __name__ == "__main__":
    main()
