"""Plain Python / numpy model of the face tracker (include/facehip.h, "face tracker": steps 1-4 of the update, the flagged select and
the stream plan).  Boxes are Python ints; the iou is FaceDetector::iou (src/face_detector.cpp:340-354): integer intersection and areas,
then ONE fp32 division, evaluated under np.errstate(all="ignore") so that 0 / 0 is NaN.  Not a test module: the CPU tests hold this
model to hand-written scenarios, the GPU tests hold the kernels to this model bit for bit."""
from __future__ import annotations

import numpy as np

FIELDS = ("id", "x", "y", "w", "h", "last_seen", "last_embed", "hits")


def iou(a, b) -> np.float32:
    """a, b = (x, y, w, h) ints."""
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    x2, y2 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = max(0, x2 - x1) * max(0, y2 - y1)
    union = a[2] * a[3] + b[2] * b[3] - inter
    with np.errstate(all="ignore"):
        return np.float32(inter) / np.float32(union)


def plan(stream_of, streams):
    """(order, starts): the stable counting sort of the frame indices by stream."""
    stream_of = np.asarray(stream_of, np.int64)
    order = np.argsort(stream_of, kind="stable").astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(np.bincount(stream_of, minlength=streams))]).astype(np.int32)
    return order, starts


class Stream:
    def __init__(self, max_tracks):
        self.frame_no = 0
        self.next_id = 0
        self.slots = [None] * max_tracks            # None = free, else a dict of FIELDS

    def live(self):
        return [tuple(s[k] for k in FIELDS) for s in self.slots if s is not None]


class Tracker:
    def __init__(self, streams=1, max_tracks=64, iou_thr=0.3, max_missed=0, refresh=0):
        self.iou_thr = np.float32(iou_thr)
        self.max_tracks, self.max_missed, self.refresh = max_tracks, max_missed, refresh
        self.streams = [Stream(max_tracks) for _ in range(streams)]
        self.events = set()                         # what happened, for tests that must prove a hazard occurred

    def reset(self, stream=-1):
        for s in (range(len(self.streams)) if stream < 0 else [stream]):
            self.streams[s] = Stream(self.max_tracks)

    def state(self, stream=0):
        st = self.streams[stream]
        return st.live(), st.frame_no, st.next_id

    def frame(self, stream, boxes):
        """One frame of `stream`: boxes = the considered detections [(x, y, w, h)] in score order.  Returns [(track id, embed flag)]."""
        st = self.streams[stream]
        t = st.frame_no
        for i, s in enumerate(st.slots):                                             # 1. expire
            if s is not None and t - s["last_seen"] - 1 > self.max_missed:
                st.slots[i] = None
                self.events.add("expired")
        taken = set()
        out = []
        for box in boxes:
            box = _box(box)
            best = None                                                              # 2. match
            n_qual = 0
            for i, s in enumerate(st.slots):
                if s is None or i in taken:
                    continue
                v = iou((s["x"], s["y"], s["w"], s["h"]), box)
                if np.isnan(v):
                    self.events.add("nan")
                if not (v > self.iou_thr):                                           # strict; NaN fails
                    continue
                n_qual += 1
                if best is not None and v == best[0]:
                    self.events.add("tie")
                if best is None or v > best[0] or (v == best[0] and s["id"] < st.slots[best[1]]["id"]):
                    best = (v, i)
            if n_qual > 1:
                self.events.add("contest")
            if best is not None:
                s = st.slots[best[1]]
                s["x"], s["y"], s["w"], s["h"] = box
                s["last_seen"] = t
                s["hits"] += 1
                taken.add(best[1])
                again = int(self.refresh > 0 and t - s["last_embed"] >= self.refresh)
                if again:
                    s["last_embed"] = t
                    self.events.add("refresh")
                out.append((s["id"], again))
                continue
            free = [i for i, s in enumerate(st.slots) if s is None]                  # 3. open
            if free:
                i = free[0]
                st.slots[i] = dict(id=st.next_id, x=box[0], y=box[1], w=box[2], h=box[3], last_seen=t, last_embed=t, hits=1)
                st.next_id += 1
                taken.add(i)
                out.append((st.slots[i]["id"], 1))
            else:
                self.events.add("exhausted")
                out.append((-1, 1))
        st.frame_no += 1                                                             # 4. close
        return out

    def update(self, det, counts, per_frame, stream_of=None):
        """det = [n][per_frame] records with x, y, w, h fields (or an int array [n][per_frame][4]); counts = [n].  Returns
        (track [n][per_frame] int32, embed [n][per_frame] int32), walking each stream's frames in batch order."""
        n = len(counts)
        stream_of = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64)
        track = np.full((n, per_frame), -1, np.int32)
        embed = np.zeros((n, per_frame), np.int32)
        order, _ = plan(stream_of, len(self.streams))
        for f in order:
            c = min(max(int(counts[f]), 0), per_frame)
            if int(counts[f]) <= 0:
                self.events.add("empty" if int(counts[f]) == 0 else "negative")
            if int(counts[f]) > per_frame:
                self.events.add("overfull")
            boxes = [_box(det[f][j]) for j in range(c)]
            for j, (tid, flag) in enumerate(self.frame(int(stream_of[f]), boxes)):
                track[f, j], embed[f, j] = tid, flag
        return track, embed


def _box(r):
    if getattr(r, "dtype", None) is not None and r.dtype.names:
        return int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])
    return tuple(int(v) for v in r[:4])


def select(embed, track):
    """The flagged entries in (frame, slot) order: (flat indices into [n * per_frame], frame_of, track_of)."""
    embed = np.asarray(embed)
    n, per = embed.shape
    flat = np.flatnonzero(embed.reshape(-1) != 0)
    return flat, (flat // per).astype(np.int32), np.asarray(track).reshape(-1)[flat].astype(np.int32)
