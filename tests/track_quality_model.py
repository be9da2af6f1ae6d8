"""Plain Python / numpy model of face quality and best-shot re-embedding (include/facehip.h, "face quality"; face_quality.hip, the
extended track.hip and track_ident.hip).  It extends the existing models by import, without editing them:

  * quality()  the score q = (S * Z * P) >> 8: S from Python ints (unbounded, so the int64 sums of the contract cannot overflow here),
    P from np.float32 operations in the stated order;
  * Tracker    tests/track_model.py's tracker plus the best-shot rule.  A frame's embed decisions touch nothing but the matched slot's
    last_embed and best_q, and a slot is matched at most once per frame, so the rule is applied to what the base model's frame() returns;
  * IdentTracker  tests/track_ident_model.py's identity on that tracker, plus the quality-weighted pool.

Not a test module."""
from __future__ import annotations

import numpy as np

from tests import gallery_fuse_model as gm
from tests import track_ident_model as im
from tests import track_model as tm

POOL_WEIGHTED = 2
MIN_SIDE, GRID, MAX_SIZE = 8, 64, 112


# ---------------------------------------------------------------------------------------------- the score
def luma(img):
    """int64 [rows][cols] of a uint8 [rows][cols][3] BGR image."""
    a = np.asarray(img).astype(np.int64)
    return (29 * a[..., 0] + 150 * a[..., 1] + 77 * a[..., 2] + 128) >> 8


def window(x, y, w, h, rows, cols):
    """(x0, y0, x1, y1, d) of the sampled window, or None when it is smaller than 8 x 8."""
    x0, y0 = max(int(x), 1), max(int(y), 1)
    x1, y1 = min(int(x) + int(w), cols - 1), min(int(y) + int(h), rows - 1)
    if x1 - x0 < MIN_SIDE or y1 - y0 < MIN_SIDE:
        return None
    return x0, y0, x1, y1, max(1, min(x1 - x0, y1 - y0) // GRID)


def sharpness(img, x, y, w, h, events=None):
    rows, cols = (np.asarray(img).shape[:2] if img is not None else (0, 0))
    win = window(x, y, w, h, rows, cols)
    if win is None:
        return 0
    x0, y0, x1, y1, d = win
    if events is not None and d > 1:
        events.add("strided")
    Y = luma(img)
    px, py = np.arange(x0, x1, d), np.arange(y0, y1, d)
    c = Y[np.ix_(py, px)]
    lap = np.abs(4 * c - Y[np.ix_(py, px - 1)] - Y[np.ix_(py, px + 1)] - Y[np.ix_(py - 1, px)] - Y[np.ix_(py + 1, px)])
    return int(lap.sum()) // (len(px) * len(py))


def size(w, h):
    return min(max(min(int(w), int(h)), 0), MAX_SIZE)


def pose(lm):
    f = np.float32
    lm = np.asarray(lm, np.float32)
    lex, rex, nx = lm[0], lm[2], lm[4]
    with np.errstate(all="ignore"):
        dx = np.abs(rex - lex)
        e = dx if dx > f(1.0) else f(1.0)
        m = (lex + rex) * f(0.5)
        v = f(256.0) * (f(1.0) - f(2.0) * np.abs(nx - m) / e)
    if not (v > f(0.0)):
        return 0
    return min(int(v if v < f(256.0) else f(256.0)), 256)


def quality(img, rec, events=None):
    """The score of one record (a FACE_DTYPE row) on one image (None: an empty frame)."""
    S = sharpness(img, rec["x"], rec["y"], rec["w"], rec["h"], events)
    return (S * size(rec["w"], rec["h"]) * pose(rec["lm"])) >> 8


def quality_batch(frames, det, counts, per_frame, events=None):
    """int32 [n][per_frame]: frames = a list of images (or None), det = [n][per_frame] records, counts = [n]."""
    out = np.zeros((len(frames), per_frame), np.int32)
    for f, img in enumerate(frames):
        for j in range(min(max(int(counts[f]), 0), per_frame)):
            out[f, j] = quality(img, det[f][j], events)
    return out


# ---------------------------------------------------------------------------------------------- the update with the best-shot rule
class Tracker(tm.Tracker):
    def __init__(self, bestshot=None, **kw):
        """bestshot = (num, den, min_gap), or None: the policy is off."""
        super().__init__(**kw)
        self.best = [[0] * self.max_tracks for _ in self.streams]
        self.set_bestshot(bestshot)

    def set_bestshot(self, bestshot):
        self.bestshot = bestshot
        self.best = [[0] * self.max_tracks for _ in self.streams]

    def reset(self, stream=-1):
        super().reset(stream)
        for s in (range(len(self.streams)) if stream < 0 else [stream]):
            self.best[s] = [0] * self.max_tracks

    def frame(self, stream, boxes, quals=None):
        st = self.streams[stream]
        t, first_new = st.frame_no, st.next_id
        before = {s["id"]: s["last_embed"] for s in st.slots if s is not None}
        out = super().frame(stream, boxes)
        if self.bestshot is None or quals is None:
            return out
        num, den, gap = self.bestshot
        where = {s["id"]: i for i, s in enumerate(st.slots) if s is not None}
        for j, (tid, flag) in enumerate(out):
            if tid < 0:
                continue                                            # untracked: as it was
            i, q = where[tid], int(quals[j])
            if tid >= first_new:                                    # opened in this frame
                self.best[stream][i] = q
                continue
            if q * den == self.best[stream][i] * num:
                self.events.add("exact_ratio")
            better = q * den > self.best[stream][i] * num
            if better and not flag and t - before[tid] < gap:
                self.events.add("held_back")
            better = better and t - before[tid] >= gap
            if better and not flag:
                self.events.add("bestshot")
            if flag or better:
                st.slots[i]["last_embed"] = t
                self.best[stream][i] = max(self.best[stream][i], q)
                out[j] = (tid, 1)
        return out

    def update(self, det, counts, per_frame, stream_of=None, quality=None):
        if quality is None:
            return super().update(det, counts, per_frame, stream_of)
        track, embed, _ = _update(self, self, det, counts, per_frame, stream_of, quality)
        return track, embed

    def best_quality(self, stream=0):
        return np.array([self.best[stream][i] for i, s in enumerate(self.streams[stream].slots) if s is not None], np.int32)


def _update(trk, framer, det, counts, per_frame, stream_of, quality):
    """The batch walk of tm.Tracker.update with the qualities handed to frame(); framer.frame returns 2- or 3-tuples."""
    n = len(counts)
    stream_of = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64)
    track = np.full((n, per_frame), -1, np.int32)
    embed = np.zeros((n, per_frame), np.int32)
    slot = np.full((n, per_frame), -1, np.int32)
    order, _ = tm.plan(stream_of, len(trk.streams))
    for f in order:
        c = min(max(int(counts[f]), 0), per_frame)
        boxes = [tm._box(det[f][j]) for j in range(c)]
        quals = None if quality is None else [int(quality[f][j]) for j in range(c)]
        for j, res in enumerate(framer.frame(int(stream_of[f]), boxes, quals)):
            track[f, j], embed[f, j] = res[0], res[1]
            if len(res) > 2:
                slot[f, j] = res[2]
    return track, embed, slot


# ---------------------------------------------------------------------------------------------- identity with the weighted pool
class IdentTracker(im.IdentTracker):
    def __init__(self, dim, pool=im.POOL_SUM, bestshot=None, **kw):
        super().__init__(dim, pool, **kw)
        self.trk = Tracker(bestshot, **kw)

    def frame(self, stream, boxes, quals=None):
        out = self.trk.frame(stream, boxes, quals)
        where = {s["id"]: i for i, s in enumerate(self.trk.streams[stream].slots) if s is not None}
        return [(tid, flag, where[tid] if tid >= 0 else -1) for tid, flag in out]

    def update(self, det, counts, per_frame, stream_of=None, quality=None):
        return _update(self.trk, self, det, counts, per_frame, stream_of, quality)

    def pool_queries(self, track, slot, embed, emb, total=None, stream_of=None, quality=None):
        """Stage A; POOL_WEIGHTED: sum = wq * row on a (re)opened slot, else sum = sum + wq * row — one float32 multiply, then one
        float32 add per component — with wq = float32(max(q, 1))."""
        if self.pool != POOL_WEIGHTED:
            return super().pool_queries(track, slot, embed, emb, total, stream_of)
        embed = np.asarray(embed)
        rank = self.ranks(embed)
        total = int((embed != 0).sum()) if total is None else total
        emb = np.asarray(emb, np.float32).reshape(-1, self.dim)
        q = np.zeros((total, self.dim), np.float64)
        verbatim = np.ones(total, bool)
        touched = set()
        for s, f, j in self._walk(embed.shape, stream_of):
            e = int(rank[f, j])
            if embed[f, j] == 0 or e >= total:
                continue
            tid, sl = int(track[f, j]), int(slot[f, j])
            row = emb[e]
            if sl < 0:
                self.events.add("untracked")
                q[e] = row
                continue
            wq = np.float32(max(int(quality[f][j]), 1))
            if int(quality[f][j]) <= 0:
                self.events.add("weight_one")
            st = self.ident[s][sl]
            if st.owner != tid:
                if (s, sl) in touched:
                    self.events.add("reopened")
                st.owner, st.n_emb, st.sum = tid, 1, (wq * row).astype(np.float32)
                q[e] = row
            else:
                st.n_emb += 1
                st.sum = (st.sum + (wq * row).astype(np.float32)).astype(np.float32)
                q[e] = gm.unit64(st.sum[None], [2])[0]
                verbatim[e] = False
                self.events.add("pooled")
            touched.add((s, sl))
        return q, verbatim
