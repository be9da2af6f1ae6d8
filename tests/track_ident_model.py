"""Plain Python / numpy model of per-track identity (include/facehip.h, "track identity"; track_ident.hip).  It wraps the tracker model
(tests/track_model.py) without editing it: after each frame() it finds the slot of every returned track id (a matched or opened track
is live at the end of its frame), which is what fh_track_update_slots_dev reports, and it restates stages A (pool) and C (carry) of
fh_track_identify_dev.  Stage B — the gallery — is a parameter: a callable queries -> (labels, scores).

Sums are sequential float32 adds in time order, so the device's sums are held to their bits; the unit form of a pooled query is computed
in float64 from the exact float32 sums, as tests/gallery_fuse_model.py: unit64, so the device's float32 normalisation is held to that
module's tolerance.  Not a test module."""
from __future__ import annotations

import numpy as np

from tests import gallery_fuse_model as gm
from tests import track_model as tm

POOL_LAST, POOL_SUM = 0, 1
NONE = (-1, 0, -1, np.float32(-1.0))                                # owner, n_emb, label, score of an entry nobody owns


class Entry:
    """The identity state of one (stream, slot)."""

    def __init__(self, dim):
        self.owner, self.n_emb, self.label, self.score = NONE
        self.named = -1                                             # the track id the label belongs to (the owner as stage C sees it)
        self.sum = np.zeros(dim, np.float32)


class IdentTracker:
    def __init__(self, dim, pool=POOL_SUM, **kw):
        self.trk = tm.Tracker(**kw)
        self.dim, self.pool = dim, pool
        self.max_tracks = self.trk.max_tracks
        self.ident = [[Entry(dim) for _ in range(self.max_tracks)] for _ in self.trk.streams]
        self.events = set()                                         # reopened, pooled, label_changed, untracked, carried

    # ------------------------------------------------------------------------------------------ the tracker with slots
    def reset(self, stream=-1):
        self.trk.reset(stream)
        for s in (range(len(self.ident)) if stream < 0 else [stream]):
            self.ident[s] = [Entry(self.dim) for _ in range(self.max_tracks)]

    def frame(self, stream, boxes):
        """[(track id, embed flag, slot)] of one frame."""
        out = self.trk.frame(stream, boxes)
        slots = self.trk.streams[stream].slots
        where = {s["id"]: i for i, s in enumerate(slots) if s is not None}
        return [(tid, flag, where[tid] if tid >= 0 else -1) for tid, flag in out]

    def update(self, det, counts, per_frame, stream_of=None):
        """tm.Tracker.update plus the slots: (track, embed, slot), each [n][per_frame] int32."""
        n = len(counts)
        stream_of = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64)
        track = np.full((n, per_frame), -1, np.int32)
        embed = np.zeros((n, per_frame), np.int32)
        slot = np.full((n, per_frame), -1, np.int32)
        order, _ = tm.plan(stream_of, len(self.trk.streams))
        for f in order:
            c = min(max(int(counts[f]), 0), per_frame)
            boxes = [tm._box(det[f][j]) for j in range(c)]
            for j, (tid, flag, sl) in enumerate(self.frame(int(stream_of[f]), boxes)):
                track[f, j], embed[f, j], slot[f, j] = tid, flag, sl
        return track, embed, slot

    # ------------------------------------------------------------------------------------------ identify
    @staticmethod
    def ranks(embed):
        """rank [n][per_frame] of every flagged entry among the flagged ones in (frame, slot) order (meaningless elsewhere)."""
        flat = (np.asarray(embed).reshape(-1) != 0).astype(np.int64)
        return (np.cumsum(flat) - flat).reshape(np.asarray(embed).shape)

    def _walk(self, shape, stream_of):
        n, per = shape
        stream_of = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64)
        order, _ = tm.plan(stream_of, len(self.ident))
        for f in order:                                             # each stream's frames in time order, j ascending
            for j in range(per):
                yield int(stream_of[f]), int(f), j

    def pool_queries(self, track, slot, embed, emb, total=None, stream_of=None):
        """Stage A.  Returns (queries [total][dim] float64, verbatim [total] bool): a verbatim query is its embedding's bits exactly; a
        pooled one is the float64 unit form of the exact float32 sum."""
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
            st = self.ident[s][sl]
            if st.owner != tid:
                if (s, sl) in touched:
                    self.events.add("reopened")
                st.owner, st.n_emb, st.sum = tid, 1, row.copy()
                q[e] = row
            else:
                st.n_emb += 1
                if self.pool == POOL_SUM:
                    st.sum = st.sum + row                           # one float32 add per component
                    q[e] = gm.unit64(st.sum[None], [2])[0]
                    verbatim[e] = False
                else:
                    st.sum = row.copy()
                    q[e] = row
            touched.add((s, sl))
            if st.n_emb >= 3:
                self.events.add("pooled")
        return q, verbatim

    def carry(self, track, slot, embed, labels, scores, total=None, stream_of=None):
        """Stage C.  labels / scores = the answers of the `total` queries.  Returns (label int32, score float32), each [n][per_frame]."""
        embed = np.asarray(embed)
        rank = self.ranks(embed)
        total = int((embed != 0).sum()) if total is None else total
        out_l = np.full(embed.shape, -1, np.int32)
        out_s = np.full(embed.shape, -1.0, np.float32)
        for s, f, j in self._walk(embed.shape, stream_of):
            tid, sl, e = int(track[f, j]), int(slot[f, j]), int(rank[f, j])
            if embed[f, j] != 0:
                if e >= total:
                    continue                                        # behind `total`: (-1, -1.0), the state stays
                out_l[f, j], out_s[f, j] = labels[e], scores[e]
                if sl >= 0:
                    st = self.ident[s][sl]
                    if st.named == tid and st.label != int(labels[e]):
                        self.events.add("label_changed")
                    st.owner = st.named = tid
                    st.label, st.score = int(labels[e]), np.float32(scores[e])
            elif sl >= 0:
                st = self.ident[s][sl]
                out_l[f, j], out_s[f, j] = st.label, st.score
                if st.label >= 0:
                    self.events.add("carried")
        return out_l, out_s

    def identify(self, track, slot, embed, emb, label_fn, total=None, stream_of=None):
        """Stages A, B (label_fn: queries float64 [total][dim] -> (labels, scores)) and C.  Returns (label, score, queries, verbatim)."""
        q, verbatim = self.pool_queries(track, slot, embed, emb, total, stream_of)
        labels, scores = label_fn(q) if len(q) else (np.zeros(0, np.int32), np.zeros(0, np.float32))
        out_l, out_s = self.carry(track, slot, embed, labels, scores, total, stream_of)
        return out_l, out_s, q, verbatim

    def identity(self, stream=0):
        """What fh_tracker_get_identity reports: ([(id, n_emb, label, score)], sums [live][dim]) of the live slots, ascending."""
        recs, sums = [], []
        for i, s in enumerate(self.trk.streams[stream].slots):
            if s is None:
                continue
            st = self.ident[stream][i]
            mine = st.owner == s["id"]
            recs.append((s["id"], st.n_emb, st.label, np.float32(st.score)) if mine else (s["id"],) + NONE[1:])
            sums.append(st.sum if mine else np.zeros(self.dim, np.float32))
        return recs, np.array(sums, np.float32).reshape(len(recs), self.dim)


def gallery_labels(rows, threshold, ids=None):
    """A float64 stage B over unit rows: label_fn(queries) -> (labels, scores) with score = (dot + 1) / 2, the best row's index (or its
    id) when the score is > threshold, else -1."""
    rows64 = np.asarray(rows, np.float64)

    def label_fn(q):
        sc = (np.asarray(q, np.float64) @ rows64.T + 1.0) / 2.0
        best = sc.argmax(1)
        top = sc[np.arange(len(q)), best]
        lab = best if ids is None else np.asarray(ids)[best]
        return np.where(top > threshold, lab, -1).astype(np.int32), top.astype(np.float32)
    return label_fn
