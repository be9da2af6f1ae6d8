"""Plain Python / numpy model of track re-linking (include/facehip.h, "track re-linking"; track_link_kernel in track_ident.hip).  It
wraps the identity models (tests/track_ident_model.py through tests/track_quality_model.py, which adds the weighted pool) without
editing them: the slot rows of the table ARE their Entry objects, extended by root / last_seen / links; the memory rows are Record
objects.  With re-linking never enabled every method is the parent's.  It restates

  * the table and fh_tracker_get_links (links());
  * stage A's serial walk: open events, continued tracks, last_seen, the root output;
  * the score, with explicit np.float32 products and adds in the contract's lane / butterfly order (score());
  * the retiring rule.

Stage B stays a callable, stage C is the parent's carry().  Not a test module."""
from __future__ import annotations

import numpy as np

from tests import gallery_fuse_model as gm
from tests import track_ident_model as im
from tests import track_model as tm
from tests import track_quality_model as qm

POOL_LAST, POOL_SUM, POOL_WEIGHTED = im.POOL_LAST, im.POOL_SUM, qm.POOL_WEIGHTED
MEMORY_MAX = 256
FREE = (-1, -1, 0, -1, np.float32(-1.0), 0, 0, 0)                   # owner, root, n_emb, label, score, last_seen, links, pad
f32 = np.float32


# ---------------------------------------------------------------------------------------------- the score
def lane_dot(x, y):
    """dot(x, y) as one wave computes it: lane l owns the float4 columns l, l + 64, ...; per column acc = acc + (((x0 y0 + x1 y1) +
    x2 y2) + x3 y3); then the xor butterfly 32 .. 1.  Every product and add is one float32 operation."""
    p = (np.asarray(x, f32) * np.asarray(y, f32)).reshape(-1, 4)
    col = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
    acc = np.zeros(64, f32)
    for c0 in range(0, len(col), 64):
        part = col[c0:c0 + 64]
        acc[:len(part)] = acc[:len(part)] + part
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    assert acc.dtype == f32
    return acc[0]


def score(emb, total_sum):
    """The link score of a face against a record's template, a float32 (possibly NaN)."""
    with np.errstate(all="ignore"):
        d, ss = lane_dot(emb, total_sum), lane_dot(total_sum, total_sum)
        nrm = np.sqrt(ss)
        c = d / nrm if nrm > f32(0.0) else d
        return f32((c + f32(1.0)) * f32(0.5))


# ---------------------------------------------------------------------------------------------- the table
class Record:
    """A memory row."""

    def __init__(self, dim):
        self.owner, self.root, self.n_emb, self.label, self.score, self.last_seen, self.links, _ = FREE
        self.sum = np.zeros(dim, f32)


def _extend(entry):
    """A slot's Entry as a table row.  a_label / a_score are the record's (label, score) as stage A sees them during a call (the Entry's
    own label / score are stage C's); since = (call number, "opened" | "resumed") of the open event that put the record there."""
    entry.root, entry.last_seen, entry.links = -1, 0, 0
    entry.a_label, entry.a_score, entry.since = -1, f32(-1.0), None
    return entry


class LinkTracker(qm.IdentTracker):
    def __init__(self, dim, pool=POOL_SUM, bestshot=None, **kw):
        super().__init__(dim, pool, bestshot, **kw)
        self.relink = None                                          # (memory, link_thr, max_age)
        self.memory = []
        self.opens = self.links_made = self.calls = 0                # open events / links / stage A calls, ever

    # ------------------------------------------------------------------------------------------ state
    def enable_relink(self, memory, link_thr, max_age):
        assert 0 <= memory <= MEMORY_MAX and np.isfinite(link_thr) and max_age > self.trk.max_missed
        self.relink = (int(memory), f32(link_thr), int(max_age))
        for s in range(len(self.ident)):
            self._clear(s)

    def _clear(self, s):
        self.ident[s] = [_extend(im.Entry(self.dim)) for _ in range(self.max_tracks)]
        while len(self.memory) <= s:
            self.memory.append([])
        self.memory[s] = [Record(self.dim) for _ in range(self.relink[0])]

    def reset(self, stream=-1):
        super().reset(stream)
        if self.relink is not None:
            for s in (range(len(self.ident)) if stream < 0 else [stream]):
                self._clear(s)

    def links(self, stream=0):
        """What fh_tracker_get_links reports: ([(owner, root, n_emb, label, score, last_seen, links, pad)] by row, sums [rows][dim])."""
        rows = list(self.ident[stream]) + list(self.memory[stream])
        recs = [FREE if r.owner == -1 else (r.owner, r.root, r.n_emb, r.label, f32(r.score), r.last_seen, r.links, 0) for r in rows]
        sums = np.array([np.zeros(self.dim, f32) if r.owner == -1 else r.sum for r in rows], f32).reshape(len(rows), self.dim)
        return recs, sums

    # ------------------------------------------------------------------------------------------ stage A
    def frame_times(self, n, stream_of):
        """t [n]: the update's frame time of every frame of the call that has just been through update()."""
        stream_of = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64)
        order, starts = tm.plan(stream_of, len(self.ident))
        t = np.zeros(n, np.int64)
        for s in range(len(self.ident)):
            b, e = int(starts[s]), int(starts[s + 1])
            for i in range(b, e):
                t[order[i]] = self.trk.streams[s].frame_no - (e - i)
        return t

    def own_roots(self, track, slot):
        """d_root with re-linking off."""
        return np.where(np.asarray(slot) >= 0, np.asarray(track), -1).astype(np.int32)

    def _dead_in_reach(self, r, t):
        _, _, max_age = self.relink
        gap = t - r.last_seen - 1
        return r.owner != -1 and gap > self.trk.max_missed and gap <= max_age

    def _retire(self, s, old, t):
        memory, _, max_age = self.relink
        if old.since is not None and old.since[0] == self.calls:    # the record came into its slot earlier in THIS call
            self.events.add("retired_" + old.since[1] + "_this_call")
            if old.since[2] >= 0:
                self.events.add("retired_from_a_named_slot")        # ... a slot that an earlier call's stage C had named
        if memory == 0:
            self.events.add("dropped_no_memory")
            return
        rows = self.memory[s]
        to = next((m for m, r in enumerate(rows) if r.owner == -1 or t - r.last_seen - 1 > max_age), None)
        if to is None:
            to = min(range(memory), key=lambda m: (rows[m].last_seen, rows[m].owner))
            self.events.add("evicted")
        rows[to] = old
        self.events.add("retired")

    def _as_record(self, entry):
        r = Record(self.dim)
        mem = isinstance(entry, Record)
        r.owner, r.root, r.n_emb = entry.owner, entry.root, entry.n_emb
        r.label, r.score = (entry.label, f32(entry.score)) if mem else (entry.a_label, f32(entry.a_score))
        r.last_seen, r.links, r.sum = entry.last_seen, entry.links, entry.sum.copy()
        r.since = None if mem else entry.since
        return r

    def _free(self, row):
        row.owner, row.root, row.n_emb, row.last_seen, row.links = -1, -1, 0, 0, 0
        row.sum = np.zeros(self.dim, f32)
        if isinstance(row, Record):
            row.label, row.score = -1, f32(-1.0)
        else:
            row.a_label, row.a_score, row.since = -1, f32(-1.0), None

    def pool_queries(self, track, slot, embed, emb, total=None, stream_of=None, quality=None):
        """Stage A.  Re-linking off: the parent's.  On: the serial walk; returns (queries, verbatim) as the parent and leaves the roots
        [n][per_frame] of the call in self.roots."""
        if self.relink is None:
            self.roots = self.own_roots(track, slot)
            if self.pool == POOL_WEIGHTED:
                return super().pool_queries(track, slot, embed, emb, total, stream_of, quality)
            return super().pool_queries(track, slot, embed, emb, total, stream_of)
        _, link_thr, _ = self.relink
        embed = np.asarray(embed)
        rank = self.ranks(embed)
        total = int((embed != 0).sum()) if total is None else total
        emb = np.asarray(emb, f32).reshape(-1, self.dim)
        q = np.zeros((total, self.dim), np.float64)
        verbatim = np.ones(total, bool)
        times = self.frame_times(embed.shape[0], stream_of)
        self.roots = np.full(embed.shape, -1, np.int32)
        weighted = self.pool == POOL_WEIGHTED
        self.calls += 1
        for row in self.ident:                                      # a slot's record starts the call with what stage C left in the slot
            for ent in row:
                ent.a_label, ent.a_score = ent.label, f32(ent.score)
        for s, f, j in self._walk(embed.shape, stream_of):
            tid, sl, e, t = int(track[f, j]), int(slot[f, j]), int(rank[f, j]), int(times[f])
            known = embed[f, j] != 0 and e < total
            if sl < 0:
                if known:
                    self.events.add("untracked")
                    q[e] = emb[e]
                continue
            rec = self.ident[s][sl]
            if known:
                row = emb[e]
                inp = (f32(max(int(quality[f][j]), 1)) * row).astype(f32) if weighted else row
                if rec.owner != tid:                                # 1. an open event
                    self.opens += 1
                    table = list(self.ident[s]) + list(self.memory[s])
                    best = None
                    for r in table:
                        if not self._dead_in_reach(r, t):
                            continue
                        sc = score(row, r.sum)
                        if sc == link_thr:
                            self.events.add("score_equals_threshold")
                        if not sc > link_thr:
                            self.events.add("refused")
                            continue
                        if best is not None and sc == best[0]:
                            self.events.add("tie_smaller_owner")
                        if best is None or sc > best[0] or (sc == best[0] and r.owner < best[1].owner):
                            best = (sc, r)
                    old = self._as_record(rec) if self._dead_in_reach(rec, t) else None
                    if best is None:
                        if old is not None:
                            self._retire(s, old, t)
                        rec.since = (self.calls, "opened", rec.label)
                        rec.owner, rec.root, rec.n_emb, rec.links, rec.sum = tid, tid, 1, 0, inp.copy()
                        rec.a_label, rec.a_score = -1, f32(-1.0)    # a fresh record is unnamed until stage C
                        q[e] = row
                    else:
                        c = best[1]
                        taken = self._as_record(c)
                        same = c is rec
                        self.events.add("same_slot" if same else "other_slot" if not isinstance(c, Record) else "from_memory")
                        self._free(c)
                        if old is not None and not same:
                            self._retire(s, old, t)
                        rec.since = (self.calls, "resumed", rec.label)
                        rec.owner, rec.root, rec.n_emb, rec.links = tid, taken.root, taken.n_emb + 1, taken.links + 1
                        rec.a_label, rec.a_score = taken.label, f32(taken.score)     # a resumed one keeps the winner's
                        self.links_made += 1
                        if self.pool == POOL_LAST:
                            rec.sum = row.copy()
                            q[e] = row
                        else:
                            rec.sum = (taken.sum + inp).astype(f32)
                            q[e] = gm.unit64(rec.sum[None], [2])[0]
                            verbatim[e] = False
                        if rec.links >= 2:
                            self.events.add("chain")
                else:                                               # 2. a continued track
                    rec.n_emb += 1
                    if self.pool == POOL_LAST:
                        rec.sum = row.copy()
                        q[e] = row
                    else:
                        rec.sum = (rec.sum + inp).astype(f32)
                        q[e] = gm.unit64(rec.sum[None], [2])[0]
                        verbatim[e] = False
            if rec.owner == tid:                                    # 3, 4
                rec.last_seen = t
                self.roots[f, j] = rec.root
        return q, verbatim

    def carry(self, track, slot, embed, labels, scores, total=None, stream_of=None):
        """Stage C: the parent's.  It replays the call's flagged faces slot by slot and ends, for a slot whose record a link took away
        later in the call, on an owner that is gone; the table's owner is stage A's, so it is put back."""
        owners = [[e.owner for e in row] for row in self.ident]
        out = super().carry(track, slot, embed, labels, scores, total, stream_of)
        if self.relink is not None:
            for row, keep in zip(self.ident, owners):
                for e, o in zip(row, keep):
                    e.owner = o
        return out

    def identify(self, track, slot, embed, emb, label_fn, total=None, stream_of=None, quality=None):
        """Stages A, B and C.  Returns (label, score, queries, verbatim, roots)."""
        q, verbatim = self.pool_queries(track, slot, embed, emb, total, stream_of, quality)
        labels, scores = label_fn(q) if len(q) else (np.zeros(0, np.int32), np.zeros(0, f32))
        out_l, out_s = self.carry(track, slot, embed, labels, scores, total, stream_of)
        return out_l, out_s, q, verbatim, self.roots
