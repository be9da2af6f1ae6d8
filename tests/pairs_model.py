"""Plain numpy model of the pair audit (csrc/pairs_plan.h: fh_pairs_from_scores, and through it fh_gallery_pairs_dev).  A helper, not a
test file, and written independently of the header: upper triangle, class and side masks, a lexsort, and a walk over the bins of
tests/roc_model.py (which come from comparing with the exact edges b/2048, not from a ceil).

  * a pair (i, j), i < j, is genuine iff ids[i] == ids[j]; cls "genuine" / "impostor" / "any" (ids None: only "any");
  * selected: in the class, score not NaN, and score > thr ("above", strict, float32) or score <= thr ("not_above"); the NaN-scored pairs
    of the class are counted in nan;
  * order: "above" score descending, "not_above" score ascending, then i, then j;
  * the cut: walk the bins from the extreme end; want = min(cap, count); the first bin at which the running total reaches want is b*;
    total(b*) <= room: returned = want, complete = 1; otherwise returned = the total before b*, complete = 0;
  * outputs: info (count, nan, returned, complete), scores [cap], rows [cap][2], ids [cap][2] with (-1.0, -1, -1) behind `returned`
    (ids all -1 without ids)."""
import numpy as np

from tests import roc_model as rm

CLASSES = ("genuine", "impostor", "any")
SIDES = ("above", "not_above")
ROOM = 65536
MAX_CAP = 1024


def selected(S, ids, cls, side, thr):
    """(scores, i, j) of the selected pairs in list order, and the number of NaN-scored pairs of the class."""
    S = np.asarray(S, np.float32)
    n = len(S)
    i, j = np.triu_indices(n, 1)
    s = S[i, j]
    if cls == "any":
        m = np.ones(len(s), bool)
    else:
        same = np.asarray(ids)[i] == np.asarray(ids)[j]
        m = same if cls == "genuine" else ~same
    isnan = np.isnan(s)
    nan = int((m & isnan).sum())
    with np.errstate(invalid="ignore"):
        above = s > np.float32(thr)
    m = m & ~isnan & (above if side == "above" else ~above)
    s, i, j = s[m], i[m], j[m]
    key = -s.astype(np.float64) if side == "above" else s.astype(np.float64)      # (exact: every float32 is a float64; -0 never occurs)
    order = np.lexsort((j, i, key))
    return s[order], i[order].astype(np.int32), j[order].astype(np.int32), nan


def cut(scores, side, cap, room):
    """(returned, complete) of the bin walk over the selected scores"""
    count = len(scores)
    if count == 0:
        return 0, 1
    h = np.bincount(rm.bins(scores), minlength=rm.BINS)
    want = min(cap, count)
    total = 0
    for b in (range(rm.BINS - 1, -1, -1) if side == "above" else range(rm.BINS)):
        before = total
        total += int(h[b])
        if total >= want:
            return (want, 1) if total <= room else (before, 0)
    raise AssertionError("the walk ends at count >= want")


def pairs(S, ids, cls, side, thr, cap, room=None):
    """(info uint64[4], scores float32[cap], rows int32[cap, 2], ids int32[cap, 2]): the model of both entry points"""
    room = max(ROOM, cap) if room is None else room
    s, i, j, nan = selected(S, ids, cls, side, thr)
    returned, complete = cut(s, side, cap, room)
    out_s = np.full(cap, -1.0, np.float32)
    out_r = np.full((cap, 2), -1, np.int32)
    out_d = np.full((cap, 2), -1, np.int32)
    out_s[:returned] = s[:returned]
    out_r[:returned, 0] = i[:returned]
    out_r[:returned, 1] = j[:returned]
    if ids is not None:
        out_d[:returned] = np.asarray(ids, np.int32)[out_r[:returned]]
    return np.array([len(s), nan, returned, complete], np.uint64), out_s, out_r, out_d


def class_total(n, ids, cls):
    if cls == "any":
        return n * (n - 1) // 2
    cnt = np.unique(np.asarray(ids), return_counts=True)[1].astype(np.int64) if n else np.zeros(0, np.int64)
    g = int((cnt * (cnt - 1) // 2).sum())
    return g if cls == "genuine" else n * (n - 1) // 2 - g
