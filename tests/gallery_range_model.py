"""Exact numpy model of the gallery's threshold (range) search (fh_gallery_range_dev, fh_range_from_scores).  A helper, not a test file.

  * a row's score is `gallery_ids_model.scores`: `oracle.dot_mfma`'s accumulator (the scan's own fma order) mapped (acc + 1) / 2 in float32;
  * row r is a hit of query q iff it is admitted ((tag[r] & mask[q]) != 0; no masks: every row; no tags: every row carries TAG_ALL), its
    score is strictly above the threshold in float32 and is not a NaN;
  * counts are exact; the lists hold the best min(count, cap) hits, (score desc, global row = base + position asc), and (-1.0, -1, -1)
    behind them."""
import numpy as np

from tests.gallery_ids_model import scores  # noqa: F401  (re-exported: the tests take their scores from here)

TAG_ALL = np.uint32(0xFFFFFFFF)


def hits(sc, thr, tags=None, masks=None):
    """[Q][G] bool."""
    h = sc > np.float32(thr)                                  # (False for a NaN)
    if masks is not None:
        t = np.full(sc.shape[1], TAG_ALL, np.uint32) if tags is None else np.asarray(tags, np.uint32)
        h &= (t[None, :] & np.asarray(masks, np.uint32)[:, None]) != 0
    return h


def one_query(s, hit, cap, base=0, ids=None):
    """One query's scores [G] and hit flags -> (count, scores[cap], rows[cap], ids[cap] or None)."""
    pos = np.flatnonzero(hit)
    o = np.lexsort((pos, -s[pos].astype(np.float64)))[:cap]   # best first (float32 -> float64 is exact and keeps the order)
    pos = pos[o]
    n = len(pos)
    S, R = np.full(cap, -1.0, np.float32), np.full(cap, -1, np.int32)
    S[:n], R[:n] = s[pos], base + pos
    D = None
    if ids is not None:
        D = np.full(cap, -1, np.int32)
        D[:n] = np.asarray(ids, np.int32)[pos]
    return int(hit.sum()), S, R, D


def range_from_scores(sc, thr, cap, base=0, tags=None, masks=None, ids=None):
    """(counts int64[Q], scores [Q][cap], rows [Q][cap], ids [Q][cap] or None)."""
    Q = sc.shape[0]
    h = hits(sc, thr, tags, masks)
    C = np.empty(Q, np.int64)
    S, R = np.empty((Q, cap), np.float32), np.empty((Q, cap), np.int32)
    D = np.empty((Q, cap), np.int32) if ids is not None else None
    for i in range(Q):
        C[i], S[i], R[i], d = one_query(sc[i], h[i], cap, base, ids)
        if ids is not None:
            D[i] = d
    return C, S, R, D
