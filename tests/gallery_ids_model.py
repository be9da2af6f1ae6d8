"""Exact numpy model of the labelled gallery's identity top-k (gallery_topk_ids_kernel + topk_merge_kernel<CACHED, true>).  A helper, not a
test file.

  * a row's score is `oracle.dot_mfma`'s accumulator (the scan's own fma order) mapped (acc + 1) / 2 in float32;
  * entry (s, r) is better than (s', r') iff s > s', or s == s' and r < r' (r = global row index = base + position);
  * an identity's representative is its best row; the answer is the first k representatives;
  * NaN scores are never listed; empty slots are (-1.0, -1, -1)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle


def scores(q, rows):
    """[Q][G] float32 mapped scores, bit for bit the scan's."""
    q = np.ascontiguousarray(q, np.float32); rows = np.ascontiguousarray(rows, np.float32)
    out = np.empty((q.shape[0], rows.shape[0]), np.float32)
    if rows.shape[0] == 0:
        return out

    def one(i):                                               # (the C call releases the GIL: queries run side by side)
        out[i] = (oracle.dot_mfma(q[i], rows) + np.float32(1.0)) / np.float32(2.0)

    with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as pool:
        list(pool.map(one, range(q.shape[0])))
    return out


def topk_from_entries(s, r, d, k, per_id=None):
    """One query: entries (score, global row, id), any order, any number per id -> (scores[k], ids[k], rows[k]).
    per_id (optional): an upper bound of the entries one id has.  Only rows of the at most k - 1 identities ahead of it can be better
    than a listed representative, fewer than k * per_id rows, so the entries below the (k * per_id)-th best SCORE cannot be listed
    and are dropped before the sort (ties with that score all stay)."""
    os_, od, orow = np.full(k, -1.0, np.float32), np.full(k, -1, np.int32), np.full(k, -1, np.int32)
    keep = ~np.isnan(s) & (r >= 0)
    s, r, d = s[keep], r[keep], d[keep]
    if per_id is not None and len(s) > 2 * k * per_id:
        m = k * per_id
        keep = s >= np.partition(s, len(s) - m)[len(s) - m]
        s, r, d = s[keep], r[keep], d[keep]
    o = np.lexsort((r, -s.astype(np.float64)))               # best first (float32 -> float64 is exact and keeps the order)
    s, r, d = s[o], r[o], d[o]
    _, first = np.unique(d, return_index=True)               # an id's first occurrence in that order is its representative
    first = np.sort(first)[:k]
    n = len(first)
    os_[:n], od[:n], orow[:n] = s[first], d[first], r[first]
    return os_, od, orow


def topk_ids_from_scores(sc, ids, k, base=0):
    Q, G = sc.shape
    ids = np.asarray(ids, np.int32)
    r = (base + np.arange(G)).astype(np.int64)
    S, D, R = np.empty((Q, k), np.float32), np.empty((Q, k), np.int32), np.empty((Q, k), np.int32)
    per_id = int(np.unique(ids, return_counts=True)[1].max()) if G else 1
    for i in range(Q):
        S[i], D[i], R[i] = topk_from_entries(sc[i], r, ids, k, per_id)
    return S, D, R


def topk_ids(q, rows, ids, k, base=0):
    """(scores, ids, rows) [Q][k] of a labelled gallery."""
    return topk_ids_from_scores(scores(q, rows), ids, k, base)


def merge_ids(ps, pd, pr, k):
    """[W][Q][k] part lists (rows < 0 = empty slot, whatever its score) -> the identity top-k of their union."""
    W, Q, _ = ps.shape
    S, D, R = np.empty((Q, k), np.float32), np.empty((Q, k), np.int32), np.empty((Q, k), np.int32)
    for i in range(Q):
        S[i], D[i], R[i] = topk_from_entries(ps[:, i].reshape(-1), pr[:, i].reshape(-1).astype(np.int64), pd[:, i].reshape(-1), k)
    return S, D, R
