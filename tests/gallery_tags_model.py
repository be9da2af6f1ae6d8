"""Exact numpy model of the tagged (watchlist) gallery queries (gallery_tags.hip).  A helper, not a test file.

Row r is admitted for query q iff (tags[r] & masks[q]) != 0; the answer of query q is the untagged answer on its admitted rows, every
row keeping its global index.  Scores come from tests/gallery_ids_model.scores (`oracle.dot_mfma`, the scan's own fma order); the
entries with (tag & mask) == 0 are dropped per query and the existing `topk_from_entries` rule is applied — for rows with every row
its own id, for identities with the rows' ids."""
import numpy as np

from tests import gallery_ids_model as ids_model

TAG_ALL = 0xFFFFFFFF

scores = ids_model.scores


def admitted(tags, masks):
    """[Q][G] bool."""
    tags = np.asarray(tags, np.uint32).reshape(-1); masks = np.asarray(masks, np.uint32).reshape(-1)
    return (tags[None, :] & masks[:, None]) != 0


def topk_ids_from_scores(sc, ids, tags, masks, k, base=0):
    """(scores, ids, rows) [Q][k]: the identity top-k over each query's admitted rows (an identity's representative is its best
    ADMITTED row)."""
    Q, G = sc.shape
    ids = np.asarray(ids, np.int32)
    adm = admitted(tags, masks)
    r = (base + np.arange(G)).astype(np.int64)
    S, D, R = np.empty((Q, k), np.float32), np.empty((Q, k), np.int32), np.empty((Q, k), np.int32)
    for i in range(Q):
        a = adm[i]
        S[i], D[i], R[i] = ids_model.topk_from_entries(sc[i][a], r[a], ids[a], k)
    return S, D, R


def topk_from_scores(sc, tags, masks, k, base=0):
    """(scores, rows) [Q][k]: the row top-k over each query's admitted rows."""
    G = sc.shape[1]
    S, _, R = topk_ids_from_scores(sc, np.arange(G, dtype=np.int32), tags, masks, k, base)
    return S, R


def topk(q, rows, tags, masks, k, base=0):
    return topk_from_scores(scores(q, rows), tags, masks, k, base)


def topk_ids(q, rows, ids, tags, masks, k, base=0):
    return topk_ids_from_scores(scores(q, rows), ids, tags, masks, k, base)


def label_from_scores(sc, tags, masks, thr, base=0, ids=None):
    """(labels, scores) [Q] of the label forms: the best admitted row (ids: its identity) when its score is strictly above thr, else
    -1; the score is the best admitted score, -1.0 when nothing is admitted."""
    S, R = topk_from_scores(sc, tags, masks, 1, base)
    s, r = S[:, 0], R[:, 0]
    ok = (r >= 0) & (s > np.float32(thr))
    lab = np.where(ok, r if ids is None else np.asarray(ids, np.int32)[np.maximum(r - base, 0)], -1).astype(np.int32)
    return lab, s
