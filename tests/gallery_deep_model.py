"""Exact numpy model of the gallery's deep top-k (fh_gallery_topk_deep_dev, fh_topk_from_scores).  A helper, not a test file.

  * the lists are BY DEFINITION the list part of the threshold search at threshold -inf with cap = k (tests/gallery_range_model.py): a row
    is eligible iff it is admitted, its score is not a NaN and is > -inf; the best min(k, eligible) rows, (score desc, global row asc),
    and (-1.0, -1, -1) behind them;
  * the block rule (csrc/deep_plan.h), restated: rows in blocks of 32 by position, m_b = the best eligible score of block b (-inf if
    none), the chosen blocks = the first min(k, #blocks with m_b > -inf) blocks by (m_b desc, b asc)."""
import numpy as np

from tests import gallery_range_model as rmodel
from tests.gallery_range_model import scores  # noqa: F401  (re-exported)

BLOCK = 32
NEG_INF = np.float32(-np.inf)


def topk_from_scores(sc, k, base=0, tags=None, masks=None, ids=None):
    """sc [Q][G] -> (None, scores [Q][k], rows [Q][k], ids [Q][k] or None): the range model's tuple with its counts dropped, so that it
    compares against a (None, s, i, d) of the device call."""
    return (None,) + rmodel.range_from_scores(sc, NEG_INF, k, base, tags, masks, ids)[1:]


def listed(sc, tags=None, masks=None):
    """[Q] the number of eligible rows of every query (the list holds min(k, that))."""
    return rmodel.hits(sc, NEG_INF, tags, masks).sum(1)


def eligible(s, tags=None, mask=rmodel.TAG_ALL):
    """One query's scores [n] -> [n] bool."""
    t = np.full(s.shape[0], rmodel.TAG_ALL, np.uint32) if tags is None else np.asarray(tags, np.uint32)
    return ((t & np.uint32(mask)) != 0) & (s > NEG_INF)       # (False for a NaN)


def chosen_blocks(s, k, tags=None, mask=rmodel.TAG_ALL):
    """One query's scores [n] -> the chosen blocks (positions), best first."""
    n = s.shape[0]
    nb = (n + BLOCK - 1) // BLOCK
    v = np.full(nb * BLOCK, NEG_INF, np.float32)
    v[:n] = np.where(eligible(s, tags, mask), s, NEG_INF)
    m = v.reshape(nb, BLOCK).max(1) if nb else np.zeros(0, np.float32)
    cand = np.flatnonzero(m > NEG_INF)
    o = np.lexsort((cand, -m[cand].astype(np.float64)))[:k]
    return cand[o]


def topk_of_blocks(s, blocks, k, base=0, tags=None, mask=rmodel.TAG_ALL):
    """The top-k over the rows of `blocks` only: (scores [k], rows [k])."""
    n = s.shape[0]
    hit = np.zeros(n, bool)
    for b in blocks:
        hit[b * BLOCK:min(n, (b + 1) * BLOCK)] = True
    hit &= eligible(s, tags, mask)
    _, S, R, _ = rmodel.one_query(s, hit, k, base)
    return S, R
