"""Model of per-track identity with a watchlist per camera (fh_tracker_set_stream_masks): tests/track_ident_model.py — not edited —
driven with a stage B built on tests/gallery_tags_model.py.  Query e of a call belongs to the frame of its flagged entry, that frame
to a stream, and the stream's mask decides which gallery rows the query may match.  A helper, not a test file."""
import numpy as np

from tests import gallery_tags_model as tags_model


def query_masks(embed, stream_of, stream_masks, total=None):
    """uint32 [total]: the mask of every query, in the queries' order (flagged entries in (frame, position) order)."""
    embed = np.asarray(embed)
    n, per = embed.shape
    stream_of = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64)
    per_entry = np.repeat(np.asarray(stream_masks, np.uint32)[stream_of], per).reshape(n, per)
    m = per_entry[embed != 0]
    return m if total is None else m[:total]


def tagged_label_fn(rows, tags, qmasks, threshold, ids=None, base=0):
    """label_fn(queries) -> (labels, scores): the tagged label call on float32 queries, exact (the scan's own scores)."""
    def label_fn(q):
        q = np.ascontiguousarray(q, np.float32)
        return tags_model.label_from_scores(tags_model.scores(q, rows), tags, qmasks[:len(q)], threshold, base, ids)
    return label_fn


def identify(model, track, slot, embed, emb, rows, tags, stream_masks, threshold, ids=None, base=0, total=None, stream_of=None,
             queries=None):
    """Stages A, B (tagged, per-stream masks) and C on a tests.track_ident_model.IdentTracker.  queries (optional, float32
    [total][dim]): label these instead of the model's own float64 queries — the device's, so that scores are held to their bits.
    Returns (label, score, queries64, verbatim, query masks)."""
    q64, verbatim = model.pool_queries(track, slot, embed, emb, total, stream_of)
    qm = query_masks(embed, stream_of, stream_masks, len(q64))
    q = q64 if queries is None else queries
    fn = tagged_label_fn(rows, tags, qm, threshold, ids, base)
    labels, scores = fn(q) if len(q) else (np.zeros(0, np.int32), np.zeros(0, np.float32))
    out_l, out_s = model.carry(track, slot, embed, labels, scores, total, stream_of)
    return out_l, out_s, q64, verbatim, qm
