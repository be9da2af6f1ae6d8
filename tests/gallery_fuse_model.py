"""Numpy restatement of template pooling (fh_gallery_fuse_ids, gallery_fuse.hip) and the inputs its tests share.  A helper, not a test
file.

  * grouping: rows sorted by (id ascending, position ascending) — a stable argsort by id; the fused gallery lists the ids ascending;
  * an identity of one template keeps that row verbatim, in both modes;
  * otherwise the identity's rows, in that order, are cut into chunks of CHUNK = 512 rows; a chunk is summed sequentially from its first
    row (p = row0; p = p + row1; ...) in float32, and the chunk partials are added sequentially in chunk order;
  * "sum" is that sum; "unit" divides it by sqrt(sum s^2) when that is > 0 and leaves it as it is otherwise — computed here in float64
    from the exact float32 sum, so the GPU's float32 normalisation is held to a tolerance, the sums to their bits."""
import numpy as np

CHUNK = 512


def group(ids):
    """(order, starts, uniq): what fh_gallery_group_ids defines."""
    ids = np.asarray(ids, np.int32).reshape(-1)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    uniq, counts = np.unique(ids, return_counts=True)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return order, starts, uniq.astype(np.int32)


def seq_sum(rows):
    """[T][dim] float32 -> row 0 + row 1 + ... strictly in that order, float32 adds vectorised over the columns."""
    p = rows[0].astype(np.float32, copy=True)
    for r in rows[1:]:
        p = p + r
    return p


def plain_sums(rows, ids):
    """The order the contract does NOT use: each identity's rows added sequentially without chunking."""
    order, starts, uniq = group(ids)
    return np.stack([seq_sum(rows[order[a:b]]) for a, b in zip(starts[:-1], starts[1:])]), uniq


def fuse_sums(rows, ids, chunk=CHUNK):
    """(sums [m][dim] float32, uniq [m], counts [m]) of FH_FUSE_SUM, bit for bit."""
    rows = np.ascontiguousarray(rows, np.float32)
    order, starts, uniq = group(ids)
    out = np.empty((len(uniq), rows.shape[1]), np.float32)
    for j, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
        idx = order[a:b]
        parts = [seq_sum(rows[idx[c:c + chunk]]) for c in range(0, len(idx), chunk)]
        out[j] = seq_sum(np.stack(parts))
    return out, uniq, np.diff(starts)


def unit64(sums, counts):
    """FH_FUSE_UNIT in float64 from the exact float32 sums; a one-template identity's row is not touched."""
    s = sums.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt((s * s).sum(1, keepdims=True))
        scale = (norm > 0) & (np.asarray(counts).reshape(-1, 1) > 1)
        return np.where(scale, s / np.where(scale, norm, 1.0), s)


def unit32(sums, counts):
    """The same in plain float32 numpy: what a float32 implementation may return."""
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt((sums * sums).sum(1, dtype=np.float32, keepdims=True))
        scale = (norm > 0) & (np.asarray(counts).reshape(-1, 1) > 1)
        return np.where(scale, sums / np.where(scale, norm, np.float32(1.0)), sums).astype(np.float32)


def unit_tolerance(dim):
    """Relative, per element: an fp32 sum of dim non-negative terms is within dim * 2^-24 of the exact one in any order, the square root
    halves that, and 8 ulps remain for sqrtf, the division and an rsqrt if one is used."""
    return (dim / 2 + 8) * 2.0 ** -24


def within_unit_tolerance(got, want64, dim):
    got = got.astype(np.float64)
    ok = np.abs(got - want64) <= unit_tolerance(dim) * np.abs(want64)
    return ok | (np.isnan(got) & np.isnan(want64))


# ------------------------------------------------------------------------------------------ shared inputs
def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def clustered_case(dim, G=5000, noise=0.05):
    """1 to 40 templates per identity (a centre plus noise, L2-normalised), rows shuffled, sparse unsorted ids; G rows in all.
    Returns (rows, ids, centres, labels): centres[i] belongs to labels[i]."""
    rng = np.random.default_rng(7000 + dim)
    per = [1, 1, 40]                                           # both ends of the range are there, whatever the draw
    while sum(per) < G:
        per.append(int(rng.integers(1, 41)))
    per[-1] -= sum(per) - G                                    # the last identity takes what is left (>= 1)
    per = np.array(per)
    assert per.min() >= 1 and per.max() <= 40 and per.sum() == G
    n_ids = len(per)
    labels = (rng.permutation(10 * n_ids)[:n_ids] * 7 + 3).astype(np.int32)
    centres = unit_rows(rng, n_ids, dim)
    rows = np.repeat(centres, per, axis=0) + np.float32(noise) * rng.standard_normal((G, dim), dtype=np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = np.repeat(labels, per)
    o = rng.permutation(G)
    return np.ascontiguousarray(rows[o], np.float32), np.ascontiguousarray(ids[o]), centres, labels


SKEW_SEED = 5


def skew_case(seed=SKEW_SEED, dim=64):
    """Identities of 512, 513 and 1 300 rows among small ones (1 to 6 rows), shuffled.  Rows are NOT clustered: with random signs the
    partial sums round differently in the chunked and in the plain order."""
    rng = np.random.default_rng(seed)
    per = np.concatenate([[512, 513, 1300], rng.integers(1, 7, 60)])
    labels = (rng.permutation(1000)[:len(per)] * 5 + 1).astype(np.int32)
    G = int(per.sum())
    rows = unit_rows(rng, G, dim)
    ids = np.repeat(labels, per)
    o = rng.permutation(G)
    return np.ascontiguousarray(rows[o], np.float32), np.ascontiguousarray(ids[o]), labels[:3]
