"""Plain Python-int / numpy model of the score histogram's bin rule and of the ROC read-out (csrc/roc_plan.h: fh_hist_bin,
fh_roc_from_hist, and the histogram epilogue behind fh_gallery_pair_hist_dev).  A helper, not a test file, and written independently of
the header: the bin comes from comparing the score with the exact edges b/2048 in float64, not from a ceil.

  * bin b holds b/2048 < s <= (b+1)/2048; bin 0 also everything at or below 1/2048, bin 2047 everything above 2047/2048; a NaN has no bin
    (-1);
  * A[b] = sum of h[b'] over b' >= b;  N = A[0];
  * operating point of max_far: the smallest b in 1..2047 with A_i[b] <= floor(max_far * float(N_i));
  * equal-error point: the smallest b in 1..2047 with A_i[b] * N_g <= (N_g - A_g[b]) * N_i (Python ints: exact);
  * a point is (threshold float32, bin, true_accepts, false_accepts, genuine, impostor); no such b: (1.0, -1, 0, 0, N_g, N_i);
  * None for N_g == 0, N_i == 0, or max_far outside [0, 1] / NaN."""
import math

import numpy as np

BINS = 2048
EDGES = np.arange(1, BINS, dtype=np.float64) / BINS            # 1/2048 .. 2047/2048: the lower edges of bins 1..2047, exact


def bins(scores):
    """int64 bins of an array of float32 scores (-1 for NaN): the number of edges strictly below the score."""
    s = np.asarray(scores, np.float32).reshape(-1).view(np.float32)
    with np.errstate(invalid="ignore"):                           # (a signalling NaN among the inputs)
        s = s.astype(np.float64)
    b = np.searchsorted(EDGES, s, side="left").astype(np.int64)      # edges e with e < s
    b[np.isnan(s)] = -1
    return b


def bin_of(score):
    return int(bins([score])[0])


def hist_from_scores(scores, genuine):
    """(hist [2][BINS] of Python-int-exact uint64, nan [2]) of scores with a boolean class mask (True = genuine)."""
    b = bins(scores)
    g = np.asarray(genuine, bool).reshape(-1)
    hist = np.zeros((2, BINS), np.uint64)
    nan = np.zeros(2, np.uint64)
    for plane, m in ((0, g), (1, ~g)):
        bb = b[m]
        nan[plane] = np.uint64((bb < 0).sum())
        hist[plane] = np.bincount(bb[bb >= 0], minlength=BINS).astype(np.uint64)
    return hist, nan


def pair_hist(S, ids):
    """The model of fh_gallery_pair_hist_dev: S = the [G][G] score matrix (its upper triangle is read), ids [G]."""
    S = np.asarray(S, np.float32)
    ids = np.asarray(ids)
    iu = np.triu_indices(len(ids), 1)
    return hist_from_scores(S[iu], ids[iu[0]] == ids[iu[1]])


def roc(hist, max_far):
    hg = [int(x) for x in np.asarray(hist)[0]]
    hi = [int(x) for x in np.asarray(hist)[1]]
    n_g, n_i = sum(hg), sum(hi)
    if n_g == 0 or n_i == 0 or not (0.0 <= max_far <= 1.0):
        return None
    allowed = int(math.floor(max_far * float(n_i)))
    a_g = [0] * (BINS + 1)
    a_i = [0] * (BINS + 1)
    for b in range(BINS - 1, -1, -1):
        a_g[b] = a_g[b + 1] + hg[b]
        a_i[b] = a_i[b + 1] + hi[b]

    def point(ok):
        for b in range(1, BINS):
            if ok(b):
                return (np.float32(b / BINS), b, a_g[b], a_i[b], n_g, n_i)
        return (np.float32(1.0), -1, 0, 0, n_g, n_i)

    return point(lambda b: a_i[b] <= allowed), point(lambda b: a_i[b] * n_g <= (n_g - a_g[b]) * n_i)
