"""Plain numpy restatement of the clustering rule (csrc/cluster_plan.h, fh_cluster_scores, fh_gallery_cluster_dev) from a score matrix.  A
helper, not a test file; it never calls the library.

  * edge (i, j), i < j, iff s[i, j] > thr, compared in float32 (NaN on either side: no edge); only the upper triangle is read;
  * core iff degree + 1 >= min_pts;
  * a cluster = a connected component (breadth-first search) of the core rows under core-core edges, labelled by its smallest position;
  * a non-core row with a core neighbour takes the label of the best one: higher score, then lower position;
  * the rest is noise: -1 ("none" / 0) or the row's own position ("self" / 1);
  * info = (clusters, core rows, border rows, noise rows)."""
from collections import deque

import numpy as np

NOISE = {"none": 0, "self": 1, 0: 0, 1: 1}


def adjacency(scores, thr):
    s = np.asarray(scores, np.float32)
    n = s.shape[0]
    with np.errstate(invalid="ignore"):
        up = np.triu(s > np.float32(thr), 1) if n else np.zeros((0, 0), bool)
    return up | up.T


def cluster(scores, thr, min_pts=1, noise="none"):
    """(labels int32[n], info int32[4])."""
    s = np.asarray(scores, np.float32)
    n = s.shape[0]
    adj = adjacency(s, thr)
    sym = np.triu(s, 1) + np.triu(s, 1).T if n else s           # the value of a pair is its upper-triangle entry
    core = adj.sum(1) + 1 >= min_pts
    labels = np.full(n, -2, np.int32)
    clusters = 0
    for seed in range(n):                                       # ascending: a component is first met at its smallest position
        if not core[seed] or labels[seed] != -2:
            continue
        clusters += 1
        labels[seed] = seed
        todo = deque([seed])
        while todo:
            i = todo.popleft()
            for j in np.flatnonzero(adj[i] & core & (labels == -2)):
                labels[j] = seed
                todo.append(j)
    border = 0
    for i in np.flatnonzero(~core):
        nb = np.flatnonzero(adj[i] & core)
        if len(nb):
            sc = sym[i, nb]
            labels[i] = labels[nb[sc == sc.max()].min()]        # (edge scores are never NaN)
            border += 1
        else:
            labels[i] = i if NOISE[noise] else -1
    info = np.array([clusters, int(core.sum()), border, n - int(core.sum()) - border], np.int32)
    return labels, info


def kinds(scores, thr, min_pts):
    """(core, border, noise) boolean masks — for the tests' claims about what a crafted case contains."""
    adj = adjacency(scores, thr)
    core = adj.sum(1) + 1 >= min_pts
    border = ~core & (adj & core[None, :]).any(1)
    return core, border, ~core & ~border
