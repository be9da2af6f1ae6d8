// cluster_plan.h — the ONE definition of how rows are clustered from their pairwise scores (fh_cluster_scores, and through it the
// contract of fh_gallery_cluster_dev): exact DBSCAN over the graph "score above the threshold".  Host code, no GPU, no HIP header: a
// stand-alone program can include it (tests/native/cluster_plan_sanitize.cpp).
//   edge     (i, j), i != j, iff s(i, j) > threshold — strict, in fp32 (a NaN score or threshold: no edge).  Only the entries with i < j
//            are read: the matrix is taken as symmetric, the diagonal and the lower triangle are never touched.
//   core     deg(i) + 1 >= min_pts (a row counts itself; min_pts == 1: every row, i.e. single linkage)
//   cluster  a connected component of the core rows under core-core edges; its label is its smallest core position
//   border   a non-core row with a core neighbour takes the label of its best one (higher score, then lower position: gal_better);
//            border rows never link clusters
//   noise    the rest: label -1 (noise == 0) or the row's own position (noise == 1; no collision: a cluster's label is a core row)
//   info[4]  {clusters, core rows, border rows, noise rows} (may be null)
// Returns the number of clusters, or -1 — nothing written — for n < 0, min_pts < 1, an unknown noise mode, or a null scores / labels
// with n > 0.  Three passes over the upper triangle and 12 bytes per row of scratch; all indexing in 64 bits.
#pragma once
#include <cstddef>
#include <vector>

namespace fh {

constexpr int kClusterNoiseNone = 0, kClusterNoiseSelf = 1;

inline int cluster_scores(const float* scores, int n, float threshold, int min_pts, int noise, int* labels, int* info) {
    if (n < 0 || min_pts < 1 || (noise != kClusterNoiseNone && noise != kClusterNoiseSelf)) return -1;
    if (n > 0 && (!scores || !labels)) return -1;
    const size_t N = (size_t)n;
    auto at = [&](size_t i, size_t j) { return scores[i * N + j]; };
    std::vector<int> deg(N, 0), parent(N), best(N, -1);
    std::vector<float> best_s(N, 0.f);
    for (size_t i = 0; i < N; ++i) {
        parent[i] = (int)i;
        for (size_t j = i + 1; j < N; ++j)
            if (at(i, j) > threshold) { ++deg[i]; ++deg[j]; }
    }
    auto core = [&](size_t i) { return (long long)deg[i] + 1 >= (long long)min_pts; };
    auto find = [&](int x) {
        while (parent[(size_t)x] != x) {
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    };
    // a border row's candidate (s, c) replaces the one it holds iff it is better: higher score, then lower position
    auto offer = [&](size_t b, float s, size_t c) {
        if (best[b] < 0 || s > best_s[b] || (s == best_s[b] && (int)c < best[b])) { best[b] = (int)c; best_s[b] = s; }
    };
    for (size_t i = 0; i < N; ++i)
        for (size_t j = i + 1; j < N; ++j) {
            if (!(at(i, j) > threshold)) continue;
            const bool ci = core(i), cj = core(j);
            if (ci && cj) {
                const int a = find((int)i), b = find((int)j);                // the smaller root stays a root: a component's root is its minimum
                if (a < b) parent[(size_t)b] = a;
                else if (b < a) parent[(size_t)a] = b;
            } else if (ci) {
                offer(j, at(i, j), i);
            } else if (cj) {
                offer(i, at(i, j), j);
            }
        }
    int cnt[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < N; ++i) {
        if (core(i)) {
            labels[i] = find((int)i);
            ++cnt[1];
            if (labels[i] == (int)i) ++cnt[0];
        } else if (best[i] >= 0) {
            labels[i] = find(best[i]);
            ++cnt[2];
        } else {
            labels[i] = noise == kClusterNoiseSelf ? (int)i : -1;
            ++cnt[3];
        }
    }
    if (info)
        for (int k = 0; k < 4; ++k) info[k] = cnt[k];
    return cnt[0];
}

}  // namespace fh
