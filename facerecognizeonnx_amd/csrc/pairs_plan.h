// pairs_plan.h — the ONE definition of the pair audit behind fh_pairs_from_scores and fh_gallery_pairs_dev (the two new epilogues of
// gallery_cluster.hip and gallery_pairs.hip run the same rule on the pair pass's accumulators): WHICH genuine / impostor pairs lie on one
// side of a threshold, most extreme first.  Host code, no GPU, no HIP header: a stand-alone program can include it
// (tests/native/pairs_plan_sanitize.cpp); the per-pair test and the cut are also compiled for the device, behind FH_ROC_HD.
//   class     a pair (i, j), i < j, is genuine iff ids[i] == ids[j]; cls picks the genuine pairs, the impostor pairs or all of them.
//             Without ids only kPairsAny is legal.  Only the entries with i < j of scores[n][n] are read.
//   selected  the pair is in the class, its score is not a NaN, and it passes the side test in fp32: kPairsAbove `s > threshold` (the
//             strict test of labelling, clustering and range search), kPairsNotAbove `s <= threshold`.  A NaN-scored pair of the class is
//             selected by neither side and counted in `nan`: count(above) + count(not above) + nan = the class's pairs, at any threshold.
//   order     most extreme first: above = (score descending, i ascending, j ascending), not above = (score ascending, i, j); scores
//             compared as fp32 values.
//   the cut   selected pairs are binned by hist_bin (roc_plan.h); a bin's RANK is its distance from the extreme end (above: 2047 - bin,
//             not above: bin) and cum(r) = the selected pairs of rank <= r.  want = min(cap, count); r* = the first rank with
//             cum(r*) >= want.  cum(r*) <= room: returned = want, complete = 1.  Otherwise returned = cum(r* - 1) (< cap), complete = 0.
//             Either way the list is EXACTLY the first `returned` entries of the full ordered list (bins are monotone in the score), and
//             at most `room` pairs are ever held.  count == 0: returned = 0, complete = 1.
//   outputs   info[4] = {count (never clipped), nan, returned, complete}; out_scores [cap], out_rows [cap][2] (positions i < j),
//             out_ids [cap][2] (the two rows' ids; -1 when ids is null) — each may be null; slots behind `returned` are (-1.0f, -1, -1).
//   returns   `returned`, or -1 — nothing written — for n < 0, a null scores with n > 0, a null info, a NaN threshold, an unknown cls or
//             side, a class other than kPairsAny without ids, cap outside 1..kPairsMaxCap, room < cap.  All indexing in 64 bits.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "roc_plan.h"

namespace fh {

constexpr int kPairsGenuine = 0, kPairsImpostor = 1, kPairsAny = 2;
constexpr int kPairsAbove = 0, kPairsNotAbove = 1;
constexpr int kPairsMaxCap = 1024;

FH_ROC_HD inline bool pairs_in_class(int cls, int id_i, int id_j) { return cls == kPairsAny || (id_i == id_j) == (cls == kPairsGenuine); }

// the rank of a selected score's bin (0 = the extreme end), -1 for a score on the other side of the threshold, -2 for a NaN
FH_ROC_HD inline int pairs_rank(float s, int side, float threshold) {
    if (s != s) return -2;
    const bool above = s > threshold;
    if (above != (side == kPairsAbove)) return -1;
    const int b = hist_bin(s);
    return side == kPairsAbove ? kHistBins - 1 - b : b;
}

// is (s1, i1, j1) listed before (s2, i2, j2)?
FH_ROC_HD inline bool pairs_before(int side, float s1, int i1, int j1, float s2, int i2, int j2) {
    if (s1 != s2) return side == kPairsAbove ? s1 > s2 : s1 < s2;
    return i1 < i2 || (i1 == i2 && j1 < j2);
}

// The cut over by_rank[kHistBins] (selected pairs per rank): info[0], [2], [3] = count, returned, complete (info[1] is the caller's);
// returns the last rank to collect, -1 for none.
FH_ROC_HD inline int pairs_cut(const uint64_t* by_rank, int cap, uint64_t room, unsigned long long info[4]) {
    uint64_t count = 0;
    for (int r = 0; r < kHistBins; ++r) count += by_rank[r];
    const uint64_t want = count < (uint64_t)cap ? count : (uint64_t)cap;
    info[0] = count; info[2] = 0; info[3] = 1;
    if (count == 0) return -1;
    uint64_t cum = 0;
    for (int r = 0; r < kHistBins; ++r) {
        const uint64_t strict = cum;
        cum += by_rank[r];
        if (cum < want) continue;
        if (cum <= room) { info[2] = want; return r; }
        info[2] = strict; info[3] = 0;
        return r - 1;
    }
    return -1;                                                     // (not reached: cum ends at count >= want)
}

inline int pairs_from_scores(const float* scores, int n, const int* ids, int cls, int side, float threshold, int cap, long long room,
                             unsigned long long* info, float* out_scores, int* out_rows, int* out_ids) {
    if (n < 0 || (n > 0 && !scores) || !info || threshold != threshold) return -1;
    if ((cls != kPairsGenuine && cls != kPairsImpostor && cls != kPairsAny) || (side != kPairsAbove && side != kPairsNotAbove)) return -1;
    if ((cls != kPairsAny && !ids) || cap < 1 || cap > kPairsMaxCap || room < (long long)cap) return -1;
    const size_t N = (size_t)n;
    const auto rank_of = [&](size_t i, size_t j) {                  // -3: not in the class
        if (!pairs_in_class(cls, ids ? ids[i] : 0, ids ? ids[j] : 0)) return -3;
        return pairs_rank(scores[i * N + j], side, threshold);
    };
    std::vector<uint64_t> by_rank((size_t)kHistBins, 0);
    uint64_t nan = 0;
    for (size_t i = 0; i < N; ++i)
        for (size_t j = i + 1; j < N; ++j) {
            const int r = rank_of(i, j);
            if (r >= 0) ++by_rank[(size_t)r];
            else if (r == -2) ++nan;
        }
    unsigned long long res[4] = {0, nan, 0, 1};
    const int last = pairs_cut(by_rank.data(), cap, (uint64_t)room, res);
    struct Entry { float s; int i, j; };
    std::vector<Entry> cand;                                      // at most `room` entries by the cut
    if (last >= 0)
        for (size_t i = 0; i < N; ++i)
            for (size_t j = i + 1; j < N; ++j) {
                const int r = rank_of(i, j);
                if (r >= 0 && r <= last) cand.push_back(Entry{scores[i * N + j], (int)i, (int)j});
            }
    std::sort(cand.begin(), cand.end(), [&](const Entry& a, const Entry& b) { return pairs_before(side, a.s, a.i, a.j, b.s, b.i, b.j); });
    const size_t listed = (size_t)res[2];
    for (int k = 0; k < 4; ++k) info[k] = res[k];
    for (size_t k = 0; k < (size_t)cap; ++k) {
        const bool live = k < listed;
        if (out_scores) out_scores[k] = live ? cand[k].s : -1.0f;
        if (out_rows) { out_rows[2 * k] = live ? cand[k].i : -1; out_rows[2 * k + 1] = live ? cand[k].j : -1; }
        if (out_ids) {
            out_ids[2 * k] = live && ids ? ids[(size_t)cand[k].i] : -1;
            out_ids[2 * k + 1] = live && ids ? ids[(size_t)cand[k].j] : -1;
        }
    }
    return (int)listed;
}

}  // namespace fh
