// deep_plan.h — the ONE definition of the deep top-k (1 <= k <= 1024 entries per query, no threshold) behind fh_topk_from_scores and
// fh_gallery_topk_deep_dev, and of the BLOCK RULE that bounds the device call's work (gallery_deep.hip runs the same rule on the scan's
// accumulators).  Host code, no GPU, no HIP header: a stand-alone program can include it (tests/native/deep_plan_sanitize.cpp).
//   eligible   row r (r < n) of one query's mapped scores is eligible iff
//                * it is admitted: (tag[r] & mask) != 0, where tag[r] = tags ? tags[r] : kRangeTagAll (a gallery without tags);
//                * scores[r] is not a NaN;
//                * scores[r] > -inf.
//   list       the best min(k, #eligible) rows, ranked by (score descending, global index ascending) with global index = index_base + r,
//              go to out_scores / out_indices [k] (either may be null); the slots behind them are (-1.0f, -1).
//              This is BY DEFINITION the list part of range_from_scores(threshold = -inf, cap = k) (range_plan.h): "above -inf and
//              not a NaN" is that rule's hit test, and topk_from_scores below is written as that call, so the two cannot drift apart.
//   returns    the number listed, or -1 — nothing written — for n < 0, a null scores with n > 0, k outside 1..kDeepMaxK, or a global
//              index that does not fit in 31 bits.
//
// The block rule.  Rows are cut into blocks of kDeepBlock = 32 by POSITION (block b = rows 32 b .. 32 b + 31).  m_b = the maximum eligible
// score of block b, -inf if it has no eligible row.  The CHOSEN blocks of a query are the first min(k, #blocks with m_b > -inf) blocks in
// the order (m_b descending, block index ascending).
//   Claim: every entry of the exact top-k lies in a chosen block.
//   Proof: let r be a top-k row in an unchosen block b.  r is eligible, so m_b >= score(r) > -inf: b was a candidate and was not chosen,
//   hence k chosen blocks precede b in the order.  For each of them, c, take its lowest-index row r_c attaining m_c.  Either m_c > m_b >=
//   score(r): r_c is strictly better scored than r.  Or m_c == m_b and c < b: then score(r_c) = m_b >= score(r) and r_c lies in an earlier
//   block, hence at a lower index, so r_c ranks ahead of r in either case of that comparison.  The r_c are k distinct eligible rows (one per
//   block) that all rank ahead of r: r is not in the top k.  Contradiction.
//   Consequence: the top-k of the rows of the chosen blocks — at most 32 k rows, whatever the data — IS the top-k of the gallery.  Ties and
//   duplicates are covered: the proof uses nothing but the total order (score descending, index ascending).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "range_plan.h"

namespace fh {

constexpr int kDeepMaxK = 1024;
constexpr int kDeepBlock = 32;
static_assert(kDeepMaxK == kRangeMaxCap, "a deep list is a range list with the threshold at -inf");

inline bool deep_eligible(float score, uint32_t tag, uint32_t mask) { return (tag & mask) != 0 && score > -INFINITY; }   // (false for a NaN)

inline int topk_from_scores(const float* scores, long long n, long long index_base, const uint32_t* tags, uint32_t mask, int k, float* out_scores,
                            int* out_indices) {
    long long count = 0;
    return range_from_scores(scores, n, index_base, tags, mask, -INFINITY, k, &count, out_scores, out_indices);
}

// The chosen blocks of one query, in the rule's order, into *blocks (block indices by position); returns their number (<= k), or -1 —
// *blocks untouched — for the arguments topk_from_scores refuses (no index base here: block indices are positions).
inline int deep_chosen_blocks(const float* scores, long long n, const uint32_t* tags, uint32_t mask, int k, std::vector<long long>* blocks) {
    if (n < 0 || (n > 0 && !scores) || k < 1 || k > kDeepMaxK || !blocks) return -1;
    typedef std::pair<float, long long> Entry;
    const auto better = [](const Entry& a, const Entry& b) { return range_better(a.first, a.second, b.first, b.second); };
    std::vector<Entry> best;                                  // at most 2 k entries: cut back to the best k whenever it fills
    best.reserve(2 * (size_t)k);
    for (long long b = 0; b * kDeepBlock < n; ++b) {
        float m = -INFINITY;
        const long long r1 = std::min<long long>(n, (b + 1) * kDeepBlock);
        for (long long r = b * kDeepBlock; r < r1; ++r)
            if (deep_eligible(scores[r], tags ? tags[r] : kRangeTagAll, mask) && scores[r] > m) m = scores[r];
        if (!(m > -INFINITY)) continue;
        best.push_back(Entry(m, b));
        if (best.size() == 2 * (size_t)k) {
            std::nth_element(best.begin(), best.begin() + k, best.end(), better);
            best.resize((size_t)k);
        }
    }
    std::sort(best.begin(), best.end(), better);
    if (best.size() > (size_t)k) best.resize((size_t)k);
    blocks->clear();
    for (const Entry& e : best) blocks->push_back(e.second);
    return (int)best.size();
}

// What the device call computes: the top-k of the rows of the chosen blocks only.  By the claim above it equals topk_from_scores; the
// tests hold the two against each other.  Same arguments, outputs and returns as topk_from_scores.
inline int topk_from_chosen_blocks(const float* scores, long long n, long long index_base, const uint32_t* tags, uint32_t mask, int k,
                                   float* out_scores, int* out_indices) {
    if (index_base < 0 || index_base > (long long)INT_MAX - std::max<long long>(n, 0)) return -1;
    std::vector<long long> blocks;
    if (deep_chosen_blocks(scores, n, tags, mask, k, &blocks) < 0) return -1;
    typedef std::pair<float, long long> Entry;
    std::vector<Entry> best;
    for (long long b : blocks) {
        const long long r1 = std::min<long long>(n, (b + 1) * kDeepBlock);
        for (long long r = b * kDeepBlock; r < r1; ++r)
            if (deep_eligible(scores[r], tags ? tags[r] : kRangeTagAll, mask)) best.push_back(Entry(scores[r], index_base + r));
    }
    std::sort(best.begin(), best.end(), [](const Entry& a, const Entry& b) { return range_better(a.first, a.second, b.first, b.second); });
    const int listed = (int)std::min<size_t>(best.size(), (size_t)k);
    for (int i = 0; i < k; ++i) {
        if (out_scores) out_scores[i] = i < listed ? best[(size_t)i].first : -1.0f;
        if (out_indices) out_indices[i] = i < listed ? (int)best[(size_t)i].second : -1;
    }
    return listed;
}

}  // namespace fh
