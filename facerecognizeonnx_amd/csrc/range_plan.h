// range_plan.h — the ONE definition of the threshold (range) search rule behind fh_range_from_scores and fh_gallery_range_dev
// (gallery_range.hip runs the same rule on the scan's accumulators).  Host code, no GPU, no HIP header: a stand-alone program can include
// it (tests/native/range_plan_sanitize.cpp).
//   hit      row r (r < n) of one query's mapped scores is a hit iff
//              * it is admitted: (tag[r] & mask) != 0, where tag[r] = tags ? tags[r] : kRangeTagAll (a gallery without tags) — the
//                unmasked device call is tags == nullptr with mask == kRangeTagAll;
//              * scores[r] > threshold, compared in fp32 (the strict test of fh_gallery_label_dev and of the clustering);
//              * scores[r] is not a NaN (the comparison is false for one).
//   count    *count = the exact number of hits, never clipped by cap.
//   lists    the best min(*count, cap) hits, ranked by (score descending, global index ascending) with global index = index_base + r, go
//            to out_scores / out_indices [cap] (either may be null); the slots behind them are (-1.0f, -1).  Nothing else is written.
//   returns  the number of entries listed, or -1 — nothing written — for n < 0, a null scores with n > 0, a null count, a NaN threshold,
//            cap outside 1..kRangeMaxCap, or a global index that does not fit in 31 bits.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <utility>
#include <vector>

namespace fh {

constexpr int kRangeMaxCap = 1024;
constexpr uint32_t kRangeTagAll = 0xFFFFFFFFu;

inline bool range_better(float s1, long long i1, float s2, long long i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

inline int range_from_scores(const float* scores, long long n, long long index_base, const uint32_t* tags, uint32_t mask, float threshold, int cap,
                             long long* count, float* out_scores, int* out_indices) {
    if (n < 0 || (n > 0 && !scores) || !count || threshold != threshold || cap < 1 || cap > kRangeMaxCap) return -1;
    if (index_base < 0 || index_base > (long long)INT_MAX - n) return -1;
    typedef std::pair<float, long long> Entry;
    const auto better = [](const Entry& a, const Entry& b) { return range_better(a.first, a.second, b.first, b.second); };
    std::vector<Entry> best;                                  // at most 2 * cap entries: cut back to the best cap whenever it fills
    best.reserve(2 * (size_t)cap);
    long long hits = 0;
    for (long long r = 0; r < n; ++r) {
        const uint32_t tag = tags ? tags[r] : kRangeTagAll;
        if ((tag & mask) == 0 || !(scores[r] > threshold)) continue;
        ++hits;
        best.push_back(Entry(scores[r], index_base + r));
        if (best.size() == 2 * (size_t)cap) {
            std::nth_element(best.begin(), best.begin() + cap, best.end(), better);
            best.resize((size_t)cap);
        }
    }
    std::sort(best.begin(), best.end(), better);
    const int listed = (int)std::min<long long>((long long)best.size(), cap);
    *count = hits;
    for (int i = 0; i < cap; ++i) {
        if (out_scores) out_scores[i] = i < listed ? best[(size_t)i].first : -1.0f;
        if (out_indices) out_indices[i] = i < listed ? (int)best[(size_t)i].second : -1;
    }
    return listed;
}

}  // namespace fh
