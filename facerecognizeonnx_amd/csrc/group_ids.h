// group_ids.h — the ONE definition of how a labelled gallery's rows are grouped by identity (fh_gallery_group_ids, and through it
// fh_gallery_fuse_ids).  Host code, no GPU, no HIP header: a stand-alone program can include it (tests/native/group_ids_sanitize.cpp).
//   order[n]      row positions sorted by (id ascending, position ascending)
//   uniq[m]       the distinct ids, ascending
//   starts[m + 1] each identity's offset into order
// Returns m, or -1 for a negative id or n beyond the int positions `order` can hold.  Any output pointer may be null.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

namespace fh {

inline long long group_ids(const int* ids, long long n, int* order, long long* starts, int* uniq) {
    if (n < 0 || n > INT_MAX) return -1;
    if (n == 0) {
        if (starts) starts[0] = 0;
        return 0;
    }
    // one 64-bit key per row, id in the high half and position in the low half: a plain sort of the keys IS the (id, position) order
    std::vector<uint64_t> key((size_t)n);
    for (long long r = 0; r < n; ++r) {
        if (ids[r] < 0) return -1;
        key[(size_t)r] = ((uint64_t)(uint32_t)ids[r] << 32) | (uint32_t)r;
    }
    std::sort(key.begin(), key.end());
    long long m = 0;
    for (long long i = 0; i < n; ++i) {
        const int id = (int)(key[(size_t)i] >> 32);
        if (order) order[i] = (int)(uint32_t)key[(size_t)i];
        if (i == 0 || id != (int)(key[(size_t)i - 1] >> 32)) {
            if (uniq) uniq[m] = id;
            if (starts) starts[m] = i;
            ++m;
        }
    }
    if (starts) starts[m] = n;
    return m;
}

}  // namespace fh
