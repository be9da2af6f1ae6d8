// Stand-alone host program: fh::group_ids (csrc/group_ids.h, the grouping behind fh_gallery_group_ids / fh_gallery_fuse_ids) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/test_group_ids_sanitize.py builds and runs it).  Every output array is
// a heap block of EXACTLY the documented size (order[n], starts[m + 1], uniq[m]; m from a first call without outputs), so a write past
// any of them is a report; the results are checked against std::stable_sort.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/group_ids.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void one_case(const std::vector<int>& ids) {
    const long long n = (long long)ids.size();
    const long long m = fh::group_ids(ids.data(), n, nullptr, nullptr, nullptr);
    std::vector<int> want((size_t)n);
    std::iota(want.begin(), want.end(), 0);
    std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return ids[(size_t)a] < ids[(size_t)b]; });
    std::vector<int> u(ids);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    CHECK(m == (long long)u.size());
    if (m < 0) return;
    std::unique_ptr<int[]> order(new int[(size_t)n]), uniq(new int[(size_t)m]);
    std::unique_ptr<long long[]> starts(new long long[(size_t)m + 1]);
    CHECK(fh::group_ids(ids.data(), n, order.get(), starts.get(), uniq.get()) == m);
    CHECK(std::equal(want.begin(), want.end(), order.get()));
    CHECK(std::equal(u.begin(), u.end(), uniq.get()));
    CHECK(starts[0] == 0 && starts[(size_t)m] == n);
    for (long long j = 0; j < m; ++j)
        for (long long i = starts[(size_t)j]; i < starts[(size_t)j + 1]; ++i) CHECK(ids[(size_t)order[(size_t)i]] == uniq[(size_t)j]);
    // each output on its own
    CHECK(fh::group_ids(ids.data(), n, order.get(), nullptr, nullptr) == m);
    CHECK(fh::group_ids(ids.data(), n, nullptr, starts.get(), nullptr) == m);
    CHECK(fh::group_ids(ids.data(), n, nullptr, nullptr, uniq.get()) == m);
}

int main() {
    std::mt19937 rng(12345);
    one_case({});
    one_case({0});
    one_case({2147483647, 0, 2147483647, 0, 5});
    one_case(std::vector<int>(1000, 42));
    for (int rep = 0; rep < 200; ++rep) {
        const int n = 1 + (int)(rng() % 3000), span = 1 + (int)(rng() % (rep % 2 ? 20 : 2000000000));
        std::vector<int> ids((size_t)n);
        for (int& v : ids) v = (int)(rng() % (unsigned)span);
        one_case(ids);
    }
    {   // a negative id: -1, and nothing is written (the outputs here are too small to write to)
        std::vector<int> ids{4, 7, -1, 3};
        int o = 99, q = 99;
        long long s = 99;
        CHECK(fh::group_ids(ids.data(), 4, &o, &s, &q) == -1 && o == 99 && s == 99 && q == 99);
        CHECK(fh::group_ids(ids.data(), -1, nullptr, nullptr, nullptr) == -1);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
