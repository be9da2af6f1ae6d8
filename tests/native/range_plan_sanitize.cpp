// Stand-alone host program: fh::range_from_scores (csrc/range_plan.h, the rule behind fh_range_from_scores and fh_gallery_range_dev) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/test_range_plan_sanitize.py builds and runs it).  Scores, tags and both
// output lists are heap blocks of EXACTLY n and cap elements, so a read or write past either is a report; the results are checked
// against a restatement that sorts every hit.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/range_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// runs the rule into exactly sized outputs and holds it to the restatement; returns the count
static long long one_case(const std::vector<float>& sc, long long base, const std::vector<uint32_t>* tags, uint32_t mask, float thr, int cap) {
    const long long n = (long long)sc.size();
    std::unique_ptr<float[]> s(new float[(size_t)n]);                    // exactly n (n == 0: a zero-length block)
    std::unique_ptr<uint32_t[]> t(tags ? new uint32_t[(size_t)n] : nullptr);
    for (long long r = 0; r < n; ++r) { s[(size_t)r] = sc[(size_t)r]; if (tags) t[(size_t)r] = (*tags)[(size_t)r]; }
    std::unique_ptr<float[]> os(new float[(size_t)cap]);
    std::unique_ptr<int[]> oi(new int[(size_t)cap]);
    long long count = -7;
    const int listed = fh::range_from_scores(s.get(), n, base, t.get(), mask, thr, cap, &count, os.get(), oi.get());
    struct E { float s; long long i; };
    std::vector<E> hits;
    for (long long r = 0; r < n; ++r) {
        const uint32_t tg = tags ? (*tags)[(size_t)r] : 0xFFFFFFFFu;
        if ((tg & mask) != 0 && !std::isnan(sc[(size_t)r]) && sc[(size_t)r] > thr) hits.push_back({sc[(size_t)r], base + r});
    }
    std::stable_sort(hits.begin(), hits.end(), [](const E& a, const E& b) { return a.s > b.s; });      // (pushed in index order: ties keep it)
    CHECK(count == (long long)hits.size());
    CHECK(listed == (int)std::min<size_t>(hits.size(), (size_t)cap));
    for (int k = 0; k < cap; ++k) {
        if (k < listed) CHECK(fbits(os[(size_t)k]) == fbits(hits[(size_t)k].s) && oi[(size_t)k] == (int)hits[(size_t)k].i);
        else CHECK(os[(size_t)k] == -1.0f && oi[(size_t)k] == -1);
    }
    // either list may be null: the same count, the other list the same bytes
    std::unique_ptr<float[]> os2(new float[(size_t)cap]);
    std::unique_ptr<int[]> oi2(new int[(size_t)cap]);
    long long c2 = -7, c3 = -7, c4 = -7;
    CHECK(fh::range_from_scores(s.get(), n, base, t.get(), mask, thr, cap, &c2, os2.get(), nullptr) == listed && c2 == count);
    CHECK(fh::range_from_scores(s.get(), n, base, t.get(), mask, thr, cap, &c3, nullptr, oi2.get()) == listed && c3 == count);
    CHECK(fh::range_from_scores(s.get(), n, base, t.get(), mask, thr, cap, &c4, nullptr, nullptr) == listed && c4 == count);
    CHECK(std::memcmp(os.get(), os2.get(), (size_t)cap * sizeof(float)) == 0 && std::memcmp(oi.get(), oi2.get(), (size_t)cap * sizeof(int)) == 0);
    return count;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::mt19937 rng(91);
    std::uniform_real_distribution<float> u(-0.1f, 1.1f);
    // ---- random scores with NaNs, infinities and many equal values; every cap regime; with and without tags
    for (int rep = 0; rep < 300; ++rep) {
        const long long n = rep < 10 ? rep : (long long)(rng() % 6000u);
        std::vector<float> sc((size_t)n);
        for (auto& x : sc) x = u(rng);
        for (long long k = 0; k < n / 5; ++k) sc[(size_t)(rng() % (unsigned)n)] = sc[(size_t)(rng() % (unsigned)n)];
        for (long long k = 0; k < n / 20; ++k) sc[(size_t)(rng() % (unsigned)n)] = k % 3 == 0 ? nan : k % 3 == 1 ? inf : -inf;
        std::vector<uint32_t> tags((size_t)n);
        for (auto& x : tags) x = rng() % 10u == 0 ? 0u : (1u << (rng() % 8u)) | (rng() % 8u == 0 ? 0x80000000u : 0u);
        const int caps[] = {1, 2, 8, 100, 1023, 1024};
        const float thrs[] = {0.0f, 0.5f, 0.9f, 1.05f, -1.0f, -inf, inf, n ? sc[(size_t)(rng() % (unsigned)n)] : 0.3f};
        const uint32_t masks[] = {0xFFFFFFFFu, 1u, 6u, 0x80000000u, 0u, 1u << 20};
        const int cap = caps[rep % 6];
        const float thr = thrs[rep % 8];
        const long long base = rep % 4 == 0 ? 0 : (long long)(rng() % 1000000u);
        one_case(sc, base, nullptr, 0xFFFFFFFFu, thr, cap);
        one_case(sc, base, &tags, masks[rep % 6], thr, cap);
        one_case(sc, base, nullptr, masks[(rep + 3) % 6], thr, cap);
    }
    {   // the strict test at a score, and one float below it
        std::vector<float> sc = {0.25f, 0.75f, 0.5f, 0.75f, 0.9f};
        CHECK(one_case(sc, 0, nullptr, 0xFFFFFFFFu, 0.75f, 8) == 1);
        CHECK(one_case(sc, 0, nullptr, 0xFFFFFFFFu, std::nextafter(0.75f, -inf), 8) == 3);
        CHECK(one_case(sc, 0, nullptr, 0xFFFFFFFFu, std::nextafter(0.75f, -inf), 2) == 3);   // the cap cuts between rows 1 and 3
    }
    {   // a count far above the largest cap, all scores equal: the first 1024 rows
        std::vector<float> sc(5000, 0.8f);
        CHECK(one_case(sc, 7, nullptr, 0xFFFFFFFFu, 0.5f, 1024) == 5000);
        CHECK(one_case(sc, INT_MAX - 5000LL, nullptr, 0xFFFFFFFFu, 0.5f, 1) == 5000);        // the largest index is INT_MAX - 1
    }
    {   // the errors: -1, and nothing is written (the outputs here hold a pattern)
        std::unique_ptr<float[]> s(new float[2]{0.6f, 0.7f});
        std::unique_ptr<float[]> os(new float[4]);
        std::unique_ptr<int[]> oi(new int[4]);
        for (int k = 0; k < 4; ++k) { os[(size_t)k] = 7.0f; oi[(size_t)k] = -7; }
        long long c = -5;
        CHECK(fh::range_from_scores(s.get(), 2, 0, nullptr, 1u, 0.5f, 0, &c, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(s.get(), 2, 0, nullptr, 1u, 0.5f, fh::kRangeMaxCap + 1, &c, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(s.get(), 2, 0, nullptr, 1u, nan, 4, &c, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(s.get(), -1, 0, nullptr, 1u, 0.5f, 4, &c, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(nullptr, 2, 0, nullptr, 1u, 0.5f, 4, &c, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(s.get(), 2, 0, nullptr, 1u, 0.5f, 4, nullptr, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(s.get(), 2, (long long)INT_MAX - 1, nullptr, 1u, 0.5f, 4, &c, os.get(), oi.get()) == -1);
        CHECK(fh::range_from_scores(s.get(), 2, -1, nullptr, 1u, 0.5f, 4, &c, os.get(), oi.get()) == -1);
        CHECK(c == -5);
        for (int k = 0; k < 4; ++k) CHECK(os[(size_t)k] == 7.0f && oi[(size_t)k] == -7);
        CHECK(fh::range_from_scores(nullptr, 0, 0, nullptr, 1u, 0.5f, 4, &c, os.get(), oi.get()) == 0 && c == 0 && oi[0] == -1 && os[3] == -1.0f);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
