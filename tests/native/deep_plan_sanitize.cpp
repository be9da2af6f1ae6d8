// Stand-alone host program: csrc/deep_plan.h (the rule behind fh_topk_from_scores and fh_gallery_topk_deep_dev, and the block rule the
// device call relies on) under AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/test_deep_plan_sanitize.py builds and runs
// it).  Scores, tags and both output lists are heap blocks of EXACTLY n and k elements, so a read or write past either is a report; the
// results are checked against a restatement that sorts every eligible row, against range_from_scores(-inf, cap = k), and against the
// top-k of the chosen blocks' rows.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/deep_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// runs the rule into exactly sized outputs and holds it to the restatement, the range rule and the block rule; returns the number listed
static int one_case(const std::vector<float>& sc, long long base, const std::vector<uint32_t>* tags, uint32_t mask, int k) {
    const long long n = (long long)sc.size();
    std::unique_ptr<float[]> s(new float[(size_t)n]);                    // exactly n (n == 0: a zero-length block)
    std::unique_ptr<uint32_t[]> t(tags ? new uint32_t[(size_t)n] : nullptr);
    for (long long r = 0; r < n; ++r) { s[(size_t)r] = sc[(size_t)r]; if (tags) t[(size_t)r] = (*tags)[(size_t)r]; }
    std::unique_ptr<float[]> os(new float[(size_t)k]);
    std::unique_ptr<int[]> oi(new int[(size_t)k]);
    const int listed = fh::topk_from_scores(s.get(), n, base, t.get(), mask, k, os.get(), oi.get());
    struct E { float s; long long i; };
    std::vector<E> el;
    std::set<long long> live_blocks;
    for (long long r = 0; r < n; ++r) {
        const uint32_t tg = tags ? (*tags)[(size_t)r] : 0xFFFFFFFFu;
        const float v = sc[(size_t)r];
        if ((tg & mask) != 0 && !std::isnan(v) && v != -std::numeric_limits<float>::infinity()) { el.push_back({v, base + r}); live_blocks.insert(r / 32); }
    }
    std::stable_sort(el.begin(), el.end(), [](const E& a, const E& b) { return a.s > b.s; });      // (pushed in index order: ties keep it)
    CHECK(listed == (int)std::min<size_t>(el.size(), (size_t)k));
    for (int j = 0; j < k; ++j) {
        if (j < listed) CHECK(fbits(os[(size_t)j]) == fbits(el[(size_t)j].s) && oi[(size_t)j] == (int)el[(size_t)j].i);
        else CHECK(os[(size_t)j] == -1.0f && oi[(size_t)j] == -1);
    }
    // either list may be null: the other list the same bytes
    std::unique_ptr<float[]> os2(new float[(size_t)k]);
    std::unique_ptr<int[]> oi2(new int[(size_t)k]);
    CHECK(fh::topk_from_scores(s.get(), n, base, t.get(), mask, k, os2.get(), nullptr) == listed);
    CHECK(fh::topk_from_scores(s.get(), n, base, t.get(), mask, k, nullptr, oi2.get()) == listed);
    CHECK(std::memcmp(os.get(), os2.get(), (size_t)k * sizeof(float)) == 0 && std::memcmp(oi.get(), oi2.get(), (size_t)k * sizeof(int)) == 0);
    // the list part of the range rule at -inf
    long long count = -7;
    CHECK(fh::range_from_scores(s.get(), n, base, t.get(), mask, -std::numeric_limits<float>::infinity(), k, &count, os2.get(), oi2.get()) == listed);
    CHECK(count == (long long)el.size());
    CHECK(std::memcmp(os.get(), os2.get(), (size_t)k * sizeof(float)) == 0 && std::memcmp(oi.get(), oi2.get(), (size_t)k * sizeof(int)) == 0);
    // the block rule: at most k blocks, all of them live, in the rule's order; the top-k of their rows is the top-k
    std::vector<long long> blocks;
    const int nb = fh::deep_chosen_blocks(s.get(), n, t.get(), mask, k, &blocks);
    CHECK(nb == (int)std::min<size_t>(live_blocks.size(), (size_t)k) && (size_t)nb == blocks.size());
    for (long long b : blocks) CHECK(live_blocks.count(b) == 1);
    CHECK(std::set<long long>(blocks.begin(), blocks.end()).size() == blocks.size());
    for (int j = 0; j < k; ++j) { os2[(size_t)j] = 7.0f; oi2[(size_t)j] = -7; }
    CHECK(fh::topk_from_chosen_blocks(s.get(), n, base, t.get(), mask, k, os2.get(), oi2.get()) == listed);
    CHECK(std::memcmp(os.get(), os2.get(), (size_t)k * sizeof(float)) == 0 && std::memcmp(oi.get(), oi2.get(), (size_t)k * sizeof(int)) == 0);
    return listed;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::mt19937 rng(92);
    std::uniform_real_distribution<float> u(-0.1f, 1.1f);
    const int ks[] = {1, 2, 8, 16, 17, 100, 1023, 1024};
    const uint32_t masks[] = {0xFFFFFFFFu, 1u, 6u, 0x80000000u, 0u, 1u << 20};
    // ---- random scores with NaNs, infinities and many equal values; every k regime; with and without tags
    for (int rep = 0; rep < 300; ++rep) {
        const long long n = rep < 10 ? rep : rep % 7 == 0 ? (long long)(rng() % 40000u) : (long long)(rng() % 6000u);
        std::vector<float> sc((size_t)n);
        for (auto& x : sc) x = u(rng);
        for (long long j = 0; j < n / 5; ++j) sc[(size_t)(rng() % (unsigned)n)] = sc[(size_t)(rng() % (unsigned)n)];
        for (long long j = 0; j < n / 20; ++j) sc[(size_t)(rng() % (unsigned)n)] = j % 3 == 0 ? nan : j % 3 == 1 ? inf : -inf;
        std::vector<uint32_t> tags((size_t)n);
        for (auto& x : tags) x = rng() % 10u == 0 ? 0u : (1u << (rng() % 8u)) | (rng() % 8u == 0 ? 0x80000000u : 0u);
        const int k = ks[rep % 8];
        const long long base = rep % 4 == 0 ? 0 : (long long)(rng() % 1000000u);
        one_case(sc, base, nullptr, 0xFFFFFFFFu, k);
        one_case(sc, base, &tags, masks[rep % 6], k);
        one_case(sc, base, nullptr, masks[(rep + 3) % 6], k);
    }
    {   // all rows equal: rows base .. base + k - 1, one empty slot at k = n + 1
        std::vector<float> sc(300, 0.8f);
        for (int k : {1, 8, 9, 10, 33, 300, 301}) CHECK(one_case(sc, 7, nullptr, 0xFFFFFFFFu, k) == std::min(k, 300));
        std::vector<float> big(5000, 0.8f);
        CHECK(one_case(big, INT_MAX - 5000LL, nullptr, 0xFFFFFFFFu, 1024) == 1024);          // the largest index is INT_MAX - 1
    }
    {   // duplicates of the best score at block borders; k cuts between them
        std::vector<float> sc(300);
        for (auto& x : sc) x = 0.5f * u(rng);
        for (int r : {31, 32, 33, 95, 96, 127, 128, 255, 256}) sc[(size_t)r] = 0.9f;
        for (int k = 1; k <= 12; ++k) one_case(sc, 3, nullptr, 0xFFFFFFFFu, k);
    }
    {   // one block holds the whole top
        std::vector<float> sc(300);
        for (auto& x : sc) x = 0.5f * u(rng);
        for (int r = 32; r < 64; ++r) sc[(size_t)r] = 0.6f + 0.01f * (float)(r - 32);
        for (int k : {8, 32, 33}) {
            one_case(sc, 0, nullptr, 0xFFFFFFFFu, k);
            std::vector<long long> blocks;
            CHECK(fh::deep_chosen_blocks(sc.data(), 300, nullptr, 0xFFFFFFFFu, k, &blocks) == std::min(k, 10) && blocks[0] == 1);
        }
    }
    {   // the errors: -1, and nothing is written (the outputs here hold a pattern)
        std::unique_ptr<float[]> s(new float[2]{0.6f, 0.7f});
        std::unique_ptr<float[]> os(new float[4]);
        std::unique_ptr<int[]> oi(new int[4]);
        for (int j = 0; j < 4; ++j) { os[(size_t)j] = 7.0f; oi[(size_t)j] = -7; }
        std::vector<long long> blocks(1, 99);
        CHECK(fh::topk_from_scores(s.get(), 2, 0, nullptr, 1u, 0, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_scores(s.get(), 2, 0, nullptr, 1u, fh::kDeepMaxK + 1, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_scores(s.get(), -1, 0, nullptr, 1u, 4, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_scores(nullptr, 2, 0, nullptr, 1u, 4, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_scores(s.get(), 2, (long long)INT_MAX - 1, nullptr, 1u, 4, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_scores(s.get(), 2, -1, nullptr, 1u, 4, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_chosen_blocks(s.get(), 2, (long long)INT_MAX - 1, nullptr, 1u, 4, os.get(), oi.get()) == -1);
        CHECK(fh::topk_from_chosen_blocks(s.get(), 2, 0, nullptr, 1u, 0, os.get(), oi.get()) == -1);
        CHECK(fh::deep_chosen_blocks(s.get(), 2, nullptr, 1u, 0, &blocks) == -1);
        CHECK(fh::deep_chosen_blocks(s.get(), 2, nullptr, 1u, fh::kDeepMaxK + 1, &blocks) == -1);
        CHECK(fh::deep_chosen_blocks(nullptr, 2, nullptr, 1u, 4, &blocks) == -1);
        CHECK(fh::deep_chosen_blocks(s.get(), -1, nullptr, 1u, 4, &blocks) == -1);
        CHECK(fh::deep_chosen_blocks(s.get(), 2, nullptr, 1u, 4, nullptr) == -1);
        CHECK(blocks.size() == 1 && blocks[0] == 99);
        for (int j = 0; j < 4; ++j) CHECK(os[(size_t)j] == 7.0f && oi[(size_t)j] == -7);
        CHECK(fh::topk_from_scores(nullptr, 0, 0, nullptr, 1u, 4, os.get(), oi.get()) == 0 && oi[0] == -1 && os[3] == -1.0f);
        CHECK(fh::deep_chosen_blocks(nullptr, 0, nullptr, 1u, 4, &blocks) == 0 && blocks.empty());
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
