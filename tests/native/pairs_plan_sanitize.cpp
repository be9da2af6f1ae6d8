// Stand-alone host program: fh::pairs_from_scores (csrc/pairs_plan.h, the rule behind fh_pairs_from_scores and fh_gallery_pairs_dev) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/test_pairs_plan_sanitize.py builds and runs it).  The score matrix, the
// ids, info and the three lists are heap blocks of EXACTLY n * n, n, 4, cap, 2 cap and 2 cap elements, so a read or write past any of
// them is a report; the results are checked against a restatement that sorts every selected pair and walks the bins itself.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/pairs_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct P { float s; int i, j; };

// runs the rule into exactly sized outputs and holds it to the restatement; returns info[3] (complete)
static int one_case(const std::vector<float>& sc, int n, const std::vector<int>* ids, int cls, int side, float thr, int cap, long long room) {
    const size_t N = (size_t)n;
    std::unique_ptr<float[]> s(new float[N * N]);
    std::unique_ptr<int[]> d(ids ? new int[N] : nullptr);
    for (size_t k = 0; k < N * N; ++k) s[k] = sc[k];
    for (size_t k = 0; ids && k < N; ++k) d[k] = (*ids)[k];
    std::unique_ptr<unsigned long long[]> info(new unsigned long long[4]);
    std::unique_ptr<float[]> os(new float[(size_t)cap]);
    std::unique_ptr<int[]> orow(new int[2 * (size_t)cap]), oid(new int[2 * (size_t)cap]);
    const int listed = fh::pairs_from_scores(s.get(), n, d.get(), cls, side, thr, cap, room, info.get(), os.get(), orow.get(), oid.get());
    std::vector<P> sel;
    unsigned long long nan = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const float v = sc[(size_t)i * N + (size_t)j];
            const bool genuine = ids && (*ids)[(size_t)i] == (*ids)[(size_t)j];
            if (cls == fh::kPairsGenuine && !genuine) continue;
            if (cls == fh::kPairsImpostor && genuine) continue;
            if (std::isnan(v)) { ++nan; continue; }
            if (side == fh::kPairsAbove ? v > thr : v <= thr) sel.push_back({v, i, j});
        }
    std::stable_sort(sel.begin(), sel.end(), [&](const P& a, const P& b) { return side == fh::kPairsAbove ? a.s > b.s : a.s < b.s; });   // (pushed in (i, j) order: ties keep it)
    // the walk: groups of equal bin from the front of the sorted list
    const size_t want = std::min(sel.size(), (size_t)cap);
    size_t returned = 0, complete = 1;
    for (size_t a = 0; a < sel.size() && want > 0;) {
        size_t b = a;
        while (b < sel.size() && fh::hist_bin(sel[b].s) == fh::hist_bin(sel[a].s)) ++b;
        if (b >= want) {
            if ((long long)b <= room) returned = want;
            else { returned = a; complete = 0; }
            break;
        }
        a = b;
    }
    CHECK(info[0] == sel.size() && info[1] == nan && info[2] == returned && info[3] == complete);
    CHECK(listed == (int)returned);
    for (size_t k = 0; k < (size_t)cap; ++k) {
        if (k < returned) {
            CHECK(fbits(os[k]) == fbits(sel[k].s) && orow[2 * k] == sel[k].i && orow[2 * k + 1] == sel[k].j);
            CHECK(oid[2 * k] == (ids ? (*ids)[(size_t)sel[k].i] : -1) && oid[2 * k + 1] == (ids ? (*ids)[(size_t)sel[k].j] : -1));
        } else {
            CHECK(os[k] == -1.0f && orow[2 * k] == -1 && orow[2 * k + 1] == -1 && oid[2 * k] == -1 && oid[2 * k + 1] == -1);
        }
    }
    // any of the lists may be null: the same info, the other lists the same bytes
    std::unique_ptr<unsigned long long[]> info2(new unsigned long long[4]);
    std::unique_ptr<int[]> orow2(new int[2 * (size_t)cap]);
    CHECK(fh::pairs_from_scores(s.get(), n, d.get(), cls, side, thr, cap, room, info2.get(), nullptr, orow2.get(), nullptr) == listed);
    CHECK(std::memcmp(info.get(), info2.get(), 4 * sizeof(unsigned long long)) == 0);
    CHECK(std::memcmp(orow.get(), orow2.get(), 2 * (size_t)cap * sizeof(int)) == 0);
    CHECK(fh::pairs_from_scores(s.get(), n, d.get(), cls, side, thr, cap, room, info2.get(), nullptr, nullptr, nullptr) == listed);
    return (int)info[3];
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::mt19937 rng(17);
    std::uniform_real_distribution<float> u(-0.1f, 1.1f);
    int incomplete = 0;
    for (int rep = 0; rep < 240; ++rep) {
        const int n = rep < 6 ? rep / 2 : (int)(rng() % 70u);
        const size_t N = (size_t)n;
        std::vector<float> sc(N * N);
        for (auto& x : sc) x = u(rng);
        if (rep % 3 == 0)
            for (auto& x : sc) x = std::round(x * 64.0f) / 64.0f;                           // few distinct values, all on bin edges
        for (size_t k = 0; k < N * N / 30; ++k) sc[rng() % (N * N)] = k % 3 == 0 ? nan : k % 3 == 1 ? inf : -inf;
        for (size_t i = 0; i < N; ++i)
            for (size_t j = 0; j < i; ++j) sc[i * N + j] = -7.0f;                           // never read: the lower triangle and the diagonal
        for (size_t i = 0; i < N; ++i) sc[i * N + i] = nan;
        std::vector<int> ids(N);
        for (auto& x : ids) x = (int)(rng() % 9u) * 1000003;
        const int caps[] = {1, 2, 7, 100, 1023, 1024};
        const float thrs[] = {0.0f, 0.5f, 0.75f, 1.05f, -1.0f, -inf, inf, 517.0f / 2048.0f};
        const int cap = caps[rep % 6];
        const float thr = thrs[rep % 8];
        const long long rooms[] = {cap, cap + 1LL, 4LL * cap, 65536};
        for (int cls = 0; cls < 3; ++cls)
            for (int side = 0; side < 2; ++side)
                incomplete += 1 - one_case(sc, n, &ids, cls, side, thr, cap, rooms[(rep + cls + side) % 4]);
        one_case(sc, n, nullptr, fh::kPairsAny, rep % 2, thr, cap, rooms[rep % 4]);
    }
    CHECK(incomplete > 10);                                                                 // the overflow branch was taken
    {   // all scores equal: the first pairs in (i, j) order; room == cap: nothing fits
        const int n = 48;
        std::vector<float> sc((size_t)n * n, 0.8f);
        std::vector<int> ids((size_t)n, 5);
        CHECK(one_case(sc, n, &ids, fh::kPairsGenuine, fh::kPairsAbove, 0.5f, 100, 65536) == 1);
        CHECK(one_case(sc, n, &ids, fh::kPairsGenuine, fh::kPairsNotAbove, 0.8f, 1024, 1128) == 1);      // 48 * 47 / 2 = 1128: exactly the room
        CHECK(one_case(sc, n, &ids, fh::kPairsGenuine, fh::kPairsNotAbove, 0.8f, 1024, 1127) == 0);
        CHECK(one_case(sc, n, &ids, fh::kPairsAny, fh::kPairsAbove, 0.5f, 8, 8) == 0);
        CHECK(one_case(sc, n, &ids, fh::kPairsImpostor, fh::kPairsAbove, 0.5f, 8, 8) == 1);              // no impostor pair at all
    }
    {   // the errors: -1, and nothing is written (the outputs here hold a pattern)
        std::unique_ptr<float[]> s(new float[4]{0.f, 0.6f, 0.f, 0.f});
        std::unique_ptr<int[]> d(new int[2]{1, 2});
        std::unique_ptr<unsigned long long[]> info(new unsigned long long[4]{9, 9, 9, 9});
        std::unique_ptr<float[]> os(new float[4]{7.f, 7.f, 7.f, 7.f});
        std::unique_ptr<int[]> orow(new int[8]), oid(new int[8]);
        for (int k = 0; k < 8; ++k) { orow[(size_t)k] = -7; oid[(size_t)k] = -7; }
        const auto call = [&](const float* sp, int n, const int* dp, int cls, int side, float thr, int cap, long long room, unsigned long long* ip) {
            return fh::pairs_from_scores(sp, n, dp, cls, side, thr, cap, room, ip, os.get(), orow.get(), oid.get());
        };
        CHECK(call(s.get(), -1, d.get(), 0, 0, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(nullptr, 2, d.get(), 0, 0, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), 0, 0, 0.5f, 4, 4, nullptr) == -1);
        CHECK(call(s.get(), 2, d.get(), 0, 0, nan, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), 3, 0, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), -1, 0, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), 0, 2, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, nullptr, 0, 0, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, nullptr, 1, 0, 0.5f, 4, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), 0, 0, 0.5f, 0, 4, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), 0, 0, 0.5f, fh::kPairsMaxCap + 1, 65536, info.get()) == -1);
        CHECK(call(s.get(), 2, d.get(), 0, 0, 0.5f, 4, 3, info.get()) == -1);
        for (int k = 0; k < 4; ++k) CHECK(info[(size_t)k] == 9 && os[(size_t)k] == 7.f);
        for (int k = 0; k < 8; ++k) CHECK(orow[(size_t)k] == -7 && oid[(size_t)k] == -7);
        CHECK(call(s.get(), 2, d.get(), 1, 0, 0.5f, 4, 4, info.get()) == 1 && info[0] == 1 && orow[0] == 0 && orow[1] == 1 && oid[1] == 2 && orow[2] == -1);
        CHECK(call(nullptr, 0, nullptr, 2, 1, 0.5f, 4, 4, info.get()) == 0 && info[0] == 0 && info[3] == 1 && os[0] == -1.0f);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
