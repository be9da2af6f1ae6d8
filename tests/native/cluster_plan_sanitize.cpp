// Stand-alone host program: fh::cluster_scores (csrc/cluster_plan.h, the rule behind fh_cluster_scores / fh_gallery_cluster_dev) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/test_cluster_plan_sanitize.py builds and runs it).  The matrix, labels
// and info are heap blocks of EXACTLY n * n, n and 4 elements, so a read or write past any of them is a report; the results are checked
// against a breadth-first restatement of the rule.
#include <cmath>
#include <cstdio>
#include <deque>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/cluster_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

struct Mat {
    int n;
    std::unique_ptr<float[]> v;
    explicit Mat(int n_, float fill = 0.f) : n(n_), v(new float[(size_t)n_ * (size_t)n_]) {
        for (size_t i = 0; i < (size_t)n * (size_t)n; ++i) v[i] = fill;
    }
    float& at(int i, int j) { return v[(size_t)i * (size_t)n + (size_t)j]; }
    void link(int i, int j, float s) { at(i, j) = s; at(j, i) = s; }
};

// the rule again, by breadth-first search over the upper triangle
static void model(Mat& m, float thr, int min_pts, int noise, std::vector<int>& labels, int (&info)[4]) {
    const int n = m.n;
    auto s = [&](int i, int j) { return i < j ? m.at(i, j) : m.at(j, i); };
    auto edge = [&](int i, int j) { return i != j && s(i, j) > thr; };
    std::vector<char> core((size_t)n);
    for (int i = 0; i < n; ++i) {
        int deg = 0;
        for (int j = 0; j < n; ++j) deg += edge(i, j);
        core[(size_t)i] = deg + 1 >= min_pts;
    }
    labels.assign((size_t)n, -2);
    info[0] = info[1] = info[2] = info[3] = 0;
    for (int seed = 0; seed < n; ++seed) {
        if (!core[(size_t)seed] || labels[(size_t)seed] != -2) continue;
        ++info[0];
        labels[(size_t)seed] = seed;
        std::deque<int> todo{seed};
        while (!todo.empty()) {
            const int i = todo.front();
            todo.pop_front();
            for (int j = 0; j < n; ++j)
                if (core[(size_t)j] && labels[(size_t)j] == -2 && edge(i, j)) { labels[(size_t)j] = seed; todo.push_back(j); }
        }
    }
    for (int i = 0; i < n; ++i) {
        if (core[(size_t)i]) { ++info[1]; continue; }
        int best = -1;
        for (int j = 0; j < n; ++j)
            if (core[(size_t)j] && edge(i, j) && (best < 0 || s(i, j) > s(i, best))) best = j;      // ascending j: ties keep the lower position
        if (best >= 0) { labels[(size_t)i] = labels[(size_t)best]; ++info[2]; }
        else { labels[(size_t)i] = noise ? i : -1; ++info[3]; }
    }
}

// runs the rule into exactly sized outputs and holds it to the model; returns the labels
static std::vector<int> one_case(Mat& m, float thr, int min_pts, int noise, int (&info_out)[4]) {
    const int n = m.n;
    std::unique_ptr<int[]> labels(new int[(size_t)n]), info(new int[4]);
    const int rc = fh::cluster_scores(n ? m.v.get() : nullptr, n, thr, min_pts, noise, n ? labels.get() : nullptr, info.get());
    std::vector<int> want;
    int winfo[4];
    model(m, thr, min_pts, noise, want, winfo);
    CHECK(rc == winfo[0]);
    for (int k = 0; k < 4; ++k) { CHECK(info[(size_t)k] == winfo[k]); info_out[k] = info[(size_t)k]; }
    CHECK(info[1] + info[2] + info[3] == n);
    for (int i = 0; i < n; ++i) CHECK(labels[(size_t)i] == want[(size_t)i]);
    CHECK(fh::cluster_scores(n ? m.v.get() : nullptr, n, thr, min_pts, noise, n ? labels.get() : nullptr, nullptr) == rc);     // info may be null
    return std::vector<int>(labels.get(), labels.get() + n);
}

static Mat two_clusters() {     // {0, 1, 2, 7} and {3, 4, 5, 8} fully linked; 6 and 9 on their own
    Mat m(10);
    const int grp[2][4] = {{0, 1, 2, 7}, {3, 4, 5, 8}};
    for (auto& g : grp)
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b) m.link(g[a], g[b], 0.9f);
    return m;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int info[4];
    for (int min_pts : {1, 2, 3}) {
        for (int noise : {0, 1}) {
            Mat m0(0), m1(1, 0.99f);
            one_case(m0, 0.5f, min_pts, noise, info);
            CHECK(info[0] == 0 && info[3] == 0);
            const std::vector<int> l = one_case(m1, 0.5f, min_pts, noise, info);     // its own 0.99 on the diagonal is no edge
            CHECK(info[0] == (min_pts == 1) && l[0] == (min_pts == 1 || noise ? 0 : -1));
        }
    }
    {   // a chain: single linkage at min_pts 1; at 3 the two ends are border rows of the cluster labelled 1
        Mat m(9, 0.1f);
        for (int t = 0; t + 1 < 9; ++t) m.link(t, t + 1, 0.9f);
        std::vector<int> l = one_case(m, 0.5f, 1, 0, info);
        CHECK(info[0] == 1 && info[1] == 9 && l[8] == 0);
        l = one_case(m, 0.5f, 3, 0, info);
        CHECK(info[0] == 1 && info[1] == 7 && info[2] == 2 && info[3] == 0 && l[0] == 1 && l[8] == 1);
    }
    {   // a border row tied between two clusters: the lower position; one ulp more: the other
        Mat m = two_clusters();
        m.link(6, 4, 0.75f); m.link(6, 1, 0.75f);
        std::vector<int> l = one_case(m, 0.5f, 4, 0, info);
        CHECK(info[0] == 2 && info[2] == 1 && info[3] == 1 && l[6] == 0 && l[9] == -1);
        m.link(6, 4, std::nextafter(0.75f, 1.0f));
        l = one_case(m, 0.5f, 4, 1, info);
        CHECK(l[6] == 3 && l[9] == 9);
    }
    {   // a border row next to two clusters does not merge them; as a core row (min_pts 1) it does
        Mat m = two_clusters();
        m.link(6, 2, 0.8f); m.link(6, 3, 0.7f);
        std::vector<int> l = one_case(m, 0.5f, 4, 0, info);
        CHECK(info[0] == 2 && info[2] == 1 && l[6] == 0 && l[3] == 3);
        l = one_case(m, 0.5f, 1, 0, info);
        CHECK(info[0] == 2 && l[3] == 0 && l[9] == 9);
    }
    {   // NaN entries, a NaN threshold, the strict threshold
        Mat m = two_clusters();
        m.link(6, 2, nan); m.link(9, 0, nan); m.link(6, 3, 0.7f);
        std::vector<int> l = one_case(m, 0.5f, 4, 0, info);
        CHECK(info[0] == 2 && info[2] == 1 && info[3] == 1 && l[6] == 3 && l[9] == -1);
        l = one_case(m, nan, 1, 0, info);
        CHECK(info[0] == 10);
        l = one_case(m, nan, 2, 1, info);
        CHECK(info[0] == 0 && info[3] == 10 && l[7] == 7);
        l = one_case(m, 0.7f, 4, 0, info);
        CHECK(l[6] == -1 && info[3] == 2);
        l = one_case(m, std::nextafter(0.7f, 0.0f), 4, 0, info);
        CHECK(l[6] == 3 && info[2] == 1);
    }
    {   // garbage below and on the diagonal is never read
        Mat m = two_clusters();
        m.link(6, 2, 0.8f);
        int want_info[4];
        const std::vector<int> want = one_case(m, 0.5f, 4, 0, want_info);
        const float junk[5] = {nan, inf, -inf, 1e30f, 0.99f};
        for (int i = 0; i < 10; ++i)
            for (int j = 0; j <= i; ++j) m.at(i, j) = junk[(i * 7 + j) % 5];
        std::unique_ptr<int[]> labels(new int[10]), inf4(new int[4]);
        CHECK(fh::cluster_scores(m.v.get(), 10, 0.5f, 4, 0, labels.get(), inf4.get()) == want_info[0]);
        for (int i = 0; i < 10; ++i) CHECK(labels[(size_t)i] == want[(size_t)i]);
        for (int k = 0; k < 4; ++k) CHECK(inf4[(size_t)k] == want_info[k]);
    }
    std::mt19937 rng(2024);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    for (int rep = 0; rep < 120; ++rep) {
        const int n = (int)(rng() % 90u);
        Mat m(n);
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) m.link(i, j, u(rng));
        const float thr = 1.0f - (float)(1 + rep % 6) / (float)(n + 1);
        one_case(m, thr, 1 + rep % 5, rep & 1, info);
    }
    {   // the argument errors: -1, and nothing is written (the outputs here are too small to write to)
        Mat m = two_clusters();
        int l = 99, i4 = 99;
        CHECK(fh::cluster_scores(m.v.get(), -1, 0.5f, 1, 0, &l, &i4) == -1 && l == 99 && i4 == 99);
        CHECK(fh::cluster_scores(m.v.get(), 10, 0.5f, 0, 0, &l, &i4) == -1 && l == 99 && i4 == 99);
        CHECK(fh::cluster_scores(m.v.get(), 10, 0.5f, 1, 2, &l, &i4) == -1 && l == 99 && i4 == 99);
        CHECK(fh::cluster_scores(nullptr, 10, 0.5f, 1, 0, &l, &i4) == -1 && l == 99 && i4 == 99);
        CHECK(fh::cluster_scores(m.v.get(), 10, 0.5f, 1, 0, nullptr, &i4) == -1 && i4 == 99);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
