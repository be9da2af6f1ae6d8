// AddressSanitizer + UndefinedBehaviorSanitizer over the tracker's host plan (csrc/track_plan.h, behind fh_track_plan and
// fh_track_update_dev): exactly sized heap arrays, so a write past order[n] or starts[streams + 1] is caught; the result is checked
// against a plain stable sort.  Stand-alone CPU program (tests/test_track_model_cpu.py builds and runs it).
#include <algorithm>
#include <cstdio>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/track_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void run(const std::vector<int>& stream_of, int streams, bool null_stream_of = false) {
    const int n = (int)stream_of.size();
    std::unique_ptr<int[]> so(new int[n]), order(new int[n]), starts(new int[streams + 1]);
    std::copy(stream_of.begin(), stream_of.end(), so.get());
    CHECK(fh::track_plan(null_stream_of ? nullptr : so.get(), n, streams, order.get(), starts.get()) == 0);
    std::vector<int> want(n);
    std::iota(want.begin(), want.end(), 0);
    std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return stream_of[a] < stream_of[b]; });
    CHECK(std::equal(want.begin(), want.end(), order.get()));
    CHECK(starts[0] == 0 && starts[streams] == n);
    for (int s = 0; s < streams; ++s) {
        CHECK(starts[s] <= starts[s + 1]);
        for (int i = starts[s]; i < starts[s + 1]; ++i) CHECK(stream_of[order[i]] == s);
    }
}

int main() {
    std::mt19937 rng(7);
    run({0}, 1);
    run(std::vector<int>(9, 0), 1);
    run(std::vector<int>(5, 0), 3, true);
    run({2, 0, 1, 2, 0, 1, 2, 0, 1, 1, 1, 0}, 3);
    run({3, 0, 3, 0, 0}, 5);
    for (int streams : {1, 2, 63, 64, 4096})
        for (int n : {1, 2, 130, 4096}) {
            std::vector<int> so((size_t)n);
            for (int& v : so) v = (int)(rng() % (unsigned)streams);
            run(so, streams);
        }
    // rejected arguments: nothing may be written (the arrays are one element long)
    int so1[3] = {0, 3, 1}, one[1] = {-7}, st[1] = {-7};
    CHECK(fh::track_plan(so1, 3, 3, one, st) == -1);
    so1[1] = -1;
    CHECK(fh::track_plan(so1, 3, 3, one, st) == -1);
    CHECK(fh::track_plan(so1, 0, 3, one, st) == -1 && fh::track_plan(so1, 1, 0, one, st) == -1);
    CHECK(fh::track_plan(so1, 4097, 1, one, st) == -1 && fh::track_plan(so1, 1, 4097, one, st) == -1);
    CHECK(one[0] == -7 && st[0] == -7);
    std::printf("%d failures\n", failures);
    return failures != 0;
}
