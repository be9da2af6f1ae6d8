// Stand-alone host program: fh::tile_plan (csrc/tile_plan.h, the plan behind fh_tile_plan and the tiled detector) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/test_tiles_cpu.py builds and runs it).  The view array is a heap block of
// EXACTLY the counted size, so a write past it is a report; the plan's properties are checked on every case: tiles inside the frame,
// every pixel covered, neighbours overlapping by at least `overlap`, the edge masks, and the argument errors.
#include <climits>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../facerecognizeonnx_amd/csrc/tile_plan.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void one_case(int rows, int cols, fh::Tiling t) {
    const int n = fh::tile_plan(rows, cols, &t, nullptr, 0);
    CHECK(n >= 1);
    if (n < 1) return;
    std::unique_ptr<fh::View[]> v(new fh::View[(size_t)n]);
    CHECK(fh::tile_plan(rows, cols, &t, v.get(), n) == n);
    if (n > 1) {
        std::unique_ptr<fh::View[]> small(new fh::View[(size_t)n - 1]);
        CHECK(fh::tile_plan(rows, cols, &t, small.get(), n - 1) == fh::kTilePlanBadArg);      // cap too small: nothing written
    }
    CHECK(v[0].x == 0 && v[0].y == 0 && v[0].w == cols && v[0].h == rows && v[0].edges == 0);
    CHECK((n == 1) == (cols <= t.tile_w && rows <= t.tile_h));
    if (n == 1) return;
    std::vector<char> covered((size_t)rows * cols, 0);
    for (int i = 1; i < n; ++i) {
        const fh::View& a = v[(size_t)i];
        CHECK(a.x >= 0 && a.y >= 0 && a.w > 0 && a.h > 0 && a.x + a.w <= cols && a.y + a.h <= rows);
        CHECK(a.w == (cols < t.tile_w ? cols : t.tile_w) && a.h == (rows < t.tile_h ? rows : t.tile_h));
        CHECK(a.edges == ((a.x > 0) | (a.y > 0) << 1 | (a.x + a.w < cols) << 2 | (a.y + a.h < rows) << 3));
        for (int y = a.y; y < a.y + a.h; ++y)
            for (int x = a.x; x < a.x + a.w; ++x) covered[(size_t)y * cols + x] = 1;
        if (i + 1 < n) {                                                       // row-major neighbours
            const fh::View& b = v[(size_t)i + 1];
            if (b.y == a.y) CHECK(b.x > a.x && a.x + a.w - b.x >= t.overlap);
            else CHECK(b.y > a.y && b.x == 0 && a.y + a.h - b.y >= t.overlap);
        }
    }
    for (char c : covered) if (!c) { CHECK(!"uncovered pixel"); break; }
}

int main() {
    const fh::Tiling tilings[] = {{128, 128, 32, 2}, {64, 96, 16, 2}, {128, 128, 0, -1}, {16, 16, 15, 0}, {17, 40, 3, 5}};
    int cases = 0;
    for (const fh::Tiling& t : tilings)
        for (int rows = 1; rows <= 300; rows += (rows < 40 ? 1 : 13))
            for (int cols = 1; cols <= 300; cols += (cols < 40 ? 1 : 11)) { one_case(rows, cols, t); ++cases; }
    fh::Tiling ok{128, 128, 32, 2};
    fh::View one;
    CHECK(fh::tile_plan(0, 10, &ok, &one, 1) == 0 && fh::tile_plan(10, -3, &ok, nullptr, 0) == 0);
    CHECK(fh::tile_plan(10, 10, nullptr, nullptr, 0) == fh::kTilePlanBadArg);
    const fh::Tiling bad[] = {{15, 128, 0, 0}, {128, 15, 0, 0}, {128, 128, -1, 0}, {128, 64, 64, 0}, {64, 128, 64, 0}, {16, 16, 16, 0}};
    for (const fh::Tiling& t : bad) CHECK(fh::tile_plan(100, 100, &t, nullptr, 0) == fh::kTilePlanBadArg);
    // the extremes of int: counted in 64 bits, refused when the count does not fit
    fh::Tiling dense{16, 16, 15, 0};
    CHECK(fh::tile_plan(INT_MAX, INT_MAX, &dense, nullptr, 0) == fh::kTilePlanBadArg);
    CHECK(fh::tile_plan(1, INT_MAX, &dense, nullptr, 0) == INT_MAX - 16 + 1 + 1);
    CHECK(fh::tile_plan(INT_MAX, 1, &ok, nullptr, 0) == (int)(((long long)INT_MAX - 128 + 95) / 96 + 1) + 1);
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
