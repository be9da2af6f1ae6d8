// tile_plan.h — the tile plan of a tiled detection (include/facehip.h: fh_tile_plan), the ONE place it lives.  Host code, plain C++, no
// HIP: api.cpp exposes it, the detector plans through it, and tests/native/tile_plan_sanitize.cpp runs it under the sanitizers.
//
// Per axis (x shown, y alike), integers only:  cols <= tile_w -> one tile at 0, cols wide;  otherwise  sx = tile_w - overlap,
// nx = ceil((cols - tile_w) / sx) + 1,  x_j = min(j * sx, cols - tile_w),  tile_w wide — the last tile is shifted inward, never cut
// short.  View 0 is the whole frame (edges = 0); when nx * ny > 1 the nx * ny tiles follow, row-major.  An edge of a tile is INTERIOR
// (bit 0 left, 1 top, 2 right, 3 bottom) when it is not an edge of the frame: x > 0, y > 0, x + w < cols, y + h < rows.
#pragma once
#include <cstdint>

namespace fh {

struct Tiling { int32_t tile_w, tile_h, overlap, border; };       // layout of fh_tiling
struct View { int32_t x, y, w, h, edges; };                       // layout of fh_view

constexpr int kTileMinSide = 16;
constexpr int kTilePlanBadArg = -1;                                // = FH_ERR_ARG

inline bool tiling_ok(const Tiling* t) {
    if (!t || t->tile_w < kTileMinSide || t->tile_h < kTileMinSide || t->overlap < 0) return false;
    return t->overlap < (t->tile_w < t->tile_h ? t->tile_w : t->tile_h);
}

// tiles along one axis of `len` pixels
inline long long tile_axis_count(int len, int tile, int overlap) {
    if (len <= tile) return 1;
    const long long s = (long long)tile - overlap;
    return ((long long)len - tile + s - 1) / s + 1;
}
inline int tile_axis_origin(long long j, int len, int tile, int overlap) {
    if (len <= tile) return 0;
    const long long o = j * ((long long)tile - overlap), last = (long long)len - tile;
    return (int)(o < last ? o : last);
}

// Returns the number of views (0 for an empty image), or kTilePlanBadArg: a bad tiling, more views than an int holds, or — with
// views != nullptr — more views than `cap`.  views == nullptr only counts.  Nothing is written on failure.
inline int tile_plan(int rows, int cols, const Tiling* t, View* views, int cap) {
    if (!tiling_ok(t)) return kTilePlanBadArg;
    if (rows <= 0 || cols <= 0) return 0;
    const long long nx = tile_axis_count(cols, t->tile_w, t->overlap), ny = tile_axis_count(rows, t->tile_h, t->overlap);
    const long long tiles = nx * ny;                               // (each factor < 2^31)
    const long long total = tiles == 1 ? 1 : tiles + 1;
    if (total > 0x7fffffffLL) return kTilePlanBadArg;
    if (!views) return (int)total;
    if (total > (long long)(cap > 0 ? cap : 0)) return kTilePlanBadArg;
    views[0] = View{0, 0, cols, rows, 0};
    if (tiles == 1) return 1;
    const int tw = cols <= t->tile_w ? cols : t->tile_w, th = rows <= t->tile_h ? rows : t->tile_h;
    View* v = views + 1;
    for (long long iy = 0; iy < ny; ++iy) {
        const int y = tile_axis_origin(iy, rows, t->tile_h, t->overlap);
        for (long long ix = 0; ix < nx; ++ix, ++v) {
            const int x = tile_axis_origin(ix, cols, t->tile_w, t->overlap);
            const int edges = (x > 0 ? 1 : 0) | (y > 0 ? 2 : 0) | (x + tw < cols ? 4 : 0) | (y + th < rows ? 8 : 0);
            *v = View{x, y, tw, th, edges};
        }
    }
    return (int)total;
}

}  // namespace fh
