// face_quality.h — the face quality score q = (S * Z * P) >> 8 (contract: include/facehip.h, "face quality"), the ONE place that states
// the formula: replace these functions (and tests/track_quality_model.py) to try another one.  S = sharpness: the mean absolute
// 4-neighbour Laplacian of the luma over a grid of about 64 samples per side of the clipped box, integers only; Z = size: the shorter
// side, capped at the recogniser's 112; P = pose: how centred the nose is between the eyes, fp32 in a fixed order with one division (as
// face_iou.h), cut to 0 .. 256.  Records may hold anything: the box is clipped in int64, a NaN landmark fails the comparison.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace fh {

constexpr int kQualityMinSide = 8;       // a clipped box narrower or lower than this has S = 0
constexpr int kQualityGrid = 64;         // samples per (shorter) side before the stride grows
constexpr int kQualityMaxSize = 112;     // the recogniser's input side: a larger face adds nothing

// the sampled window of a box: pixels px = x0 + i * d < x1, py = y0 + k * d < y1, all of which have their 4 neighbours inside the frame
struct QualityWindow { int x0, y0, x1, y1, d; };

__device__ __forceinline__ bool quality_window(const FaceRec& r, int rows, int cols, QualityWindow* win) {
    const long long x0 = max((long long)r.x, 1LL), y0 = max((long long)r.y, 1LL);
    const long long x1 = min((long long)r.x + r.w, (long long)cols - 1), y1 = min((long long)r.y + r.h, (long long)rows - 1);
    if (x1 - x0 < kQualityMinSide || y1 - y0 < kQualityMinSide) return false;
    *win = QualityWindow{(int)x0, (int)y0, (int)x1, (int)y1, max(1, (int)(min(x1 - x0, y1 - y0) / kQualityGrid))};
    return true;
}

__device__ __forceinline__ int quality_luma(const uint8_t* bgr) { return (29 * bgr[0] + 150 * bgr[1] + 77 * bgr[2] + 128) >> 8; }

// |4 Y(p) - Y(left) - Y(right) - Y(up) - Y(down)| at the pixel p points to; the neighbour distance is 1 whatever the sample stride
__device__ __forceinline__ int quality_laplacian(const uint8_t* p, size_t step) {
    return abs(4 * quality_luma(p) - quality_luma(p - 3) - quality_luma(p + 3) - quality_luma(p - step) - quality_luma(p + step));
}

__device__ __forceinline__ int quality_size(const FaceRec& r) { return min(max(min(r.w, r.h), 0), kQualityMaxSize); }

// landmarks in the record's order: left eye, right eye, nose, ...
__device__ __forceinline__ int quality_pose(const FaceRec& r) {
    const float lex = r.lm[0], rex = r.lm[2], nx = r.lm[4];
    const float dx = fabsf(rex - lex);
    const float e = dx > 1.0f ? dx : 1.0f;                               // (NaN: 1; the sum below is NaN then anyway)
    const float m = (lex + rex) * 0.5f;
    const float v = 256.0f * (1.0f - 2.0f * fabsf(nx - m) / e);
    return v > 0.0f ? min((int)(v < 256.0f ? v : 256.0f), 256) : 0;      // NaN fails v > 0
}

__device__ __forceinline__ int quality_score(int S, int Z, int P) { return (int)(((long long)S * Z * P) >> 8); }

}  // namespace fh
