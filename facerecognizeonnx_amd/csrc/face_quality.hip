// face_quality.hip — one quality score per detected face, from the frame and the record (contract: include/facehip.h, "face quality";
// the formula: face_quality.h).  Integers plus the one fp32 pose term, so that a CPU model (tests/track_quality_model.py) holds it to
// the bit.  Compiled with -ffp-contract=off, as track.hip.
#include <hip/hip_runtime.h>

#include "face_quality.h"
#include "kernels.h"

namespace fh {

// ------------------------------------------------------------------------------------------
// One wave per record [f][j].  An entry behind the frame's count costs one store.  Otherwise lanes stride over the samples of a row,
// so at stride 1 neighbouring lanes read neighbouring pixels, and each lane walks its sample column down the box, four sample rows
// per step: their loads are independent, so they are in flight together (a wave that took one row at a time waited out one memory
// latency per row, and a call has only as many waves as faces).  A lane fetches its 5 pixels as 15 plain byte loads: the 9 contiguous
// bytes of the centre row and 3 each from the rows above and below.  Packing them into dwords would need an aligned base, which a BGR
// row at any pitch does not give; the wave's 64 x 9 bytes of a row are a few cache lines that the lanes share, and the rows above and
// below are the neighbouring sample rows' lines at stride 1, so the bytes come from the vector cache, not from memory.  Per-lane
// partial sums are int64 and reduced by a butterfly: integer addition, any order, one result.
// No atomics.  table == nullptr: frame f is frames + f * stride with the uniform geometry; otherwise row f of the ragged table (an
// empty frame has rows = cols = 0: no window, no read).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void face_quality_kernel(const uint8_t* __restrict__ frames, long stride, int rows, int cols, int step,
                                                           const FrameDesc* __restrict__ table, const FaceRec* __restrict__ det,
                                                           const int* __restrict__ counts, int per_frame, long total,
                                                           int* __restrict__ quality) {
    const long w = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (w >= total) return;
    const int f = (int)(w / per_frame), j = (int)(w - (long)f * per_frame);
    if (j >= min(max(counts[f], 0), per_frame)) {
        if (lane == 0) quality[w] = 0;
        return;
    }
    const FaceRec r = det[w];
    const uint8_t* img = frames + (size_t)f * stride;
    if (table) { img = table[f].bgr; rows = table[f].rows; cols = table[f].cols; step = table[f].step; }

    long long sum = 0, samples = 1;
    QualityWindow win;
    if (quality_window(r, rows, cols, &win)) {                           // (uniform: every lane holds the same record)
        const size_t pitch = (size_t)step, down = pitch * win.d;
        for (int px = win.x0 + lane * win.d; px < win.x1; px += 64 * win.d) {
            const uint8_t* p = img + (size_t)win.y0 * pitch + 3 * (size_t)px;
            int left = (win.y1 - win.y0 + win.d - 1) / win.d;            // sample rows
            for (; left >= 4; left -= 4, p += 4 * down)
                sum += quality_laplacian(p, pitch) + quality_laplacian(p + down, pitch) + quality_laplacian(p + 2 * down, pitch) +
                       quality_laplacian(p + 3 * down, pitch);
            for (; left > 0; --left, p += down) sum += quality_laplacian(p, pitch);
        }
        samples = (long long)((win.x1 - win.x0 + win.d - 1) / win.d) * ((win.y1 - win.y0 + win.d - 1) / win.d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) quality[w] = quality_score((int)(sum / samples), quality_size(r), quality_pose(r));
}

void launch_face_quality(const uint8_t* frames, long stride, int rows, int cols, int step, const FrameDesc* table, int n, const FaceRec* det,
                         const int* counts, int per_frame, int* quality, hipStream_t s) {
    const long total = (long)n * per_frame;
    hipLaunchKernelGGL(face_quality_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, frames, stride, rows, cols, step, table, det,
                       counts, per_frame, total, quality);
}

}  // namespace fh
