// face_emit.h — the two device pieces every decode / threshold kernel shares (face_kernels.hip, tiled_kernels.hip): the sort key and
// FaceDetector::postprocess' row arithmetic (src/face_detector.cpp:249-278).  Include from files built with -ffp-contract=off only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace fh {

// score descending, then the 32-bit index ascending — the total order this build fixes for the reference's unstable std::sort (:357)
__device__ __forceinline__ unsigned long long make_key(float score, unsigned idx) {
    unsigned u = __float_as_uint(score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // ascending-orderable
    return ((unsigned long long)(~u) << 32) | idx;          // descending score, ascending index
}

// /scale, int truncation, width from the float difference
__device__ __forceinline__ void emit_face(const float* o15, float scale, FaceRec* f) {
    const float x1 = o15[0] / scale, y1 = o15[1] / scale, x2 = o15[2] / scale, y2 = o15[3] / scale;
    f->x = (int)x1; f->y = (int)y1; f->w = (int)(x2 - x1); f->h = (int)(y2 - y1);
    f->score = o15[4];
#pragma unroll
    for (int j = 0; j < 10; ++j) f->lm[j] = o15[5 + j] / scale;
}

}  // namespace fh
