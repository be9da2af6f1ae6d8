// tiled_kernels.hip — tiled detection of large frames (include/facehip.h: fh_det_detect_tiled_dev): the view-aware twins of
// scrfd_decode_kernel / rows_threshold_kernel (face_kernels.hip).  A call's views — the whole frame and its overlapping tiles, for every
// frame — went through the network as ONE ragged batch; here each view's candidates get the reference's row arithmetic (emit_face, in
// VIEW coordinates), then
//   the border rule   tiles only: a box within `border` pixels of an INTERIOR edge of its tile is dropped (the face is cut there;
//                     the neighbouring tile or the whole-frame view sees it whole),
//   the shift         x += view.x, y += view.y in integers, every landmark coordinate + (float)view.x / (float)view.y (one fp32 add
//                     after the division; view 0 is at the origin and is not touched, so a one-view frame keeps the ragged path's bits),
// and the key is appended to the FRAME's list with the frame's counter; its low word local_view * cap + index makes the sort's order
// (score descending, view ascending, index ascending).  The payload stays in the per-view [view][cap] blocks.  One NMS per frame
// follows (sort_nms_frames_kernel).  Compiled with -ffp-contract=off, as face_kernels.hip: the decode's cx + d * s must not fuse.
#include <hip/hip_runtime.h>

#include "face_emit.h"
#include "kernels.h"

namespace fh {

__device__ __forceinline__ void emit_view_face(const float* o15, const ViewDesc& v, int gv, int r, const TiledArgs& a) {
    FaceRec f;
    emit_face(o15, v.scale, &f);
    if (a.border >= 0 && v.edges) {                          // (view 0: edges == 0)
        const long long b = a.border;
        if ((v.edges & 1) && f.x <= b) return;
        if ((v.edges & 2) && f.y <= b) return;
        if ((v.edges & 4) && (long long)f.x + f.w >= v.w - b) return;
        if ((v.edges & 8) && (long long)f.y + f.h >= v.h - b) return;
    }
    if (v.local != 0) {
        const float fx = (float)v.x, fy = (float)v.y;
        f.x = (int)((unsigned)f.x + (unsigned)v.x); f.y = (int)((unsigned)f.y + (unsigned)v.y);
#pragma unroll
        for (int j = 0; j < 5; ++j) { f.lm[2 * j] += fx; f.lm[2 * j + 1] += fy; }
    }
    a.cand[(size_t)gv * a.cap + r] = f;
    const FrameSeg sg = a.segs[v.frame];
    const int pos = atomicAdd(a.count + v.frame, 1);
    if (pos < sg.seg_cap) a.keys[(size_t)sg.key_off + pos] = make_key(f.score, (unsigned)(v.local * a.cap + r));
}

// grid = ceil(anchors / 256) x V: one grid row per view (the head tensors hold one row block per view, in plan order)
__global__ __launch_bounds__(256) void scrfd_decode_tiled_kernel(const TiledHeads h, const TiledArgs a) {
    const int gw8 = h.inW / 8, gh8 = h.inH / 8, gw16 = h.inW / 16, gh16 = h.inH / 16, gw32 = h.inW / 32, gh32 = h.inH / 32;
    const int n8 = gw8 * gh8 * 2, n16 = gw16 * gh16 * 2, n32 = gw32 * gh32 * 2;
    const int N = n8 + n16 + n32;
    const int b = blockIdx.y;
    const ViewDesc v = a.views[b];
    if (!(v.scale > 0.f)) return;                            // a dead view emits nothing
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < N; r += gridDim.x * blockDim.x) {
        int si, i, gw, s, ns;
        if (r < n8) { si = 0; i = r; gw = gw8; s = 8; ns = n8; }
        else if (r < n8 + n16) { si = 1; i = r - n8; gw = gw16; s = 16; ns = n16; }
        else { si = 2; i = r - n8 - n16; gw = gw32; s = 32; ns = n32; }
        const float score = h.score[si][(size_t)b * ns + i];
        if (!(score > a.thr) || r >= a.cap) continue;
        const int cell = i >> 1;
        const int gy = cell / gw, gx = cell - gy * gw;
        const float cx = (float)(gx * s), cy = (float)(gy * s), fs = (float)s;
        const float* d = h.bbox[si] + ((size_t)b * ns + i) * 4;
        const float* k = h.kps[si] + ((size_t)b * ns + i) * 10;
        float o[15];
        o[0] = cx - d[0] * fs; o[1] = cy - d[1] * fs; o[2] = cx + d[2] * fs; o[3] = cy + d[3] * fs;
        o[4] = score;
#pragma unroll
        for (int j = 0; j < 5; ++j) { o[5 + 2 * j] = cx + k[2 * j] * fs; o[6 + 2 * j] = cy + k[2 * j + 1] * fs; }
        emit_view_face(o, v, b, r, a);
    }
}

void launch_scrfd_decode_tiled(const TiledHeads& h, const TiledArgs& a, hipStream_t s) {
    const int N = ((h.inW / 8) * (h.inH / 8) + (h.inW / 16) * (h.inH / 16) + (h.inW / 32) * (h.inH / 32)) * 2;
    if (N <= 0 || a.V <= 0) return;
    hipLaunchKernelGGL(scrfd_decode_tiled_kernel, dim3((N + 255) / 256, a.V), dim3(256), 0, s, h, a);
}

// the reference's own layout: rows [V][n][feat >= 15] = x1,y1,x2,y2,score,kps (src/face_detector.cpp:242-325); grid = blocks x V
__global__ __launch_bounds__(256) void rows_threshold_tiled_kernel(const float* __restrict__ rows, int n, int feat, const TiledArgs a) {
    const int b = blockIdx.y;
    const ViewDesc v = a.views[b];
    if (!(v.scale > 0.f)) return;
    const float* vr = rows + (size_t)b * n * feat;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const float* o = vr + (size_t)r * feat;
        const float score = o[4];
        if (!(score > a.thr) || r >= a.cap) continue;
        float o15[15];
#pragma unroll
        for (int j = 0; j < 15; ++j) o15[j] = o[j];
        emit_view_face(o15, v, b, r, a);
    }
}

void launch_rows_threshold_tiled(const float* rows, int rows_per_view, int feat, const TiledArgs& a, hipStream_t s) {
    if (rows_per_view <= 0 || a.V <= 0) return;
    const int blocks = (rows_per_view + 255) / 256;
    hipLaunchKernelGGL(rows_threshold_tiled_kernel, dim3(blocks < 4096 ? blocks : 4096, a.V), dim3(256), 0, s, rows, rows_per_view, feat, a);
}

}  // namespace fh
