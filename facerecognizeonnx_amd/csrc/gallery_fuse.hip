// gallery_fuse.hip — template pooling of a LABELLED gallery (fh_gallery_fuse_ids) and the mislabel audit that goes with it
// (fh_gallery_self_scores_dev).
//   * pooling: one row per identity = the sum of that identity's rows, L2-normalised (FH_FUSE_UNIT) or as it is (FH_FUSE_SUM).  The
//     host groups the ids (group_ids.h) and uploads `order` (row positions by id, then position) and a work list of FuseItem; the
//     device reads every source row exactly once.  "Sum per destination through an inverted index": no atomics, a fixed order, so the
//     result reproduces bit for bit and does not depend on timing.
//   * order of the additions (the contract, restated by tests/gallery_fuse_model.py): an identity's rows, in row order, are cut into
//     chunks of FH_FUSE_CHUNK = 512; a chunk is summed sequentially from its first row (p = row0; p = p + row1; ...); the chunk partials
//     are added sequentially in chunk order.  An identity of one row keeps that row verbatim, whatever the mode.  The split keeps an
//     "unknown" bucket of 100 000 rows from running on one wave while every other wave has long finished.
//   * one wave per work item, each lane owns the 16-byte columns lane, lane + 64, ... (dim 64: 16 lanes work), several rows' loads in
//     flight.  Items of at most one chunk write their identity's final row; chunk items write partials to scratch, and a second launch
//     of the same kernel adds an identity's partials (consecutive scratch rows) in chunk order.
//   * FH_FUSE_UNIT is FaceRecognizer::normalize (src/face_recognizer.cpp:306-318): s / sqrt(sum s^2) when that is > 0, else s as it is
//     (a cancelled sum stays zero, a NaN stays NaN).  The sum of squares is a lane-strided partial + butterfly, as l2norm_kernel's.
// Everything that decides the SUMS is an addition: there is nothing here that contraction could change.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernels.h"

namespace fh {

namespace {

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// NV = 16-byte columns per lane and pass (a pass covers NV * 64 columns = NV * 256 floats), ROWS = rows whose loads are in flight.
// order == nullptr: the list is the consecutive rows begin, begin + 1, ... (the partials of one identity).
template <int NV, int ROWS>
__global__ __launch_bounds__(256) void fuse_sum_kernel(const float4* __restrict__ src, const int* __restrict__ order,
                                                       const FuseItem* __restrict__ items, long n_items, int vpr, float4* __restrict__ dst,
                                                       float4* __restrict__ part, int unit) {
    const long w = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (w >= n_items) return;
    const FuseItem it = items[w];
    float4* const out = (it.final ? dst : part) + (long)it.out * vpr;
    const bool one_pass = vpr <= NV * 64;
    float4 acc[NV];
    float sq = 0.f;
    for (int cb = 0; cb < vpr; cb += NV * 64) {
        bool act[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) act[v] = cb + v * 64 + lane < vpr;
        const int col = cb + lane;
        auto row_of = [&](int i) -> const float4* { return src + (long)(order ? order[it.begin + i] : it.begin + i) * vpr + col; };
        float4 buf[ROWS][NV];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
            if (r < it.count) {
                const float4* p = row_of(r);
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    if (act[v]) buf[r][v] = p[v * 64];
            }
        for (int i = 0; i < it.count; i += ROWS) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                if (i + r >= it.count) break;
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    if (act[v]) acc[v] = (i + r == 0) ? buf[r][v] : add4(acc[v], buf[r][v]);      // strictly in list order
                if (i + r + ROWS < it.count) {
                    const float4* p = row_of(i + r + ROWS);
#pragma unroll
                    for (int v = 0; v < NV; ++v)
                        if (act[v]) buf[r][v] = p[v * 64];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (act[v]) {
                sq += acc[v].x * acc[v].x + acc[v].y * acc[v].y + acc[v].z * acc[v].z + acc[v].w * acc[v].w;
                if (!one_pass) out[col + v * 64] = acc[v];
            }
    }
    // a one-row identity stays verbatim; partials are never normalised
    float norm = 0.f;
    if (unit && it.final && it.count > 1) norm = sqrtf(wave_sum(sq));
    const bool scale = norm > 0.f;                                // false for a zero sum and for NaN
    if (one_pass) {
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (v * 64 + lane < vpr) {
                const float4 a = acc[v];
                out[v * 64 + lane] = scale ? make_float4(a.x / norm, a.y / norm, a.z / norm, a.w / norm) : a;
            }
    } else if (scale) {                                           // dim > NV * 256: every lane re-reads the sums it stored itself
        for (int c = lane; c < vpr; c += 64) {
            const float4 a = out[c];
            out[c] = make_float4(a.x / norm, a.y / norm, a.z / norm, a.w / norm);
        }
    }
}

// one wave per src row: binary search of its id in tmpl's ascending distinct ids, then a 16-byte-per-lane dot product.  (A form with
// four rows per wave, their searches and loads interleaved, was measured slower at 1 M x 512: profiles/gallery_fuse.md.)
__global__ __launch_bounds__(256) void self_score_kernel(const float4* __restrict__ src, const int* __restrict__ src_ids, long n,
                                                         const float4* __restrict__ tmpl, const int* __restrict__ tmpl_ids, long m, int vpr,
                                                         float* __restrict__ out) {
    const long r = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const int id = src_ids[r];
    long lo = 0, hi = m;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (tmpl_ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (lo >= m || tmpl_ids[lo] != id) {
        if (lane == 0) out[r] = -1.0f;
        return;
    }
    const float4 *a = src + r * vpr, *b = tmpl + lo * vpr;
    float s = 0.f;
    for (int c = lane; c < vpr; c += 64) {
        const float4 x = a[c], y = b[c];
        s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    s = wave_sum(s);
    if (lane == 0) out[r] = (s + 1.0f) / 2.0f;
}

}  // namespace

void launch_gallery_fuse_sum(const float* src, const int* order, const FuseItem* items, long n_items, int dim, float* dst, float* part,
                             bool unit, hipStream_t s) {
    if (n_items <= 0) return;
    if (dim <= 0 || dim % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    const int vpr = dim / 4;
    const dim3 grid((unsigned)((n_items + 3) / 4)), block(256);
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4 *d4 = reinterpret_cast<float4*>(dst), *p4 = reinterpret_cast<float4*>(part);
    // 4 rows in flight per wave; 2 with eight columns per lane (rows of > 1024 floats), whose 4 rows would take 128 VGPRs on their own
    if (vpr <= 64) hipLaunchKernelGGL((fuse_sum_kernel<1, 4>), grid, block, 0, s, s4, order, items, n_items, vpr, d4, p4, unit ? 1 : 0);
    else if (vpr <= 128) hipLaunchKernelGGL((fuse_sum_kernel<2, 4>), grid, block, 0, s, s4, order, items, n_items, vpr, d4, p4, unit ? 1 : 0);
    else if (vpr <= 256) hipLaunchKernelGGL((fuse_sum_kernel<4, 4>), grid, block, 0, s, s4, order, items, n_items, vpr, d4, p4, unit ? 1 : 0);
    else hipLaunchKernelGGL((fuse_sum_kernel<8, 2>), grid, block, 0, s, s4, order, items, n_items, vpr, d4, p4, unit ? 1 : 0);
}

void launch_gallery_self_scores(const float* src, const int* src_ids, long n, const float* tmpl, const int* tmpl_ids, long m, int dim,
                                float* out, hipStream_t s) {
    if (n <= 0) return;
    if (dim <= 0 || dim % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    hipLaunchKernelGGL(self_score_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(src), src_ids, n,
                       reinterpret_cast<const float4*>(tmpl), tmpl_ids, m, dim / 4, out);
}

}  // namespace fh
