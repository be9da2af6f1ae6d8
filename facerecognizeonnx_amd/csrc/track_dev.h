// track_dev.h — the device pieces that the tracker's kernels share (track.hip, track_ident.hip): the per-frame prefix of the embed
// flags, the walk over a stream's entries, and the ONE pooling step of a track's template.  Both files are built with -ffp-contract=off;
// the fp32 here is in a stated order, which tests/track_ident_model.py and tests/track_link_model.py restate bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace fh {
namespace {
__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(const float w, const float4 a) { return make_float4(w * a.x, w * a.y, w * a.z, w * a.w); }
// component-wise choice (a float4 chosen whole at run time would live in scratch)
__device__ __forceinline__ float4 sel4(bool c, const float4 a, const float4 b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// offs[0 .. n] = the flagged entries before each frame (offs[n] = all of them), n <= 4096 frames: the per-frame counts by the
// workgroup's 256 threads, then a serial scan by thread 0.  Called by the whole workgroup; offs (LDS, n + 1 ints) is ready on return.
__device__ __forceinline__ void flagged_prefix(const int* __restrict__ embed, int n, int per_frame, int* offs) {
    for (int b = threadIdx.x; b < n; b += 256) {
        int c = 0;
        for (int j = 0; j < per_frame; ++j) c += embed[(size_t)b * per_frame + j] != 0;
        offs[b + 1] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        offs[0] = 0;
        for (int b = 1; b <= n; ++b) { acc += offs[b]; offs[b] = acc; }
    }
    __syncthreads();
}

// The entries of frames order[b .. e) in time order, 64 per round, one per lane.  per_frame <= 64: a round holds the next 64 / per_frame
// whole frames, lane = k * per_frame + j; otherwise a round is one 64-entry piece of one frame.  body(valid, k, nk, idx, flagged, rank)
// is called by the WHOLE wave once per round: k = the lane's frame within the round (nk of them), idx = f * per_frame + j, rank = the
// entry's position among the call's flagged entries in (frame, slot) order (meaningful where flagged).  Every loop bound is uniform.
template <class Body>
__device__ __forceinline__ void walk_entries(const int* __restrict__ order, int b, int e, int per_frame, const int* __restrict__ embed,
                                             const int* __restrict__ frame_off, int lane, Body&& body) {
    if (per_frame <= 64) {
        const int G = 64 / per_frame, k = lane / per_frame, j = lane - k * per_frame;
        const unsigned long long before = ((1ull << j) - 1ull) << (k * per_frame);      // the lanes of my frame in front of me
        for (int i0 = b; i0 < e; i0 += G) {
            const int nk = min(G, e - i0);
            const bool valid = k < nk;
            const int f = valid ? order[i0 + k] : 0;
            const size_t idx = (size_t)f * per_frame + j;
            const bool fl = valid && embed[idx] != 0;
            const unsigned long long flm = __ballot(fl);
            body(valid, k, nk, idx, fl, frame_off[f] + __popcll(flm & before));
        }
    } else {
        for (int i = b; i < e; ++i) {
            const int f = order[i];
            int base = frame_off[f];
            for (int j0 = 0; j0 < per_frame; j0 += 64) {
                const bool valid = j0 + lane < per_frame;
                const size_t idx = (size_t)f * per_frame + j0 + lane;
                const bool fl = valid && embed[idx] != 0;
                const unsigned long long flm = __ballot(fl);
                body(valid, 0, 1, idx, fl, base + __popcll(flm & ((1ull << lane) - 1ull)));
                base += __popcll(flm);
            }
        }
    }
}

// One face enters a track's template: the whole wave, each lane on the 16-byte columns lane, lane + 64, ... of the rows (vpr columns).
// in = wq * row when `weighted`, else row: one multiply, then (accumulating) one add per component.
//   * accumulate == false — a track that opens, unlinked, or POOL_LAST (never weighted): sm = in, and the query q is the row verbatim;
//   * accumulate == true: sm = base + in, and q = sm / ||sm|| — the sum of squares over the lane's own columns in ascending order,
//     then the butterfly, then sqrtf, one division per component; unscaled when the norm is 0 or NaN.  base is sm itself for a
//     continued track and the winner's row for a track that resumes a lost one.
// retire (may be null) takes the slot's OLD sums.  Every column is read whole before it is written, by its lane: the rows may coincide.
__device__ __forceinline__ void pool_row(float4* sm, const float4* base, const float4* row, float4* q, float4* retire, float wq,
                                         bool weighted, bool accumulate, int lane, int vpr) {
    float sq = 0.f;
    for (int c = lane; c < vpr; c += 64) {
        const float4 old = sm[c], b4 = base[c], v = row[c];
        const float4 in = sel4(weighted, mul4(wq, v), v);
        if (retire) retire[c] = old;
        if (accumulate) {
            const float4 a = add4(b4, in);
            sm[c] = a;
            sq += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
        } else {
            sm[c] = in;
            q[c] = v;
        }
    }
    if (!accumulate) return;
    const float norm = sqrtf(wave_sum(sq));
    const bool scale = norm > 0.f;                                       // false for a zero sum and for NaN
    for (int c = lane; c < vpr; c += 64) {                               // (every lane re-reads the sums it stored itself)
        const float4 a = sm[c];
        q[c] = scale ? make_float4(a.x / norm, a.y / norm, a.z / norm, a.w / norm) : a;
    }
}
}  // namespace
}  // namespace fh
