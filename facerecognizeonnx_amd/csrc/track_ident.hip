// track_ident.hip — per-track identity on the device (contract: include/facehip.h, "track identity"; fh_track_identify_dev).  After an
// update the flagged faces of a call have embeddings; stage A pools each of them into its track's running template and writes one query
// row per flagged face, the gallery labels all queries at once (the existing 1:N calls, no code here), and stage C carries the answers
// to every face of the call.  Both kernels walk a stream's entries in the order of track_plan.h, 64 entries per round.
//   * the SUMS are plain fp32 additions in time order, so they reproduce bit for bit (tests/track_ident_model.py restates them); the
//     unit form is FaceRecognizer::normalize (src/face_recognizer.cpp:306-318) with gallery_fuse.hip's reduction: a lane-strided sum
//     of squares, then a butterfly.  Compiled with -ffp-contract=off, as track.hip.
//   * no atomics and nothing that depends on timing: a (stream, slot) chain belongs to one wave, a stream's labels to one wave.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace fh {

namespace {

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(const float w, const float4 a) { return make_float4(w * a.x, w * a.y, w * a.z, w * a.w); }
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
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

}  // namespace

// ------------------------------------------------------------------------------------------
// The flagged entries before each frame (track_select_kernel's prefix, kept): frame_off[0 .. n].  n <= 4096 frames.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void track_ranks_kernel(const int* __restrict__ embed, int n, int per_frame, int* __restrict__ frame_off) {
    __shared__ int offs[4097];
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
    for (int b = threadIdx.x; b <= n; b += 256) frame_off[b] = offs[b];
}

// ------------------------------------------------------------------------------------------
// Stage A.  Wave (s, l), l < max_tracks, owns slot l of stream s: it picks the flagged entries whose slot is l with a ballot and runs
// their chain in time order — (re)open: sum = row, query = row verbatim; else sum += row (POOL_SUM; POOL_LAST: sum = row) and the
// query is the normalised sum.  POOL_WEIGHTED is POOL_SUM with every row entering the sum as wq * row, wq = (float)max(quality, 1): one
// multiply, then one add per component (the file is built without contraction).  Wave (s, max_tracks) copies the rows of the stream's
// untracked faces.  Each lane owns the 16-byte
// columns lane, lane + 64, ...; the sum row lives in the state and is read, added to and written back by the lane that owns the column.
// A flagged entry of rank >= total is nobody's.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void track_pool_kernel(TrackIdent* __restrict__ ident, float4* __restrict__ sums, int streams,
                                                         int max_tracks, int vpr, int pool, const int* __restrict__ track,
                                                         const int* __restrict__ slot, const int* __restrict__ embed,
                                                         const int* __restrict__ quality, const int* __restrict__ frame_off, const float4* __restrict__ emb, int total,
                                                         int per_frame, const int* __restrict__ order, const int* __restrict__ starts,
                                                         float4* __restrict__ queries) {
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (w >= streams * (max_tracks + 1)) return;
    const int s = w / (max_tracks + 1), l = w - s * (max_tracks + 1);
    const int my = l < max_tracks ? l : -1;                              // -1: the untracked faces
    const int b = starts[s], e = starts[s + 1];
    if (b == e) return;
    TrackIdent* const id = ident + (size_t)s * max_tracks + (my < 0 ? 0 : my);
    float4* const sm = sums + ((size_t)s * max_tracks + (my < 0 ? 0 : my)) * vpr;
    int owner = -1, n_emb = 0;
    if (my >= 0) { owner = id->owner; n_emb = id->n_emb; }
    const bool weighted = pool == kTrackPoolWeighted;

    walk_entries(order, b, e, per_frame, embed, frame_off, lane, [&](bool, int, int, size_t idx, bool fl, int rank) {
        const int sl = fl ? slot[idx] : -2;
        const int tid = fl ? track[idx] : -1;
        const int qual = (weighted && fl) ? quality[idx] : 1;
        unsigned long long m = __ballot(fl && rank < total && sl == my);
        while (m != 0) {                                                 // ascending lanes = (frame, slot) order = time order
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int q_e = __shfl(rank, src), t_e = __shfl(tid, src);
            const float wq = (float)max(__shfl(qual, src), 1);
            const float4* const row = emb + (size_t)q_e * vpr;
            float4* const q = queries + (size_t)q_e * vpr;
            if (my < 0) {
                for (int c = lane; c < vpr; c += 64) q[c] = row[c];
            } else if (owner != t_e || pool == kTrackPoolLast) {
                if (owner != t_e) { owner = t_e; n_emb = 1; } else ++n_emb;
                for (int c = lane; c < vpr; c += 64) {
                    const float4 v = row[c];
                    sm[c] = weighted ? mul4(wq, v) : v;
                    q[c] = v;
                }
            } else {
                ++n_emb;
                float sq = 0.f;
                for (int c = lane; c < vpr; c += 64) {
                    const float4 a = add4(sm[c], weighted ? mul4(wq, row[c]) : row[c]);
                    sm[c] = a;
                    sq += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
                }
                const float norm = sqrtf(wave_sum(sq));
                const bool scale = norm > 0.f;                           // false for a zero sum and for NaN
                for (int c = lane; c < vpr; c += 64) {                   // (every lane re-reads the sums it stored itself)
                    const float4 a = sm[c];
                    q[c] = scale ? make_float4(a.x / norm, a.y / norm, a.z / norm, a.w / norm) : a;
                }
            }
        }
    });
    if (my >= 0 && lane == 0) { id->owner = owner; id->n_emb = n_emb; }
}

// ------------------------------------------------------------------------------------------
// Stage C.  One wave per stream; lane l holds (owner, label, score) of slot l in registers for the whole walk (loaded once, stored
// once), as track_update_kernel holds its slots.  A round's frames are taken in time order; inside one frame a slot occurs at most
// once, so its carried reads (a shuffle from the slot's lane) and its refreshes (one step per flagged face) do not meet.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void track_propagate_kernel(TrackIdent* __restrict__ ident, int max_tracks, const int* __restrict__ track,
                                                             const int* __restrict__ slot, const int* __restrict__ embed,
                                                             const int* __restrict__ frame_off, const int* __restrict__ ans_label,
                                                             const float* __restrict__ ans_score, int total, int per_frame,
                                                             const int* __restrict__ order, const int* __restrict__ starts,
                                                             int* __restrict__ label, float* __restrict__ score) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = starts[s], e = starts[s + 1];
    if (b == e) return;
    const bool usable = lane < max_tracks;
    TrackIdent st{-1, 0, -1, -1.0f};
    if (usable) st = ident[(size_t)s * max_tracks + lane];

    walk_entries(order, b, e, per_frame, embed, frame_off, lane, [&](bool valid, int k, int nk, size_t idx, bool fl, int rank) {
        const int sl = valid ? slot[idx] : -1;
        const int tid = valid ? track[idx] : -1;
        int ol = -1;
        float os = -1.0f;
        const bool known = fl && rank < total;                           // a flagged entry behind `total` answers (-1, -1) and changes nothing
        if (known) { ol = ans_label[rank]; os = ans_score[rank]; }
        const bool upd = known && sl >= 0, carry = valid && !fl && sl >= 0;
        for (int kk = 0; kk < nk; ++kk) {
            if (__ballot(carry && k == kk) != 0) {
                const int cl = __shfl(st.label, sl & 63);
                const float cs = __shfl(st.score, sl & 63);
                if (carry && k == kk) { ol = cl; os = cs; }
            }
            unsigned long long m = __ballot(upd && k == kk);
            while (m != 0) {
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int t_slot = __shfl(sl, src), t_id = __shfl(tid, src), t_label = __shfl(ol, src);
                const float t_score = __shfl(os, src);
                if (lane == t_slot) { st.owner = t_id; st.label = t_label; st.score = t_score; }
            }
        }
        if (valid) { label[idx] = ol; score[idx] = os; }
    });
    if (usable) {
        TrackIdent* const id = ident + (size_t)s * max_tracks + lane;
        id->owner = st.owner; id->label = st.label; id->score = st.score;      // (n_emb is stage A's)
    }
}

void launch_track_ranks(const int* embed, int n, int per_frame, int* frame_off, hipStream_t s) {
    hipLaunchKernelGGL(track_ranks_kernel, dim3(1), dim3(256), 0, s, embed, n, per_frame, frame_off);
}

void launch_track_pool(TrackIdent* ident, float* sums, int streams, int max_tracks, int dim, int pool, const int* track, const int* slot,
                       const int* embed, const int* quality, const int* frame_off, const float* emb, int total, int per_frame, const int* order,
                       const int* starts, float* queries, hipStream_t s) {
    const int waves = streams * (max_tracks + 1);
    hipLaunchKernelGGL(track_pool_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, ident, reinterpret_cast<float4*>(sums), streams,
                       max_tracks, dim / 4, pool, track, slot, embed, quality, frame_off, reinterpret_cast<const float4*>(emb), total, per_frame,
                       order, starts, reinterpret_cast<float4*>(queries));
}

void launch_track_propagate(TrackIdent* ident, int streams, int max_tracks, const int* track, const int* slot, const int* embed,
                            const int* frame_off, const int* ans_label, const float* ans_score, int total, int per_frame, const int* order,
                            const int* starts, int* label, float* score, hipStream_t s) {
    hipLaunchKernelGGL(track_propagate_kernel, dim3(streams), dim3(64), 0, s, ident, max_tracks, track, slot, embed, frame_off, ans_label,
                       ans_score, total, per_frame, order, starts, label, score);
}

}  // namespace fh
