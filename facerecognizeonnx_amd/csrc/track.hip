// track.hip — the device-resident face tracker between the detector's NMS and the face selection (contract: include/facehip.h, "face
// tracker").  Integers and FaceDetector::iou (face_iou.h) only, so that a CPU model (tests/track_model.py) holds it to the bit.
// Compiled with -ffp-contract=off, as face_kernels.hip.
#include <hip/hip_runtime.h>

#include "face_iou.h"
#include "kernels.h"
#include "track_dev.h"

namespace fh {

static_assert(sizeof(TrackState) == 32, "fh_track_state is 32 bytes");

// every non-NaN float as an unsigned that orders the same way (and is never 0)
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ------------------------------------------------------------------------------------------
// One wave per stream; lane l owns slot l in registers for the whole walk of the stream's slice of `order` (state loaded once, stored
// once).  Per frame: expire, then for each detection in score order the live, not yet taken slots compute their IoU in lanes; the
// winner is the largest (iou, then smaller id) — found by a 64-lane butterfly on (ordered iou bits, 0x7fffffff - id) when more than
// one slot qualifies — and an unmatched detection opens the lowest free slot (__ballot + find-first-set).  Every branch below that
// contains a cross-lane operation is taken by the whole wave: its condition comes from a ballot, a shuffle or a kernel argument.
// No atomics: a stream belongs to one wave.  slot (optional, [n][per_frame]): the lane that holds the detection's track, -1 for an untracked
// detection and for the entries behind the count — what the identity step (track_ident.hip) keys its per-slot state by.
// Best shot (quality and best_q both given, else nothing below differs from the plain update): lane l also keeps best_q of slot l in a
// register beside st — the quality of the best face of the track embedded so far; an opened track starts it, and a matched track whose
// face has become better than best_q by the ratio num / den, min_gap frames or more after its last embedding, is embedded again.  The
// qualities of a chunk travel through LDS with its boxes.  BESTSHOT is a template parameter so that the plain update compiles to the
// code it was: nothing of the policy is left in it.
// ------------------------------------------------------------------------------------------
template <bool BESTSHOT>
__global__ __launch_bounds__(64) void track_update_kernel(int* __restrict__ heads, TrackState* __restrict__ slots, TrackParams p,
                                                          const FaceRec* __restrict__ det, const int* __restrict__ counts, int per_frame,
                                                          const int* __restrict__ order, const int* __restrict__ starts,
                                                          int* __restrict__ track, int* __restrict__ embed, int* __restrict__ slot,
                                                          const int* __restrict__ quality, int* __restrict__ best_q) {
    __shared__ int4 sbox[64];
    __shared__ int squal[64];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = starts[s], e = starts[s + 1];
    if (b == e) return;                                                 // no frame of this stream in the call
    const bool usable = lane < p.max_tracks;
    TrackState st = kFreeTrack;
    if (usable) st = slots[(size_t)s * p.max_tracks + lane];
    constexpr bool bestshot = BESTSHOT;                                 // (the launcher: quality and best_q are both given)
    int bq = 0;
    if (bestshot && usable) bq = best_q[(size_t)s * p.max_tracks + lane];
    int t = heads[2 * s], next_id = heads[2 * s + 1];

    for (int i0 = b; i0 < e; i0 += 64) {
        // the next 64 frames of the slice and their counts: one round of loads, handed out by shuffles
        const int nf = min(64, e - i0);
        int my_f = 0, my_c = 0;
        if (lane < nf) {
            my_f = order[i0 + lane];
            my_c = min(max(counts[my_f], 0), per_frame);
        }
        for (int k = 0; k < nf; ++k) {
            const int f = __shfl(my_f, k), c = __shfl(my_c, k);
            const size_t row = (size_t)f * per_frame;
            // 1. expire: more than max_missed frames have passed without this track
            if (st.id >= 0 && t - st.last_seen - 1 > p.max_missed) st.id = -1;
            bool taken = false;                                         // matched or opened in this frame
            for (int j0 = 0; j0 < c; j0 += 64) {
                const int nj = min(64, c - j0);
                __syncthreads();                                        // (one wave: orders the LDS reads of the previous chunk)
                if (lane < nj) {
                    const FaceRec& r = det[row + j0 + lane];
                    sbox[lane] = make_int4(r.x, r.y, r.w, r.h);
                    if (bestshot) squal[lane] = quality[row + j0 + lane];
                }
                __syncthreads();
                for (int jj = 0; jj < nj; ++jj) {
                    const int4 box = sbox[jj];
                    const size_t o = row + j0 + jj;
                    // 2. match
                    const float iou = iou_int(make_int4(st.x, st.y, st.w, st.h), box) + 0.0f;    // (+ 0: -0 and +0 are one value)
                    const bool qual = st.id >= 0 && !taken && iou > p.iou_thr;                   // strict: NaN fails
                    const unsigned long long qm = __ballot(qual);
                    if (qm != 0) {
                        int win = __ffsll((long long)qm) - 1;
                        if (qm & (qm - 1)) {                            // several candidates: the largest (iou, then smaller id)
                            const unsigned hi = qual ? ordered_bits(iou) : 0u, lo = qual ? 0x7fffffffu - (unsigned)st.id : 0u;
                            unsigned mh = hi, ml = lo;
                            for (int off = 32; off > 0; off >>= 1) {
                                const unsigned oh = __shfl_xor(mh, off), ol = __shfl_xor(ml, off);
                                if (oh > mh || (oh == mh && ol > ml)) { mh = oh; ml = ol; }
                            }
                            win = __ffsll((long long)__ballot(qual && hi == mh && lo == ml)) - 1;    // ids are distinct: one lane
                        }
                        if (lane == win) {
                            st.x = box.x; st.y = box.y; st.w = box.z; st.h = box.w;
                            st.last_seen = t;
                            st.hits += 1;
                            taken = true;
                            int again = (p.refresh > 0 && t - st.last_embed >= p.refresh) ? 1 : 0;
                            if (bestshot) {
                                const int q = squal[jj];
                                if ((long long)q * p.bs_den > (long long)bq * p.bs_num && t - st.last_embed >= p.bs_gap) again = 1;
                                if (again) bq = max(bq, q);
                            }
                            if (again) st.last_embed = t;
                            track[o] = st.id;
                            embed[o] = again;
                            if (slot) slot[o] = lane;
                        }
                    } else {
                        // 3. open: the lowest free slot, or untracked (and embedded, as the reference embeds every face)
                        const unsigned long long fm = __ballot(usable && st.id < 0);
                        if (fm != 0) {
                            if (lane == __ffsll((long long)fm) - 1) {
                                st = TrackState{next_id, box.x, box.y, box.z, box.w, t, t, 1};
                                if (bestshot) bq = squal[jj];
                                taken = true;
                                track[o] = next_id;
                                embed[o] = 1;
                                if (slot) slot[o] = lane;
                            }
                            ++next_id;
                        } else if (lane == 0) {
                            track[o] = -1;
                            embed[o] = 1;
                            if (slot) slot[o] = -1;
                        }
                    }
                }
            }
            // 4. close the frame
            for (int j = c + lane; j < per_frame; j += 64) {
                track[row + j] = -1;
                embed[row + j] = 0;
                if (slot) slot[row + j] = -1;
            }
            ++t;
        }
    }
    if (usable) slots[(size_t)s * p.max_tracks + lane] = st;
    if (bestshot && usable) best_q[(size_t)s * p.max_tracks + lane] = bq;
    if (lane == 0) { heads[2 * s] = t; heads[2 * s + 1] = next_id; }
}

void launch_track_update(int* heads, TrackState* slots, int streams, TrackParams p, const FaceRec* det, const int* counts, int per_frame,
                         const int* order, const int* starts, int* track, int* embed, int* slot, const int* quality, int* best_q,
                         hipStream_t s) {
    if (quality && best_q)
        hipLaunchKernelGGL(track_update_kernel<true>, dim3(streams), dim3(64), 0, s, heads, slots, p, det, counts, per_frame, order, starts,
                           track, embed, slot, quality, best_q);
    else
        hipLaunchKernelGGL(track_update_kernel<false>, dim3(streams), dim3(64), 0, s, heads, slots, p, det, counts, per_frame, order, starts,
                           track, embed, slot, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------
// The flagged twin of select_faces_kernel (face_kernels.hip): the records whose embed flag is set, densely in (frame, slot) order,
// each with its frame index and track id.  total[0] = their number.  n <= 4096 frames.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void track_select_kernel(const FaceRec* __restrict__ det, const int* __restrict__ embed,
                                                           const int* __restrict__ trk, int n, int per_frame, FaceRec* __restrict__ faces,
                                                           int* __restrict__ frame_of, int* __restrict__ track_of, int* __restrict__ total) {
    __shared__ int offs[4097];
    flagged_prefix(embed, n, per_frame, offs);
    if (threadIdx.x == 0) total[0] = offs[n];
    for (int b = threadIdx.x; b < n; b += 256) {
        int o = offs[b];
        for (int j = 0; j < per_frame; ++j) {
            const size_t src = (size_t)b * per_frame + j;
            if (embed[src] == 0) continue;
            faces[o] = det[src];
            frame_of[o] = b;
            track_of[o] = trk[src];
            ++o;
        }
    }
}

void launch_track_select(const FaceRec* det, const int* embed, const int* track, int n, int per_frame, FaceRec* faces, int* frame_of,
                         int* track_of, int* total, hipStream_t s) {
    hipLaunchKernelGGL(track_select_kernel, dim3(1), dim3(256), 0, s, det, embed, track, n, per_frame, faces, frame_of, track_of, total);
}

}  // namespace fh
