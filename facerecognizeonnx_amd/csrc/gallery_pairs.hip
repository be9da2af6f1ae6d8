// gallery_pairs.hip — the one-workgroup kernels of the pair audit (fh_gallery_pairs_dev; the rule: pairs_plan.h; the two pair passes and
// the scratch layout: gallery_cluster.hip).
//   cut      after the count pass: pairs_cut — the host rule's own function — over the 2048 counters by rank.  Writes the caller's
//            info {count, nan, returned, complete} and, into the scratch, the last rank the collect pass takes and `returned`.
//   select   after the collect pass: the candidates {score, i, j} lie in the scratch in an order that depends on timing; the kernel keeps
//            the best `cap` under the TOTAL order pairs_before (score, then i, then j: no two candidates compare equal) — best so far +
//            the next 1024, bitonic sort in LDS, as range_list_kernel does with two fields — so the lists do not depend on that order.
//            Then scores, positions, the ids of the listed rows, and (-1.0f, -1, -1) behind `returned`.
//   empty    an empty gallery: info {0, 0, 0, 1} and empty lists.
// Everything here reads what an EARLIER launch wrote: plain loads.
#include <hip/hip_runtime.h>

#include <climits>

#include "kernels.h"
#include "pairs_plan.h"

namespace fh {

namespace {
constexpr int PS_BATCH = 1024;                // candidates per sort = the largest cap
static_assert(PS_BATCH >= kPairsMaxCap && kPairsSlots == kHistBins + 1, "a batch holds the largest cap; kernels.h mirrors roc_plan.h");

__global__ __launch_bounds__(256) void pairs_cut_kernel(unsigned long long* scratch, int cap, unsigned long long room, unsigned long long* info) {
    __shared__ uint64_t by_rank[kHistBins];
    for (int i = threadIdx.x; i < kHistBins; i += 256) by_rank[i] = scratch[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long res[4] = {0ull, scratch[kHistBins], 0ull, 1ull};
    const int last = pairs_cut(by_rank, cap, room, res);
    for (int k = 0; k < 4; ++k) info[k] = res[k];
    reinterpret_cast<int*>(scratch + kPairsSlots)[0] = last;
    scratch[kPairsSlots + 1] = res[2];
}

__device__ __forceinline__ void pairs_write(int i, bool live, float s, int r0, int r1, const int* ids, float* out_s, int* out_rows, int* out_ids) {
    if (out_s) out_s[i] = live ? s : -1.0f;
    if (out_rows) { out_rows[2 * i] = live ? r0 : -1; out_rows[2 * i + 1] = live ? r1 : -1; }
    if (out_ids) { out_ids[2 * i] = live ? ids[r0] : -1; out_ids[2 * i + 1] = live ? ids[r1] : -1; }
}

__global__ __launch_bounds__(256) void pairs_select_kernel(const unsigned long long* __restrict__ scratch, unsigned room, int side, int cap,
                                                           const int* __restrict__ ids, float* out_s, int* out_rows, int* out_ids) {
    __shared__ float ss[2 * PS_BATCH];        // [best so far (<= cap) | candidates of the batch | padding], sorted in place
    __shared__ int si[2 * PS_BATCH];
    __shared__ int sj[2 * PS_BATCH];
    const int tid = threadIdx.x;
    const unsigned appended = reinterpret_cast<const unsigned*>(scratch + kPairsSlots)[1];
    const unsigned total = appended < room ? appended : room;              // (the cut keeps appended <= room)
    const unsigned long long returned = scratch[kPairsSlots + 1];
    const int4* cand = reinterpret_cast<const int4*>(scratch + kPairsHead);
    const float worst = side == kPairsAbove ? -INFINITY : INFINITY;
    int nbest = 0;                            // (workgroup-uniform)
    for (unsigned c0 = 0; c0 < total; c0 += PS_BATCH) {
        const int take = (int)(total - c0 < (unsigned)PS_BATCH ? total - c0 : (unsigned)PS_BATCH);
        __syncthreads();
        for (int i = tid; i < take; i += 256) {
            const int4 v = cand[c0 + i];
            ss[nbest + i] = __uint_as_float((unsigned)v.x); si[nbest + i] = v.y; sj[nbest + i] = v.z;
        }
        const int n = nbest + take;
        int N = 2;
        while (N < n) N <<= 1;
        for (int i = n + tid; i < N; i += 256) { ss[i] = worst; si[i] = INT_MAX; sj[i] = INT_MAX; }     // behind every candidate
        __syncthreads();
        for (int k2 = 2; k2 <= N; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < N; i += 256) {
                    const int o = i ^ j;
                    if (o > i) {
                        const float s1 = ss[i], s2 = ss[o];
                        const int i1 = si[i], i2 = si[o], j1 = sj[i], j2 = sj[o];
                        const bool swap = (i & k2) == 0 ? pairs_before(side, s2, i2, j2, s1, i1, j1) : pairs_before(side, s1, i1, j1, s2, i2, j2);
                        if (swap) { ss[i] = s2; si[i] = i2; sj[i] = j2; ss[o] = s1; si[o] = i1; sj[o] = j1; }
                    }
                }
                __syncthreads();
            }
        nbest = n < cap ? n : cap;
    }
    __syncthreads();
    const int listed = returned < (unsigned long long)nbest ? (int)returned : nbest;      // (returned <= nbest by the cut rule)
    for (int i = tid; i < cap; i += 256) {
        const bool live = i < listed;
        pairs_write(i, live, live ? ss[i] : 0.f, live ? si[i] : 0, live ? sj[i] : 0, ids, out_s, out_rows, out_ids);
    }
}

__global__ __launch_bounds__(256) void pairs_empty_kernel(int cap, unsigned long long* info, float* out_s, int* out_rows, int* out_ids) {
    const int tid = threadIdx.x;
    if (tid < 4) info[tid] = tid == 3 ? 1ull : 0ull;
    for (int i = tid; i < cap; i += 256) pairs_write(i, false, 0.f, 0, 0, nullptr, out_s, out_rows, out_ids);
}
}  // namespace

void launch_pairs_cut(unsigned long long* scratch, int cap, long room, unsigned long long* info, hipStream_t s) {
    hipLaunchKernelGGL(pairs_cut_kernel, dim3(1), dim3(256), 0, s, scratch, cap, (unsigned long long)room, info);
}

void launch_pairs_select(const unsigned long long* scratch, long room, int side, int cap, const int* ids, float* out_s, int* out_rows,
                         int* out_ids, hipStream_t s) {
    if (!out_s && !out_rows && !out_ids) return;
    hipLaunchKernelGGL(pairs_select_kernel, dim3(1), dim3(256), 0, s, scratch, (unsigned)room, side, cap, ids, out_s, out_rows, out_ids);
}

void launch_pairs_empty(int cap, unsigned long long* info, float* out_s, int* out_rows, int* out_ids, hipStream_t s) {
    hipLaunchKernelGGL(pairs_empty_kernel, dim3(1), dim3(256), 0, s, cap, info, out_s, out_rows, out_ids);
}

}  // namespace fh
