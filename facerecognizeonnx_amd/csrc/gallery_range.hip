// gallery_range.hip — exact threshold (range) search behind fh_gallery_range_dev: EVERY row whose mapped score is above a threshold, not
// the best k <= 16 of them.  The rule is range_plan.h's; the score is the fp32 scan's, bit for bit.  Three stages, none with an atomic or
// anything that depends on timing:
//   1. gallery_range_kernel: the streaming scan of gallery_scan.h instantiated with RANGE — the same K loop, operand placement and k
//      order, then the hit test on the accumulators and ONE 32-bit word per (32-row block, query) into the hit bitmap
//      hits[ceil(G / 128) * 4][tiles_n * 64] (at most ceil(G / 32) * 256 * 4 bytes: 1.6 % of the fp32 rows at dim 512).  A wave's 64 words
//      are 256 contiguous bytes.  No seed pass, no part lists, no merge; every tile is multiplied (no tile skip for masks), a
//      workgroup's tiles are the contiguous run of gallery_parts_for.  Every word of the bitmap is written, so it is never cleared.
//   2. range_unit_count_kernel + range_total_kernel: popcounts per (unit of 256 row blocks = 8192 rows, query), then their sum per query
//      = d_counts.  The count-only form of the call ends here.
//   3. range_list_kernel, one workgroup per query: it walks the units that hold a hit in row order (the unit counts say which), turns
//      the bits into row positions (a prefix sum over the 256 words of a unit keeps row order), re-scores them 32 at a time from the
//      fp32 rows with gal_rescore32 — the scan's own score of a single pair — and keeps the best `cap` by a bitonic sort in LDS of
//      [best so far | the next <= 1024 candidates] under gal_better.  So a count above cap still yields the BEST cap hits.  Then the
//      lists are written, with ids gathered if asked for, and empty slots (-1.0f, -1, -1).
// The cost of stage 3 grows with the number of hits: a threshold that admits a large share of the gallery is slow, and still right.
#include <hip/hip_runtime.h>

#include <climits>
#include <stdexcept>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

// ------------------------------------------------------------------------------------------ 1. the hit bitmap
__global__ __launch_bounds__(256, 2) void gallery_range_kernel(const GalArgs p) { gallery_scan_body<float, 1, true, false, false, true>(p); }

namespace {
constexpr int RG_UNIT = GAL_RANGE_UNIT;       // row blocks per unit: one word per thread of the list kernel
constexpr int RG_BATCH = 1024;                // candidates per sort = the largest cap
static_assert(RG_UNIT == 256 && RG_BATCH >= 1024, "one word per thread; a batch holds the largest cap");

long range_blocks(long G) { return (G + GAL_BM - 1) / GAL_BM * (GAL_BM / 32); }
long range_units(long G) { return (range_blocks(G) + RG_UNIT - 1) / RG_UNIT; }
int range_qstride(int Q) { return (Q + GAL_BN - 1) / GAL_BN * GAL_BN; }
}  // namespace

size_t gallery_range_hits_bytes(long G, int Q) { return (size_t)range_blocks(G) * range_qstride(Q) * sizeof(unsigned); }
size_t gallery_range_units_bytes(long G, int Q) { return (size_t)range_units(G) * range_qstride(Q) * sizeof(int); }

// ------------------------------------------------------------------------------------------ 2. counts
// grid (units, query tiles); thread (query ql, quarter sub) sums 64 words of its column: a wave reads 256 contiguous bytes per step
__global__ __launch_bounds__(256) void range_unit_count_kernel(const unsigned* __restrict__ hits, long nblocks, int qs, int* __restrict__ unit_cnt) {
    __shared__ int part[4][GAL_BN];
    const int ql = threadIdx.x & 63, sub = threadIdx.x >> 6, q = blockIdx.y * GAL_BN + ql;
    const long b0 = (long)blockIdx.x * RG_UNIT + sub * (RG_UNIT / 4);
    int c = 0;
    for (int i = 0; i < RG_UNIT / 4; ++i)
        if (b0 + i < nblocks) c += __popc(hits[(size_t)(b0 + i) * qs + q]);
    part[sub][ql] = c;
    __syncthreads();
    if (sub == 0) unit_cnt[(size_t)blockIdx.x * qs + q] = part[0][ql] + part[1][ql] + part[2][ql] + part[3][ql];
}

// grid (query tiles): counts[q] = sum over the units, in 64 bits
__global__ __launch_bounds__(256) void range_total_kernel(const int* __restrict__ unit_cnt, long nunits, int qs, int Q, long long* __restrict__ counts) {
    __shared__ long long part[4][GAL_BN];
    const int ql = threadIdx.x & 63, sub = threadIdx.x >> 6, q = blockIdx.x * GAL_BN + ql;
    long long c = 0;
    for (long u = sub; u < nunits; u += 4) c += unit_cnt[(size_t)u * qs + q];
    part[sub][ql] = c;
    __syncthreads();
    if (sub == 0 && q < Q) counts[q] = part[0][ql] + part[1][ql] + part[2][ql] + part[3][ql];
}

// ------------------------------------------------------------------------------------------ 3. lists
struct RangeList {
    const float* gal;       // fp32 rows [G][dim]
    const float* q;         // queries [>= Q][dim]
    const float* zeros;
    const unsigned* hits;   // [nblocks][qs]
    const int* unit_cnt;    // [nunits][qs]
    const int* ids;         // identity id of every row, or null
    long nblocks, nunits, idx_base;
    int dim, qs, cap;
    float* out_s;           // [Q][cap], each may be null
    int* out_i;
    int* out_d;
};

__global__ __launch_bounds__(256) void range_list_kernel(const RangeList p) {
    __shared__ float ss[2 * RG_BATCH];        // [best so far (<= cap) | candidates of the batch | padding], sorted in place
    __shared__ int si[2 * RG_BATCH];
    __shared__ int pend[RG_BATCH];            // row positions of the batch, in row order
    __shared__ int ucnt[256];
    __shared__ int wsum[4];
    const int qn = blockIdx.x, tid = threadIdx.x, lane = tid & 63, fr = lane & 31, fh2 = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = p.dim, chunks = K / 64;
    const float* qrow = p.q + (size_t)qn * K;
    int nbest = 0, npend = 0;                 // (workgroup-uniform: every branch on them is)

    // the batch: re-score, append behind the best so far, sort, keep the best cap.  Called by all threads; ends behind a barrier.
    auto flush = [&]() {
        for (int g = wv; g < (npend + 31) / 32; g += 4) {                  // a wave per 32 candidates
            const int c = g * 32 + fr;
            const bool live = c < npend;
            const int pos = live ? pend[c] : 0;
            const GalSrc<float> a = gal_row_or_zeros(live, p.gal, (size_t)pos, K, p.zeros, fh2 * 4, 64);
            const v16f acc = gal_rescore32(a.ptr, a.step, qrow + fh2 * 4, chunks);
            if (fr == 0) {                                                 // column 0: candidates gal_acc_row(e) + 4 * fh2 of the group
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int r = g * 32 + gal_acc_row(e) + 4 * fh2;
                    if (r < npend) ss[nbest + r] = gal_score(acc[e]);
                }
            }
            if (live && fh2 == 0) si[nbest + c] = (int)(p.idx_base + pos);
        }
        const int n = nbest + npend;
        int N = 2;
        while (N < n) N <<= 1;
        for (int i = n + tid; i < N; i += 256) { ss[i] = -INFINITY; si[i] = INT_MAX; }      // below every hit (a hit's score is above a threshold)
        __syncthreads();
        for (int k2 = 2; k2 <= N; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < N; i += 256) {
                    const int o = i ^ j;
                    if (o > i) {
                        const float s1 = ss[i], s2 = ss[o];
                        const int i1 = si[i], i2 = si[o];
                        const bool swap = (i & k2) == 0 ? gal_better(s2, i2, s1, i1) : gal_better(s1, i1, s2, i2);
                        if (swap) { ss[i] = s2; si[i] = i2; ss[o] = s1; si[o] = i1; }
                    }
                }
                __syncthreads();
            }
        nbest = min(n, p.cap);
        npend = 0;
    };

    for (long u0 = 0; u0 < p.nunits; u0 += 256) {                          // 256 unit counts at a time, then only the units that hold a hit
        __syncthreads();
        ucnt[tid] = u0 + tid < p.nunits ? p.unit_cnt[(size_t)(u0 + tid) * p.qs + qn] : 0;
        __syncthreads();
        for (int j = 0; j < 256; ++j) {
            const int total = ucnt[j];
            if (total == 0) continue;
            const long b = (u0 + j) * RG_UNIT + tid;                       // this thread's row block
            const unsigned w = b < p.nblocks ? p.hits[(size_t)b * p.qs + qn] : 0u;
            const int c = __popc(w);
            int incl = c;                                                  // inclusive prefix sum of c over the workgroup: row order
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            int off = incl - c;
            for (int v = 0; v < wv; ++v) off += wsum[v];
            for (int done = 0; done < total;) {                            // append the unit's hits, a batch's room at a time
                const int take = min(RG_BATCH - npend, total - done);
                unsigned ww = w;
                for (int o = off; ww; ++o) {
                    const int bit = __ffs((int)ww) - 1;
                    ww &= ww - 1;
                    if (o >= done && o < done + take) pend[npend + o - done] = (int)(b * 32 + bit);
                }
                npend += take; done += take;
                __syncthreads();                                           // (also: wsum has been read before the next unit writes it)
                if (npend == RG_BATCH) flush();
            }
        }
    }
    if (npend > 0) flush();
    __syncthreads();
    for (int i = tid; i < p.cap; i += 256) {
        const bool live = i < nbest;
        const size_t o = (size_t)qn * p.cap + i;
        const int gi = live ? si[i] : -1;
        if (p.out_s) p.out_s[o] = live ? ss[i] : -1.0f;
        if (p.out_i) p.out_i[o] = gi;
        if (p.out_d) p.out_d[o] = live ? p.ids[gi - p.idx_base] : -1;
    }
}

// ------------------------------------------------------------------------------------------ the call
void launch_gallery_range(const float* rows, long G, int dim, const float* qpacked, const unsigned* tags, const unsigned* masks, int Q,
                          long idx_base, float thr, int cap, unsigned* hits, int* unit_cnt, const int* ids, long long* counts, float* out_s,
                          int* out_i, int* out_d, hipStream_t s) {
    if (Q <= 0) return;
    if (dim % 64 || cap < 1 || cap > RG_BATCH) throw std::runtime_error("gallery range: need dim % 64 == 0 and 1 <= cap <= 1024");
    if (G < 0 || idx_base + G > (long)INT_MAX) throw std::runtime_error("gallery: global row indices must fit in 31 bits");
    const int tiles_n = (Q + GAL_BN - 1) / GAL_BN, qs = tiles_n * GAL_BN;
    const long nblocks = range_blocks(G), nunits = range_units(G);
    if (G > 0) {
        GalArgs a{};
        a.gal = rows; a.q = qpacked; a.zeros = conv_zero_line(); a.G = G; a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.k = 1;
        a.tiles_n = tiles_n; a.row_tiles = (int)((G + GAL_BM - 1) / GAL_BM);
        a.tags = masks ? tags : nullptr; a.qmask = masks;
        a.range_thr = thr; a.hits = hits;
        const int parts = gallery_parts_for(G, Q, GAL_WG_PER_CU, LONG_MAX, &a.tiles_per_part);
        hipLaunchKernelGGL(gallery_range_kernel, dim3((unsigned)(parts * tiles_n)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(range_unit_count_kernel, dim3((unsigned)nunits, (unsigned)tiles_n), dim3(256), 0, s, hits, nblocks, qs, unit_cnt);
    }
    hipLaunchKernelGGL(range_total_kernel, dim3((unsigned)tiles_n), dim3(256), 0, s, unit_cnt, nunits, qs, Q, counts);
    if (!out_s && !out_i && !out_d) return;
    RangeList l{};
    l.gal = rows; l.q = qpacked; l.zeros = conv_zero_line(); l.hits = hits; l.unit_cnt = unit_cnt; l.ids = ids;
    l.nblocks = nblocks; l.nunits = nunits; l.idx_base = idx_base; l.dim = dim; l.qs = qs; l.cap = cap;
    l.out_s = out_s; l.out_i = out_i; l.out_d = out_d;
    hipLaunchKernelGGL(range_list_kernel, dim3((unsigned)Q), dim3(256), 0, s, l);
}

}  // namespace fh
