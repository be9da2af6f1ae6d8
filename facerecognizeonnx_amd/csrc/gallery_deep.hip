// gallery_deep.hip — exact top-k beyond the depth of the scan's register lists, behind fh_gallery_topk_deep_dev: the best k <= 1024 rows
// of every query, no threshold asked of the caller.  The rule, the block rule and its proof are deep_plan.h's; the score is the fp32
// scan's, bit for bit.  Three stages, none with an atomic or anything that depends on timing:
//   1. gallery_bmax_kernel: the streaming scan of gallery_scan.h instantiated with DEEP — the same K loop, operand placement and k order,
//      then the maximum eligible score per (32-row block, query) into bmax[ceil(G / 128) * 4][tiles_n * 64] (the size of the range call's
//      hit bitmap: 1.6 % of the fp32 rows at dim 512 and 256 queries).  A wave's 64 floats are 256 contiguous bytes.  No seed pass, no
//      part lists, no merge; every tile is multiplied (no tile skip for masks), a workgroup's tiles are the contiguous run of
//      gallery_parts_for.  Every word of bmax is written, so it is never cleared.
//   2. the CHOSEN blocks — the best min(k, #blocks with a maximum) blocks of a query by (maximum descending, block ascending).
//      deep_transpose_kernel turns bmax into bmax_t[query][block] through 64 x 64 LDS tiles, both sides coalesced (a query's column of
//      bmax is one word per 256-byte-or-longer row: read in place by one workgroup it costs a cache line per word, measured at 0.2 ms
//      per call at 1 M rows); then deep_select_kernel<false>, one workgroup per query, streams the query's row of bmax_t through the
//      "best so far + next batch, bitonic sort under gal_better" loop of range_list_kernel.  A block no better than the current k-th
//      entry never enters a batch.  The chosen blocks go to chosen[query][k], -1 behind them.
//   3. the rows of the chosen blocks.  deep_rescore_kernel, a wave per (query, chosen block): the block's 32 rows re-scored from the
//      fp32 rows with gal_rescore32 — the scan's own score of a single pair — eligibility applied per row, into cand[query][k][32]
//      (-inf for a row that is not eligible).  The 32 x 32 MFMA computes the query in every column, so this is matrix-core time, 256
//      MFMAs per block at dim 512: a grid over (query, block) spreads it over the chip.  Then deep_select_kernel<true>, one workgroup
//      per query, keeps the best k of the query's <= 32 k candidates by the same loop under gal_better on (score, global index), and
//      writes the lists, with ids gathered if asked for, and empty slots (-1.0f, -1, -1).
// By the block rule every entry of the exact top-k lies in a chosen block, so stage 3 reads at most 32 k rows per query whatever the data.
#include <hip/hip_runtime.h>

#include <climits>
#include <stdexcept>

#include "deep_plan.h"
#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

// ------------------------------------------------------------------------------------------ 1. the block maxima
__global__ __launch_bounds__(256, 2) void gallery_bmax_kernel(const GalArgs p) { gallery_scan_body<float, 1, true, false, false, false, true>(p); }

namespace {
constexpr int DP_THREADS = 1024, DP_WAVES = DP_THREADS / 64;
constexpr int DP_KMAX = GAL_DEEP_MAX;         // the deepest list
constexpr int DP_BATCH = 2048;                // candidates per sort
constexpr int DP_LOADS = 4;                   // words a thread has in flight
static_assert(DP_KMAX == kDeepMaxK && kDeepBlock == 32, "deep_plan.h's rule: blocks of 32 rows = one gal_rescore32");
static_assert(DP_BATCH >= 2 * DP_THREADS && DP_KMAX <= DP_BATCH && (DP_BATCH & (DP_BATCH - 1)) == 0,
              "a batch that is at most half full takes a step of the stream; [best | batch] sorts as 2 * DP_BATCH entries at most");

long deep_blocks(long G) { return (G + GAL_BM - 1) / GAL_BM * (GAL_BM / 32); }       // (a multiple of 4)
long deep_blocks_t(long G) { return (deep_blocks(G) + 63) / 64 * 64; }               // row length of bmax_t: whole 64-block tiles
int deep_qstride(int Q) { return (Q + GAL_BN - 1) / GAL_BN * GAL_BN; }
}  // namespace

size_t gallery_deep_bmax_bytes(long G, int Q) { return (size_t)deep_blocks(G) * deep_qstride(Q) * sizeof(float); }
size_t gallery_deep_bmax_t_bytes(long G, int Q) { return (size_t)deep_blocks_t(G) * deep_qstride(Q) * sizeof(float); }
size_t gallery_deep_chosen_bytes(int Q, int k) { return (size_t)Q * k * sizeof(int); }
size_t gallery_deep_cand_bytes(int Q, int k) { return (size_t)Q * k * 32 * sizeof(float); }

// ------------------------------------------------------------------------------------------ 2a. bmax [block][query] -> bmax_t [query][block]
// grid (64-block tiles, query tiles); blocks behind nblocks: -inf
__global__ __launch_bounds__(256) void deep_transpose_kernel(const float* __restrict__ bmax, long nblocks, int qs, long nbt, float* __restrict__ bmax_t) {
    __shared__ float tile[64][65];
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const long b0 = (long)blockIdx.x * 64;
    const int q0 = blockIdx.y * 64;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + 4 * i;
        tile[r][c] = b0 + r < nblocks ? bmax[(size_t)(b0 + r) * qs + q0 + c] : -INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + 4 * i;
        bmax_t[(size_t)(q0 + r) * nbt + b0 + c] = tile[c][r];
    }
}

// ------------------------------------------------------------------------------------------ 2b. / 3b. the best k of a stream of candidates
struct DeepSelect {
    const float* src;       // candidates of query qn: src[qn * stride + c], c < n; -inf: no candidate
    long stride;
    int n, k;
    const int* chosen_in;   // ROWS: [Q][k] the chosen blocks; candidate c is row c & 31 of block chosen_in[qn][c >> 5]
    long idx_base;
    const int* ids;         // ROWS: identity id of every row, or null
    int* chosen_out;        // !ROWS: [Q][k]
    float* out_s;           // ROWS: [Q][k], each may be null
    int* out_i;
    int* out_d;
};

// ROWS = false: candidate c is block c with its maximum, the list goes to chosen_out.  ROWS = true: candidate c is a row of a chosen
// block with its score, ranked with its global index; the list is the call's answer.
template <bool ROWS>
__global__ __launch_bounds__(DP_THREADS) void deep_select_kernel(const DeepSelect p) {
    __shared__ float ss[2 * DP_BATCH];        // [best so far (<= k) | candidates of the batch | padding], sorted in place
    __shared__ int si[2 * DP_BATCH];
    __shared__ int wsum[DP_WAVES];
    const int qn = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = p.k;
    int nbest = 0, npend = 0;                 // (workgroup-uniform: every branch on them is)
    float ts = -INFINITY;                     // the k-th entry once the list is full: what a candidate must beat
    int ti = INT_MAX;

    // a candidate per thread, or none: appended behind the batch in thread order (ballot + the waves' counts: no atomic).  Called by all
    // threads with room for DP_THREADS entries; ends behind a barrier.
    auto append = [&](bool pass, float s, int i) {
        const unsigned long long b = __ballot(pass);
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int off = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int v = 0; v < DP_WAVES; ++v) {
            const int c = wsum[v];
            off += v < wv ? c : 0;
            total += c;
        }
        if (pass) { ss[nbest + npend + off] = s; si[nbest + npend + off] = i; }
        npend += total;
        __syncthreads();                      // (also: wsum has been read before the next call writes it)
    };
    // [best so far | batch] -> sorted, the best k kept; the new k-th entry.  Called by all threads; ends behind a barrier.
    auto flush = [&]() {
        const int n = nbest + npend;
        int N = 2;
        while (N < n) N <<= 1;
        for (int i = n + tid; i < N; i += DP_THREADS) { ss[i] = -INFINITY; si[i] = INT_MAX; }      // below every candidate (each is > -inf)
        __syncthreads();
        for (int k2 = 2; k2 <= N; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < N; i += DP_THREADS) {
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
        nbest = min(n, k);
        npend = 0;
        if (nbest == k) { ts = ss[k - 1]; ti = si[k - 1]; }
    };

    const float* src = p.src + (size_t)qn * p.stride;
    for (int c0 = 0; c0 < p.n; c0 += DP_LOADS * DP_THREADS) {
        float v[DP_LOADS];
#pragma unroll
        for (int u = 0; u < DP_LOADS; ++u) {
            const int c = c0 + u * DP_THREADS + tid;
            v[u] = c < p.n ? src[c] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < DP_LOADS; ++u) {
            if (c0 + u * DP_THREADS >= p.n) break;                         // (workgroup-uniform)
            const int c = c0 + u * DP_THREADS + tid;
            const bool there = v[u] > -INFINITY;                           // (false for a NaN: stage 1 and the re-score write none)
            int i = c;
            if constexpr (ROWS) i = there ? (int)(p.idx_base + (long)p.chosen_in[(size_t)qn * k + (c >> 5)] * 32 + (c & 31)) : INT_MAX;
            if (npend + DP_THREADS > DP_BATCH) flush();
            append(there && (nbest < k || gal_better(v[u], i, ts, ti)), v[u], i);
        }
    }
    if (npend > 0) flush();
    __syncthreads();
    for (int i = tid; i < k; i += DP_THREADS) {
        const bool there = i < nbest;
        const size_t o = (size_t)qn * k + i;
        const int gi = there ? si[i] : -1;
        if constexpr (ROWS) {
            if (p.out_s) p.out_s[o] = there ? ss[i] : -1.0f;
            if (p.out_i) p.out_i[o] = gi;
            if (p.out_d) p.out_d[o] = there ? p.ids[gi - p.idx_base] : -1;
        } else {
            p.chosen_out[o] = gi;
        }
    }
}

// ------------------------------------------------------------------------------------------ 3a. the rows of the chosen blocks
struct DeepRescore {
    const float* gal;       // fp32 rows [G][dim]
    const float* q;         // queries [>= Q][dim]
    const float* zeros;
    const unsigned* tags;   // tag of every row, with masks
    const unsigned* masks;  // mask of every query, or null
    const int* chosen;      // [Q][k], -1: no block
    long G;
    int dim, k;
    float* cand;            // [Q][k][32]
};

// grid (ceil(k / 4), Q): wave wv of a workgroup takes chosen block 4 * blockIdx.x + wv of query blockIdx.y.  No LDS, no barrier.
__global__ __launch_bounds__(256) void deep_rescore_kernel(const DeepRescore p) {
    const int qn = blockIdx.y, lane = threadIdx.x & 63, fr = lane & 31, fh2 = lane >> 5;
    const int c = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (c >= p.k) return;                                                  // (wave-uniform)
    float* out = p.cand + ((size_t)qn * p.k + c) * 32;
    const int b = p.chosen[(size_t)qn * p.k + c];
    if (b < 0) {                                                           // (wave-uniform)
        if (fh2 == 0) out[fr] = -INFINITY;
        return;
    }
    const int K = p.dim;
    const long row = (long)b * 32 + fr;
    const bool live = row < p.G;
    const GalSrc<float> a = gal_row_or_zeros(live, p.gal, (size_t)row, K, p.zeros, fh2 * 4, 64);
    const v16f acc = gal_rescore32(a.ptr, a.step, p.q + (size_t)qn * K + fh2 * 4, K / 64);
    // every column of the result is the same; lane (fr, fh2) holds rows gal_acc_row(e) + 4 * fh2, and row fr = gal_acc_row(esel) + 4 * hsel:
    // one select and one exchange with lane ^ 32 put row fr of the block in lane fr
    const int esel = ((fr >> 3) << 2) | (fr & 3), hsel = (fr >> 2) & 1;
    float v = acc[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) v = e == esel ? acc[e] : v;
    const float w = __shfl_xor(v, 32);                                     // the same element of the other half
    const float sc = gal_score(hsel == fh2 ? v : w);
    const unsigned mq = p.masks ? p.masks[qn] : 0xFFFFFFFFu;
    const unsigned tag = p.masks && live ? p.tags[row] : 0xFFFFFFFFu;
    const bool ok = live && (tag & mq) != 0 && sc > -INFINITY;             // (false for a NaN score)
    if (fh2 == 0) out[fr] = ok ? sc : -INFINITY;
}

// ------------------------------------------------------------------------------------------ the call
void launch_gallery_deep(const float* rows, long G, int dim, const float* qpacked, const unsigned* tags, const unsigned* masks, int Q,
                         long idx_base, int k, float* bmax, float* bmax_t, int* chosen, float* cand, const int* ids, float* out_s,
                         int* out_i, int* out_d, hipStream_t s) {
    if (Q <= 0) return;
    if (dim % 64 || k < 1 || k > DP_KMAX) throw std::runtime_error("gallery deep top-k: need dim % 64 == 0 and 1 <= k <= 1024");
    if (G < 0 || idx_base + G > (long)INT_MAX) throw std::runtime_error("gallery: global row indices must fit in 31 bits");
    const int tiles_n = (Q + GAL_BN - 1) / GAL_BN, qs = tiles_n * GAL_BN;
    const long nblocks = deep_blocks(G), nbt = deep_blocks_t(G);
    if (G > 0) {
        GalArgs a{};
        a.gal = rows; a.q = qpacked; a.zeros = conv_zero_line(); a.G = G; a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.k = 1;
        a.tiles_n = tiles_n; a.row_tiles = (int)((G + GAL_BM - 1) / GAL_BM);
        a.tags = masks ? tags : nullptr; a.qmask = masks;
        a.bmax = bmax;
        const int parts = gallery_parts_for(G, Q, GAL_WG_PER_CU, LONG_MAX, &a.tiles_per_part);
        hipLaunchKernelGGL(gallery_bmax_kernel, dim3((unsigned)(parts * tiles_n)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(deep_transpose_kernel, dim3((unsigned)(nbt / 64), (unsigned)tiles_n), dim3(256), 0, s, bmax, nblocks, qs, nbt, bmax_t);
    }
    DeepSelect b{};
    b.src = bmax_t; b.stride = nbt; b.n = (int)nblocks; b.k = k; b.chosen_out = chosen;
    hipLaunchKernelGGL(deep_select_kernel<false>, dim3((unsigned)Q), dim3(DP_THREADS), 0, s, b);
    DeepRescore r{};
    r.gal = rows; r.q = qpacked; r.zeros = conv_zero_line(); r.tags = masks ? tags : nullptr; r.masks = masks; r.chosen = chosen;
    r.G = G; r.dim = dim; r.k = k; r.cand = cand;
    hipLaunchKernelGGL(deep_rescore_kernel, dim3((unsigned)((k + 3) / 4), (unsigned)Q), dim3(256), 0, s, r);
    DeepSelect l{};
    l.src = cand; l.stride = (long)k * 32; l.n = k * 32; l.k = k; l.chosen_in = chosen; l.idx_base = idx_base; l.ids = ids;
    l.out_s = out_s; l.out_i = out_i; l.out_d = out_d;
    hipLaunchKernelGGL(deep_select_kernel<true>, dim3((unsigned)Q), dim3(DP_THREADS), 0, s, l);
}

}  // namespace fh
