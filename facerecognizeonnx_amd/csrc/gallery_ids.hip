// gallery_ids.hip — the LABELLED gallery: every enrolled row carries an identity id, and a query is answered with its best k
// identities instead of its best k rows (a person enrolled with 20 templates takes one slot, not sixteen).
//   * row score: exactly gallery_topk_kernel's — the scan is the same code (gallery_scan.h), instantiated with identity-aware lists;
//   * order: entry (s, r) is better than (s', r') iff s > s', or s == s' and r < r' (r = global row index);
//   * an identity's representative is its best row; the answer is the first k representatives; a slot holds (score, id, row), an
//     empty slot (-1.0f, -1, -1); NaN scores are never listed.
// Per-workgroup lists go to memory as [part][Q][k] in three planes; topk_merge_ids_kernel selects the overall answer.  It is also the
// merge step of a row-sharded labelled gallery (fh_topk_merge_ids_dev), because per-part identity lists suffice:
//   suppose identity X is in the global answer and its representative lies in part p.  Every identity ahead of X within part p has a
//   part-best at least as good as X's representative, so its global best is at least as good, and it is ahead of X globally as well.
//   Fewer than k identities are ahead of X globally, so fewer than k are ahead of X in part p: X is in part p's list, with that same
//   representative.  De-duplicating the union of the part lists (keep an identity's best entry) therefore yields the global answer.
// The same argument keeps the seed pass valid: if k distinct identities of a prefix score at least tau, tau admits every member of
// the final answer.  What changes against the row-level scan is the overflow replay: many templates of one identity can pass the
// threshold of a tile while the list does not tighten (they share one slot), so the four-round replay fires more often.
// Removal (fh_gallery_remove_ids) is a stable compaction: a host-built list of the surviving positions, then a gather of whole rows
// (fp32 rows, ids, fp16 rows) into a second buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <stdexcept>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

__global__ __launch_bounds__(256, 2) void gallery_topk_ids_kernel(const GalArgs p) { gallery_scan_body<true>(p); }

// topk_merge_kernel's scheme (face_kernels.hip) with a third plane: one workgroup per query, k rounds of "best entry that comes after
// the previous pick", and an entry whose identity has been picked (at most 15 of them) is out.  CACHED: the nparts * k <= 8192 entries
// are read once into registers and a pick strikes its identity's other entries there; otherwise every round re-reads the lists from
// memory (L2) and tests the picked ids, which the workgroup keeps in LDS.
template <bool CACHED>
__global__ __launch_bounds__(256) void topk_merge_ids_kernel(const float* __restrict__ ps, const int* __restrict__ pd, const int* __restrict__ pi,
                                                             int nparts, int Q, int k, long part_stride, float* __restrict__ out_s,
                                                             int* __restrict__ out_d, int* __restrict__ out_i, const int* __restrict__ qcount) {
    __shared__ float rs[256];
    __shared__ int ri[256];
    __shared__ int rd[256];
    __shared__ int picked[GAL_KMAX];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (qcount && q >= *qcount) return;
    const int total = nparts * k;
    constexpr int E = 32;
    float es[E]; int ei[E], ed[E];
    if (CACHED) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int e = j * 256 + tid;
            es[j] = -INFINITY; ei[j] = -1; ed[j] = -1;
            if (e < total) {
                const int part = e / k, pos = e - part * k;
                const size_t o = (size_t)part * part_stride + (size_t)q * k + pos;
                es[j] = ps[o]; ei[j] = pi[o]; ed[j] = pd[o];
            }
        }
    }
    float last_s = 0.f; int last_i = -1, last_d = -1; bool have_last = false, exhausted = false;
    for (int round = 0; round < k; ++round) {
        float best_s = -INFINITY; int best_i = INT_MAX, best_d = -1;        // (emptiness is told by the row index, not by the score)
        if (CACHED) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const float sc = es[j]; const int gi = ei[j];
                const bool ok = !exhausted && gi >= 0 && (!have_last || gal_better(last_s, last_i, sc, gi)) && gal_better(sc, gi, best_s, best_i);
                best_s = ok ? sc : best_s; best_i = ok ? gi : best_i; best_d = ok ? ed[j] : best_d;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {               // wave reduction
                const float os = __shfl_xor(best_s, o); const int oi = __shfl_xor(best_i, o), od = __shfl_xor(best_d, o);
                const bool t = gal_better(os, oi, best_s, best_i);
                best_s = t ? os : best_s; best_i = t ? oi : best_i; best_d = t ? od : best_d;
            }
            if (lane == 0) { rs[wv] = best_s; ri[wv] = best_i; rd[wv] = best_d; }
            __syncthreads();
            best_s = rs[0]; best_i = ri[0]; best_d = rd[0];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (gal_better(rs[w], ri[w], best_s, best_i)) { best_s = rs[w]; best_i = ri[w]; best_d = rd[w]; }
            __syncthreads();
            last_s = best_s; last_i = best_i; last_d = best_d;
            if (last_i != INT_MAX) {
#pragma unroll
                for (int j = 0; j < E; ++j) ei[j] = ed[j] == last_d ? -1 : ei[j];     // the picked identity's other entries are out
            }
        } else {
            for (int e = tid; e < total; e += 256) {
                const int part = e / k, pos = e - part * k;
                const size_t o = (size_t)part * part_stride + (size_t)q * k + pos;
                const float sc = ps[o]; const int gi = pi[o];
                if (gi < 0 || exhausted) continue;
                if (have_last && !gal_better(last_s, last_i, sc, gi)) continue;     // must come strictly after the last pick
                if (!gal_better(sc, gi, best_s, best_i)) continue;
                const int id = pd[o];
                bool taken = false;
                for (int r = 0; r < round; ++r) taken |= picked[r] == id;
                if (!taken) { best_s = sc; best_i = gi; best_d = id; }
            }
            rs[tid] = best_s; ri[tid] = best_i; rd[tid] = best_d;
            __syncthreads();
            for (int st = 128; st > 0; st >>= 1) {
                if (tid < st && gal_better(rs[tid + st], ri[tid + st], rs[tid], ri[tid])) {
                    rs[tid] = rs[tid + st]; ri[tid] = ri[tid + st]; rd[tid] = rd[tid + st];
                }
                __syncthreads();
            }
            last_s = rs[0]; last_i = ri[0]; last_d = rd[0];
            if (tid == 0) picked[round] = last_d;
            __syncthreads();
        }
        have_last = true;
        if (tid == 0) {
            const bool found = last_i != INT_MAX;
            out_s[(size_t)q * k + round] = found ? last_s : -1.0f;
            out_d[(size_t)q * k + round] = found ? last_d : -1;
            if (out_i) out_i[(size_t)q * k + round] = found ? last_i : -1;
        }
        if (last_i == INT_MAX) exhausted = true;         // nothing left: later rounds find nothing either (workgroup-uniform)
    }
}

void launch_topk_merge_ids(const float* part_score, const int* part_id, const int* part_idx, int nparts, int Q, int k, float* out_score,
                           int* out_id, int* out_idx, hipStream_t s, const int* qcount) {
    if (Q <= 0) return;
    const long stride = (long)Q * k;
    if ((long)nparts * k <= 8192)
        hipLaunchKernelGGL(topk_merge_ids_kernel<true>, dim3(Q), dim3(256), 0, s, part_score, part_id, part_idx, nparts, Q, k, stride, out_score,
                           out_id, out_idx, qcount);
    else
        hipLaunchKernelGGL(topk_merge_ids_kernel<false>, dim3(Q), dim3(256), 0, s, part_score, part_id, part_idx, nparts, Q, k, stride, out_score,
                           out_id, out_idx, qcount);
}

// the two passes of launch_gallery_topk (gallery.hip): identity top-k of the first rows as admission thresholds, then the full scan
void launch_gallery_topk_ids(const float* gal, const int* ids, long G, int dim, const float* qpacked, int Q, int k, long idx_base,
                             float* part_score, int* part_idx, int* part_id, float* seed_score, int* seed_idx, int* seed_id, hipStream_t s) {
    if (G <= 0 || Q <= 0) return;
    if (dim % 64 || k < 1 || k > GAL_KMAX) throw std::runtime_error("gallery: need dim % 64 == 0 and 1 <= k <= 16");
    if (idx_base + G > (long)INT_MAX) throw std::runtime_error("gallery: global row indices must fit in 31 bits");
    GalArgs a{};
    a.gal = gal; a.ids = ids; a.q = qpacked; a.zeros = conv_zero_line(); a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.k = k;
    a.tiles_n = (Q + GAL_BN - 1) / GAL_BN;
    a.ps = part_score; a.pi = part_idx; a.pd = part_id;
    constexpr long GAL_SEED_ROWS = 4096;
    if (G >= 16 * GAL_SEED_ROWS && seed_score && seed_idx && seed_id) {
        a.G = GAL_SEED_ROWS;
        a.row_tiles = (int)(GAL_SEED_ROWS / GAL_BM);
        const int sp = gallery_parts(a.G, Q, &a.tiles_per_part);
        hipLaunchKernelGGL(gallery_topk_ids_kernel, dim3((unsigned)(sp * a.tiles_n)), dim3(256), 0, s, a);
        launch_topk_merge_ids(part_score, part_id, part_idx, sp, Q, k, seed_score, seed_id, seed_idx, s);
        a.seed_s = seed_score; a.seed_i = seed_idx;
    }
    a.G = G;
    a.row_tiles = (int)((G + GAL_BM - 1) / GAL_BM);
    const int parts = gallery_parts(G, Q, &a.tiles_per_part);
    hipLaunchKernelGGL(gallery_topk_ids_kernel, dim3((unsigned)(parts * a.tiles_n)), dim3(256), 0, s, a);
}

__global__ void ids_of_rows_kernel(const float* __restrict__ score, const int* __restrict__ idx, int n, const int* __restrict__ ids, long idx_base,
                                   float thr, int use_thr, int* __restrict__ out_id) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = idx[i];
    out_id[i] = (r >= 0 && (!use_thr || score[i] > thr)) ? ids[(long)r - idx_base] : -1;
}
void launch_ids_of_rows(const float* score, const int* idx, int n, const int* ids, long idx_base, float thr, bool use_thr, int* out_id,
                        hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(ids_of_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, score, idx, n, ids, idx_base, thr, use_thr ? 1 : 0, out_id);
}

// dst row j = src row map[j], 16 bytes per thread
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ map,
                                                          long m, int vec_per_row) {
    const long total = m * vec_per_row;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long j = e / vec_per_row;
        const int c = (int)(e - j * vec_per_row);
        dst[e] = src[(long)map[j] * vec_per_row + c];
    }
}
void launch_gather_rows(const void* src, void* dst, const int* map, long m, size_t row_bytes, hipStream_t s) {
    if (m <= 0) return;
    if (row_bytes % 16) throw std::runtime_error("gallery: row size must be a multiple of 16 bytes");
    const int vpr = (int)(row_bytes / 16);
    const long blocks = std::min<long>((m * vpr + 255) / 256, 65536);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const uint4*>(src), static_cast<uint4*>(dst), map, m, vpr);
}
__global__ void gather_ids_kernel(const int* __restrict__ src, int* __restrict__ dst, const int* __restrict__ map, long m) {
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (long)gridDim.x * blockDim.x) dst[j] = src[map[j]];
}
void launch_gather_ids(const int* src, int* dst, const int* map, long m, hipStream_t s) {
    if (m <= 0) return;
    const long blocks = std::min<long>((m + 255) / 256, 65536);
    hipLaunchKernelGGL(gather_ids_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, map, m);
}

}  // namespace fh
