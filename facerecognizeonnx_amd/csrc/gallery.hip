// gallery.hip — 1:N generalisation of FaceRecognizer::compareFaces (reference src/face_recognizer.cpp:320-334): every query against
// every enrolled row, mapped score (dot + 1) / 2, top-k per query ranked (score desc, global row index asc).
// Here: the row-level instantiation of the streaming scan (gallery_scan.h holds the scan, its design notes and measurements), the
// two-pass launcher every scan goes through, launch_gallery_scan — the one launcher of the four fp32 scans — and the merge of the
// per-workgroup lists — also the merge step of a row-sharded gallery (fh_topk_merge_dev, fh_topk_merge_ids_dev).
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

__global__ __launch_bounds__(256, 2) void gallery_topk_kernel(const GalArgs p) { gallery_scan_body<float, GAL_KMAX, false, false>(p); }

// parts the row range is cut into for a gallery of G rows and a query batch of Q (the caller sizes its partial-list buffers with it):
// one per resident workgroup, at most max_parts per query tile
int gallery_parts_for(long G, int Q, int wg_per_cu, long max_parts, int* tiles_per_part) {
    const int tiles_n = (Q + GAL_BN - 1) / GAL_BN;
    const long row_tiles = (G + GAL_BM - 1) / GAL_BM;
    long parts = (long)conv_num_cus() * wg_per_cu / tiles_n;
    if (parts > max_parts) parts = max_parts;
    if (parts < 1) parts = 1;
    if (parts > row_tiles) parts = row_tiles;
    const long tpp = parts > 0 ? (row_tiles + parts - 1) / parts : 1;
    if (tiles_per_part) *tiles_per_part = (int)tpp;
    return (int)(tpp > 0 ? (row_tiles + tpp - 1) / tpp : 0);
}
int gallery_parts(long G, int Q, int* tiles_per_part) { return gallery_parts_for(G, Q, GAL_WG_PER_CU, LONG_MAX, tiles_per_part); }

void gallery_check_args(const GalScan& sc, const GalArgs& a, long G) {
    if (a.dim % sc.chunk || a.k < 1 || a.k > sc.depth)
        throw std::runtime_error(std::string(sc.name) + ": need dim % " + std::to_string(sc.chunk) + " == 0 and 1 <= k <= " + std::to_string(sc.depth));
    if (a.idx_base + G > (long)INT_MAX) throw std::runtime_error("gallery: global row indices must fit in 31 bits");
    if (a.qcount && !sc.has_qcount) throw std::runtime_error("gallery: this scan takes no device query count");
}

int launch_gallery_two_pass(const GalScan& sc, GalArgs a, long G, bool seed, float* seed_s, int* seed_i, int* seed_d, hipStream_t s) {
    gallery_check_args(sc, a, G);
    a.zeros = conv_zero_line();
    a.tiles_n = (a.Q + GAL_BN - 1) / GAL_BN;
    a.seed_s = nullptr; a.seed_i = nullptr;
    constexpr long GAL_SEED_ROWS = 4096;
    if (seed && G >= 16 * GAL_SEED_ROWS && seed_s && seed_i && (seed_d || !a.pd)) {
        a.G = GAL_SEED_ROWS;
        a.row_tiles = (int)(GAL_SEED_ROWS / GAL_BM);
        const int sp = gallery_parts_for(a.G, a.Q, sc.wg_per_cu, sc.max_parts, &a.tiles_per_part);
        hipLaunchKernelGGL(sc.kernel, dim3((unsigned)(sp * a.tiles_n)), dim3(256), 0, s, a);
        if (a.pd) launch_topk_merge_ids(a.ps, a.pd, a.pi, sp, a.Q, a.k, seed_s, seed_d, seed_i, s);
        else launch_topk_merge(a.ps, a.pi, sp, a.Q, a.k, seed_s, seed_i, s);
        a.seed_s = seed_s; a.seed_i = seed_i;
    }
    a.G = G;
    a.row_tiles = (int)((G + GAL_BM - 1) / GAL_BM);
    const int parts = gallery_parts_for(G, a.Q, sc.wg_per_cu, sc.max_parts, &a.tiles_per_part);
    hipLaunchKernelGGL(sc.kernel, dim3((unsigned)(parts * a.tiles_n)), dim3(256), 0, s, a);
    return parts;
}

// The one launcher of the fp32 scans.  The kernel comes from a table indexed by (lists of identities?, tags?): a.ids / a.qmask say which.
namespace {
std::atomic<int> g_tag_skip{1};
}
void gallery_debug_tag_skip(int on) { g_tag_skip.store(on != 0); }

void launch_gallery_scan(GalArgs a, long G, float* seed_s, int* seed_i, int* seed_d, hipStream_t s) {
    if (G <= 0 || a.Q <= 0) return;
    static int seed_on = -1;
    if (seed_on < 0) { const char* e = getenv("FACEHIP_GAL_SEED"); seed_on = e ? atoi(e) : 1; }     // (0: no seed pass — A / B timing of the plain row scan)
    static const GalScan scans[2][2] = {
        {{"gallery", gallery_topk_kernel, /*chunk*/ 64, /*depth*/ GAL_KMAX, GAL_WG_PER_CU, /*max_parts*/ LONG_MAX, /*has_qcount*/ true},
         {"gallery (tagged)", gallery_topk_tagged_kernel, 64, GAL_KMAX, GAL_WG_PER_CU, LONG_MAX, true}},
        {{"gallery", gallery_topk_ids_kernel, 64, GAL_KMAX, GAL_WG_PER_CU, LONG_MAX, true},
         {"gallery (tagged)", gallery_topk_ids_tagged_kernel, 64, GAL_KMAX, GAL_WG_PER_CU, LONG_MAX, true}}};
    const bool ids = a.ids != nullptr, tags = a.qmask != nullptr;
    a.tag_skip = g_tag_skip.load();
    launch_gallery_two_pass(scans[ids][tags], a, G, ids || tags || seed_on != 0, seed_s, seed_i, seed_d, s);
}

// ------------------------------------------------------------------------------------------ the merge of the part lists
// One workgroup per query: k rounds of "best entry that comes after the previous pick".
// CACHED: the nparts * k <= 8192 candidate entries are read ONCE into registers (32 per thread) and every round is a register scan +
// a wave reduction + one LDS hand-off between the four waves; otherwise each round re-reads the lists from memory (L2).
// IDS: lists of identities (a third plane, pd / out_d); an entry whose identity has been picked (at most 15 of them) is out.  CACHED, a
// pick strikes its identity's other entries in the registers; otherwise the picked ids are kept in LDS and tested.  out_i may be null.
// ID is an empty pack (lists of rows: topk_merge_kernel<CACHED>) or one `true` (lists of identities: topk_merge_kernel<CACHED, true>): the
// id planes pd / out_d are parameters only in the second, so each instantiation has exactly the argument list it reads (a row-level
// merge's nine arguments fit one 64-byte line of the kernarg segment).
template <bool, class P> using IdPlane = P;
template <class P> __device__ __forceinline__ P id_plane() { return nullptr; }
template <class P> __device__ __forceinline__ P id_plane(P p) { return p; }
template <bool CACHED, bool... ID>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ ps, IdPlane<ID, const int* __restrict__>... pd_,
                                                         const int* __restrict__ pi, int nparts, int Q, int k, long part_stride,
                                                         float* __restrict__ out_s, IdPlane<ID, int* __restrict__>... out_d_,
                                                         int* __restrict__ out_i, const int* __restrict__ qcount) {
    constexpr bool IDS = sizeof...(ID) > 0;
    const int* __restrict__ const pd = id_plane<const int*>(pd_...);
    int* __restrict__ const out_d = id_plane<int*>(out_d_...);
    __shared__ float rs[256];
    __shared__ int ri[256];
    __shared__ int rd[IDS ? 256 : 1];
    __shared__ int picked[GAL_KMAX];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (qcount && q >= *qcount) return;                  // (optional device query count: the compacted fall-back of the f16 re-rank scan)
    const int total = nparts * k;
    constexpr int E = 32;
    float es[E]; int ei[E], ed[IDS ? E : 1];
    if (CACHED) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int e = j * 256 + tid;
            es[j] = -INFINITY; ei[j] = -1;
            if constexpr (IDS) ed[j] = -1;
            if (e < total) {
                const int part = e / k, pos = e - part * k;
                const size_t o = (size_t)part * part_stride + (size_t)q * k + pos;
                es[j] = ps[o]; ei[j] = pi[o];
                if constexpr (IDS) ed[j] = pd[o];
            }
        }
    }
    float last_s = 0.f; int last_i = -1, last_d = -1; bool have_last = false, exhausted = false;
    for (int round = 0; round < k; ++round) {
        float best_s = -INFINITY; int best_i = INT_MAX, best_d = -1;        // (emptiness is told by the index, not by the score: rows need not be unit vectors)
        if (CACHED) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const float sc = es[j]; const int gi = ei[j];
                const bool ok = !exhausted && gi >= 0 && (!have_last || gal_better(last_s, last_i, sc, gi)) && gal_better(sc, gi, best_s, best_i);
                best_s = ok ? sc : best_s; best_i = ok ? gi : best_i;
                if constexpr (IDS) best_d = ok ? ed[j] : best_d;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {               // wave reduction
                const float os = __shfl_xor(best_s, o); const int oi = __shfl_xor(best_i, o), od = IDS ? __shfl_xor(best_d, o) : -1;
                const bool t = gal_better(os, oi, best_s, best_i);
                best_s = t ? os : best_s; best_i = t ? oi : best_i; best_d = t ? od : best_d;
            }
            if (lane == 0) { rs[wv] = best_s; ri[wv] = best_i; if constexpr (IDS) rd[wv] = best_d; }
            __syncthreads();
            best_s = rs[0]; best_i = ri[0];
            if constexpr (IDS) best_d = rd[0];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (gal_better(rs[w], ri[w], best_s, best_i)) { best_s = rs[w]; best_i = ri[w]; if constexpr (IDS) best_d = rd[w]; }
            __syncthreads();
            last_s = best_s; last_i = best_i; last_d = best_d;
            if constexpr (IDS) {
                if (last_i != INT_MAX) {
#pragma unroll
                    for (int j = 0; j < E; ++j) ei[j] = ed[j] == last_d ? -1 : ei[j];     // the picked identity's other entries are out
                }
            }
        } else {
            for (int e = tid; e < total; e += 256) {
                const int part = e / k, pos = e - part * k;
                const size_t o = (size_t)part * part_stride + (size_t)q * k + pos;
                const float sc = ps[o]; const int gi = pi[o];
                if (gi < 0 || exhausted) continue;
                if (have_last && !gal_better(last_s, last_i, sc, gi)) continue;     // must come strictly after the last pick
                if (!gal_better(sc, gi, best_s, best_i)) continue;
                int id = -1;
                bool taken = false;
                if constexpr (IDS) {
                    id = pd[o];
                    for (int r = 0; r < round; ++r) taken |= picked[r] == id;
                }
                if (!taken) { best_s = sc; best_i = gi; best_d = id; }
            }
            rs[tid] = best_s; ri[tid] = best_i;
            if constexpr (IDS) rd[tid] = best_d;
            __syncthreads();
            for (int st = 128; st > 0; st >>= 1) {
                if (tid < st && gal_better(rs[tid + st], ri[tid + st], rs[tid], ri[tid])) {
                    rs[tid] = rs[tid + st]; ri[tid] = ri[tid + st];
                    if constexpr (IDS) rd[tid] = rd[tid + st];
                }
                __syncthreads();
            }
            last_s = rs[0]; last_i = ri[0];
            if constexpr (IDS) {
                last_d = rd[0];
                if (tid == 0) picked[round] = last_d;
            }
            __syncthreads();
        }
        have_last = true;
        if (tid == 0) {
            const bool found = last_i != INT_MAX;
            out_s[(size_t)q * k + round] = found ? last_s : -1.0f;
            if constexpr (IDS) out_d[(size_t)q * k + round] = found ? last_d : -1;
            if (!IDS || out_i) out_i[(size_t)q * k + round] = found ? last_i : -1;
        }
        if (last_i == INT_MAX) exhausted = true;         // nothing left: later rounds find nothing either (workgroup-uniform)
    }
}

// part_stride = words between the lists of consecutive parts (Q * k when they are packed; the sharded exchange of comm.cpp interleaves
// score and index planes per rank)
void launch_topk_merge_strided(const float* part_score, const int* part_idx, int nparts, int Q, int k, long part_stride, float* out_score,
                               int* out_idx, hipStream_t s, const int* qcount) {
    auto kernel = (long)nparts * k <= 8192 ? topk_merge_kernel<true> : topk_merge_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(Q), dim3(256), 0, s, part_score, part_idx, nparts, Q, k, part_stride, out_score, out_idx, qcount);
}
void launch_topk_merge(const float* part_score, const int* part_idx, int nparts, int Q, int k, float* out_score, int* out_idx,
                       hipStream_t s, const int* qcount) {
    launch_topk_merge_strided(part_score, part_idx, nparts, Q, k, (long)Q * k, out_score, out_idx, s, qcount);
}
void launch_topk_merge_ids(const float* part_score, const int* part_id, const int* part_idx, int nparts, int Q, int k, float* out_score,
                           int* out_id, int* out_idx, hipStream_t s, const int* qcount) {
    if (Q <= 0) return;
    auto kernel = (long)nparts * k <= 8192 ? topk_merge_kernel<true, true> : topk_merge_kernel<false, true>;
    hipLaunchKernelGGL(kernel, dim3(Q), dim3(256), 0, s, part_score, part_id, part_idx, nparts, Q, k, (long)Q * k, out_score, out_id, out_idx,
                       qcount);
}

}  // namespace fh
