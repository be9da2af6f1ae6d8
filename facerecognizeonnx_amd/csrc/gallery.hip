// gallery.hip — 1:N generalisation of FaceRecognizer::compareFaces (reference src/face_recognizer.cpp:320-334): every query against
// every enrolled row, mapped score (dot + 1) / 2, top-k per query ranked (score desc, global row index asc).
//
// One kernel streams the gallery ONCE: the dot products live only in MFMA accumulators, never in memory.
//   * The scan is an HBM stream with NO reuse on the gallery side: what limits it is bytes in flight (Little: ~50 KB per CU for 5 TB/s at
//     ~2.5 us loaded latency).  Each wave fetches ITS OWN 32 gallery rows straight into registers — the fragment layout is the one a
//     ds_read_b128 would deliver: lane (row fr, half fh2) takes 16 bytes at k = (2s + fh2) * 4 of its row; the s-steps of a 128-byte line
//     are consecutive instructions — in 64-deep chunks, one chunk (8 loads, 32 VGPRs) ahead of the one being multiplied: 8 waves x 8 KB in
//     flight per CU, no LDS traffic and no barrier on the gallery side.  Only the 64 queries of the tile (shared by the four waves) go
//     through LDS: 16 KB per chunk by LDS-DMA from L2, double buffered, 16-byte column XOR-swizzled by (row & 15) on the source side.
//   * v_mfma_f32_32x32x2_f32 with the GALLERY fragment as A and the QUERY fragment as B: a lane ends up with ONE query (column) and 16
//     gallery rows of it per 32x32 block.  Workgroup tile: 128 gallery rows x 64 queries.
//   * top-k: every workgroup owns a contiguous run of row tiles.  Thread q < 64 keeps query q's sorted k-list in REGISTERS (a compare-
//     exchange pass per insertion, no LDS latency chain) and publishes its k-th entry — the admission threshold — in LDS.  After a tile's
//     K loop each lane compares its 32 scores with the threshold of its query; the few that pass are appended to that query's slot queue
//     (LDS atomic counter) and thread q inserts them.  A queue holds 32 entries: if a tile overflows one (only the first tiles of a run
//     can, while the lists are still filling), the tile's scores — still in registers — are replayed in four 32-row rounds, which cannot.
//   * per-workgroup lists go to memory as [part][Q][k]; topk_merge_kernel (face_kernels.hip) selects the overall top-k.
// Bounds: HBM scan (G x dim x 4 bytes once) against 2*Q*G*dim FLOP on the f32 matrix cores — at Q = 64 the two meet.
//
// Round 3, measured and NOT kept (1 M x 512, Q = 64, k = 16; this kernel: 0.82 ms per call = seed pass 88 us + scan ~700 + two merges
// 39 us each): a scan with the whole 64-query tile RESIDENT in LDS (128 KB, one 8-wave workgroup per CU, no per-chunk barrier, query
// fragments read a step ahead), tried with three top-k schemes:
//   * this kernel's queues + two barriers per 256-row tile + its own seed launch: 0.86 ms (the seed launch alone 196 us: sixteen
//     workgroups each loading 128 KB of queries for one tile; a barrier stalls the whole CU on its slowest wave);
//   * wave-private lists in registers (lane l = query l, one lane^32 exchange per accumulator position, one compare-exchange pass per
//     candidate), thresholds shared through LDS, no barrier and no seed: 0.91 ms — the K loop + loads alone 0.67 ms, but the
//     insertions cost 0.3 ms: the k-th score of ONE wave's rows (or the maximum of several waves' k-ths) is a far weaker threshold
//     than the k-th of their union, so ~20 of the 32 insertion passes of a tile still fire half-way through the scan;
//   * the same with chip-wide thresholds through atomicMax on 64 words: 1.18 ms (contended atomics, and the maximum of per-workgroup
//     k-ths is still not a chip-wide k-th).
// Where a call's 0.82 ms go (rocprofv3, 1 M x 512, Q = 64, k = 16): seed scan 89 us (32 workgroups, one tile each: a latency chain plus the
// first-tile insertions) + seed merge 26 + main scan 658 (67.1 GFLOP = 102 TFLOP/s: at Q = 64 the f32 matrix cores bind, not HBM —
// 0.43 ms at the nominal peak, ~0.58 at the 115 TFLOP/s plateau) + final merge 50.  Without the seed pass (FACEHIP_GAL_SEED=0) the call
// takes 0.844 ms: the per-workgroup list warm-up costs more than the 115 us the seed does.  A pruned final merge (threshold = best over
// the parts of a full part's worst entry, survivors compacted to LDS, one entry per thread in the rounds) ran 35 us SLOWER with
// part-per-thread loads (64 lines per load instruction) and was not kept.
// Side results worth keeping: a wave streaming its own 32 rows into registers reaches 6.2 TB/s whatever the lane-to-row mapping
// (scripts/ubench/row_stream.hip: 32, 16, 8 rows per instruction or fully coalesced, all 6.2-6.5 TB/s), so the scan is not bound by
// its access pattern; with loads and top-k switched off the MFMA + fragment-read loop alone runs at ~75 % of the f32 peak.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <stdexcept>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

// the scan itself: gallery_scan.h (shared with gallery_topk_ids_kernel, gallery_ids.hip); this is its row-level instantiation
__global__ __launch_bounds__(256, 2) void gallery_topk_kernel(const GalArgs p) { gallery_scan_body<false>(p); }

// parts the row range is cut into for a gallery of G rows and a query batch of Q (the caller sizes its partial-list buffers with it)
int gallery_parts(long G, int Q, int* tiles_per_part) {
    const int tiles_n = (Q + GAL_BN - 1) / GAL_BN;
    const long row_tiles = (G + GAL_BM - 1) / GAL_BM;
    const int slots = conv_num_cus() * 2;                       // 2 resident workgroups per CU (3 measured: no faster, and 768 lists per query leave the merge its slow path)
    long parts = slots / tiles_n;
    if (parts < 1) parts = 1;
    if (parts > row_tiles) parts = row_tiles;
    const long tpp = parts > 0 ? (row_tiles + parts - 1) / parts : 1;
    if (tiles_per_part) *tiles_per_part = (int)tpp;
    return (int)(tpp > 0 ? (row_tiles + tpp - 1) / tpp : 0);
}

// queries: packed [ceil64(Q)][dim] with zero rows behind Q; part_score / part_idx: [gallery_parts][Q][k]; seed_score / seed_idx: [Q][k] scratch.
// Two passes for a large gallery: the exact top-k of the first GAL_SEED_ROWS rows (same kernel + merge) gives every query an admission
// threshold, then the full scan runs with it — without the seed every workgroup spends its first tiles sorting rows that cannot matter.
void launch_gallery_topk(const float* gal, long G, int dim, const float* qpacked, int Q, int k, long idx_base, float* part_score, int* part_idx,
                         float* seed_score, int* seed_idx, hipStream_t s, const int* qcount) {
    if (G <= 0 || Q <= 0) return;
    if (dim % 64 || k < 1 || k > GAL_KMAX) throw std::runtime_error("gallery: need dim % 64 == 0 and 1 <= k <= 16");
    if (idx_base + G > (long)INT_MAX) throw std::runtime_error("gallery: global row indices must fit in 31 bits");
    GalArgs a{};
    a.gal = gal; a.q = qpacked; a.zeros = conv_zero_line(); a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.k = k;
    a.tiles_n = (Q + GAL_BN - 1) / GAL_BN;
    a.ps = part_score; a.pi = part_idx; a.qcount = qcount;
    constexpr long GAL_SEED_ROWS = 4096;
    static int seed_on = -1;
    if (seed_on < 0) { const char* e = getenv("FACEHIP_GAL_SEED"); seed_on = e ? atoi(e) : 1; }     // (0: no seed pass — A / B timing)
    if (seed_on && G >= 16 * GAL_SEED_ROWS && seed_score && seed_idx) {
        a.G = GAL_SEED_ROWS;
        a.row_tiles = (int)(GAL_SEED_ROWS / GAL_BM);
        const int sp = gallery_parts(a.G, Q, &a.tiles_per_part);
        hipLaunchKernelGGL(gallery_topk_kernel, dim3((unsigned)(sp * a.tiles_n)), dim3(256), 0, s, a);
        launch_topk_merge(part_score, part_idx, sp, Q, k, seed_score, seed_idx, s);
        a.seed_s = seed_score; a.seed_i = seed_idx;
    }
    a.G = G;
    a.row_tiles = (int)((G + GAL_BM - 1) / GAL_BM);
    const int parts = gallery_parts(G, Q, &a.tiles_per_part);
    hipLaunchKernelGGL(gallery_topk_kernel, dim3((unsigned)(parts * a.tiles_n)), dim3(256), 0, s, a);
}

}  // namespace fh
