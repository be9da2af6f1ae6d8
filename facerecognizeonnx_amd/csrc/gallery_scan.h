// gallery_scan.h — the streaming 1:N scan of the gallery: ONE body, instantiated as gallery_topk_kernel (gallery.hip: fp32 rows, lists of
// rows), gallery_topk_ids_kernel (gallery_ids.hip: fp32 rows, lists of identities), their tagged twins (gallery_tags.hip) and
// gal16_scan_kernel (gallery_f16.hip: fp16 rows, 32-deep candidate lists) and gallery_range_kernel (gallery_range.hip: fp32 rows, no
// lists at all — a bit per (row, query) whose score is above a threshold) and gallery_bmax_kernel (gallery_deep.hip: fp32 rows, no lists —
// the best score per (32-row block, query)); with it the ranking predicate, the kernel arguments, the
// two-pass launcher the top-k scans share, the one launcher of the four fp32 top-k scans and the re-score of single (row, query) pairs.
// The multiply of one (128-row tile, 64-row tile) pair — THE K loop — is gal_tile_dot below, written once: this body calls it with the
// query tile as B, cluster_pair_body (gallery_cluster.hip: DBSCAN's degree / link passes and the pair histogram) with gallery rows as B.
//
// One kernel streams the gallery ONCE: the dot products live only in MFMA accumulators, never in memory.
//   * The scan is an HBM stream with NO reuse on the gallery side: what limits it is bytes in flight (Little: ~50 KB per CU for 5 TB/s at
//     ~2.5 us loaded latency).  Each wave fetches ITS OWN 32 gallery rows straight into registers — the fragment layout is the one a
//     ds_read_b128 would deliver: lane (row fr, half fh2) takes 16 bytes at k = (2s + fh2) * 4 of its row; the s-steps of a 128-byte line
//     are consecutive instructions — in 64-deep chunks, one chunk (8 loads, 32 VGPRs) ahead of the one being multiplied: 8 waves x 8 KB in
//     flight per CU, no LDS traffic and no barrier on the gallery side.  Only the 64 queries of the tile (shared by the four waves) go
//     through LDS: 16 KB per chunk, through registers (see gal_tile_dot), double buffered, 16-byte column XOR-swizzled by (row & 15) on the
//     source side.
//   * v_mfma_f32_32x32x2_f32 with the GALLERY fragment as A and the QUERY fragment as B: a lane ends up with ONE query (column) and 16
//     gallery rows of it per 32x32 block.  Workgroup tile: 128 gallery rows x 64 queries.
//   * top-k: every workgroup owns a contiguous run of row tiles.  Thread q < 64 keeps query q's sorted k-list in REGISTERS (a compare-
//     exchange pass per insertion, no LDS latency chain) and publishes its k-th entry — the admission threshold — in LDS.  After a tile's
//     K loop each lane compares its 32 scores with the threshold of its query; the few that pass are appended to that query's slot queue
//     (LDS atomic counter) and thread q inserts them.  A queue holds 32 entries: if a tile overflows one (only the first tiles of a run
//     can, while the lists are still filling), the tile's scores — still in registers — are replayed in four 32-row rounds, which cannot.
//   * per-workgroup lists go to memory as [part][Q][k]; topk_merge_kernel (gallery.hip) selects the overall top-k.
// Bounds: HBM scan (G x dim x 4 bytes once) against 2*Q*G*dim FLOP on the f32 matrix cores — at Q = 64 the two meet.
//
// The instantiations differ only behind `if constexpr`:
//   * IDS = false compiles to exactly the row-level kernel, and both fp32 instantiations run the same K loop with the same operand
//     placement and k order, so a score has the same bits in either.
//   * T = _Float16 (gal16_scan_kernel): 8 elements per 16-byte column, so a chunk is 128 deep and 256 bytes per row — the loads, the
//     column swizzle and the LDS image of a chunk are those of the 64-deep f32 chunk — multiplied by v_mfma_f32_32x32x16_f16 with f32
//     accumulation: 8 MFMAs per 32x32 block and chunk where the f32 kernels issue 32.  Its lists are KD = 32 deep and k IS the list
//     depth (KFIX), so the threshold entry is ls[31] instead of a select by k - 1.  It is launched at one workgroup per CU (the 32-deep
//     lists + two row chunks in flight need more than the 256 registers of two waves per SIMD: 104 bytes of spills at (256, 2)).
//   * RANGE (gallery_range_kernel): the same K loop, then an epilogue of its own INSTEAD of the lists, queues, thresholds and seeds —
//     every lane turns its 2 x 16 accumulators into hit bits ((acc + 1) / 2 > thr, row < G, tag & mask) and the wave stores one 32-bit
//     word per (32-row block, query).  No LDS beyond the query chunks, no barrier beyond the K loop's, no atomics; masks are optional at
//     run time (p.qmask), every tile is multiplied and a workgroup's tiles are the contiguous run.
//   * DEEP (gallery_bmax_kernel, gallery_deep.hip): the twin of RANGE — the same K loop, then every lane reduces its 2 x 16 accumulators
//     to the MAXIMUM score over its eligible rows (row < G, admitted, not a NaN, > -inf; -inf if none), takes the maximum with lane
//     fr ^ 32 and the wave stores one float per (32-row block, query): the block maxima the deep top-k selects its blocks from.
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
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <type_traits>

namespace fh {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

constexpr int GAL_BM = 128, GAL_BN = 64, GAL_KMAX = 16, GAL_QCAP = 32;

struct GalArgs {
    const void* gal;        // [G][dim], elements of the instantiation's type T
    const void* q;          // [tiles_n * 64][dim], rows >= Q are zero
    const void* zeros;
    long G, idx_base;
    int dim, Q, k, tiles_n, row_tiles, tiles_per_part;
    float* ps;              // [parts][Q][k]
    int* pi;
    const float* seed_s;    // optional [Q][k]: exact top-k of a PREFIX of the gallery — its k-th entry is a valid admission threshold for
    const int* seed_i;      // the whole scan (k rows at least as good exist), so the per-workgroup lists start almost closed
    const int* qcount;      // optional (device), fp32 scans: query tiles at or beyond *qcount exit at once (null: all Q)
    const int* ids;         // IDS: identity id of every row [G]
    int* pd;                // IDS: [parts][Q][k] identity ids beside ps / pi
    // TAGS (gallery_tags.hip) — behind everything else, so that the other instantiations read their arguments where they always did
    const unsigned* tags;     // tag word of every row [G]
    const unsigned* qmask;    // mask word of every query [Q]
    const unsigned* tile_or;  // OR of the tags of each 128-row tile, by position [row tiles of the WHOLE gallery]
    unsigned long long* tag_ctr;   // [2]: (workgroup, row tile) visits multiplied / skipped, one atomic add each per workgroup
    int tag_skip;             // 0: every tile is multiplied (fh_debug_tag_skip)
    // RANGE (gallery_range.hip) — behind the TAGS fields in turn; it also reads tags / qmask (qmask null: every row admitted)
    float range_thr;          // row r is a hit of query q iff (acc + 1) / 2 > range_thr (and r < G, and admitted)
    unsigned* hits;           // [row_tiles * 4][tiles_n * 64]: bit b of word [m][q] = row 32 m + b is a hit of query q
    // DEEP (gallery_deep.hip) — behind the RANGE fields in turn; it reads tags / qmask as RANGE does
    float* bmax;              // [row_tiles * 4][tiles_n * 64]: the best eligible score of rows 32 m .. 32 m + 31 for query q, -inf if none
};

// ---- host side (gallery.hip); they sit here and not in kernels.h because they speak of GalArgs
struct GalScan {            // what the host needs to know about an instantiation of the scan
    const char* name;       // for error messages
    void (*kernel)(const GalArgs);
    int chunk;              // K-chunk depth: dim must be a multiple
    int depth;              // list depth: 1 <= k <= depth
    int wg_per_cu;          // resident workgroups per CU (__launch_bounds__) = parts per CU
    long max_parts;         // cap on the parts per query tile
    bool has_qcount;        // the kernel honours GalArgs::qcount
};
constexpr int GAL_WG_PER_CU = 2;             // fp32 scans (3 measured: no faster, and 768 lists per query leave the merge its slow path)
int gallery_parts_for(long G, int Q, int wg_per_cu, long max_parts, int* tiles_per_part);
void gallery_check_args(const GalScan& sc, const GalArgs& a, long G);     // throws: dim, k, 31-bit indices, qcount
// The two passes every scan of a large gallery makes: the exact top-k of the first 4096 rows (same kernel + merge into seed_*) gives every
// query an admission threshold, then the full scan runs with it — without the seed every workgroup spends its first tiles sorting rows
// that cannot matter.  `a` carries gal / q / ids, idx_base, dim, Q, k, the part planes and qcount; seed_* = [Q][k] scratch.  The row range
// is cut into gallery_parts_for(G, Q, wg_per_cu, max_parts) parts; returns that number (the caller merges the part lists).
int launch_gallery_two_pass(const GalScan& sc, GalArgs a, long G, bool seed, float* seed_s, int* seed_i, int* seed_d, hipStream_t s);
// The fp32 scans: the four instantiations (gallery.hip, gallery_ids.hip, gallery_tags.hip) and their ONE launcher (gallery.hip).  `a` as
// above, filled by the caller; a.ids (with a.pd) asks for lists of identities, a.qmask (with a.tags, a.tile_or, a.tag_ctr) for the
// tagged scan; a.qcount only for plain lists of rows.  seed_d: needed with a.ids.  G <= 0 or Q <= 0 launches nothing.  The seed pass is
// always on, except that FACEHIP_GAL_SEED=0 switches it off for the plain row scan; fh_debug_tag_skip sets a.tag_skip.
__global__ __launch_bounds__(256, 2) void gallery_topk_kernel(const GalArgs p);
__global__ __launch_bounds__(256, 2) void gallery_topk_ids_kernel(const GalArgs p);
__global__ __launch_bounds__(256, 2) void gallery_topk_tagged_kernel(const GalArgs p);
__global__ __launch_bounds__(256, 2) void gallery_topk_ids_tagged_kernel(const GalArgs p);
void launch_gallery_scan(GalArgs a, long G, float* seed_s, int* seed_i, int* seed_d, hipStream_t s);

__device__ __forceinline__ bool gal_better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// ---- what belongs with the K loop: the three small maps every epilogue of it uses
// accumulator element e of a lane is row 8 * (e >> 2) + (e & 3) (+ 4 * fh2) of the wave's 32-row block
__device__ __forceinline__ constexpr int gal_acc_row(int e) { return 8 * (e >> 2) + (e & 3); }
// the mapped score (compareFaces' (cos + 1) / 2; a division, as there)
__device__ __forceinline__ float gal_score(float acc) { return (acc + 1.0f) / 2.0f; }
// where a lane streams a row from: the live row, or the zero line with step 0 (dead rows multiply zeros and are masked by the caller)
template <typename T> struct GalSrc { const T* ptr; int step; };
template <typename T>
__device__ __forceinline__ GalSrc<T> gal_row_or_zeros(bool live, const T* rows, size_t row, int K, const T* zeros, int off, int step) {
    return {(live ? rows + row * K : zeros) + off, live ? step : 0};
}

// THE K loop of the gallery family: acc = (the wave's 32 rows of a 128-row A tile) x (a 64-row B tile), over `chunks` chunks of 16
// 16-byte columns (64 deep in fp32, 128 in fp16).  gallery_scan_body (B = the query tile) and cluster_pair_body (gallery_cluster.hip: B =
// gallery rows) both call it, so a score has the same bits in every kernel built from either: lane (row fr, half fh2) holds k = 64 kc +
// 8 s + 4 fh2 + e of its row, loop kc, s = 0..7, e = 0..3, both 32-column blocks per step, accumulators from 0.
//   a_ptr / a_step: the lane's row + fh2 columns and its step per chunk (gal_row_or_zeros); each wave streams ITS OWN 32 rows into
//   registers, one chunk (8 loads, 32 VGPRs) ahead of the one being multiplied.
//   fetch_b(qv): loads the calling thread's four 16-byte pieces of the NEXT B chunk — piece i is row 16 i + (tid >> 4), source column
//   (tid & 15) ^ (row & 15) — and advances the caller's pointers.  The scan passes one pointer and a stride, the pair pass four row
//   pointers; the helper does not care (and the scans have no registers to spare for the general form).
//   ldsq: the double-buffered B chunk [64 rows][16 columns], 16-byte column XOR (row & 15).  The CALLER issues the barrier that frees it
//   from the previous tile; everything from the first fetch to the last MFMA is here.
// The B chunk goes global -> registers -> LDS (not by LDS-DMA): the compiler makes every LDS read wait for ALL vector-memory traffic
// while an LDS-DMA is in flight (it cannot tell the two halves of ldsq apart: `s_waitcnt vmcnt(0)` in front of each multiply, i.e. every
// chunk waited out its own gallery-row loads).  Through registers the dependencies are exact: the 4 B loads are issued BEFORE the 8 row
// loads, so the ds_write after the multiply waits with vmcnt(8) and the row loads fly on until the next barrier.  sched_barrier: left
// alone, the scheduler sinks the row loads below the multiply (one register set instead of two) and serialises them with it.
template <typename T, typename FetchB>
__device__ __forceinline__ void gal_tile_dot(v4f (&ldsq)[2][GAL_BN * 16], const T* a_ptr, int a_step, int chunks, int tid, int fr, int fh2,
                                             FetchB&& fetch_b, v16f (&acc)[GAL_BN / 32]) {
    constexpr bool F16 = std::is_same<T, _Float16>::value;
    constexpr int TN = GAL_BN / 32, EC = 16 / (int)sizeof(T);
    const int fsw = fr & 15;
    v4f xa[2][8], qv[4];
    v16f c[TN];                                               // accumulators of the loop: locals, written to acc ONCE at the end (with acc itself
                                                              // in the loop the compiler copies all 32 registers at the loop's exit)
    auto load_a = [&](v4f (&x)[8]) {                          // 16-byte column 2s + fh2 of the chunk
#pragma unroll
        for (int s = 0; s < 8; ++s) x[s] = *reinterpret_cast<const v4f*>(a_ptr + s * 2 * EC);
        a_ptr += a_step;
    };
    auto multiply = [&](const v4f (&x)[8], int buf) {
        const v4f* Wt = ldsq[buf] + fr * 16;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int col = (2 * s + fh2) ^ fsw;
            if constexpr (F16) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const v4f w = Wt[j * 32 * 16 + col];
                    c[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, x[s]), __builtin_bit_cast(v8h, w), c[j], 0, 0, 0);
                }
            } else {
                v4f w[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) w[j] = Wt[j * 32 * 16 + col];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < TN; ++j) c[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s][e], w[j][e], c[j], 0, 0, 0);
            }
        }
    };
    auto store_b = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ldsq[buf][i * 256 + tid] = qv[i];
    };
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) c[j][e] = 0.f;
    fetch_b(qv);
    load_a(xa[0]);
    store_b(0);
    int kc = 0;
    for (; kc + 2 <= chunks; kc += 2) {
        __syncthreads();                                   // B of chunk kc is in LDS (and xa[0] has landed: the barrier drains vmcnt)
        fetch_b(qv);
        load_a(xa[1]);
        __builtin_amdgcn_sched_barrier(0);
        multiply(xa[0], 0);
        store_b(1);
        __syncthreads();
        if (kc + 2 < chunks) { fetch_b(qv); load_a(xa[0]); }
        __builtin_amdgcn_sched_barrier(0);
        multiply(xa[1], 1);
        if (kc + 2 < chunks) store_b(0);
    }
    if (kc < chunks) {                                     // odd number of chunks
        __syncthreads();
        multiply(xa[0], 0);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = c[j];
}

// The fp32 scan's score of up to 32 single (row, query) pairs, by one wave: the multiply of gal_tile_dot with the query in EVERY
// column of B — lane (row fr, half fh2) holds k = kc * 64 + (2s + fh2) * 4 + e of its row; loop kc, s = 0..7, e = 0..3; accumulator from
// 0.  One output element depends only on its row, its column and that sequence, so (acc + 1) / 2 has the bits the scan gives the pair.
// a_ptr: the lane's row + fh2 * 4 (a dead lane: the zero line, a_step 0; else a_step 64); b_ptr: the query + fh2 * 4.  Every column of
// the result is the same: element e of a lane is row gal_acc_row(e) + 4 * fh2.  (No LDS, no double buffering: a loop of its own.)
__device__ __forceinline__ v16f gal_rescore32(const float* a_ptr, int a_step, const float* b_ptr, int chunks) {
    v16f acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int kc = 0; kc < chunks; ++kc) {
        v4f x[8], w[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) { x[s] = *reinterpret_cast<const v4f*>(a_ptr + s * 8); w[s] = *reinterpret_cast<const v4f*>(b_ptr + s * 8); }
        a_ptr += a_step; b_ptr += 64;
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s][e], w[s][e], acc, 0, 0, 0);
    }
    return acc;
}

// IDS: thread q's list holds at most ONE entry per identity — the identity's best row seen so far — so its k-th entry is the k-th
// DISTINCT identity and a valid admission threshold: k identities already have a row at least that good, and a listed identity only
// ever improves.  A row's id is fetched (4-byte gather) only when the row passes the threshold, and travels through the slot queue
// as a third word.  The insertion stays ONE compare-exchange pass: whatever the pass holds in hand after position pos — the new
// entry (not yet placed: the listed one is better, the new one is dropped) or the entry it displaced (the new one is better and took
// an earlier place) — is discarded when the entry listed at pos carried the new entry's id.
//
// TAGS: row r is ADMITTED for query q iff (tags[r] & qmask[q]) != 0, and only admitted rows pass the push test.  Nothing else changes:
// the list then holds admitted rows only, so its k-th entry is the k-th ADMITTED row — k admitted rows at least that good exist — and
// stays a valid threshold for the admitted sub-gallery; the same holds for a seed list computed with the same masks (a seed list with
// fewer than k admitted rows has an empty k-th slot and gives no threshold).  A score does not depend on the tags: same K loop, same
// operand placement.  The 64 masks of the query tile sit in LDS for the whole run (queries behind Q: mask 0), the 128 tags of a row
// tile beside them for the tile (rows behind G: tag 0).  U = the OR of the workgroup's masks lives in an SGPR; a tile whose tile_or has
// no bit of U holds no admitted row for any of the 64 queries and is skipped before any of its loads or barriers is issued.  So that
// the tiles left over spread evenly, a TAGS workgroup walks the row tiles strided by the number of parts (see the tile loop).
//
// T: element type of rows and queries (float | _Float16); KD: list depth; KFIX: k is KD (else the runtime p.k <= KD).
// RANGE: no lists — the epilogue is the hit bitmap (KD, KFIX, IDS and TAGS play no part; see the header).
// DEEP: no lists — the epilogue is the block maxima (as RANGE; never both).
template <typename T, int KD, bool KFIX, bool IDS, bool TAGS = false, bool RANGE = false, bool DEEP = false>
__device__ __forceinline__ void gallery_scan_body(const GalArgs& p) {
    constexpr bool F16 = std::is_same<T, _Float16>::value;
    static_assert(!RANGE || (!F16 && !IDS && !TAGS), "the threshold scan reads fp32 rows and takes its masks at run time");
    static_assert(!DEEP || (!F16 && !IDS && !TAGS && !RANGE), "the block-maximum scan reads fp32 rows and takes its masks at run time");
    constexpr bool LISTS = !RANGE && !DEEP;                   // the top-k scans: lists, queues, thresholds, seeds
    constexpr int BM = GAL_BM, BN = GAL_BN, TN = BN / 32;
    constexpr int EC = 16 / (int)sizeof(T), CD = 16 * EC;     // elements per 16-byte column, chunk depth (16 columns)
    __shared__ v4f ldsq[2][BN * 16];                          // query chunk [64 rows][CD k], 16-byte column XOR (row & 15)
    __shared__ float tau_s[BN];                               // admission threshold per query = the k-th entry of its list
    __shared__ int tau_i[BN];
    __shared__ float que_s[BN][GAL_QCAP];
    __shared__ int que_i[BN][GAL_QCAP];
    __shared__ int que_d[IDS ? BN : 1][GAL_QCAP];
    __shared__ int cnt[BN];
    __shared__ int overflow;
    __shared__ unsigned mask_s[TAGS ? BN : 1];
    __shared__ __attribute__((aligned(16))) unsigned tag_s[TAGS ? BM : 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh2 = lane >> 5;
    int t;
    {
        const int nb = gridDim.x, qq = nb >> 3, r8 = nb & 7, x = blockIdx.x & 7;
        t = x * qq + min(x, r8) + (int)(blockIdx.x >> 3);
    }
    const int tile_n = t % p.tiles_n, part = t / p.tiles_n;
    const int n0 = tile_n * BN;
    if constexpr (!F16 && LISTS) {                            // (the fp16 scan is never the compacted fall-back: no test, its scalar side stays lean)
        if (p.qcount && n0 >= *p.qcount) return;              // (workgroup-uniform, before any barrier)
    }
    const int K = p.dim, chunks = K / CD, k = KFIX ? KD : p.k;
    const int rt0 = part * p.tiles_per_part, rt1 = min(p.row_tiles, rt0 + p.tiles_per_part);

    float ls[KD];                                             // thread q < 64: sorted list of query q (entries >= k stay sentinels)
    int li[KD];
    int ld[IDS ? KD : 1];
#pragma unroll
    for (int i = 0; i < KD; ++i) { ls[i] = -INFINITY; li[i] = INT_MAX; }
    if constexpr (IDS) {
#pragma unroll
        for (int i = 0; i < KD; ++i) ld[i] = -1;
    }
    if (LISTS && tid < BN) {
        float ts = -INFINITY; int ti = INT_MAX;                   // (-inf, INT_MAX): below every real entry, whatever the rows' norms (compareFaces does not clamp, face_recognizer.cpp:320-334)
        if (p.seed_i && n0 + tid < p.Q) {
            const size_t o = (size_t)(n0 + tid) * k + (k - 1);
            if (p.seed_i[o] >= 0) { ts = p.seed_s[o]; ti = p.seed_i[o]; }
        }
        cnt[tid] = 0; tau_s[tid] = ts; tau_i[tid] = ti;
    }
    if (LISTS && tid == 0) overflow = 0;
    unsigned U = 0;                                           // TAGS: OR of the tile's 64 masks (every wave forms it: no barrier needed)
    int n_scan = 0, n_skip = 0;
    if constexpr (TAGS) {
        unsigned m = n0 + lane < p.Q ? p.qmask[n0 + lane] : 0u;
        if (tid < BN) mask_s[tid] = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m |= (unsigned)__shfl_xor((int)m, o);
        U = (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    }

    // query loader: pass i fills rows i*16 + (tid >> 4), slot tid & 15 <- source 16-byte column (tid & 15) ^ (row & 15)
    const int qrow = tid >> 4;
    const T* const gal = static_cast<const T*>(p.gal);
    const T* const zeros = static_cast<const T*>(p.zeros);
    const T* const q_base = static_cast<const T*>(p.q) + (size_t)(n0 + qrow) * K + (((tid & 15) ^ (qrow & 15)) * EC);
    const size_t q16 = (size_t)16 * K;

    // TAGS: part p walks the tiles p, p + parts, p + 2 parts, ... instead of a contiguous run — enrolments grouped by tag are long
    // contiguous blocks, and with contiguous runs the few workgroups that own an admitted block would multiply all of their tiles
    // while the others skip all of theirs: the call would take as long as a full scan.  Strided, every workgroup owns its share of
    // every block.  (The part lists are merged whatever rows they cover.)
    const int rt_first = TAGS ? part : rt0, rt_last = TAGS ? p.row_tiles : rt1, rt_step = TAGS ? (int)gridDim.x / p.tiles_n : 1;
    for (int rt = rt_first; rt < rt_last; rt += rt_step) {
        const long m0 = (long)rt * BM;
        unsigned my_tag = 0;
        if constexpr (TAGS) {
            if (p.tag_skip && (p.tile_or[rt] & U) == 0) { ++n_skip; continue; }      // (workgroup-uniform: rt and U are scalars)
            ++n_scan;
            if (tid < BM && m0 + tid < p.G) my_tag = p.tags[m0 + tid];
        }
        const long myrow = m0 + wid * 32 + fr;
        const bool live = myrow < p.G;
        const GalSrc<T> a = gal_row_or_zeros(live, gal, (size_t)myrow, K, zeros, fh2 * EC, CD);      // (dead rows are masked below)
        const T* q_src = q_base;
        auto fetch_q = [&](v4f (&qv)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = *reinterpret_cast<const v4f*>(q_src + i * q16);
            q_src += CD;
        };
        v16f acc[TN];
        __syncthreads();                                   // previous tile's epilogue is done with the LDS lists / queues (and ldsq)
        if constexpr (TAGS) {
            if (tid < BM) tag_s[tid] = my_tag;             // (read behind the K loop's barriers)
        }
        gal_tile_dot<T>(ldsq, a.ptr, a.step, chunks, tid, fr, fh2, fetch_q, acc);
        const long rbase = m0 + wid * 32 + 4 * fh2;
        // ---- threshold epilogue: bit 4 * fh2 + 8 * (e >> 2) + (e & 3) of the lane's word = its row of that position in the wave's 32-row
        // block; the lane pair (fr, fr ^ 32) holds the two interleaved halves of one query's word, so after one exchange per query block
        // lane l owns the whole word of query n0 + l and the wave stores 64 words = 256 contiguous bytes of row [block] of the bitmap
        if constexpr (RANGE) {
            static_assert(TN == 2, "one query block per lane half");
            unsigned tg[16];                               // the tags of the lane's 16 rows (rows behind G, and a call without masks: unused)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long row = rbase + gal_acc_row(e);
                tg[e] = p.qmask && row < p.G ? p.tags[row] : 0xFFFFFFFFu;
            }
            unsigned word[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int qn = n0 + j * 32 + fr;
                const unsigned mq = qn >= p.Q ? 0u : p.qmask ? p.qmask[qn] : 0xFFFFFFFFu;     // (queries behind Q: no hits)
                unsigned bits = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const long row = rbase + gal_acc_row(e);
                    const float sc = gal_score(acc[j][e]);
                    const bool hit = row < p.G && (tg[e] & mq) != 0 && sc > p.range_thr;      // (false for a NaN score)
                    bits |= (hit ? 1u : 0u) << (4 * fh2 + gal_acc_row(e));
                }
                word[j] = bits | (unsigned)__shfl_xor((int)bits, 32);
            }
            // word [32-row block of the gallery][query, padded to whole tiles]: every word of the bitmap is written by exactly one lane
            p.hits[((size_t)rt * 4 + wid) * ((size_t)p.tiles_n * BN) + n0 + lane] = fh2 ? word[1] : word[0];
            continue;
        }
        // ---- block-maximum epilogue: the same lane pairs as the threshold epilogue — after one exchange per query block lane l owns the
        // maximum of query n0 + l over the wave's 32 rows, and the wave stores 64 floats = 256 contiguous bytes of row [block] of bmax
        if constexpr (DEEP) {
            static_assert(TN == 2, "one query block per lane half");
            unsigned tg[16];                               // the tags of the lane's 16 rows (rows behind G, and a call without masks: unused)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long row = rbase + gal_acc_row(e);
                tg[e] = p.qmask && row < p.G ? p.tags[row] : 0xFFFFFFFFu;
            }
            float best[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int qn = n0 + j * 32 + fr;
                const unsigned mq = qn >= p.Q ? 0u : p.qmask ? p.qmask[qn] : 0xFFFFFFFFu;     // (queries behind Q: no eligible row)
                float m = -INFINITY;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const long row = rbase + gal_acc_row(e);
                    const float sc = gal_score(acc[j][e]);
                    const bool ok = row < p.G && (tg[e] & mq) != 0 && sc > m;                 // (false for a NaN score, and for -inf)
                    m = ok ? sc : m;
                }
                const float o = __shfl_xor(m, 32);
                best[j] = o > m ? o : m;
            }
            // every word of bmax is written by exactly one lane
            p.bmax[((size_t)rt * 4 + wid) * ((size_t)p.tiles_n * BN) + n0 + lane] = fh2 ? best[1] : best[0];
            continue;
        }
        // ---- top-k epilogue
        auto push = [&](int g_lo, int g_hi) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int qi = j * 32 + fr;
                const float ts = tau_s[qi];
                const int ti = tau_i[qi];
                unsigned mq = 0;
                if constexpr (TAGS) mq = mask_s[qi];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if ((e >> 2) < g_lo || (e >> 2) >= g_hi) continue;
                    const long row = rbase + gal_acc_row(e);
                    const float sc = gal_score(acc[j][e]);
                    const int gi = (int)(p.idx_base + row);
                    bool admitted = true;
                    if constexpr (TAGS) {                  // a lane's rows are four runs of four: one 16-byte LDS read per run, two addresses per wave
                        const uint4 tg = *reinterpret_cast<const uint4*>(&tag_s[wid * 32 + 4 * fh2 + 8 * (e >> 2)]);
                        const unsigned tw = (e & 3) == 0 ? tg.x : (e & 3) == 1 ? tg.y : (e & 3) == 2 ? tg.z : tg.w;
                        admitted = (tw & mq) != 0;
                    }
                    if (row < p.G && admitted && !gal_better(ts, ti, sc, gi)) {          // at least as good as the threshold entry (which may be this very row)
                        const int slot = atomicAdd(&cnt[qi], 1);
                        if (slot < GAL_QCAP) {
                            que_s[qi][slot] = sc; que_i[qi][slot] = gi;
                            if constexpr (IDS) que_d[qi][slot] = p.ids[row];
                        } else overflow = 1;
                    }
                }
            }
        };
        auto insert = [&]() {                                // thread q: its queue into its register list, then publish the new threshold
            if (tid < BN) {
                const int n = min(cnt[tid], GAL_QCAP);
                for (int c = 0; c < n; ++c) {
                    float s = que_s[tid][c];
                    int gi = que_i[tid][c];
                    if constexpr (IDS) {
                        const int idn = que_d[tid][c];
                        int d = idn;
#pragma unroll
                        for (int pos = 0; pos < KD; ++pos) {  // the same pass; the entry in hand is discarded behind the listed entry of identity idn
                            const bool sw = gal_better(s, gi, ls[pos], li[pos]);
                            const float os = ls[pos]; const int oi = li[pos], od = ld[pos];
                            ls[pos] = sw ? s : os; li[pos] = sw ? gi : oi; ld[pos] = sw ? d : od;
                            const bool drop = od == idn;
                            s = drop ? -INFINITY : sw ? os : s; gi = drop ? INT_MAX : sw ? oi : gi; d = drop ? -1 : sw ? od : d;
                        }
                    } else {
#pragma unroll
                        for (int pos = 0; pos < KD; ++pos) {      // one compare-exchange pass keeps all KD slots sorted (score desc, index asc)
                            const bool sw = gal_better(s, gi, ls[pos], li[pos]);
                            const float os = ls[pos]; const int oi = li[pos];
                            ls[pos] = sw ? s : os; li[pos] = sw ? gi : oi;
                            s = sw ? os : s; gi = sw ? oi : gi;
                        }
                    }
                }
                if (n > 0) {
                    float ts = ls[KD - 1]; int ti = li[KD - 1];     // the k-th entry: the last one, or selected by the runtime k
                    if constexpr (!KFIX) {
                        int km1 = k - 1;
#if defined(__HIP_DEVICE_COMPILE__)
                        asm volatile("" : "+v"(km1));            // (keeps the 16 position tests on the vector side: no SGPR mask per slot)
#endif
                        ts = ls[0]; ti = li[0];
#pragma unroll
                        for (int pos = 1; pos < KD; ++pos) { ts = pos == km1 ? ls[pos] : ts; ti = pos == km1 ? li[pos] : ti; }
                    }
                    // the local k-th entry bounds the global one as soon as the list holds k real rows; keep the tighter of it and the seed
                    if (ti != INT_MAX && gal_better(ts, ti, tau_s[tid], tau_i[tid])) { tau_s[tid] = ts; tau_i[tid] = ti; }
                }
                cnt[tid] = 0;
            }
        };
        push(0, 4);
        __syncthreads();
        if (overflow) {
            __syncthreads();
            if (tid < BN) cnt[tid] = 0;
            if (tid == 0) overflow = 0;
            __syncthreads();
            for (int g = 0; g < 4; ++g) {
                push(g, g + 1);
                __syncthreads();
                insert();
                __syncthreads();
            }
        } else {
            insert();
        }
    }
    if (LISTS && tid < BN && n0 + tid < p.Q) {
        const size_t o = ((size_t)part * p.Q + n0 + tid) * k;
#pragma unroll
        for (int pos = 0; pos < KD; ++pos)
            if (pos < k) {
                p.ps[o + pos] = li[pos] == INT_MAX ? -1.0f : ls[pos]; p.pi[o + pos] = li[pos] == INT_MAX ? -1 : li[pos];
                if constexpr (IDS) p.pd[o + pos] = li[pos] == INT_MAX ? -1 : ld[pos];
            }
    }
    if constexpr (TAGS) {
        if (tid == 0) {
            atomicAdd(&p.tag_ctr[0], (unsigned long long)n_scan);
            atomicAdd(&p.tag_ctr[1], (unsigned long long)n_skip);
        }
    }
}

}  // namespace fh
