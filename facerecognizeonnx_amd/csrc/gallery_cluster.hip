// gallery_cluster.hip — exact DBSCAN over the rows of a gallery (fh_gallery_cluster_dev): the rule of cluster_plan.h on the matrix
// s(i, j) = the mapped score the fp32 scan (gallery_scan.h) reports for query = row i against row j.
//
// The pair pass is the scan's arithmetic with another epilogue.  Tile layout and operand placement are gallery_scan_body's: the gallery
// is the A operand — each wave streams ITS OWN 32 rows into registers, one 64-deep chunk ahead — and it is also the B operand: a 64-row
// tile goes through the swizzled, double-buffered LDS image the scan keeps its queries in, loaded from the rows themselves.  Rows at or
// beyond G read the zero line and are masked.  The K loop IS the scan's — gal_tile_dot (gallery_scan.h), the one definition, called here
// with a B fetch from four row pointers — so an accumulator has the scan's bits by construction (k0 = 64 kc + 8 s + e, k1 = k0 + 4); the
// chain is symmetric in its operands (a product commutes), so s(i, j) and s(j, i) have the same bits and every unordered pair is
// evaluated ONCE: a workgroup owns one B tile (64 columns) and a run of A tiles (128 rows each); A tiles wholly below the diagonal are
// skipped and `row < col` masks the straddling ones.
//
// Launches of one call, all on the caller's stream:
//   init      deg[i] = 0, parent[i] = i, best[i] = 0, info[0..3] = 0
//   degree    (skipped when min_pts == 1) deg[i] = edges at i.  The B side — one column per lane pair — is counted in registers over
//             the run, summed through LDS and flushed with one global atomicAdd per column per run.  The A side needs a reduction across
//             lanes: __ballot of the edge predicate per accumulator position holds, in its low and high 32 bits, the counts of the two
//             rows of that position; lane r of the wave keeps row r's count and adds it once per tile.
//   link      the same pass with core[i] = deg[i] + 1 >= min_pts.  An edge between two cores is a union in a lock-free union-find on
//             parent[]: find both roots, CAS the LARGER root's parent from itself to the smaller root, on failure go on from the value
//             the CAS returned.  parent[x] <= x always and only ever decreases, so there are no cycles and a component's final root is
//             its smallest core position — the label the rule asks for, whatever order the edges arrive in.  An edge from a core to a
//             non-core row is a 64-bit atomicMax on best[non-core]: monotone-mapped score bits in the high word, ~position of the core
//             in the low word, so the maximum is exactly gal_better's choice (a real key is never 0: ~position has its top bit set).
//   flatten   label = root for cores, root of best's core for border rows, -1 / own position for noise; the four counters.
//
// fh_gallery_pair_hist_dev is the same pair pass with a third epilogue (clear the scratch, histogram pass, write-out):
//   histogram every live pair (row < col < G) is ONE LDS atomicAdd into the workgroup's uint32 [2][2048] histogram — plane = the two rows'
//             ids differ, bin = hist_bin (roc_plan.h) of the mapped score — or into one of two NaN counters.  A lane keeps the id of
//             row wrow0 + (lane & 31) of the current A tile and an accumulator's row id comes by shuffle; its two column ids are loaded
//             once per run.  16 KB of LDS beside the body's 32 KB: two workgroups per CU as before.  At the end of the run the non-zero
//             counters are flushed to the scratch histogram with 64-bit global atomics.
//   write-out the caller's hist [2][2048] and nan [2] (may be null) are overwritten from the scratch.
//
// fh_gallery_pairs_dev (the rule: pairs_plan.h) is the pair pass twice more — clear the scratch, count pass, cut, collect pass, select
// (the cut and the select kernel: gallery_pairs.hip):
//   count     the histogram epilogue with the selection filter in front: a live pair of the class on the asked side of the threshold is
//             ONE LDS atomicAdd into the workgroup's histogram BY RANK (pairs_rank: bin 2047 - b for "above", b for "not above"), a
//             NaN-scored pair of the class one into the NaN counter; flushed as the histogram pass flushes.  Row ids come by shuffle as
//             above; with class "any" no id is read at all (an unlabelled gallery has none).
//   collect   the cut kernel left the last rank to collect in the scratch (-1: nothing, the workgroups leave at once).  A selected pair
//             of rank <= cut is appended to the candidate buffer {score, i, j, -}: per accumulator position a wave takes __ballot of the
//             hit predicate, its first hit lane adds __popcll of it to the ONE device-scope counter, and lane l stores at
//             base + the hits below l.  By the cut rule the counter never exceeds `room`; the store is bounded by room all the same.
//             One 16-byte vector store per candidate.  The buffer is read by a later launch (the select kernel): plain loads there.
//
// Memory model (MI355X: eight XCDs whose L2s are not coherent with each other, and a vector L1 that another CU's stores never refresh):
// inside the link kernel EVERY read of parent[] is an agent-scope relaxed atomic load (served by L2, never by a stale L1 line) and
// every write is an atomic RMW (atomicCAS; atomicMin for the path halving).  A find that kept seeing a stale "I am a root" would fail
// its CAS for ever.  No loop in these kernels waits for another workgroup: a failed CAS means some thread has ALREADY linked that
// root, and the retry starts from the returned parent, strictly below the root it tried — the larger of the two roots in hand strictly
// descends, so a union ends after at most `position` rounds whatever the others do.  deg[] and best[] are only written (atomics) in the
// kernel that builds them and read by plain loads in a later launch.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "gallery_scan.h"
#include "kernels.h"
#include "pairs_plan.h"
#include "roc_plan.h"

namespace fh {

namespace {

struct ClusterArgs {
    const float* gal;                   // [G][dim]
    const float* zeros;
    long G;
    int dim, tiles_n, row_tiles, tiles_per_wg, min_pts;
    float thr;
    int* deg;                           // [G]
    int* parent;                        // [G]
    unsigned long long* best;           // [G]
    // the histogram pass only
    const int* ids;                     // [G]
    unsigned long long* hist;           // [copies][kHistSlots]
    int copies;
    // the two passes of the pair audit only (ids: null for class "any"; hist: kPairsSlots counters by rank; thr: the threshold)
    int pcls, pside;
    const int* cut;                     // the last rank to collect (written by the cut kernel, an earlier launch)
    unsigned* cand_cnt;                 // the one slot counter
    int4* cand;                         // [room] {score bits, i, j, 0}
    unsigned room;
};

// one histogram: [2][kHistBins] bins (plane 0 genuine, plane 1 impostor), then the two NaN counters
constexpr int kHistSlots = 2 * kHistBins + 2;
enum { PAIR_DEGREE = 0, PAIR_LINK = 1, PAIR_HIST = 2, PAIR_COUNT = 3, PAIR_COLLECT = 4 };
static_assert(kPairsSlots <= kHistSlots, "the count pass keeps its counters in the histogram pass's LDS");
constexpr int kHistDefaultCopies = 1;     // measured: 1, 8, 64 and 512 copies time the same (profiles/gallery_hist.md)

// the histogram pass's per-workgroup counters: 16 KB + 8 bytes beside the body's 32 KB, so two workgroups still share a CU's 160 KB
__device__ __forceinline__ unsigned* pair_hist_lds() {
    __shared__ unsigned h[kHistSlots];
    return h;
}

__device__ __forceinline__ int parent_load(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x; halves the path on the way (atomicMin: a parent only ever decreases, and a grandparent is an ancestor)
__device__ __forceinline__ int cluster_find(int* parent, int x) {
    int p = parent_load(parent, x);
    while (p != x) {
        const int gp = parent_load(parent, p);
        if (gp != p) atomicMin(parent + x, gp);
        x = p; p = gp;
    }
    return x;
}

__device__ __forceinline__ void cluster_union(int* parent, int a, int b) {
    int ra = cluster_find(parent, a), rb = cluster_find(parent, b);
    while (ra != rb) {                                       // (roots already equal: no atomic at all — the common case in a dense cluster)
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) break;                                // linked
        ra = cluster_find(parent, old);                      // hi had been linked already: old < hi, go on from there
        rb = cluster_find(parent, lo);
    }
}

// score bits -> unsigned, monotone in the score (scores here are (acc + 1) / 2, never NaN past the edge test and never -0)
__device__ __forceinline__ unsigned long long cluster_key(float s, int pos) {
    const unsigned u = __float_as_uint(s);
    const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)m << 32) | (unsigned)~pos;
}

// what an epilogue knows about the lane's two columns (one per 32-column block), for the whole run
struct PairCols {
    long col[2];
    bool ok[2];                         // col < G
    bool core[2];                       // link
    int deg[2];                         // degree: edges counted at the column over the run
    int id[2];                          // histogram
};

// The three epilogues of one tile: accumulator e of block j is (row wrow0 + 4 * fh2 + gal_acc_row(e), column c.col[j]).
// degree: the A side needs a reduction across lanes — __ballot per accumulator position; lane r < 32 keeps row wrow0 + r's count
__device__ __forceinline__ void pair_degree_tile(const ClusterArgs& p, const v16f (&acc)[2], PairCols& c, long wrow0, int lane, int fh2) {
    const long rbase = wrow0 + 4 * fh2;
    int row_deg = 0;                                       // lane r < 32: edges found at row wrow0 + r in this tile
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const long row = rbase + gal_acc_row(e);
        int lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float sc = gal_score(acc[j][e]);
            const bool edge = c.ok[j] && row < c.col[j] && sc > p.thr;      // (row < col < G)
            c.deg[j] += edge ? 1 : 0;
            const unsigned long long b = __ballot(edge);
            lo += __popc((unsigned)b); hi += __popc((unsigned)(b >> 32));
        }
        const int r_lo = gal_acc_row(e);
        row_deg += lane == r_lo ? lo : lane == r_lo + 4 ? hi : 0;
    }
    if (lane < 32 && row_deg > 0) atomicAdd(p.deg + wrow0 + lane, row_deg);    // (row_deg > 0 implies the row is below G)
}

__device__ __forceinline__ void pair_link_tile(const ClusterArgs& p, const v16f (&acc)[2], const PairCols& c, long wrow0, int fr, int fh2) {
    const long arow = wrow0 + fr;
    const unsigned row_core = (unsigned)__ballot(arow < p.G && p.deg[arow < p.G ? arow : 0] + 1 >= p.min_pts);   // bit r: row wrow0 + r
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = gal_acc_row(e) + 4 * fh2;
        const long row = wrow0 + r;
        const bool rc = (row_core >> r) & 1u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float sc = gal_score(acc[j][e]);
            if (c.ok[j] && row < c.col[j] && sc > p.thr) {
                if (rc && c.core[j]) cluster_union(p.parent, (int)row, (int)c.col[j]);
                else if (rc) atomicMax(p.best + c.col[j], cluster_key(sc, (int)row));
                else if (c.core[j]) atomicMax(p.best + row, cluster_key(sc, (int)c.col[j]));
            }
        }
    }
}

// lane r (and r + 32) holds the id of row wrow0 + r; an accumulator's row id comes by shuffle.  Every live pair is one LDS atomic: bin
// `hist_bin(sc)` of its class' plane, or the class' NaN counter.
__device__ __forceinline__ void pair_hist_tile(const ClusterArgs& p, const v16f (&acc)[2], const PairCols& c, long wrow0, int fr, int fh2) {
    unsigned* h = pair_hist_lds();
    const long arow = wrow0 + fr;
    const int my_id = arow < p.G ? p.ids[arow] : 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = gal_acc_row(e) + 4 * fh2;
        const long row = wrow0 + r;
        const int row_id = __shfl(my_id, r);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float sc = gal_score(acc[j][e]);
            if (c.ok[j] && row < c.col[j]) {                            // (row < col < G)
                const int b = hist_bin(sc);
                const int cls = row_id == c.id[j] ? 0 : 1;
                atomicAdd(&h[b >= 0 ? cls * kHistBins + b : 2 * kHistBins + cls], 1u);
            }
        }
    }
}

// The two epilogues of the pair audit.  rank: pairs_rank of an accumulator that is a live pair of the class, -1 otherwise.
__device__ __forceinline__ int pair_audit_rank(const ClusterArgs& p, float sc, bool live, int row_id, int col_id) {
    return live && pairs_in_class(p.pcls, row_id, col_id) ? pairs_rank(sc, p.pside, p.thr) : -1;
}

// count: the histogram epilogue behind the selection filter; counters by rank, then the class's NaN counter
__device__ __forceinline__ void pair_count_tile(const ClusterArgs& p, const v16f (&acc)[2], const PairCols& c, long wrow0, int fr, int fh2) {
    unsigned* h = pair_hist_lds();
    const long arow = wrow0 + fr;
    const int my_id = p.ids && arow < p.G ? p.ids[arow] : 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = gal_acc_row(e) + 4 * fh2;
        const long row = wrow0 + r;
        const int row_id = __shfl(my_id, r);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int rank = pair_audit_rank(p, gal_score(acc[j][e]), c.ok[j] && row < c.col[j], row_id, c.id[j]);
            if (rank >= 0) atomicAdd(&h[rank], 1u);
            else if (rank == -2) atomicAdd(&h[kHistBins], 1u);
        }
    }
}

// collect: selected pairs of rank <= cut go to the candidate buffer; one atomic per wave and accumulator position that has a hit
__device__ __forceinline__ void pair_collect_tile(const ClusterArgs& p, const v16f (&acc)[2], const PairCols& c, long wrow0, int lane, int cut) {
    const int fr = lane & 31, fh2 = lane >> 5;
    const long arow = wrow0 + fr;
    const int my_id = p.ids && arow < p.G ? p.ids[arow] : 0;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = gal_acc_row(e) + 4 * fh2;
        const long row = wrow0 + r;
        const int row_id = __shfl(my_id, r);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float sc = gal_score(acc[j][e]);
            const int rank = pair_audit_rank(p, sc, c.ok[j] && row < c.col[j], row_id, c.id[j]);
            const bool hit = rank >= 0 && rank <= cut;
            const unsigned long long b = __ballot(hit);
            if (b == 0ull) continue;                               // (wave-uniform)
            const int first = __ffsll((long long)b) - 1;
            unsigned base = 0u;
            if (lane == first) base = atomicAdd(p.cand_cnt, (unsigned)__popcll(b));
            base = (unsigned)__shfl((int)base, first);
            const unsigned slot = base + (unsigned)__popcll(b & below);
            if (hit && slot < p.room) p.cand[slot] = make_int4((int)__float_as_uint(sc), (int)row, (int)c.col[j], 0);
        }
    }
}

// setup -> per A tile: gal_tile_dot (gallery_scan.h: THE K loop, with the B chunks fetched from gallery rows) + the mode's epilogue -> flush
template <int MODE>
__device__ __forceinline__ void cluster_pair_body(const ClusterArgs& p) {
    constexpr int BM = GAL_BM, BN = GAL_BN, TN = BN / 32, CD = 64;
    static_assert(TN == 2, "PairCols holds one column per 32-column block");
    __shared__ v4f ldsq[2][BN * 16];                          // B chunk [64 rows][64 k], 16-byte column XOR (row & 15)
    __shared__ int colcnt[BN];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh2 = lane >> 5;
    const int bt = (int)(blockIdx.x % (unsigned)p.tiles_n), run = (int)(blockIdx.x / (unsigned)p.tiles_n);
    const long n0 = (long)bt * BN;
    // A tiles that hold a row below some column of this B tile: rt * 128 <= n0 + 62
    const int rt0 = run * p.tiles_per_wg, rt1 = min(min(p.row_tiles, (int)((n0 + BN - 2) / BM) + 1), rt0 + p.tiles_per_wg);
    if (rt0 >= rt1) return;                                   // (workgroup-uniform, before any barrier)
    const int K = p.dim, chunks = K / CD;
    if (tid < BN) colcnt[tid] = 0;
    if constexpr (MODE == PAIR_HIST) {
        unsigned* h = pair_hist_lds();
        for (int i = tid; i < kHistSlots; i += 256) h[i] = 0u;           // (the first tile's barriers come before the first add)
    }
    if constexpr (MODE == PAIR_COUNT) {
        unsigned* h = pair_hist_lds();
        for (int i = tid; i < kPairsSlots; i += 256) h[i] = 0u;
    }
    int cut = -1;                                                        // collect: the last rank to take (workgroup-uniform)
    if constexpr (MODE == PAIR_COLLECT) {
        cut = *p.cut;
        if (cut < 0) return;                                             // nothing to collect (before any barrier)
    }

    // B loader: pass i fills rows i*16 + (tid >> 4), slot tid & 15 <- source 16-byte column (tid & 15) ^ (row & 15)
    const int qrow = tid >> 4;
    GalSrc<float> b_row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long brow = n0 + qrow + 16 * i;
        b_row[i] = gal_row_or_zeros(brow < p.G, p.gal, (size_t)brow, K, p.zeros, ((tid & 15) ^ (qrow & 15)) * 4, CD);
    }

    PairCols c;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        c.col[j] = n0 + j * 32 + fr;
        c.ok[j] = c.col[j] < p.G;
        c.deg[j] = 0;
        c.core[j] = false;
        c.id[j] = 0;
        if constexpr (MODE == PAIR_LINK) c.core[j] = c.ok[j] && p.deg[c.col[j]] + 1 >= p.min_pts;
        if constexpr (MODE == PAIR_HIST) c.id[j] = c.ok[j] ? p.ids[c.col[j]] : 0;
        if constexpr (MODE == PAIR_COUNT || MODE == PAIR_COLLECT) c.id[j] = p.ids && c.ok[j] ? p.ids[c.col[j]] : 0;
    }

    for (int rt = rt0; rt < rt1; ++rt) {
        const long m0 = (long)rt * BM;
        const long myrow = m0 + wid * 32 + fr;
        const GalSrc<float> a = gal_row_or_zeros(myrow < p.G, p.gal, (size_t)myrow, K, p.zeros, fh2 * 4, CD);
        const float* b_src[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) b_src[i] = b_row[i].ptr;
        auto fetch_b = [&](v4f (&qv)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { qv[i] = *reinterpret_cast<const v4f*>(b_src[i]); b_src[i] += b_row[i].step; }
        };
        v16f acc[TN];
        __syncthreads();                                   // the previous tile's last multiply is done with ldsq
        gal_tile_dot<float>(ldsq, a.ptr, a.step, chunks, tid, fr, fh2, fetch_b, acc);
        const long wrow0 = m0 + wid * 32;                  // the wave's 32-row block
        if constexpr (MODE == PAIR_DEGREE) pair_degree_tile(p, acc, c, wrow0, lane, fh2);
        else if constexpr (MODE == PAIR_LINK) pair_link_tile(p, acc, c, wrow0, fr, fh2);
        else if constexpr (MODE == PAIR_HIST) pair_hist_tile(p, acc, c, wrow0, fr, fh2);
        else if constexpr (MODE == PAIR_COUNT) pair_count_tile(p, acc, c, wrow0, fr, fh2);
        else pair_collect_tile(p, acc, c, wrow0, lane, cut);
    }
    if constexpr (MODE == PAIR_COUNT) {
        // as the histogram pass below: a 32-bit counter holds a run's adds, non-zero counters go to the scratch with 64-bit atomics
        unsigned* h = pair_hist_lds();
        __syncthreads();
        for (int i = tid; i < kPairsSlots; i += 256) {
            const unsigned cnt = h[i];
            if (cnt) atomicAdd(p.hist + i, (unsigned long long)cnt);
        }
    }
    if constexpr (MODE == PAIR_HIST) {
        // A run of t tiles adds at most t * 128 * 64 = t * 8192 to one 32-bit counter; the launcher keeps t <= 2^18 (automatic runs are at
        // most 8 tiles), so a counter never exceeds 2^31.  Non-zero counters go to the scratch histogram (copy blockIdx.x % copies of it)
        // with 64-bit atomics.
        unsigned* h = pair_hist_lds();
        unsigned long long* dst = p.hist + (size_t)(blockIdx.x % (unsigned)p.copies) * kHistSlots;
        __syncthreads();
        for (int i = tid; i < kHistSlots; i += 256) {
            const unsigned cnt = h[i];
            if (cnt) atomicAdd(dst + i, (unsigned long long)cnt);
        }
    }
    if constexpr (MODE == PAIR_DEGREE) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
            if (c.deg[j] > 0) atomicAdd(&colcnt[j * 32 + fr], c.deg[j]);
        __syncthreads();
        if (tid < BN && colcnt[tid] > 0) atomicAdd(p.deg + n0 + tid, colcnt[tid]);     // (a count > 0 implies the column is below G)
    }
}

__global__ __launch_bounds__(256, 2) void cluster_degree_kernel(const ClusterArgs p) { cluster_pair_body<PAIR_DEGREE>(p); }
__global__ __launch_bounds__(256, 2) void cluster_link_kernel(const ClusterArgs p) { cluster_pair_body<PAIR_LINK>(p); }
__global__ __launch_bounds__(256, 2) void cluster_hist_kernel(const ClusterArgs p) { cluster_pair_body<PAIR_HIST>(p); }
__global__ __launch_bounds__(256, 2) void cluster_pairs_count_kernel(const ClusterArgs p) { cluster_pair_body<PAIR_COUNT>(p); }
__global__ __launch_bounds__(256, 2) void cluster_pairs_collect_kernel(const ClusterArgs p) { cluster_pair_body<PAIR_COLLECT>(p); }

// sums the privatised copies into the caller's buffers (both overwritten); d_nan may be null
__global__ __launch_bounds__(256) void cluster_hist_reduce_kernel(const unsigned long long* __restrict__ part, int copies,
                                                                  unsigned long long* __restrict__ hist, unsigned long long* __restrict__ nan) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kHistSlots) return;
    unsigned long long s = 0ull;
    for (int c = 0; c < copies; ++c) s += part[(size_t)c * kHistSlots + i];
    if (i < 2 * kHistBins) hist[i] = s;
    else if (nan) nan[i - 2 * kHistBins] = s;
}

__global__ __launch_bounds__(256) void cluster_init_kernel(long G, int* deg, int* parent, unsigned long long* best, int* info) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < G) { deg[i] = 0; parent[i] = (int)i; best[i] = 0ull; }
    if (info && i < 4) info[i] = 0;
}

// a separate launch: everything the link kernel wrote is visible, plain loads are fine
__global__ __launch_bounds__(256) void cluster_flatten_kernel(long G, int min_pts, int noise_self, const int* __restrict__ deg,
                                                              const int* __restrict__ parent, const unsigned long long* __restrict__ best,
                                                              int* __restrict__ labels, int* info) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool core = false, border = false, root = false, noise = false;
    if (i < G) {
        core = deg[i] + 1 >= min_pts;
        const unsigned long long b = best[i];
        border = !core && b != 0ull;
        noise = !core && !border;
        int label = noise_self ? (int)i : -1;
        if (core || border) {
            int x = core ? (int)i : (int)~(unsigned)b;
            while (parent[x] != x) x = parent[x];
            label = x;
            root = core && x == (int)i;
        }
        labels[i] = label;
    }
    if (info) {
        const int c0 = __popcll(__ballot(root)), c1 = __popcll(__ballot(core)), c2 = __popcll(__ballot(border)), c3 = __popcll(__ballot(noise));
        if ((threadIdx.x & 63) == 0) {
            if (c0) atomicAdd(info + 0, c0);
            if (c1) atomicAdd(info + 1, c1);
            if (c2) atomicAdd(info + 2, c2);
            if (c3) atomicAdd(info + 3, c3);
        }
    }
}

int g_cluster_tiles = 0;
int g_hist_copies = 0;
long g_pairs_room = 0;

// the pair passes' grid: tiles, the run length (A tiles per workgroup) and the number of workgroups
unsigned cluster_pair_grid(ClusterArgs& a, long G) {
    a.tiles_n = (int)((G + GAL_BN - 1) / GAL_BN);
    a.row_tiles = (int)((G + GAL_BM - 1) / GAL_BM);
    // A tiles per workgroup: a longer run flushes the column counts less often and re-reads the core flags less often, a shorter one
    // balances the triangle better; runs only grow once every CU has several workgroups' worth of live tile pairs anyway
    const long pairs = (long)a.tiles_n * a.row_tiles / 2;
    long t = g_cluster_tiles;
    if (t <= 0) {
        t = pairs / (16L * conv_num_cus());
        t = t < 1 ? 1 : t > 8 ? 8 : t;
    }
    t = t > (1L << 18) ? (1L << 18) : t;                                 // (the histogram pass's 32-bit LDS counters: t * 8192 < 2^32)
    a.tiles_per_wg = (int)(t > a.row_tiles ? a.row_tiles : t);
    // a rectangular grid of (B tile, run): the last B tile reaches every row tile; runs wholly below a B tile's diagonal exit at once
    const long runs = (a.row_tiles + a.tiles_per_wg - 1) / a.tiles_per_wg;
    const long grid = runs * a.tiles_n;
    if (grid > 0x7fffffffL) throw std::runtime_error("gallery: too many rows for one clustering launch");
    return (unsigned)grid;
}

}  // namespace

void cluster_debug_tiles(int tiles_per_wg) { g_cluster_tiles = tiles_per_wg > 0 ? tiles_per_wg : 0; }
void cluster_debug_hist_copies(int copies) { g_hist_copies = copies > 0 ? (copies > 4096 ? 4096 : copies) : 0; }
void pairs_debug_room(long room) { g_pairs_room = room > 0 ? (room > (1L << 24) ? (1L << 24) : room) : 0; }

void launch_gallery_cluster(const float* gal, long G, int dim, float thr, int min_pts, bool noise_self, int* deg, int* parent,
                            unsigned long long* best, int* labels, int* info, hipStream_t s) {
    if (G <= 0) return;
    if (dim % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    ClusterArgs a{};
    a.gal = gal; a.zeros = conv_zero_line(); a.G = G; a.dim = dim; a.min_pts = min_pts; a.thr = thr;
    a.deg = deg; a.parent = parent; a.best = best;
    const unsigned grid = cluster_pair_grid(a, G);
    const unsigned gb = (unsigned)((G + 255) / 256);
    hipLaunchKernelGGL(cluster_init_kernel, dim3(gb), dim3(256), 0, s, G, deg, parent, best, info);
    if (min_pts > 1) hipLaunchKernelGGL(cluster_degree_kernel, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cluster_link_kernel, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(gb), dim3(256), 0, s, G, min_pts, noise_self ? 1 : 0, deg, parent, best, labels, info);
}

// The workgroups flush into a scratch histogram and a small kernel writes the caller's two buffers from it (d_nan may be null, and the
// 64-bit atomics stay off the caller's memory).  The impostor scores of real embeddings pile into a few hundred bins and every live
// workgroup flushes those same bins, so the scratch may hold several privatised copies (copy = blockIdx.x % copies) that the small
// kernel sums — measured at G = 65 536 and 262 144, 1 to 512 copies change the call's time by under 1 % either way
// (profiles/gallery_hist.md: the flush is not what the epilogue costs), so the default is one; cluster_debug_hist_copies re-measures.
int gallery_pair_hist_copies() { return g_hist_copies > 0 ? g_hist_copies : kHistDefaultCopies; }
size_t gallery_pair_hist_scratch_bytes() { return (size_t)gallery_pair_hist_copies() * kHistSlots * sizeof(unsigned long long); }

void launch_gallery_pair_hist(const float* gal, const int* ids, long G, int dim, unsigned long long* scratch, unsigned long long* hist,
                              unsigned long long* nan, hipStream_t s) {
    if (G <= 0) return;
    if (dim % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    ClusterArgs a{};
    a.gal = gal; a.zeros = conv_zero_line(); a.G = G; a.dim = dim;
    a.ids = ids; a.hist = scratch; a.copies = gallery_pair_hist_copies();
    const unsigned grid = cluster_pair_grid(a, G);
    FH_HIP(hipMemsetAsync(scratch, 0, gallery_pair_hist_scratch_bytes(), s));
    hipLaunchKernelGGL(cluster_hist_kernel, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cluster_hist_reduce_kernel, dim3((kHistSlots + 255) / 256), dim3(256), 0, s, scratch, a.copies, hist, nan);
}

// The pair audit.  scratch: kPairsHead 64-bit words — the counters by rank, the NaN counter, {cut, slot counter}, {returned, -} — then
// the candidates; the head is cleared on s first.  At most `room` candidates are ever appended (the cut sees to it).
long gallery_pairs_room(int cap) {
    const long room = g_pairs_room > 0 ? g_pairs_room : kPairsRoom;
    return room > cap ? room : cap;
}
size_t gallery_pairs_scratch_bytes(int cap) { return kPairsHead * sizeof(unsigned long long) + (size_t)gallery_pairs_room(cap) * sizeof(int4); }

void launch_gallery_pairs(const float* gal, const int* ids, long G, int dim, int cls, int side, float thr, int cap,
                          unsigned long long* scratch, unsigned long long* info, float* out_s, int* out_rows, int* out_ids, hipStream_t s) {
    if (G <= 0) return;
    if (dim % 64) throw std::runtime_error("gallery: dim must be a multiple of 64");
    const long room = gallery_pairs_room(cap);
    ClusterArgs a{};
    a.gal = gal; a.zeros = conv_zero_line(); a.G = G; a.dim = dim; a.thr = thr;
    a.ids = cls == kPairsAny ? nullptr : ids; a.hist = scratch; a.copies = 1;
    a.pcls = cls; a.pside = side;
    int* words = reinterpret_cast<int*>(scratch + kPairsSlots);
    a.cut = words; a.cand_cnt = reinterpret_cast<unsigned*>(words + 1);
    a.cand = reinterpret_cast<int4*>(scratch + kPairsHead); a.room = (unsigned)room;
    const unsigned grid = cluster_pair_grid(a, G);
    FH_HIP(hipMemsetAsync(scratch, 0, kPairsHead * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(cluster_pairs_count_kernel, dim3(grid), dim3(256), 0, s, a);
    launch_pairs_cut(scratch, cap, room, info, s);
    if (!out_s && !out_rows && !out_ids) return;                         // the count-only form
    hipLaunchKernelGGL(cluster_pairs_collect_kernel, dim3(grid), dim3(256), 0, s, a);
    launch_pairs_select(scratch, room, side, cap, ids, out_s, out_rows, out_ids, s);
}

}  // namespace fh
