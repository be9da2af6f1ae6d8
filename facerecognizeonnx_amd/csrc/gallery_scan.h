// gallery_scan.h — the streaming 1:N scan shared by gallery_topk_kernel (gallery.hip: lists of rows) and gallery_topk_ids_kernel
// (gallery_ids.hip: lists of identities).  The design notes and measurements are in gallery.hip's header; IDS = false compiles to
// exactly the row-level kernel (every identity statement sits behind `if constexpr (IDS)`), and both instantiations run the same K
// loop with the same operand placement and k order, so a score has the same bits in either.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace fh {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int GAL_BM = 128, GAL_BN = 64, GAL_KMAX = 16, GAL_QCAP = 32;

struct GalArgs {
    const float* gal;       // [G][dim]
    const float* q;         // [tiles_n * 64][dim], rows >= Q are zero
    const float* zeros;
    long G, idx_base;
    int dim, Q, k, tiles_n, row_tiles, tiles_per_part;
    float* ps;              // [parts][Q][k]
    int* pi;
    const float* seed_s;    // optional [Q][k]: exact top-k of a PREFIX of the gallery — its k-th entry is a valid admission threshold for
    const int* seed_i;      // the whole scan (k rows at least as good exist), so the per-workgroup lists start almost closed
    const int* qcount;      // optional (device): query tiles at or beyond *qcount exit at once (null: all Q)
    const int* ids;         // IDS: identity id of every row [G]
    int* pd;                // IDS: [parts][Q][k] identity ids beside ps / pi
};

__device__ __forceinline__ bool gal_better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// IDS: thread q's list holds at most ONE entry per identity — the identity's best row seen so far — so its k-th entry is the k-th
// DISTINCT identity and a valid admission threshold: k identities already have a row at least that good, and a listed identity only
// ever improves.  A row's id is fetched (4-byte gather) only when the row passes the threshold, and travels through the slot queue
// as a third word.  The insertion stays ONE compare-exchange pass: whatever the pass holds in hand after position pos — the new
// entry (not yet placed: the listed one is better, the new one is dropped) or the entry it displaced (the new one is better and took
// an earlier place) — is discarded when the entry listed at pos carried the new entry's id.
template <bool IDS>
__device__ __forceinline__ void gallery_scan_body(const GalArgs& p) {
    constexpr int BM = GAL_BM, BN = GAL_BN, TN = BN / 32;
    __shared__ v4f ldsq[2][BN * 16];                          // query chunk [64 rows][64 k], 16-byte column XOR (row & 15)
    __shared__ float tau_s[BN];                               // admission threshold per query = the k-th entry of its list
    __shared__ int tau_i[BN];
    __shared__ float que_s[BN][GAL_QCAP];
    __shared__ int que_i[BN][GAL_QCAP];
    __shared__ int que_d[IDS ? BN : 1][GAL_QCAP];
    __shared__ int cnt[BN];
    __shared__ int overflow;
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
    if (p.qcount && n0 >= *p.qcount) return;                  // (workgroup-uniform, before any barrier)
    const int K = p.dim, chunks = K / 64, k = p.k;
    const int rt0 = part * p.tiles_per_part, rt1 = min(p.row_tiles, rt0 + p.tiles_per_part);

    float ls[GAL_KMAX];                                       // thread q < 64: sorted list of query q (entries >= k stay sentinels)
    int li[GAL_KMAX];
    int ld[IDS ? GAL_KMAX : 1];
#pragma unroll
    for (int i = 0; i < GAL_KMAX; ++i) { ls[i] = -INFINITY; li[i] = INT_MAX; }
    if constexpr (IDS) {
#pragma unroll
        for (int i = 0; i < GAL_KMAX; ++i) ld[i] = -1;
    }
    if (tid < BN) {
        float ts = -INFINITY; int ti = INT_MAX;                   // (-inf, INT_MAX): below every real entry, whatever the rows' norms (compareFaces does not clamp, face_recognizer.cpp:320-334)
        if (p.seed_i && n0 + tid < p.Q) {
            const size_t o = (size_t)(n0 + tid) * k + (k - 1);
            if (p.seed_i[o] >= 0) { ts = p.seed_s[o]; ti = p.seed_i[o]; }
        }
        cnt[tid] = 0; tau_s[tid] = ts; tau_i[tid] = ti;
    }
    if (tid == 0) overflow = 0;

    // query loader: pass i fills rows i*16 + (tid >> 4), slot tid & 15 <- source column (tid & 15) ^ (row & 15)
    const int qrow = tid >> 4;
    const float* const q_base = p.q + (size_t)(n0 + qrow) * K + (((tid & 15) ^ (qrow & 15)) * 4);
    const size_t q16 = (size_t)16 * K;
    const int fsw = fr & 15;

    for (int rt = rt0; rt < rt1; ++rt) {
        const long m0 = (long)rt * BM;
        const long myrow = m0 + wid * 32 + fr;
        const bool live = myrow < p.G;
        const float* a_ptr = (live ? p.gal + (size_t)myrow * K : p.zeros) + fh2 * 4;       // dead rows read the zero line (and are masked below)
        const int a_step = live ? 64 : 0;
        const float* q_src = q_base;
        v4f xa[2][8];
        auto load_a = [&](v4f (&x)[8]) {
#pragma unroll
            for (int s = 0; s < 8; ++s) x[s] = *reinterpret_cast<const v4f*>(a_ptr + s * 8);
            a_ptr += a_step;
        };
        v16f acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
        auto multiply = [&](const v4f (&x)[8], int buf) {
            const v4f* Wt = ldsq[buf] + fr * 16;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int col = (2 * s + fh2) ^ fsw;
                v4f w[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) w[j] = Wt[j * 32 * 16 + col];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s][e], w[j][e], acc[j], 0, 0, 0);
            }
        };
        // The query chunk goes global -> registers -> LDS (not by LDS-DMA): the compiler makes every LDS read wait for ALL vector-memory
        // traffic while an LDS-DMA is in flight (it cannot tell the two halves of ldsq apart: `s_waitcnt vmcnt(0)` in front of each
        // multiply, i.e. every chunk waited out its own gallery-row loads).  Through registers the dependencies are exact: the 4 query
        // loads are issued BEFORE the 8 row loads, so the ds_write after the multiply waits with vmcnt(8) and the row loads fly on until
        // the next barrier.  sched_barrier: left alone, the scheduler sinks the row loads below the multiply (one register set instead
        // of two) and serialises them with it.
        v4f qv[4];
        auto fetch_q = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = *reinterpret_cast<const v4f*>(q_src + i * q16);
            q_src += 64;
        };
        auto store_q = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ldsq[buf][i * 256 + tid] = qv[i];
        };
        __syncthreads();                                   // previous tile's epilogue is done with the LDS lists / queues
        fetch_q();
        load_a(xa[0]);
        store_q(0);
        int kc = 0;
        for (; kc + 2 <= chunks; kc += 2) {
            __syncthreads();                               // queries of chunk kc are in LDS (and xa[0] has landed: the barrier drains vmcnt)
            fetch_q();
            load_a(xa[1]);
            __builtin_amdgcn_sched_barrier(0);
            multiply(xa[0], 0);
            store_q(1);
            __syncthreads();
            if (kc + 2 < chunks) { fetch_q(); load_a(xa[0]); }
            __builtin_amdgcn_sched_barrier(0);
            multiply(xa[1], 1);
            if (kc + 2 < chunks) store_q(0);
        }
        if (kc < chunks) {                                 // odd number of 64-deep chunks
            __syncthreads();
            multiply(xa[0], 0);
        }
        // ---- top-k epilogue (as gallery_topk_kernel)
        const long rbase = m0 + wid * 32 + 4 * fh2;
        auto push = [&](int g_lo, int g_hi) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int qi = j * 32 + fr;
                const float ts = tau_s[qi];
                const int ti = tau_i[qi];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if ((e >> 2) < g_lo || (e >> 2) >= g_hi) continue;
                    const long row = rbase + 8 * (e >> 2) + (e & 3);
                    const float sc = (acc[j][e] + 1.0f) / 2.0f;
                    const int gi = (int)(p.idx_base + row);
                    if (row < p.G && !gal_better(ts, ti, sc, gi)) {          // at least as good as the threshold entry (which may be this very row)
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
                        for (int pos = 0; pos < GAL_KMAX; ++pos) {  // the same pass; the entry in hand is discarded behind the listed entry of identity idn
                            const bool sw = gal_better(s, gi, ls[pos], li[pos]);
                            const float os = ls[pos]; const int oi = li[pos], od = ld[pos];
                            ls[pos] = sw ? s : os; li[pos] = sw ? gi : oi; ld[pos] = sw ? d : od;
                            const bool drop = od == idn;
                            s = drop ? -INFINITY : sw ? os : s; gi = drop ? INT_MAX : sw ? oi : gi; d = drop ? -1 : sw ? od : d;
                        }
                    } else {
#pragma unroll
                        for (int pos = 0; pos < GAL_KMAX; ++pos) {      // one compare-exchange pass keeps all 16 slots sorted (score desc, index asc)
                            const bool sw = gal_better(s, gi, ls[pos], li[pos]);
                            const float os = ls[pos]; const int oi = li[pos];
                            ls[pos] = sw ? s : os; li[pos] = sw ? gi : oi;
                            s = sw ? os : s; gi = sw ? oi : gi;
                        }
                    }
                }
                if (n > 0) {
                    int km1 = k - 1;
#if defined(__HIP_DEVICE_COMPILE__)
                    asm volatile("" : "+v"(km1));                // (keeps the 16 position tests on the vector side: no SGPR mask per slot)
#endif
                    float ts = ls[0]; int ti = li[0];
#pragma unroll
                    for (int pos = 1; pos < GAL_KMAX; ++pos) { ts = pos == km1 ? ls[pos] : ts; ti = pos == km1 ? li[pos] : ti; }
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
    if (tid < BN && n0 + tid < p.Q) {
        const size_t o = ((size_t)part * p.Q + n0 + tid) * k;
#pragma unroll
        for (int pos = 0; pos < GAL_KMAX; ++pos)
            if (pos < k) {
                p.ps[o + pos] = li[pos] == INT_MAX ? -1.0f : ls[pos]; p.pi[o + pos] = li[pos] == INT_MAX ? -1 : li[pos];
                if constexpr (IDS) p.pd[o + pos] = li[pos] == INT_MAX ? -1 : ld[pos];
            }
    }
}

}  // namespace fh
