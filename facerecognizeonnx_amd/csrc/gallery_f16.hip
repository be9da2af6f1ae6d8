// gallery_f16.hip — the opt-in F16_RERANK scan of the 1:N gallery (fh_gallery_set_scan).  Same answer as gallery.hip, bit for bit:
//   1. gal16_convert_kernel: an fp16 copy of the rows (round to nearest even) beside the fp32 rows, and in the same pass the bounds the
//      certificate needs: max ||g||, max ||g^||, max ||g - g^|| (g^ = the fp16 row; the difference is exact in f32), rounded up.
//   2. gal16_scan_kernel: gallery_topk_kernel's design on v_mfma_f32_32x32x16_f16 with f32 accumulation — per-wave rows straight into
//      registers, the 64-query tile through LDS, thread q's sorted list in registers, threshold-gated LDS queues with the four-round
//      replay, the seed pass, per-part lists + topk_merge_kernel — keeping the top GAL16_KC (32) rows per query by fp16 mapped score,
//      total order (score desc, index asc).  A 128-deep chunk of fp16 rows is 256 bytes per row: the loads, the 16-byte column swizzle
//      and the LDS image of one chunk are those of gallery_topk_kernel's 64-deep f32 chunk, and a chunk is 8 MFMAs per 32x32 block where
//      the f32 kernel issues 32.  Needs dim % 128 == 0 (other dims take the fp32 scan).  One workgroup per CU (register budget), and at
//      most 8192 / 32 = 256 parts per query tile, so that the merge of 32-deep lists stays on topk_merge_kernel's cached path.
//   3. gal16_rescore_kernel: one wave per query re-scores its 32 candidates from the FP32 rows with v_mfma_f32_32x32x2_f32 in exactly
//      the operand placement and k order of gallery_topk_kernel's multiply (lane (row fr, half fh2) holds k = kc*64 + (2s + fh2)*4 + e;
//      loop kc, s = 0..7, e = 0..3; accumulator from 0; score = (acc + 1) / 2).  One output element depends only on its row, its column
//      and that sequence, so the scores are bitwise those of the fp32 scan; the top-k of the candidates by (score desc, index asc) follows.
//   4. the certificate: with s16_min = the fp16 score of the 32nd candidate and D_q a rigorous bound on |s32 - s16| over
//      all rows (doubled for safety), the query is certified iff the re-scored k-th score > s16_min + D_q: every other row then scores
//      strictly below the k-th in fp32 and can neither enter nor tie.  A list that is not full must hold all G rows.
//   5. uncertified queries are compacted on the device (count + indices) and answered by the fp32 scan + merge with a device query count
//      (gallery.hip / face_kernels.hip: workgroups beyond the count exit at once), then scattered into the output.  No host round trip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "kernels.h"

namespace fh {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

constexpr int G16_BM = 128, G16_BN = 64, G16_KC = GAL16_KC, G16_QCAP = 32;
static_assert(G16_KC == 32, "the list / replay logic below assumes 32-deep lists");

__device__ __forceinline__ bool g16_better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// sqrt of a non-negative double sum, rounded UP to float (the bounds must not be underestimated)
__device__ __forceinline__ float g16_sqrt_up(double ss) {
    const double r = sqrt(ss) * (1.0 + 1e-12);
    float f = (float)r;
    if ((double)f < r) f = nextafterf(f, INFINITY);
    return f;
}

// ------------------------------------------------------------------------------------------ 1. conversion + bounds, one wave per row
__global__ __launch_bounds__(256) void gal16_convert_kernel(const float* __restrict__ rows, _Float16* __restrict__ rows16, long n, int dim,
                                                            unsigned* __restrict__ stats) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* g = rows + (size_t)row * dim;
    _Float16* h = rows16 + (size_t)row * dim;
    double sg = 0.0, sh = 0.0, sd = 0.0;
    int bad = 0;
    for (int i = lane; i < dim; i += 64) {
        const float x = g[i];
        const _Float16 xh = (_Float16)x;                           // round to nearest even
        const float xb = (float)xh;
        h[i] = xh;
        if (!(fabsf(x) <= 65504.0f)) bad = 1;                      // non-finite, or beyond the fp16 range
        const double d = (double)x - (double)xb;                  // exact
        sg += (double)x * x; sh += (double)xb * xb; sd += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sg += __shfl_xor(sg, o); sh += __shfl_xor(sh, o); sd += __shfl_xor(sd, o);
        bad |= __shfl_xor(bad, o);
    }
    if (lane == 0) {                                               // non-negative floats order like their bit patterns
        atomicMax(&stats[0], __float_as_uint(g16_sqrt_up(sg)));
        atomicMax(&stats[1], __float_as_uint(g16_sqrt_up(sh)));
        atomicMax(&stats[2], __float_as_uint(g16_sqrt_up(sd)));
        if (bad) atomicOr(&stats[3], 1u);
    }
}

void launch_gallery16_convert(const float* rows, uint16_t* rows16, long n, int dim, unsigned* stats, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(gal16_convert_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, rows, reinterpret_cast<_Float16*>(rows16), n, dim,
                       stats);
}

// queries f32 [Q][dim] -> fp16 [qrows][dim], zero rows behind Q
__global__ __launch_bounds__(256) void gal16_pack_q_kernel(const float* __restrict__ q, _Float16* __restrict__ q16, int Q, long total, int dim) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    q16[i] = i / dim < Q ? (_Float16)q[i] : (_Float16)0.0f;
}

// ------------------------------------------------------------------------------------------ 2. fp16 scan
struct Gal16Args {
    const _Float16* gal;    // [G][dim]
    const _Float16* q;      // [tiles_n * 64][dim], rows >= Q are zero
    const _Float16* zeros;
    long G, idx_base;
    int dim, Q, tiles_n, row_tiles, tiles_per_part;
    float* ps;              // [parts][Q][32]
    int* pi;
    const float* seed_s;    // optional [Q][32]: exact fp16 top-32 of a prefix of the gallery (its 32nd entry: an admission threshold)
    const int* seed_i;
};

__global__ __launch_bounds__(256, 1) void gal16_scan_kernel(const Gal16Args p) {
    constexpr int BM = G16_BM, BN = G16_BN, TN = BN / 32, KC = G16_KC;
    __shared__ v4f ldsq[2][BN * 16];                          // query chunk [64 rows][128 k] fp16, 16-byte column XOR (row & 15)
    __shared__ float tau_s[BN];                               // admission threshold per query = the 32nd entry of its list
    __shared__ int tau_i[BN];
    __shared__ float que_s[BN][G16_QCAP];
    __shared__ int que_i[BN][G16_QCAP];
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
    const int K = p.dim, chunks = K / 128;
    const int rt0 = part * p.tiles_per_part, rt1 = min(p.row_tiles, rt0 + p.tiles_per_part);

    float ls[KC];                                             // thread q < 64: sorted list of query q
    int li[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) { ls[i] = -INFINITY; li[i] = INT_MAX; }
    if (tid < BN) {
        float ts = -INFINITY; int ti = INT_MAX;
        if (p.seed_i && n0 + tid < p.Q) {
            const size_t o = (size_t)(n0 + tid) * KC + (KC - 1);
            if (p.seed_i[o] >= 0) { ts = p.seed_s[o]; ti = p.seed_i[o]; }
        }
        cnt[tid] = 0; tau_s[tid] = ts; tau_i[tid] = ti;
    }
    if (tid == 0) overflow = 0;

    // query loader: pass i fills rows i*16 + (tid >> 4), slot tid & 15 <- source 16-byte column (tid & 15) ^ (row & 15)
    const int qrow = tid >> 4;
    const _Float16* const q_base = p.q + (size_t)(n0 + qrow) * K + (((tid & 15) ^ (qrow & 15)) * 8);
    const size_t q16 = (size_t)16 * K;
    const int fsw = fr & 15;

    for (int rt = rt0; rt < rt1; ++rt) {
        const long m0 = (long)rt * BM;
        const long myrow = m0 + wid * 32 + fr;
        const bool live = myrow < p.G;
        const _Float16* a_ptr = (live ? p.gal + (size_t)myrow * K : p.zeros) + fh2 * 8;
        const int a_step = live ? 128 : 0;
        const _Float16* q_src = q_base;
        v4f xa[2][8];
        auto load_a = [&](v4f (&x)[8]) {                      // 16-byte column 2s + fh2 of the chunk: k = s*16 + fh2*8 .. +7
#pragma unroll
            for (int s = 0; s < 8; ++s) x[s] = *reinterpret_cast<const v4f*>(a_ptr + s * 16);
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
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const v4f w = Wt[j * 32 * 16 + col];
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, x[s]), __builtin_bit_cast(v8h, w), acc[j], 0, 0, 0);
                }
            }
        };
        v4f qv[4];
        auto fetch_q = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = *reinterpret_cast<const v4f*>(q_src + i * q16);
            q_src += 128;
        };
        auto store_q = [&](int buf) {
#pragma unroll
            for (int i = 0; i < 4; ++i) ldsq[buf][i * 256 + tid] = qv[i];
        };
        __syncthreads();
        fetch_q();
        load_a(xa[0]);
        store_q(0);
        int kc = 0;
        for (; kc + 2 <= chunks; kc += 2) {
            __syncthreads();
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
        if (kc < chunks) {
            __syncthreads();
            multiply(xa[0], 0);
        }
        // ---- top-32 epilogue (gallery_topk_kernel's, 32-deep lists)
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
                    if (row < p.G && !g16_better(ts, ti, sc, gi)) {
                        const int slot = atomicAdd(&cnt[qi], 1);
                        if (slot < G16_QCAP) { que_s[qi][slot] = sc; que_i[qi][slot] = gi; }
                        else overflow = 1;
                    }
                }
            }
        };
        auto insert = [&]() {
            if (tid < BN) {
                const int n = min(cnt[tid], G16_QCAP);
                for (int c = 0; c < n; ++c) {
                    float s = que_s[tid][c];
                    int gi = que_i[tid][c];
#pragma unroll
                    for (int pos = 0; pos < KC; ++pos) {
                        const bool sw = g16_better(s, gi, ls[pos], li[pos]);
                        const float os = ls[pos]; const int oi = li[pos];
                        ls[pos] = sw ? s : os; li[pos] = sw ? gi : oi;
                        s = sw ? os : s; gi = sw ? oi : gi;
                    }
                }
                if (n > 0) {
                    const float ts = ls[KC - 1]; const int ti = li[KC - 1];
                    if (ti != INT_MAX && g16_better(ts, ti, tau_s[tid], tau_i[tid])) { tau_s[tid] = ts; tau_i[tid] = ti; }
                }
                cnt[tid] = 0;
            }
        };
        push(0, 4);
        __syncthreads();
        if (overflow) {                                       // replay in four 32-row rounds: at most 32 entries per query each
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
        const size_t o = ((size_t)part * p.Q + n0 + tid) * KC;
#pragma unroll
        for (int pos = 0; pos < KC; ++pos) { p.ps[o + pos] = li[pos] == INT_MAX ? -1.0f : ls[pos]; p.pi[o + pos] = li[pos] == INT_MAX ? -1 : li[pos]; }
    }
}

// parts of the row range for G rows and Q queries: ONE workgroup per CU (the 32-deep lists + two row chunks in flight need more than the
// 256 registers of two waves per SIMD: 104 bytes of spills at (256, 2)), at most 256 per query tile (merge of 32-deep lists: 8192 entries)
int gallery16_parts(long G, int Q, int* tiles_per_part) {
    const int tiles_n = (Q + G16_BN - 1) / G16_BN;
    const long row_tiles = (G + G16_BM - 1) / G16_BM;
    long parts = (long)conv_num_cus() / tiles_n;
    if (parts > 8192 / G16_KC) parts = 8192 / G16_KC;
    if (parts < 1) parts = 1;
    if (parts > row_tiles) parts = row_tiles;
    const long tpp = parts > 0 ? (row_tiles + parts - 1) / parts : 1;
    if (tiles_per_part) *tiles_per_part = (int)tpp;
    return (int)(tpp > 0 ? (row_tiles + tpp - 1) / tpp : 0);
}

void launch_gallery16_candidates(const uint16_t* rows16, long G, int dim, const float* q, uint16_t* q16, int Q, long idx_base, float* part_score,
                                 int* part_idx, float* seed_score, int* seed_idx, float* cand_score, int* cand_idx, hipStream_t s) {
    if (G <= 0 || Q <= 0) return;
    if (dim % 128) throw std::runtime_error("gallery f16 scan: need dim % 128 == 0");
    if (idx_base + G > (long)INT_MAX) throw std::runtime_error("gallery: global row indices must fit in 31 bits");
    const int tiles_n = (Q + G16_BN - 1) / G16_BN;
    const long qtotal = (long)tiles_n * G16_BN * dim;
    hipLaunchKernelGGL(gal16_pack_q_kernel, dim3((unsigned)((qtotal + 255) / 256)), dim3(256), 0, s, q, reinterpret_cast<_Float16*>(q16), Q, qtotal,
                       dim);
    Gal16Args a{};
    a.gal = reinterpret_cast<const _Float16*>(rows16); a.q = reinterpret_cast<const _Float16*>(q16);
    a.zeros = reinterpret_cast<const _Float16*>(conv_zero_line());
    a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.tiles_n = tiles_n;
    a.ps = part_score; a.pi = part_idx;
    constexpr long SEED_ROWS = 4096;                         // as gallery.hip: the exact top-32 of a prefix closes the lists early
    if (G >= 16 * SEED_ROWS && seed_score && seed_idx) {
        a.G = SEED_ROWS;
        a.row_tiles = (int)(SEED_ROWS / G16_BM);
        const int sp = gallery16_parts(a.G, Q, &a.tiles_per_part);
        hipLaunchKernelGGL(gal16_scan_kernel, dim3((unsigned)(sp * tiles_n)), dim3(256), 0, s, a);
        launch_topk_merge(part_score, part_idx, sp, Q, G16_KC, seed_score, seed_idx, s);
        a.seed_s = seed_score; a.seed_i = seed_idx;
    }
    a.G = G;
    a.row_tiles = (int)((G + G16_BM - 1) / G16_BM);
    const int parts = gallery16_parts(G, Q, &a.tiles_per_part);
    hipLaunchKernelGGL(gal16_scan_kernel, dim3((unsigned)(parts * tiles_n)), dim3(256), 0, s, a);
    launch_topk_merge(part_score, part_idx, parts, Q, G16_KC, cand_score, cand_idx, s);
}

// ------------------------------------------------------------------------------------------ 3. + 4. re-score, top-k, certificate
struct Gal16Rescore {
    const float* gal;       // fp32 rows [G][dim]
    const float* q;         // queries [Q][dim]
    const float* zeros;
    const float* cand_s;    // [Q][32] fp16 mapped scores, (score desc, index asc)
    const int* cand_i;      // [Q][32] global indices, -1 = empty
    long G, idx_base;
    int dim, Q, k;
    float gn, ghn, dn;      // max ||g||, max ||g^||, max ||g - g^||
    float* out_s;
    int* out_i;
    int* fb_count;
    int* fb_idx;
    unsigned long long* counters;
};

__global__ __launch_bounds__(64) void gal16_rescore_kernel(const Gal16Rescore p) {
    __shared__ float cs[G16_KC];
    __shared__ int ci[G16_KC];
    __shared__ float kth;
    const int qn = blockIdx.x, lane = threadIdx.x, fr = lane & 31, fh2 = lane >> 5;
    const int K = p.dim, chunks = K / 64, k = p.k;
    const float* qrow = p.q + (size_t)qn * K;
    const int gi = p.cand_i[(size_t)qn * G16_KC + fr];
    const bool live = gi >= 0;
    // the fp32 score of candidate fr: gallery_topk_kernel's multiply, with the query in every column of B
    const float* a_ptr = (live ? p.gal + (size_t)(gi - p.idx_base) * K : p.zeros) + fh2 * 4;
    const int a_step = live ? 64 : 0;
    const float* b_ptr = qrow + fh2 * 4;
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
    if (fr == 0) {                                            // column 0: rows 8 * (e >> 2) + 4 * fh2 + (e & 3)
#pragma unroll
        for (int e = 0; e < 16; ++e) cs[8 * (e >> 2) + 4 * fh2 + (e & 3)] = (acc[e] + 1.0f) / 2.0f;
    }
    if (lane < G16_KC) ci[lane] = gi;
    // query norms (the same f16 conversion the scan's queries went through)
    double sq = 0.0, sh = 0.0, sd = 0.0;
    for (int i = lane; i < K; i += 64) {
        const float x = qrow[i];
        const float xb = (float)(_Float16)x;
        const double d = (double)x - (double)xb;
        sq += (double)x * x; sh += (double)xb * xb; sd += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sq += __shfl_xor(sq, o); sh += __shfl_xor(sh, o); sd += __shfl_xor(sd, o); }
    __syncthreads();
    // rank of candidate `lane` among the valid ones by (score desc, index asc)
    int nvalid = 0, rank = 0;
    const float my_s = lane < G16_KC ? cs[lane] : 0.f;
    for (int c = 0; c < G16_KC; ++c) {
        const int oi = ci[c];
        if (oi < 0) continue;
        ++nvalid;
        if (lane < G16_KC && live && g16_better(cs[c], oi, my_s, gi)) ++rank;
    }
    if (lane < G16_KC && live && rank == k - 1) kth = my_s;
    __syncthreads();
    bool cert;
    const float s16_last = p.cand_s[(size_t)qn * G16_KC + (G16_KC - 1)];
    if ((long)nvalid == p.G) {
        cert = true;                                           // every row is a candidate
    } else if (ci[G16_KC - 1] < 0) {
        cert = false;                                          // (a list that is not full must hold every row)
    } else {
        // D = gamma_d (|q| max|g| + |q^| max|g^|) + |q - q^| max|g^| + |q| max|g - g^| on raw dots; halved for mapped scores, plus the
        // rounding of the two (dot + 1) mappings; times 2 (the MFMA's internal summation order is not specified)
        const double nq = sqrt(sq) * (1.0 + 1e-12), nqh = sqrt(sh) * (1.0 + 1e-12), ndq = sqrt(sd) * (1.0 + 1e-12);
        const double u = 5.9604644775390625e-08, du = (double)K * u;           // 2^-24
        const double gamma = du / (1.0 - du);
        const double big = nq * p.gn + nqh * p.ghn;
        const double raw = gamma * big + ndq * p.ghn + nq * p.dn;
        const double delta = 2.0 * (0.5 * raw + u * (2.0 + big) + 1e-30);
        cert = nvalid >= k && (double)kth > (double)s16_last + delta;         // (false for NaN)
    }
    if (cert) {
        if (lane < G16_KC && live && rank < k) { p.out_s[(size_t)qn * k + rank] = my_s; p.out_i[(size_t)qn * k + rank] = gi; }
        if (lane >= nvalid && lane < k) { p.out_s[(size_t)qn * k + lane] = -1.0f; p.out_i[(size_t)qn * k + lane] = -1; }
        if (lane == 0) atomicAdd(&p.counters[0], 1ull);
    } else if (lane == 0) {
        const int slot = atomicAdd(p.fb_count, 1);
        p.fb_idx[slot] = qn;
        atomicAdd(&p.counters[1], 1ull);
    }
}

void launch_gallery16_rescore(const float* rows, long G, int dim, const float* q, int Q, int k, long idx_base, const float* cand_score,
                              const int* cand_idx, float gn, float ghn, float dn, float* out_score, int* out_idx, int* fb_count, int* fb_idx,
                              unsigned long long* counters, hipStream_t s) {
    if (Q <= 0) return;
    if (dim % 64 || k < 1 || k > 16) throw std::runtime_error("gallery: need dim % 64 == 0 and 1 <= k <= 16");
    Gal16Rescore a{};
    a.gal = rows; a.q = q; a.zeros = conv_zero_line(); a.cand_s = cand_score; a.cand_i = cand_idx;
    a.G = G; a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.k = k; a.gn = gn; a.ghn = ghn; a.dn = dn;
    a.out_s = out_score; a.out_i = out_idx; a.fb_count = fb_count; a.fb_idx = fb_idx; a.counters = counters;
    hipLaunchKernelGGL(gal16_rescore_kernel, dim3((unsigned)Q), dim3(64), 0, s, a);
}

// ------------------------------------------------------------------------------------------ 5. the fall-back's compaction and scatter
__global__ __launch_bounds__(256) void gal16_gather_kernel(const float* __restrict__ q, int dim, const int* __restrict__ fb_count,
                                                           const int* __restrict__ fb_idx, float* __restrict__ qpacked) {
    const int r = blockIdx.x, n = *fb_count;
    float* dst = qpacked + (size_t)r * dim;
    if (r < n) {
        const float* src = q + (size_t)fb_idx[r] * dim;
        for (int i = threadIdx.x; i < dim; i += 256) dst[i] = src[i];
    } else if (r < (n + 63) / 64 * 64) {                      // zero rows behind the count inside the last live 64-query tile
        for (int i = threadIdx.x; i < dim; i += 256) dst[i] = 0.f;
    }
}

void launch_gallery16_gather(const float* q, int Q, int dim, const int* fb_count, const int* fb_idx, float* qpacked, hipStream_t s) {
    if (Q > 0) hipLaunchKernelGGL(gal16_gather_kernel, dim3((unsigned)((Q + 63) / 64 * 64)), dim3(256), 0, s, q, dim, fb_count, fb_idx, qpacked);
}

__global__ __launch_bounds__(256) void gal16_scatter_kernel(const float* __restrict__ fs, const int* __restrict__ fi, int Q, int k,
                                                            const int* __restrict__ fb_count, const int* __restrict__ fb_idx,
                                                            float* __restrict__ out_s, int* __restrict__ out_i) {
    const int e = blockIdx.x * 256 + threadIdx.x, r = e / k;
    if (e >= Q * k || r >= *fb_count) return;
    const size_t o = (size_t)fb_idx[r] * k + (e - r * k);
    out_s[o] = fs[e]; out_i[o] = fi[e];
}

void launch_gallery16_scatter(const float* fb_score, const int* fb_idx_out, int Q, int k, const int* fb_count, const int* fb_idx, float* out_score,
                              int* out_idx, hipStream_t s) {
    if (Q > 0)
        hipLaunchKernelGGL(gal16_scatter_kernel, dim3((unsigned)((Q * k + 255) / 256)), dim3(256), 0, s, fb_score, fb_idx_out, Q, k, fb_count, fb_idx,
                           out_score, out_idx);
}

}  // namespace fh
