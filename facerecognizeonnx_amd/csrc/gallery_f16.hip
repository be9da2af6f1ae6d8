// gallery_f16.hip — the opt-in F16_RERANK scan of the 1:N gallery (fh_gallery_set_scan).  Same answer as gallery.hip, bit for bit:
//   1. gal16_convert_kernel: an fp16 copy of the rows (round to nearest even) beside the fp32 rows, and in the same pass the bounds the
//      certificate needs: max ||g||, max ||g^||, max ||g - g^|| (g^ = the fp16 row; the difference is exact in f32), rounded up.
//   2. gal16_scan_kernel: the streaming scan of gallery_scan.h (its header states what the fp16 instantiation changes) on
//      v_mfma_f32_32x32x16_f16 with f32 accumulation, keeping the top GAL16_KC (32) rows per query by fp16 mapped score, total order
//      (score desc, index asc); seed pass, per-part lists + topk_merge_kernel as the fp32 scan.  Needs dim % 128 == 0 (other dims take
//      the fp32 scan).  One workgroup per CU, and at most 8192 / 32 = 256 parts per query tile, so that the merge of 32-deep lists stays
//      on topk_merge_kernel's cached path.
//   3. gal16_rescore_kernel: one wave per query re-scores its 32 candidates from the FP32 rows with v_mfma_f32_32x32x2_f32 in exactly
//      the operand placement and k order of gallery_topk_kernel's multiply (lane (row fr, half fh2) holds k = kc*64 + (2s + fh2)*4 + e;
//      loop kc, s = 0..7, e = 0..3; accumulator from 0; score = (acc + 1) / 2).  One output element depends only on its row, its column
//      and that sequence, so the scores are bitwise those of the fp32 scan; the top-k of the candidates by (score desc, index asc) follows.
//   4. the certificate: with s16_min = the fp16 score of the 32nd candidate and D_q a rigorous bound on |s32 - s16| over
//      all rows (doubled for safety), the query is certified iff the re-scored k-th score > s16_min + D_q: every other row then scores
//      strictly below the k-th in fp32 and can neither enter nor tie.  A list that is not full must hold all G rows.
//   5. uncertified queries are compacted on the device (count + indices) and answered by the fp32 scan + merge with a device query count
//      (gallery.hip: workgroups beyond the count exit at once), then scattered into the output.  No host round trip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "gallery_scan.h"
#include "kernels.h"

namespace fh {

constexpr int G16_KC = GAL16_KC;

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
__global__ __launch_bounds__(256, 1) void gal16_scan_kernel(const GalArgs p) { gallery_scan_body<_Float16, G16_KC, true, false>(p); }

// ONE workgroup per CU, at most 256 parts per query tile (merge of 32-deep lists: 8192 entries); no device query count
static const GalScan g16_scan{"gallery f16 scan", gal16_scan_kernel, /*chunk*/ 128, /*depth*/ G16_KC, /*wg_per_cu*/ 1, /*max_parts*/ 8192 / G16_KC, /*has_qcount*/ false};
int gallery16_parts(long G, int Q, int* tiles_per_part) { return gallery_parts_for(G, Q, g16_scan.wg_per_cu, g16_scan.max_parts, tiles_per_part); }

void launch_gallery16_candidates(const uint16_t* rows16, long G, int dim, const float* q, uint16_t* q16, int Q, long idx_base, float* part_score,
                                 int* part_idx, float* seed_score, int* seed_idx, float* cand_score, int* cand_idx, hipStream_t s) {
    if (G <= 0 || Q <= 0) return;
    GalArgs a{};
    a.gal = rows16; a.q = q16; a.idx_base = idx_base; a.dim = dim; a.Q = Q; a.k = G16_KC;
    a.ps = part_score; a.pi = part_idx;
    gallery_check_args(g16_scan, a, G);                      // (ahead of the first launch)
    const long qtotal = (long)((Q + GAL_BN - 1) / GAL_BN) * GAL_BN * dim;
    hipLaunchKernelGGL(gal16_pack_q_kernel, dim3((unsigned)((qtotal + 255) / 256)), dim3(256), 0, s, q, reinterpret_cast<_Float16*>(q16), Q, qtotal,
                       dim);
    const int parts = launch_gallery_two_pass(g16_scan, a, G, true, seed_score, seed_idx, nullptr, s);
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
    // (gal_rescore32, gallery_scan.h)
    const GalSrc<float> a = gal_row_or_zeros(live, p.gal, (size_t)(gi - p.idx_base), K, p.zeros, fh2 * 4, 64);
    const v16f acc = gal_rescore32(a.ptr, a.step, qrow + fh2 * 4, chunks);
    if (fr == 0) {                                            // column 0: rows gal_acc_row(e) + 4 * fh2
#pragma unroll
        for (int e = 0; e < 16; ++e) cs[gal_acc_row(e) + 4 * fh2] = gal_score(acc[e]);
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
        if (lane < G16_KC && live && gal_better(cs[c], oi, my_s, gi)) ++rank;
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
