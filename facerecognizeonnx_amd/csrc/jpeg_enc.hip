// jpeg_enc.hip — the forward path of the JPEG encoder on the device (contract: include/facehip.h, "JPEG out").  Everything in front of the
// Huffman coder runs here for a whole batch in two launches; the host codes the coefficients (image_io.cpp, fh_jpeg_write):
//   jpeg_sample_kernel  four samples of a component row per lane: BGR -> Y / Cb / Cr (jccolor.c), edge replication by clamped index,
//                       h2v1 / h2v2 down-sampling (jcsample.c, no smoothing), -> the component's u8 plane over its REAL blocks
//   jpeg_fdct_kernel    one 8x8 block of the padded grid per lane: libjpeg's "islow" forward DCT (jfdctint.c) on samples - 128, the
//                       quantiser (jcdctmgr.c), jccoefct.c's dummy blocks, -> int16 coefficients in natural order
// Integer arithmetic end to end: the coefficients equal fh_jpeg_forward's (the host's, which stays the oracle: tests/test_gpu_jpeg_enc.py)
// for every descriptor fh_jpeg_enc_check accepts and every pixel value.
//
// Word sizes of the FDCT.  The host runs both passes in 32-bit `int`, as libjpeg does for 8-bit samples, and so does this file; no
// intermediate leaves 32 bits.  A centred sample is in [-128, 127].  Row pass: a butterfly sum of up to four differences is at most
// 4 * 255 < 2^10 in magnitude, its product with a 13-bit-scaled constant (all below 2^15) below 2^25, and an output adds at most four
// such products and the rounding constant: below 2^27.  Its results are the 1-D transform scaled by 4, at most 2^13 in magnitude (2^12
// on the DC path: 8 * 128 * 4).  Column pass: every output is 2^13 times a 2-D transform value whose magnitude is below 2^15 (the DC
// one is the sum of the 64 samples, 2^13), so the final sums are below 2^28 + 2^14; on the way a sum of four differences is at most
// 2^16, times 9633 below 2^30, and the other products (two differences times a constant below 2^15) below 2^29, with opposite signs
// where they are large — the host twin runs the same expressions on the pixel extremes under UndefinedBehaviorSanitizer without a
// report (tests/native/jpeg_enc_sanitize.cpp).  The quantiser divides a magnitude of at most 2^15 + 1020 by 8 q <= 2040: an exact
// unsigned integer division, no reciprocal.
#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>

#include "jpeg_enc.h"
#include "kernels.h"

namespace fh {

namespace {

// One image of the batch as the kernels see it; the table is [n] of these, then the two group tables below.
struct EncImg {
    fh_jpeg_desc d;
    long long coef_base;             // of the image in d_coef, int16 elements
    long long plane_off[3];          // of a component's (bh*8) x (bw*8) plane in the workspace, bytes (a multiple of 64)
    const uint8_t* bgr;              // nullptr: the slot is skipped (no group of either kernel points at it)
    int32_t step, pad_;
    int32_t hx[3], vx[3];            // hmax / h, vmax / v of a component: 1 or 2 (vx == 2 only with hx == 2)
    int32_t bw[3], bh[3];            // the component's REAL blocks: ceil(dw / 8) x ceil(dh / 8); the grid wblocks x hblocks is padded to whole MCUs
};
static_assert(sizeof(EncImg) % 8 == 0, "the group tables behind the rows are int64");

constexpr int kSampleLanes = 256;    // lanes per workgroup of jpeg_sample_kernel, four samples of a row each
constexpr int kFdctLanes = 64;       // 8x8 blocks per workgroup of jpeg_fdct_kernel

// the entry whose run of workgroups holds g: start[e] <= g < start[e + 1] (empty entries have start[e] == start[e + 1] and are never hit).
// Uniform over the workgroup: g is blockIdx.x.  (A private copy: jpeg_dev.hip keeps its own, so that its kernels stay as they are.)
__device__ __forceinline__ int find_entry(const long long* __restrict__ start, int entries, long long g) {
    int lo = 0, hi = entries;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------
// One lane per FOUR neighbouring samples of a component row, 256 lanes of one image per workgroup.  The group table maps the workgroup to
// its entry = image * 2 + kind: kind 0 = component 0 (Y, always at full resolution), kind 1 = components 1 and 2 together (Cb and Cr share
// their geometry and their pixels, so one lane forms both from the same loads; a grey picture has no kind 1 groups).  A sample of a
// down-sampled component averages hx * vx pixels with libjpeg's alternating bias.  Every pixel index is clamped to the picture — column
// min(x, W - 1), row min(y, H - 1) — and the sample row to min(sy, dh - 1) FIRST: rows below the picture repeat the last DOWN-SAMPLED
// row, not the last picture row (jcprepct.c pads full-resolution rows to a multiple of vmax only).  So nothing outside
// [row * step, row * step + cols * 3) of a real row is read, whatever the frame's address and pitch: byte loads.  The four samples
// leave as one dword store (the plane's pitch is a multiple of 8, its base of 64).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSampleLanes) void jpeg_sample_kernel(const EncImg* __restrict__ imgs, const long long* __restrict__ start, int entries,
                                                                   uint8_t* __restrict__ planes) {
    const long long g = blockIdx.x;
    const int e = find_entry(start, entries, g);
    const int ii = e >> 1, kind = e & 1;
    const EncImg& im = imgs[ii];
    const fh_jpeg_comp& c = im.d.comp[kind];
    const int bw = im.bw[kind], bh = im.bh[kind];
    const unsigned qpr = 2u * (unsigned)bw;                                 // quads per sample row; rows * qpr <= 2^16 * 2^14
    const unsigned q = (unsigned)(g - start[e]) * kSampleLanes + threadIdx.x;
    if (q >= (unsigned)bh * 8u * qpr) return;
    const int sy = (int)(q / qpr), sx0 = (int)(q - (unsigned)sy * qpr) * 4;
    const int W = im.d.width, H = im.d.height, hx = im.hx[kind], vx = im.vx[kind];
    const int y = min(sy, c.dh - 1);
    const uint8_t* const row0 = im.bgr + (size_t)min(y * vx, H - 1) * im.step;
    const uint8_t* const row1 = im.bgr + (size_t)min(y * vx + vx - 1, H - 1) * im.step;
    const int shift = hx == 1 ? 0 : vx == 1 ? 1 : 2;
    uint32_t w0 = 0, w1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sx = sx0 + k;
        const int bias = hx == 1 ? 0 : vx == 1 ? (sx & 1) : 1 + (sx & 1);
        int a0 = bias, a1 = bias;
        for (int dy = 0; dy < vx; ++dy) {
            const uint8_t* const row = dy ? row1 : row0;
            for (int dx = 0; dx < hx; ++dx) {
                const uint8_t* const p = row + (size_t)min(sx * hx + dx, W - 1) * 3;
                const int b = p[0], gr = p[1], r = p[2];
                if (kind == 0) {
                    a0 += (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16;
                } else {
                    a0 += (-11059 * r - 21709 * gr + 32768 * b + (128 << 16) + 32767) >> 16;
                    a1 += (32768 * r - 27439 * gr - 5329 * b + (128 << 16) + 32767) >> 16;
                }
            }
        }
        w0 |= (uint32_t)(a0 >> shift) << (8 * k);
        w1 |= (uint32_t)(a1 >> shift) << (8 * k);
    }
    const size_t at = (size_t)sy * (size_t)bw * 8 + (size_t)sx0;
    *reinterpret_cast<uint32_t*>(planes + im.plane_off[kind] + at) = w0;
    if (kind) *reinterpret_cast<uint32_t*>(planes + im.plane_off[2] + at) = w1;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c's 1-D transform on d[0], d[S], ... d[7 S], in place.  PASS 0: rows (outputs scaled up by PASS1_BITS = 2); PASS 1: columns.
template <int PASS, int S>
__device__ __forceinline__ void fdct_1d(int* d) {
    constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
                  F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    constexpr int N = PASS ? 15 : 11;                                      // CONST_BITS + PASS1_BITS / CONST_BITS - PASS1_BITS
    int tmp0 = d[0] + d[7 * S], tmp7 = d[0] - d[7 * S], tmp1 = d[S] + d[6 * S], tmp6 = d[S] - d[6 * S];
    int tmp2 = d[2 * S] + d[5 * S], tmp5 = d[2 * S] - d[5 * S], tmp3 = d[3 * S] + d[4 * S], tmp4 = d[3 * S] - d[4 * S];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (PASS == 0) { d[0] = (tmp10 + tmp11) * 4; d[4 * S] = (tmp10 - tmp11) * 4; }
    else { d[0] = descale(tmp10 + tmp11, 2); d[4 * S] = descale(tmp10 - tmp11, 2); }
    int z1 = (tmp12 + tmp13) * F0_541;
    d[2 * S] = descale(z1 + tmp13 * F0_765, N);
    d[6 * S] = descale(z1 + tmp12 * (-F1_847), N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F1_175;
    tmp4 *= F0_298; tmp5 *= F2_053; tmp6 *= F3_072; tmp7 *= F1_501;
    z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
    z3 += z5; z4 += z5;
    d[7 * S] = descale(tmp4 + z1 + z3, N);
    d[5 * S] = descale(tmp5 + z2 + z4, N);
    d[3 * S] = descale(tmp6 + z2 + z3, N);
    d[S] = descale(tmp7 + z1 + z4, N);
}

// jcdctmgr.c's quantiser on a coefficient scaled by 8: round half away from zero; |c| <= 2^15, q in 1..255
__device__ __forceinline__ int quantise(int c, unsigned q) {
    const unsigned qv = q * 8u, t = (unsigned)abs(c) + (qv >> 1);
    const int m = (int)(t / qv);
    return c < 0 ? -m : m;
}

// ------------------------------------------------------------------------------------------
// One lane per 8x8 block of the PADDED grid, 64 blocks of ONE component of one image per workgroup (the group table maps the workgroup to
// its entry = image * 3 + component, uniformly).  A real block reads its 64 samples as eight 8-byte loads (the lanes of a wave hold
// neighbouring blocks of a block row, so each load instruction covers contiguous bytes), transforms them in registers — everything is
// unrolled — and quantises with the component's table (uniform addresses: scalar loads).  A dummy block (jccoefct.c) has AC zero and the
// quantised DC of a real block: right of the real ones the last real block of its row, below them the block the last position of its MCU
// column holds in the last real row (itself the row's last real block when that position is a dummy).  The unquantised DC is exactly the
// sum of the 64 centred samples (row pass: sum << 2, column pass: descale by 2), so a dummy lane sums its source block instead of
// transforming it.  The 128 bytes of a block leave as eight 16-byte stores when the block is 16-byte aligned (fh_jpeg_encode_batch's
// arena and fh_jpeg_enc_desc's coef_off always are), as int16 stores otherwise.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFdctLanes) void jpeg_fdct_kernel(const EncImg* __restrict__ imgs, const long long* __restrict__ start, int entries,
                                                               const uint8_t* __restrict__ planes, int16_t* __restrict__ coef) {
    const long long g = blockIdx.x;
    const int e = find_entry(start, entries, g);
    const int ii = e / 3, ci = e - ii * 3;
    const EncImg& im = imgs[ii];
    const fh_jpeg_comp& c = im.d.comp[ci];
    const long long b = (g - start[e]) * kFdctLanes + threadIdx.x, nb = (long long)c.wblocks * c.hblocks;
    if (b >= nb) return;
    const int by = (int)(b / c.wblocks), bx = (int)(b - (long long)by * c.wblocks);
    const int bw = im.bw[ci], bh = im.bh[ci];
    const bool real = by < bh && bx < bw;
    const int sy = min(by, bh - 1), sx = min(by < bh ? bx : bx / c.h * c.h + c.h - 1, bw - 1);
    const size_t stride = (size_t)bw * 8;
    const uint8_t* in = planes + im.plane_off[ci] + (size_t)sy * 8 * stride + (size_t)sx * 8;   // 8-byte aligned: plane_off % 64 == 0, stride % 8 == 0

    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint2 w = *reinterpret_cast<const uint2*>(in + (size_t)r * stride);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[r * 8 + k] = (int)((w.x >> (8 * k)) & 255u) - 128;
            d[r * 8 + 4 + k] = (int)((w.y >> (8 * k)) & 255u) - 128;
        }
    }
    int q[64];
    if (real) {
#pragma unroll
        for (int r = 0; r < 8; ++r) fdct_1d<0, 1>(d + r * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) fdct_1d<1, 8>(d + k);
#pragma unroll
        for (int k = 0; k < 64; ++k) q[k] = quantise(d[k], c.quant[k]);
    } else {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 64; ++k) { sum += d[k]; q[k] = 0; }
        q[0] = quantise(sum, c.quant[0]);
    }

    int16_t* out = coef + im.coef_base + c.coef_off + b * 64;
    if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int4 w;
            w.x = (q[k * 8] & 0xFFFF) | (q[k * 8 + 1] << 16);
            w.y = (q[k * 8 + 2] & 0xFFFF) | (q[k * 8 + 3] << 16);
            w.z = (q[k * 8 + 4] & 0xFFFF) | (q[k * 8 + 5] << 16);
            w.w = (q[k * 8 + 6] & 0xFFFF) | (q[k * 8 + 7] << 16);
            reinterpret_cast<int4*>(out)[k] = w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 64; ++k) out[k] = (int16_t)q[k];
    }
}

}  // namespace

void JpegEnc::forward(const fh_jpeg_desc* descs, int n, const FrameIn* frames, int16_t* d_coef, const long long* coef_base, hipStream_t s) {
    const size_t bytes = (size_t)n * sizeof(EncImg) + ((size_t)2 * n + 1 + (size_t)3 * n + 1) * sizeof(long long);
    uint8_t* const h = static_cast<uint8_t*>(table_.stage(bytes));
    EncImg* const rows = reinterpret_cast<EncImg*>(h);
    long long* const smp_start = reinterpret_cast<long long*>(h + (size_t)n * sizeof(EncImg));
    long long* const blk_start = smp_start + 2 * (size_t)n + 1;
    long long sg = 0, bg = 0;
    size_t plane_bytes = 0;
    for (int i = 0; i < n; ++i) {
        EncImg& r = rows[i];
        memset(&r, 0, sizeof(r));
        const bool live = frames[i].bgr != nullptr;
        if (live) {                                                        // (a skipped slot's descriptor was not checked: it is not copied either)
            r.d = descs[i];
            r.coef_base = coef_base[i];
            r.bgr = frames[i].bgr;
            r.step = frames[i].step;
        }
        for (int ci = 0; ci < 3; ++ci) {
            if (ci < 2) smp_start[2 * (size_t)i + ci] = sg;
            blk_start[3 * (size_t)i + ci] = bg;
            if (!live || ci >= r.d.ncomp) continue;
            const fh_jpeg_comp& c = r.d.comp[ci];
            r.hx[ci] = r.d.hmax / c.h; r.vx[ci] = r.d.vmax / c.v;
            r.bw[ci] = (c.dw + 7) / 8; r.bh[ci] = (c.dh + 7) / 8;
            r.plane_off[ci] = (long long)plane_bytes;
            plane_bytes += (size_t)r.bw[ci] * r.bh[ci] * 64;
            if (ci < 2) sg += ((long long)r.bh[ci] * 8 * (2 * r.bw[ci]) + kSampleLanes - 1) / kSampleLanes;
            bg += ((long long)c.wblocks * c.hblocks + kFdctLanes - 1) / kFdctLanes;
        }
    }
    smp_start[2 * (size_t)n] = sg;
    blk_start[3 * (size_t)n] = bg;
    if (bg == 0) return;                                                   // every slot skipped
    if (sg > 0x7FFFFFFFLL || bg > 0x7FFFFFFFLL) throw std::runtime_error("fh_jpeg_forward_batch_dev: the batch is too large for one launch");
    planes_.ensure(plane_bytes);
    const uint8_t* const dev = static_cast<const uint8_t*>(table_.send(bytes, s));
    const EncImg* const d_rows = reinterpret_cast<const EncImg*>(dev);
    const long long* const d_smp = reinterpret_cast<const long long*>(dev + (size_t)n * sizeof(EncImg));
    const long long* const d_blk = d_smp + 2 * (size_t)n + 1;
    hipLaunchKernelGGL(jpeg_sample_kernel, dim3((unsigned)sg), dim3(kSampleLanes), 0, s, d_rows, d_smp, 2 * n, planes_.as<uint8_t>());
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)bg), dim3(kFdctLanes), 0, s, d_rows, d_blk, 3 * n, planes_.as<const uint8_t>(), d_coef);
    FH_HIP(hipGetLastError());
}

}  // namespace fh
