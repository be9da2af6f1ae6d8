// jpeg_dev.hip — JPEG pixel reconstruction on the device (contract: include/facehip.h, "JPEG in two halves").  The host decodes the
// entropy-coded data (image_io.cpp, fh_jpeg_entropy); everything behind it runs here for a whole batch in two launches:
//   jpeg_idct_kernel   de-quantisation + libjpeg's "islow" inverse DCT, one 8x8 block per lane, -> the component's u8 plane
//   jpeg_pixel_kernel  four pixels per lane: chroma up-sampling (h2v1 / h2v2 / h1v2 "fancy", box replication), YCbCr -> RGB, EXIF orientation, -> BGR
// Integer arithmetic end to end: the bytes equal fh_jpeg_reconstruct's (the host's, which stays the oracle: tests/test_gpu_jpeg.py) for
// every descriptor fh_jpeg_desc_check accepts and every int16 coefficient / uint16 quantiser.
//
// Word sizes of the IDCT.  The host runs both passes in 64-bit `long`.  A de-quantised coefficient is below 2^31 in magnitude
// (32768 * 65535); the column pass multiplies sums of up to four of them by 13-bit-scaled constants below 2^15, and adds about ten such
// terms: below 2^53, so 64 bits hold it exactly and 32 do not — the column pass runs in int64 here too.  Its result w = (q + 2^10) >> 11
// can need 37 bits.  The row pass forms an integer polynomial P(w) (products with constants, sums), and the sample is
// range_limit((int)((P + 2^17) >> 18)), which reads bits 18..27 of P + 2^17 and nothing else: (int) of a long keeps the low 32 bits and
// range_limit masks with 1023.  Those bits are a function of P mod 2^28, P mod 2^32 is a function of the w mod 2^32 (ring
// homomorphism Z -> Z / 2^32), so the row pass keeps only the low 32 bits of every w and runs in wrapping uint32 arithmetic.
#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>

#include "jpeg_dev.h"
#include "kernels.h"

namespace fh {

namespace {

// One image of the batch as the kernels see it; the table is [n] of these, then the two group tables below.
struct JpegImg {
    fh_jpeg_desc d;
    long long coef_base;             // of the image in d_coef, int16 elements
    long long plane_off[3];          // of a component's (hblocks*8) x (wblocks*8) plane in the workspace, bytes (a multiple of 64)
    uint8_t* bgr;                    // nullptr: the slot is skipped (no group of either kernel points at it)
    int32_t step, pad_;
    int32_t hx[3], vx[3];            // hmax / h, vmax / v of a component: 1, 2, 3 or 4
};
static_assert(sizeof(JpegImg) % 8 == 0, "the group tables behind the rows are int64");

constexpr int kIdctLanes = 64;       // 8x8 blocks per workgroup of jpeg_idct_kernel
constexpr int kPixLanes = 256;       // lanes per workgroup of jpeg_pixel_kernel, four pixels of a row each

// the entry whose run of workgroups holds g: start[e] <= g < start[e + 1] (empty entries have start[e] == start[e + 1] and are never hit).
// Uniform over the workgroup: g is blockIdx.x.
__device__ __forceinline__ int find_entry(const long long* __restrict__ start, int entries, long long g) {
    int lo = 0, hi = entries;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// jidctint.c's 1-D kernel on eight inputs: the eight sums BEFORE the descale, in T (int64: exact; uint32: modulo 2^32).
template <class T>
__device__ __forceinline__ void idct_1d(const T* v, T* o) {
    constexpr int CB = 13;
    constexpr long long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                        F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    T z2 = v[2], z3 = v[6];
    T z1 = (z2 + z3) * (T)F0_541;
    T tmp2 = z1 + z3 * (T)(-F1_847), tmp3 = z1 + z2 * (T)F0_765;
    z2 = v[0]; z3 = v[4];
    T tmp0 = (z2 + z3) * (T)(1LL << CB), tmp1 = (z2 - z3) * (T)(1LL << CB);
    const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    T z4 = tmp1 + tmp3;
    const T z5 = (z3 + z4) * (T)F1_175;
    tmp0 *= (T)F0_298; tmp1 *= (T)F2_053; tmp2 *= (T)F3_072; tmp3 *= (T)F1_501;
    z1 *= (T)(-F0_899); z2 *= (T)(-F2_562); z3 *= (T)(-F1_961); z4 *= (T)(-F0_390);
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

__device__ __forceinline__ uint32_t range_limit(uint32_t x) {             // libjpeg's centred range-limit table, index & 1023
    const uint32_t i = x & 1023u;
    return i < 128 ? i + 128 : i < 512 ? 255u : i < 896 ? 0u : i - 896;
}

// ------------------------------------------------------------------------------------------
// One lane per 8x8 block, 64 blocks of ONE component of one image per workgroup (the group table maps the workgroup to its entry =
// image * 3 + component, uniformly).  A block's 64 coefficients are the 128 contiguous bytes of one cache line: eight 16-byte loads when
// the block is 16-byte aligned (fh_jpeg_decode_batch's arena and the parser's coef_off always are), int16 loads otherwise.  The lanes of
// a wave hold neighbouring blocks of a block row, so their 8-byte stores of one sample row are contiguous.  The quantiser addresses are
// uniform (scalar loads).  Everything is unrolled: the 64 column-pass results stay in registers as uint32 (see the file header).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIdctLanes) void jpeg_idct_kernel(const JpegImg* __restrict__ imgs, const long long* __restrict__ start, int entries,
                                                               const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
    const long long g = blockIdx.x;
    const int e = find_entry(start, entries, g);
    const int ii = e / 3, ci = e - ii * 3;
    const JpegImg& im = imgs[ii];
    const fh_jpeg_comp& c = im.d.comp[ci];
    const long long b = (g - start[e]) * kIdctLanes + threadIdx.x, nb = (long long)c.wblocks * c.hblocks;
    if (b >= nb) return;
    const int by = (int)(b / c.wblocks), bx = (int)(b - (long long)by * c.wblocks);
    const int16_t* in = coef + im.coef_base + c.coef_off + b * 64;

    int16_t cf[64];
    if ((reinterpret_cast<uintptr_t>(in) & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int4 q = reinterpret_cast<const int4*>(in)[k];
            const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { cf[k * 8 + 2 * j] = (int16_t)(w[j] & 0xFFFF); cf[k * 8 + 2 * j + 1] = (int16_t)(w[j] >> 16); }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 64; ++k) cf[k] = in[k];
    }

    uint32_t ws[64];
#pragma unroll
    for (int col = 0; col < 8; ++col) {                                    // pass 1: columns, int64, descale by CONST_BITS - PASS1_BITS = 11
        long long v[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = (long long)cf[r * 8 + col] * (long long)c.quant[r * 8 + col];
        idct_1d<long long>(v, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r * 8 + col] = (uint32_t)((o[r] + (1LL << 10)) >> 11);
    }
    const int stride = c.wblocks * 8;
    uint8_t* out = planes + im.plane_off[ci] + (size_t)by * 8 * stride + (size_t)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                                          // pass 2: rows, modulo 2^32, descale by 13 + 2 + 3 = 18
        uint32_t o[8];
        idct_1d<uint32_t>(ws + r * 8, o);
        uint32_t px[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) px[k] = range_limit((o[k] + (1u << 17)) >> 18);
        uint2 w;
        w.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        w.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        *reinterpret_cast<uint2*>(out + (size_t)r * stride) = w;          // 8-byte aligned: plane_off % 64 == 0, stride % 8 == 0
    }
}

// a / d for a >= 0 and the ratios two sampling factors can have (1, 2, 3, 4) without an integer division
__device__ __forceinline__ int div_small(int a, int d) { return d == 1 ? a : d == 2 ? a >> 1 : d == 4 ? a >> 2 : a / 3; }

// jdsample.c for ONE output sample (x, y) of the coded picture: the branch conditions of the host's row loops (image_io.cpp upsample),
// restated per pixel.  src = the component's plane, pitch sw; real size dw x dh; edge rows replicate.
__device__ __forceinline__ int upsampled(const uint8_t* __restrict__ src, int sw, int dw, int dh, int hx, int vx, int x, int y) {
    auto row = [&](int r) { return src + (size_t)min(max(r, 0), dh - 1) * sw; };
    if (hx == 1 && vx == 1) return row(y)[x];
    if (hx == 2 && vx == 1 && dw > 2) {                                    // h2v1_fancy_upsample
        const uint8_t* in = row(y);
        const int i = x >> 1;
        if (x == 0) return in[0];
        if (x == 2 * dw - 1) return in[dw - 1];
        return (x & 1) ? (in[i] * 3 + in[i + 1] + 2) >> 2 : (in[i] * 3 + in[i - 1] + 1) >> 2;
    }
    if (hx == 2 && vx == 2 && dw > 2) {                                    // h2v2_fancy_upsample
        const int sy = y >> 1;
        const uint8_t* in0 = row(sy);
        const uint8_t* in1 = row((y & 1) ? sy + 1 : sy - 1);
        const int i = x >> 1;
        const int thiscol = in0[i] * 3 + in1[i];
        if (x == 0) return (thiscol * 4 + 8) >> 4;
        if (x == 2 * dw - 1) return (thiscol * 4 + 7) >> 4;
        if (x & 1) return (thiscol * 3 + (in0[i + 1] * 3 + in1[i + 1]) + 7) >> 4;
        return (thiscol * 3 + (in0[i - 1] * 3 + in1[i - 1]) + 8) >> 4;
    }
    if (hx == 1 && vx == 2) {                                              // h1v2_fancy_upsample (libjpeg-turbo)
        const int sy = y >> 1;
        const uint8_t* in0 = row(sy);
        const uint8_t* in1 = row((y & 1) ? sy + 1 : sy - 1);
        return (in0[x] * 3 + in1[x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    return row(div_small(y, vx))[div_small(x, hx)];                        // int_upsample / h2v1 / h2v2 box replication
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ------------------------------------------------------------------------------------------
// One lane per FOUR neighbouring OUTPUT pixels of a row (after the orientation), 256 lanes of one image per workgroup, so that the stores
// of a wave are the contiguous bytes of an output row; the source position of each pixel comes from the orientation's inverse
// (image_io.cpp apply_orientation).  A chroma sample gathers at most four plane bytes; they are shared by the neighbouring lanes and
// come from the cache.  The 12 bytes of a lane leave as three dword stores when they are 4-byte aligned and all four pixels exist, as
// byte stores otherwise: a frame may start at any address and have any pitch, and nothing outside [row * step, row * step + cols * 3)
// is written.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPixLanes) void jpeg_pixel_kernel(const JpegImg* __restrict__ imgs, const long long* __restrict__ start, int entries,
                                                               const uint8_t* __restrict__ planes) {
    const long long g = blockIdx.x;
    const int e = find_entry(start, entries, g);
    const JpegImg& im = imgs[e];
    const fh_jpeg_desc& d = im.d;
    const unsigned qpr = ((unsigned)d.cols + 3u) >> 2;                      // quads per output row; rows * qpr <= 2^28
    const unsigned q = (unsigned)(g - start[e]) * kPixLanes + threadIdx.x;
    if (q >= (unsigned)d.rows * qpr) return;
    const int y = (int)(q / qpr), x0 = (int)(q - (unsigned)y * qpr) * 4;
    const int R = d.height, C = d.width, o = d.orientation;
    // source position of output (y, x): sy = ay + x * dy, sx = ax + x * dx (one of them moves with x)
    int ay, ax, dy, dx;
    switch (o) {
        case 2: ay = y; ax = C - 1; dy = 0; dx = -1; break;                // mirror horizontal
        case 3: ay = R - 1 - y; ax = C - 1; dy = 0; dx = -1; break;        // rotate 180
        case 4: ay = R - 1 - y; ax = 0; dy = 0; dx = 1; break;             // mirror vertical
        case 5: ay = 0; ax = y; dy = 1; dx = 0; break;                     // transpose
        case 6: ay = R - 1; ax = y; dy = -1; dx = 0; break;                // rotate 90 clockwise
        case 7: ay = R - 1; ax = C - 1 - y; dy = -1; dx = 0; break;        // transverse
        case 8: ay = 0; ax = C - 1 - y; dy = 1; dx = 0; break;             // rotate 270 clockwise
        default: ay = y; ax = 0; dy = 0; dx = 1; break;
    }
    const int nc = d.ncomp, color = d.color;
    uint32_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(x0 + k, d.cols - 1);                              // (a quad's pixels behind the row's end repeat the last one; not stored)
        const int sy = ay + x * dy, sx = ax + x * dx;
        int s[3];
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            if (ci >= nc) { s[ci] = 0; continue; }
            const fh_jpeg_comp& c = d.comp[ci];
            s[ci] = upsampled(planes + im.plane_off[ci], c.wblocks * 8, c.dw, c.dh, im.hx[ci], im.vx[ci], sx, sy);
        }
        int b, gr, r;
        if (color == 0) {
            b = gr = r = s[0];
        } else if (color == 2) {
            r = s[0]; gr = s[1]; b = s[2];
        } else {                                                           // jdcolor.c ycc_rgb_convert, SCALEBITS = 16: the tables' entries
            constexpr int kCrR = (int)(1.40200 * 65536.0 + 0.5), kCbB = (int)(1.77200 * 65536.0 + 0.5), kCrG = (int)(0.71414 * 65536.0 + 0.5),
                          kCbG = (int)(0.34414 * 65536.0 + 0.5);
            const int cb = s[1] - 128, cr = s[2] - 128;
            r = clamp255(s[0] + ((kCrR * cr + 32768) >> 16));
            gr = clamp255(s[0] + ((-kCbG * cb + 32768 - kCrG * cr) >> 16));
            b = clamp255(s[0] + ((kCbB * cb + 32768) >> 16));
        }
        px[3 * k] = (uint32_t)b; px[3 * k + 1] = (uint32_t)gr; px[3 * k + 2] = (uint32_t)r;
    }
    uint8_t* out = im.bgr + (size_t)y * im.step + (size_t)x0 * 3;
    if (x0 + 4 <= d.cols && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(out);
        w[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        w[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        w[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
    } else {
        const int nbytes = 3 * min(4, d.cols - x0);
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < nbytes) out[k] = (uint8_t)px[k];
    }
}

}  // namespace

void JpegDev::reconstruct(const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base, const FrameIn* frames,
                          hipStream_t s) {
    const size_t bytes = (size_t)n * sizeof(JpegImg) + ((size_t)3 * n + 1 + (size_t)n + 1) * sizeof(long long);
    uint8_t* const h = static_cast<uint8_t*>(table_.stage(bytes));
    JpegImg* const rows = reinterpret_cast<JpegImg*>(h);
    long long* const idct_start = reinterpret_cast<long long*>(h + (size_t)n * sizeof(JpegImg));
    long long* const pix_start = idct_start + 3 * (size_t)n + 1;
    long long ig = 0, pg = 0;
    size_t plane_bytes = 0;
    for (int i = 0; i < n; ++i) {
        JpegImg& r = rows[i];
        memset(&r, 0, sizeof(r));
        r.d = descs[i];
        r.coef_base = coef_base[i];
        r.bgr = const_cast<uint8_t*>(frames[i].bgr);
        r.step = frames[i].step;
        const bool live = frames[i].bgr != nullptr;
        for (int ci = 0; ci < 3; ++ci) {
            idct_start[3 * (size_t)i + ci] = ig;
            if (!live || ci >= r.d.ncomp) continue;
            const long long nb = (long long)r.d.comp[ci].wblocks * r.d.comp[ci].hblocks;
            r.hx[ci] = r.d.hmax / r.d.comp[ci].h; r.vx[ci] = r.d.vmax / r.d.comp[ci].v;
            r.plane_off[ci] = (long long)plane_bytes;
            plane_bytes += (size_t)nb * 64;
            ig += (nb + kIdctLanes - 1) / kIdctLanes;
        }
        pix_start[i] = pg;
        if (live) pg += ((long long)r.d.rows * ((r.d.cols + 3) / 4) + kPixLanes - 1) / kPixLanes;
    }
    idct_start[3 * (size_t)n] = ig;
    pix_start[n] = pg;
    if (ig == 0) return;                                                   // every slot skipped
    if (ig > 0x7FFFFFFFLL || pg > 0x7FFFFFFFLL) throw std::runtime_error("fh_jpeg_reconstruct_batch_dev: the batch is too large for one launch");
    planes_.ensure(plane_bytes);
    const uint8_t* const dev = static_cast<const uint8_t*>(table_.send(bytes, s));
    const JpegImg* const d_rows = reinterpret_cast<const JpegImg*>(dev);
    const long long* const d_idct = reinterpret_cast<const long long*>(dev + (size_t)n * sizeof(JpegImg));
    const long long* const d_pix = d_idct + 3 * (size_t)n + 1;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)ig), dim3(kIdctLanes), 0, s, d_rows, d_idct, 3 * n, d_coef, planes_.as<uint8_t>());
    hipLaunchKernelGGL(jpeg_pixel_kernel, dim3((unsigned)pg), dim3(kPixLanes), 0, s, d_rows, d_pix, n, planes_.as<const uint8_t>());
    FH_HIP(hipGetLastError());
}

}  // namespace fh
