// ops_misc.hip — the bandwidth-bound graph operators of the SCRFD / IResNet plans that are not
// MFMA work: depthwise 3x3 convolution (+bias +ReLU), stand-alone BatchNormalization (affine),
// stand-alone activations, Add and nearest 2x up-sampling.  All tensors are channels-last fp32,
// every lane moves 16 bytes (4 channels) per access so a wave covers whole 128-byte lines.
// These are the ONNX nodes ORT runs inside session_->Run (reference src/face_detector.cpp:179-183).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "plan.h"

namespace fh {

typedef float v4f __attribute__((ext_vector_type(4)));

static inline int grid_for(long n, int block = 256, int cap = 256 * 16) {
    long b = (n + block - 1) / block;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

__device__ __forceinline__ float act1(float v, int act, float slope) {
    if (act == (int)Act::RELU) return v > 0.f ? v : 0.f;
    if (act == (int)Act::PRELU) return v >= 0.f ? v : v * slope;
    if (act == (int)Act::SIGMOID) return 1.0f / (1.0f + expf(-v));
    return v;
}

// Depthwise 3x3 (+bias +ReLU).  One thread = 4 channels x a VERTICAL strip of STRIP output pixels:
// the (STRIP*stride + 2) x 3 input float4s are loaded once and reused down the strip (4.5 instead
// of 9 loads per output at stride 1), weights stay in registers.  Lanes run over the channel groups
// and then over x, so every load / store instruction of a wave touches one contiguous run of pixels
// (full 128-byte lines); a horizontal strip would scatter each instruction over 16 half-used lines.
template <int STRIDE, int STRIP>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int B, int H, int W, int C, int Ho, int Wo, int act,
                                                        const float* __restrict__ slope) {
    constexpr int ROWS = (STRIP - 1) * STRIDE + 3;
    const int C4 = C >> 2;
    const int strips = (Ho + STRIP - 1) / STRIP;
    const long total = (long)B * strips * Wo * C4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int sy = (int)(r % strips);
        const int n = (int)(r / strips);
        const int oy0 = sy * STRIP;
        v4f wk[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wk[t] = *reinterpret_cast<const v4f*>(w + t * C + c4 * 4);
        const v4f b4 = *reinterpret_cast<const v4f*>(bias + c4 * 4);
        const v4f sl4 = slope ? *reinterpret_cast<const v4f*>(slope + c4 * 4) : v4f{0.f, 0.f, 0.f, 0.f};
        v4f acc[STRIP];
#pragma unroll
        for (int o = 0; o < STRIP; ++o) acc[o] = b4;
        const int iy0 = oy0 * STRIDE - 1, ix0 = ox * STRIDE - 1;
        // UNCONDITIONAL loads from clamped coordinates, zeroed by a select afterwards: a load under a branch is waited for at the
        // branch's join — three latency chains of ROWS loads per thread instead of 3 x ROWS loads in flight (same rule as wino_input_kernel)
        const float* imgp = in + (size_t)n * H * W * C + c4 * 4;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ix0 + kx;
            const bool okx = (unsigned)ix < (unsigned)W;
            const int ixc = min(max(ix, 0), W - 1);
            v4f x[ROWS];
#pragma unroll
            for (int ridx = 0; ridx < ROWS; ++ridx) {
                const int iy = iy0 + ridx;
                const bool ok = okx && (unsigned)iy < (unsigned)H;
                const v4f ld = *reinterpret_cast<const v4f*>(imgp + ((size_t)min(max(iy, 0), H - 1) * W + ixc) * C);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[ridx][e] = ok ? ld[e] : 0.f;   // a select (v_cndmask), not a multiply: the clamped neighbour may be Inf / NaN
            }
#pragma unroll
            for (int o = 0; o < STRIP; ++o)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) acc[o] += x[o * STRIDE + ky] * wk[ky * 3 + kx];
        }
#pragma unroll
        for (int o = 0; o < STRIP; ++o) {
            const int oy = oy0 + o;
            if (oy >= Ho) break;
            v4f v = acc[o];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act1(v[e], act, sl4[e]);
            *reinterpret_cast<v4f*>(out + (((size_t)n * Ho + oy) * Wo + ox) * C + c4 * 4) = v;
        }
    }
}

// Horizontal-strip variant (strip along x): better for stride 2, where a vertical strip would make every
// wave instruction skip every other pixel.
template <int STRIDE, int STRIP>
__global__ __launch_bounds__(256) void dwconv3x3_hstrip_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                        int B, int H, int W, int C, int Ho, int Wo, int act,
                                                        const float* __restrict__ slope) {
    constexpr int COLS = (STRIP - 1) * STRIDE + 3;
    const int C4 = C >> 2;
    const int strips = (Wo + STRIP - 1) / STRIP;
    const long total = (long)B * Ho * strips * C4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        long r = idx / C4;
        const int sx = (int)(r % strips); r /= strips;
        const int oy = (int)(r % Ho);
        const int n = (int)(r / Ho);
        const int ox0 = sx * STRIP;
        v4f wk[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wk[t] = *reinterpret_cast<const v4f*>(w + t * C + c4 * 4);
        const v4f b4 = *reinterpret_cast<const v4f*>(bias + c4 * 4);
        const v4f sl4 = slope ? *reinterpret_cast<const v4f*>(slope + c4 * 4) : v4f{0.f, 0.f, 0.f, 0.f};
        v4f acc[STRIP];
#pragma unroll
        for (int o = 0; o < STRIP; ++o) acc[o] = b4;
        const int iy0 = oy * STRIDE - 1, ix0 = ox0 * STRIDE - 1;
        const float* imgp = in + (size_t)n * H * W * C + c4 * 4;           // (unconditional clamped loads: see dwconv3x3_kernel)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = iy0 + ky;
            const bool oky = (unsigned)iy < (unsigned)H;
            const float* rowp = imgp + (size_t)min(max(iy, 0), H - 1) * W * C;
            v4f x[COLS];
#pragma unroll
            for (int cidx = 0; cidx < COLS; ++cidx) {
                const int ix = ix0 + cidx;
                const bool ok = oky && (unsigned)ix < (unsigned)W;
                const v4f ld = *reinterpret_cast<const v4f*>(rowp + (size_t)min(max(ix, 0), W - 1) * C);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[cidx][e] = ok ? ld[e] : 0.f;
            }
#pragma unroll
            for (int o = 0; o < STRIP; ++o)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc[o] += x[o * STRIDE + kx] * wk[ky * 3 + kx];
        }
#pragma unroll
        for (int o = 0; o < STRIP; ++o) {
            const int ox = ox0 + o;
            if (ox >= Wo) break;
            v4f v = acc[o];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act1(v[e], act, sl4[e]);
            *reinterpret_cast<v4f*>(out + (((size_t)n * Ho + oy) * Wo + ox) * C + c4 * 4) = v;
        }
    }
}

// Lean form (round 4).  The two kernels above spend their time on instructions, not on memory: ~600 per thread (64-bit index arithmetic
// with four divisions, four selects per loaded float4, an activation switch that carries the sigmoid's exp / divide) for 36 useful float4
// FMAs — 20x20x288 at B = 128 ran 31 us against a ~15-20 us traffic floor (in + out = 118 MB, both cache-resident).  Here:
//   * grid = (output row run, strip of rows, image): image and rows are scalars; a thread is float4 column r of the output row run
//     [Wo][C / 4]; its centre tap is input column r (stride 1) or 2 r - c4 (stride 2), the neighbours are -+ C/4 from there, so no pixel
//     coordinate is ever computed (the channel group c4 = r mod C/4 comes from one multiply-high);
//   * the taps come in through BUFFER loads with a per-image descriptor: rows above / below the image are out of range and read as zero
//     in hardware; the left / right column is pushed out of range by ONE select on its offset (not four per load);
//   * activation is a template parameter.
// Same summation order as the generic kernels (stride 1: columns left to right, rows inside; stride 2: rows top to bottom, columns
// inside): bit-identical results.
constexpr unsigned DW_OOB = 0x40000000u;                                     // an offset beyond any image (images are < 1 GB: host check)
template <int STRIDE, int STRIP, int ACT>
__global__ __launch_bounds__(256) void dwconv3x3_lean_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out, int H, int Lin, int Ho,
                                                             int Lout, int C4, unsigned c4_magic, const float* __restrict__ slope) {
    constexpr int ROWS = (STRIP - 1) * STRIDE + 3;
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    if (r >= Lout) return;
    const int n = (int)blockIdx.z, oy0 = (int)blockIdx.y * STRIP;
    const int c4 = r - (int)__umulhi((unsigned)r, c4_magic) * C4;           // r % C4 (c4_magic = ceil(2^32 / C4); exact for r < 2^20)
    const int C = C4 * 4;
    const size_t img = (size_t)H * Lin * 4;                                 // floats per input image
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in + (size_t)n * img), 0, (int)(img * 4), 0x00020000);
    const unsigned rowb = (unsigned)Lin * 16u;
    const int centre = STRIDE == 1 ? r : 2 * r - c4;
    unsigned vc[3];
    vc[1] = (unsigned)centre * 16u;
    vc[0] = r >= C4 ? vc[1] - (unsigned)C4 * 16u : DW_OOB;
    vc[2] = centre + C4 < Lin ? vc[1] + (unsigned)C4 * 16u : DW_OOB;
    const unsigned row0 = (unsigned)(oy0 * STRIDE - 1) * rowb;               // (oy0 = 0: wraps to "far out of range" together with any vc)
    v4f x[3][ROWS];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ri = 0; ri < ROWS; ++ri)
            x[kx][ri] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, vc[kx] + row0 + (unsigned)ri * rowb, 0, 0));
    v4f wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = *reinterpret_cast<const v4f*>(w + t * C + c4 * 4);
    const v4f b4 = *reinterpret_cast<const v4f*>(bias + c4 * 4);
    v4f acc[STRIP];
#pragma unroll
    for (int o = 0; o < STRIP; ++o) acc[o] = b4;
    if constexpr (STRIDE == 1) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int o = 0; o < STRIP; ++o)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) acc[o] += x[kx][o + ky] * wk[ky * 3 + kx];
    } else {
#pragma unroll
        for (int o = 0; o < STRIP; ++o)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc[o] += x[kx][o * STRIDE + ky] * wk[ky * 3 + kx];
    }
    v4f sl4 = v4f{0.f, 0.f, 0.f, 0.f};
    if constexpr (ACT == (int)Act::PRELU) sl4 = *reinterpret_cast<const v4f*>(slope + c4 * 4);
    float* __restrict__ op = out + ((size_t)n * Ho + oy0) * Lout * 4 + (size_t)r * 4;
#pragma unroll
    for (int o = 0; o < STRIP; ++o) {
        if (oy0 + o >= Ho) break;
        v4f v = acc[o];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (ACT == (int)Act::RELU) v[e] = v[e] > 0.f ? v[e] : 0.f;
            else if constexpr (ACT == (int)Act::PRELU) v[e] = v[e] >= 0.f ? v[e] : v[e] * sl4[e];
        }
        *reinterpret_cast<v4f*>(op + (size_t)o * Lout * 4) = v;
    }
}

template <int STRIDE, int ACT>
static void launch_dwconv3x3_lean(const float* in, const float* w9c, const float* bias, float* out, int B, int H, int W, int C, int Ho, int Wo,
                                  const float* slope, hipStream_t s) {
    constexpr int STRIP = STRIDE == 1 ? 4 : 2;
    const int C4 = C / 4, Lin = W * C4, Lout = Wo * C4;
    const unsigned magic = (unsigned)((0x100000000ull + (unsigned)C4 - 1) / (unsigned)C4);
    hipLaunchKernelGGL((dwconv3x3_lean_kernel<STRIDE, STRIP, ACT>), dim3((unsigned)((Lout + 255) / 256), (unsigned)((Ho + STRIP - 1) / STRIP), (unsigned)B),
                       dim3(256), 0, s, in, w9c, bias, out, H, Lin, Ho, Lout, C4, magic, slope);
}
template <int STRIDE>
static void launch_dwconv3x3_lean_act(const float* in, const float* w9c, const float* bias, float* out, int B, int H, int W, int C, int Ho, int Wo,
                                      int act, const float* slope, hipStream_t s) {
    if (act == (int)Act::RELU) launch_dwconv3x3_lean<STRIDE, (int)Act::RELU>(in, w9c, bias, out, B, H, W, C, Ho, Wo, slope, s);
    else if (act == (int)Act::PRELU) launch_dwconv3x3_lean<STRIDE, (int)Act::PRELU>(in, w9c, bias, out, B, H, W, C, Ho, Wo, slope, s);
    else launch_dwconv3x3_lean<STRIDE, (int)Act::NONE>(in, w9c, bias, out, B, H, W, C, Ho, Wo, slope, s);
}

void launch_dwconv3x3(const float* in, const float* w9c, const float* bias, float* out, int B, int H, int W, int C,
                      int stride, int act, const float* slope, hipStream_t s) {
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    constexpr int STRIP = 4;
    // (row runs < 2^20 float4s: the multiply-high remainder; image < 1 GB: DW_OOB; grid y / z limits)
    static const bool lean_on = [] { const char* e = getenv("FACEHIP_DW_LEAN"); return !e || atoi(e) != 0; }();
    const bool lean = lean_on && (stride == 1 || stride == 2) && C >= 8 && (long)W * (C / 4) < (1L << 20) &&
                      (long)H * W * C * 4 + (long)W * C * 4 * 8 < (long)DW_OOB && B <= 65535 && Ho <= 65535 * 2 &&
                      (act == (int)Act::NONE || act == (int)Act::RELU || (act == (int)Act::PRELU && slope));
    if (lean) {
        if (stride == 1) launch_dwconv3x3_lean_act<1>(in, w9c, bias, out, B, H, W, C, Ho, Wo, act, slope, s);
        else launch_dwconv3x3_lean_act<2>(in, w9c, bias, out, B, H, W, C, Ho, Wo, act, slope, s);
        return;
    }
    if (stride == 1) {
        const long total = (long)B * ((Ho + STRIP - 1) / STRIP) * Wo * (C / 4);
        hipLaunchKernelGGL((dwconv3x3_kernel<1, STRIP>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, in, w9c, bias, out, B, H, W, C, Ho, Wo, act, slope);
    } else {
        const long total = (long)B * Ho * ((Wo + STRIP - 1) / STRIP) * (C / 4);
        hipLaunchKernelGGL((dwconv3x3_hstrip_kernel<2, STRIP>), dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, in, w9c, bias, out, B, H, W, C, Ho, Wo, act, slope);
    }
}

// Depthwise k x k VALID convolution over a k x k map -> one value per channel (MobileFaceNet's "GDC" layer):
// out[b][c] = bias[c] + sum_p w[p][c] * in[b][p][c].  Thread = 4 channels of one image; lanes walk the channels.
__global__ __launch_bounds__(256) void dwglobal_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int B, int taps, int C, int act, const float* __restrict__ slope) {
    const int C4 = C >> 2;
    const long total = (long)B * C4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        const long b = idx / C4;
        v4f acc = *reinterpret_cast<const v4f*>(bias + c4 * 4);
        const float* x = in + (size_t)b * taps * C + c4 * 4;
        for (int p = 0; p < taps; ++p) acc += *reinterpret_cast<const v4f*>(x + (size_t)p * C) * *reinterpret_cast<const v4f*>(w + (size_t)p * C + c4 * 4);
        const v4f sl4 = slope ? *reinterpret_cast<const v4f*>(slope + c4 * 4) : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = act1(acc[e], act, sl4[e]);
        *reinterpret_cast<v4f*>(out + (size_t)b * C + c4 * 4) = acc;
    }
}
void launch_dwglobal(const float* in, const float* w, const float* bias, float* out, int B, int taps, int C, int act, const float* slope,
                     hipStream_t s) {
    const long total = (long)B * (C / 4);
    if (total > 0) hipLaunchKernelGGL(dwglobal_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, w, bias, out, B, taps, C, act, slope);
}

// Grouped 3x3 convolution (pad 1, stride 1 | 2) with G = 2 or 4 channels per group on both sides (MobileFaceNet's second layer:
// 64 groups of 2).  A float4 of 4 consecutive output channels depends on exactly the same 4 input channels, so the kernel has the
// shape of the depthwise one with a G-wide dot product per tap.  w: [9][C][G].  Thread = 4 channels of one output pixel.
template <int G>
__global__ __launch_bounds__(256) void gconv3x3_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int B, int H, int W, int C, int Ho, int Wo, int stride, int act,
                                                       const float* __restrict__ slope) {
    const int C4 = C >> 2;
    const long total = (long)B * Ho * Wo * C4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % C4);
        long r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int n = (int)(r / Ho);
        v4f acc = *reinterpret_cast<const v4f*>(bias + c4 * 4);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * stride - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * stride - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const v4f x = *reinterpret_cast<const v4f*>(in + (((size_t)n * H + iy) * W + ix) * C + c4 * 4);
                const float* wt = w + ((size_t)(ky * 3 + kx) * C + c4 * 4) * G;      // [4 output channels][G]
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < G; ++j) acc[e] += wt[e * G + j] * x[(e / G) * G + j];
            }
        }
        const v4f sl4 = slope ? *reinterpret_cast<const v4f*>(slope + c4 * 4) : v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = act1(acc[e], act, sl4[e]);
        *reinterpret_cast<v4f*>(out + (((size_t)n * Ho + oy) * Wo + ox) * C + c4 * 4) = acc;
    }
}
void launch_gconv3x3(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int C, int G, int stride, int act,
                     const float* slope, hipStream_t s) {
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const long total = (long)B * Ho * Wo * (C / 4);
    if (total <= 0) return;
    if (G == 2) hipLaunchKernelGGL(gconv3x3_kernel<2>, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, in, w, bias, out, B, H, W, C, Ho, Wo, stride, act, slope);
    else hipLaunchKernelGGL(gconv3x3_kernel<4>, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, in, w, bias, out, B, H, W, C, Ho, Wo, stride, act, slope);
}

// generic per-channel pass, scalar channel indexing (C need not be a multiple of 4)
__global__ __launch_bounds__(256) void affine_kernel(const float* __restrict__ in, const float* __restrict__ sc,
                                                     const float* __restrict__ sh, float* __restrict__ out, long total, int C) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        out[i] = in[i] * sc[c] + sh[c];
    }
}
void launch_affine(const float* in, const float* sc, const float* sh, float* out, long pixels, int C, hipStream_t s) {
    const long total = pixels * C;
    hipLaunchKernelGGL(affine_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, sc, sh, out, total, C);
}

__global__ __launch_bounds__(256) void act_kernel(const float* __restrict__ in, const float* __restrict__ slope,
                                                  float* __restrict__ out, long total, int C, int act) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float sl = slope ? slope[i % C] : 0.f;
        out[i] = act1(in[i], act, sl);
    }
}
void launch_act(const float* in, const float* slope, float* out, long pixels, int C, int act, hipStream_t s) {
    const long total = pixels * C;
    hipLaunchKernelGGL(act_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, slope, out, total, C, act);
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}
void launch_add(const float* a, const float* b, float* out, long n, hipStream_t s) {
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, b, out, n);
}

__global__ __launch_bounds__(256) void upsample2x_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H,
                                                         int W, int C) {
    const int Ho = 2 * H, Wo = 2 * W;
    const long total = (long)B * Ho * Wo * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long pix = i / C;
        const int ox = (int)(pix % Wo); pix /= Wo;
        const int oy = (int)(pix % Ho);
        const int n = (int)(pix / Ho);
        out[i] = in[(((size_t)n * H + (oy >> 1)) * W + (ox >> 1)) * C + c];
    }
}
void launch_upsample2x(const float* in, float* out, int B, int H, int W, int C, hipStream_t s) {
    const long total = (long)B * 4 * H * W * C;
    hipLaunchKernelGGL(upsample2x_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, B, H, W, C);
}

}  // namespace fh
