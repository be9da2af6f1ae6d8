// stem_tile.h — the pieces the fused u8 stem kernels share, each written once: stem_conv_u8_kernel, stem_conv_px_kernel,
// stem_conv_border_kernel and stem_mfma_kernel (stem.hip) and the stem phase of front_kernel (dwpw_mfma.hip).
//   stem_unpack    a window row's bytes, as aligned dwords, -> floats
//   stem_mfma3     floats -> bf16 B fragment, three MFMAs against the lo / mid / hi weight terms
//   stem_byte      conv padding / letterbox canvas / pixel: which of the three a position of the net input is, and its bytes
//   stem_epilogue  activation, out1 = y, out2 = y * s2 + t2
//   stem_interior  the output pixels whose whole window is real image
// (the packed-FMA row of the thread-per-pixel kernel is stem_fma.h)
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_tile.h"
#include "plan.h"

namespace fh {

// Eight consecutive bytes in two dwords -> floats (v_cvt_f32_ubyteN).
__device__ __forceinline__ void stem_unpack8(const unsigned n0, const unsigned n1, float* f) {
    f[0] = (float)(n0 & 255u); f[1] = (float)((n0 >> 8) & 255u); f[2] = (float)((n0 >> 16) & 255u); f[3] = (float)(n0 >> 24);
    f[4] = (float)(n1 & 255u); f[5] = (float)((n1 >> 8) & 255u); f[6] = (float)((n1 >> 16) & 255u); f[7] = (float)(n1 >> 24);
}
// N = 8 | 9 bytes that start at byte sh (0..3) of the aligned dword d0 and run on through d1, d2 -> floats.
template <int N>
__device__ __forceinline__ void stem_unpack(const unsigned d0, const unsigned d1, const unsigned d2, const unsigned sh, float* f) {
    stem_unpack8(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh), f);
    if constexpr (N == 9) f[8] = (float)((d2 >> (8u * sh)) & 255u);
}

// One 16-channel block of the matrix-core stem: acc + W x f on v_mfma_f32_16x16x32_bf16, W as three bf16 terms whose sum is the fp32
// weight exactly (stem_pack_wfrag: [hi, mid, lo]), added smallest first.  f -> bf16 by truncation: exact for 0..255 and 127.5.
__device__ __forceinline__ v4f stem_mfma3(const float (&f)[8], v4f acc, const v4u w_lo, const v4u w_mid, const v4u w_hi) {
    v4u bq;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        bq[i] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, f[2 * i + 1]), __builtin_bit_cast(unsigned, f[2 * i]), 0x07060302u);
    const bf16x8 bfrag = __builtin_bit_cast(bf16x8, bq);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w_lo), bfrag, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w_mid), bfrag, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w_hi), bfrag, acc, 0, 0, 0);
    return acc;
}

// Position (iy, ix) of the net input: outside it = the convolution's zero padding; inside it but outside the pasted image = the
// letterbox canvas, u8 0; otherwise the frame's pixel.  v = NB bytes of that pixel from byte c0 on (B, G, R), 0 where there is none.
// What the padding counts as is the caller's: literal kernels skip the tap, the folded form takes 127.5 (it cancels against the bias).
enum class StemAt : int { PAD, CANVAS, PIXEL };
template <int NB>
struct StemBytes {
    StemAt at;
    float v[NB];
};
template <int NB>
__device__ __forceinline__ StemBytes<NB> stem_byte(const uint8_t* __restrict__ img, const int step, const int iy, const int ix, const int c0,
                                                   const int inH, const int inW, const int srcH, const int srcW) {
    StemBytes<NB> r;
    r.at = StemAt::PAD;
#pragma unroll
    for (int c = 0; c < NB; ++c) r.v[c] = 0.f;
    if ((unsigned)iy < (unsigned)inH && (unsigned)ix < (unsigned)inW) {
        r.at = StemAt::CANVAS;
        if (iy < srcH && ix < srcW) {
            r.at = StemAt::PIXEL;
            const uint8_t* p = img + (size_t)iy * step + (size_t)ix * 3 + c0;
#pragma unroll
            for (int c = 0; c < NB; ++c) r.v[c] = (float)p[c];
        }
    }
    return r;
}

// y = act(y), out1[o] = y, out2[o] = y * s2 + t2 for four consecutive channels.  sl / sc / sh: the slope, s2 and t2 of those channels
// wherever the kernel holds them (registers, LDS, memory) — read only where the activation / out2 asks for them.
__device__ __forceinline__ void stem_epilogue(v4f y, const int act, const v4f* sl, float* __restrict__ out1, float* __restrict__ out2,
                                              const size_t o, const v4f* sc, const v4f* sh) {
    if (act == (int)Act::RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = y[e] > 0.f ? y[e] : 0.f;
    } else if (act == (int)Act::PRELU) {
        const v4f s = *sl;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = y[e] >= 0.f ? y[e] : y[e] * s[e];
    } else if (act == (int)Act::SIGMOID) {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = 1.0f / (1.0f + expf(-y[e]));
    }
    if (out1) *reinterpret_cast<v4f*>(out1 + o) = y;
    if (out2) *reinterpret_cast<v4f*>(out2 + o) = y * *sc + *sh;
}

// Output pixels x0..x1 x y0..y1 (inclusive) whose nine taps are real pixels of the pasted image and whose rows' 12-byte windows lie
// inside their image row (not its first / last pixel): what the folded kernels compute without a bounds test.
struct StemRect {
    int x0, y0, x1, y1;
    __host__ __device__ bool empty() const { return x1 < x0 || y1 < y0; }
    __host__ __device__ bool has(const int ox, const int oy) const { return oy >= y0 && oy <= y1 && ox >= x0 && ox <= x1; }
    __host__ __device__ bool has_tile(const int ox, const int oy, const int t) const { return oy >= y0 && oy + t - 1 <= y1 && ox >= x0 && ox + t - 1 <= x1; }
};
__host__ __device__ inline StemRect stem_interior(const int stride, const int srcH, const int srcW, const int Ho, const int Wo) {
    const int x1 = (srcW - 3) / stride, y1 = (srcH - 2) / stride;
    return StemRect{(2 + stride - 1) / stride, 1, x1 < Wo - 1 ? x1 : Wo - 1, y1 < Ho - 1 ? y1 : Ho - 1};
}

}  // namespace fh
