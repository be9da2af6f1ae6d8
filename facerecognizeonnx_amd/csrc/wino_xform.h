// wino_xform.h — the streaming transforms around the Winograd F(4x4, 3x3) GEMM, each piece once: wino_input_kernel, wino_output_kernel,
// wino_fused_kernel, wino_slice_kernel and wino_mix_kernel (winograd.hip, the only file that includes this) are composed from it.
//
// Thread = one tile x 4 channels (a float4 column); every global access is a 16-byte lane access and consecutive lanes walk the channels.
//   1. 1-D transforms   B^T, A^T of F(4x4), their F(2x2) forms on the same weight matrices, the split-bf16 pack;
//   2. output phase     36 M planes -> A^T M A -> bias -> ReLU / PReLU / sigmoid -> + residual -> out1 / out2 = y * s2 + t2 -> sink;
//   3. input phase      6x6 patch from a pixel source, zero outside the map -> B^T d B -> optional pack -> 36 plane stores.
// The kernels keep what is their own: name, __launch_bounds__, the thread <-> (image, tile, channel column) mapping, the LDS address rule
// of the image between the two phases, and where a plane's float4 lives (plain pointer, or a buffer descriptor with an out-of-range offset
// for the frequencies a tile class does not have) — handed in as callables, which the compiler inlines.
//
// Two rules live HERE and nowhere else (docs/kernels.md):
//   §3.0   select, never multiply: a value outside the map is removed by a select on the loaded value or by an address that cannot return
//          it.  Memory out there may hold Inf / NaN and 0 * NaN poisons every sum; loads stay unconditional (a load under a branch is
//          waited for at the join).
//   §3.1g  residual reads go BEFORE the stores: loads and stores share the in-order vmcnt, a residual read issued after a store can only
//          be waited for together with that store's acknowledgement (16 round trips per thread otherwise).
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_tile.h"
#include "kernels.h"
#include "plan.h"

namespace fh {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// ================================================================== 1. 1-D transforms ================================================
// Split-bf16 operand format of the opt-in "bf16x2" mode (fh_rec_set_precision): a value x travels as ONE 32-bit word holding
// hi = bf16(x) in the low half and mid = bf16(x - hi) in the high half — 16 mantissa bits, same bytes as fp32, so the V / U buffers,
// their indexing and the GEMM's LDS-DMA loader do not change at all; only the matrix instruction does (three bf16 products
// hh + hm + mh with f32 accumulation instead of one f32 product).
// Range: both halves are bf16 values, so hi overflows where bf16 does.  A finite |x| >= 0x7F7F8000 (2^127 * 1.99609375, half a bf16 ulp
// under the largest bf16) rounds hi to +-Inf, the residual x - hi is -+Inf and the word holds (Inf, -Inf): it unpacks to NaN.  +-Inf
// gives (Inf, NaN) and NaN gives (NaN, NaN) — every non-finite input, and every finite one above that threshold, stays non-finite.  At
// the other end a non-zero mid is at least x's last fp32 bit, 2^-23 |x|: it can be a bf16 subnormal only for |x| < 2^-103 (the layers' values are O(1)).
__device__ __forceinline__ v4f wino_pack_bf16x2(const v4f x) {
    v4u out;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const v2f a = {x[2 * p], x[2 * p + 1]};
        const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2));        // v_cvt_pk_bf16_f32 (round to nearest even)
        const v2f r = {a[0] - __builtin_bit_cast(float, hb << 16), a[1] - __builtin_bit_cast(float, hb & 0xffff0000u)};   // exact
        const unsigned mb = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
        out[2 * p] = (hb & 0xffffu) | (mb << 16);
        out[2 * p + 1] = (hb >> 16) | (mb & 0xffff0000u);
    }
    return __builtin_bit_cast(v4f, out);
}

// B^T (6x6) applied to a 6-vector
__device__ __forceinline__ void wino_bt(const v4f (&d)[6], v4f (&t)[6]) {
    t[0] = 4.f * d[0] - 5.f * d[2] + d[4];
    t[1] = -4.f * d[1] - 4.f * d[2] + d[3] + d[4];
    t[2] = 4.f * d[1] - 4.f * d[2] - d[3] + d[4];
    t[3] = -2.f * d[1] - d[2] + 2.f * d[3] + d[4];
    t[4] = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
    t[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}
// F(2x2,3x3) with the points {0, 1, -1, inf}: B^T rows (d0 - d2, d1 + d2, d2 - d1, d1 - d3), A^T = [1 1 1 0; 0 1 -1 -1]; its G rows are
// (4, -3, -3, 1) x the rows {0, 1, 2, 5} of F(4x4,3x3)'s G, so with those factors on the B^T rows the planes multiply the F(4x4) weight
// matrices U[6 i + j] unchanged.
__device__ __forceinline__ void wino_bt2s(const v4f (&d)[6], v4f (&t)[6]) {
    t[0] = 4.f * (d[0] - d[2]);
    t[1] = -3.f * (d[1] + d[2]);
    t[2] = 3.f * (d[1] - d[2]);
    t[3] = d[1] - d[3];
    t[4] = v4f{0.f, 0.f, 0.f, 0.f};
    t[5] = t[4];
}
// A^T (4x6) applied to a 6-vector
__device__ __forceinline__ void wino_at(const v4f (&m)[6], v4f (&y)[4]) {
    y[0] = m[0] + m[1] + m[2] + m[3] + m[4];
    y[1] = m[1] - m[2] + 2.f * m[3] - 2.f * m[4];
    y[2] = m[1] + m[2] + 4.f * m[3] + 4.f * m[4];
    y[3] = m[1] - m[2] + 8.f * m[3] - 8.f * m[4] + m[5];
}
// A^T of F(2x2) on the first four entries (rows 2, 3 of an F(2) tile lie outside the map and are never stored)
__device__ __forceinline__ void wino_at2(const v4f (&m)[6], v4f (&y)[2]) {
    y[0] = m[0] + m[1] + m[2];
    y[1] = m[1] - m[2] - m[3];
}

// ================================================================== 2. output phase ==================================================
struct WinoOutArgs {
    const float* M; const float* bias; const float* slope; const float* res; float* out1; float* out2; const float* s2; const float* t2;
    int B, H, W, C, TY, TX, act;
    long NTp;
};

// Tile (b, ty, tx), channels 4 c4 .. 4 c4 + 3 of the [B,H,W,C] output.
//   fetch(f) -> v4f        the tile's float4 of frequency plane f = 6 i + j of M
//   MIXED                  the tile may be an F(2) class in its row (rF2) and / or column (cF2) direction: both 1-D transforms are
//                          evaluated and selected (these kernels are bound by their V / M traffic, not by the vector ALU)
//   RES_ALL                all 16 residual reads in front of the first store; false: a row of four in front of that row's stores, for a
//                          kernel whose register file does not hold all 16
//   FEED                   the kernel feeds a next convolution that may read y * s2 + t2 with no out2 to store: s2 / t2 are loaded whenever
//                          p.s2 is set (identity otherwise); false: only for out2
//   sink(oy, ox, v, vb)    where a finished pixel goes besides memory (v: the output, vb: v * s2 + t2)
// Residual coordinates are clamped into the map so that the reads are unconditional; pixels outside the map are skipped by the row /
// column tests, which are uniform per tile.
template <bool MIXED, bool RES_ALL, bool FEED, class Fetch, class Sink>
__device__ __forceinline__ void wino_output_phase(const WinoOutArgs& p, const int b, const int ty, const int tx, const int c4, const bool rF2,
                                                  const bool cF2, Fetch fetch, Sink sink) {
    const int C = p.C;
    v4f t[4][6];                                             // t[y][j] = (A^T M)[y][j]
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        v4f m[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = fetch(i * 6 + j);
        v4f y[4];
        wino_at(m, y);
        if constexpr (MIXED) {
            v4f y2[2];
            wino_at2(m, y2);
            y[0] = rF2 ? y2[0] : y[0];
            y[1] = rF2 ? y2[1] : y[1];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r][j] = y[r];
    }
    const v4f b4 = p.bias ? *reinterpret_cast<const v4f*>(p.bias + c4 * 4) : v4f{0.f, 0.f, 0.f, 0.f};
    auto res_at = [&](int oy, int ox) {
        return *reinterpret_cast<const v4f*>(p.res + (((size_t)b * p.H + min(oy, p.H - 1)) * p.W + min(ox, p.W - 1)) * C + c4 * 4);
    };
    v4f rs[4][4];
    if constexpr (RES_ALL) {
        if (p.res) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int x = 0; x < 4; ++x) rs[r][x] = res_at(4 * ty + r, 4 * tx + x);
        }
    }
    const v4f one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
    v4f sl = zero, s2 = FEED ? one : zero, t2 = zero;
    if (p.act == (int)Act::PRELU) sl = *reinterpret_cast<const v4f*>(p.slope + c4 * 4);
    if (FEED ? p.s2 != nullptr : p.out2 != nullptr) { s2 = *reinterpret_cast<const v4f*>(p.s2 + c4 * 4); t2 = *reinterpret_cast<const v4f*>(p.t2 + c4 * 4); }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int oy = 4 * ty + r;
        if (oy >= p.H) continue;
        v4f y[4];
        wino_at(t[r], y);
        if constexpr (MIXED) {
            if (cF2) {
                v4f y2[2];
                wino_at2(t[r], y2);
                y[0] = y2[0]; y[1] = y2[1];
            }
        }
        if constexpr (!RES_ALL) {
            if (p.res) {
#pragma unroll
                for (int x = 0; x < 4; ++x) rs[r][x] = res_at(oy, 4 * tx + x);
            }
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int ox = 4 * tx + x;
            if (ox >= p.W) continue;
            v4f v = y[x] + b4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float u = v[e];
                if (p.act == (int)Act::RELU) u = u > 0.f ? u : 0.f;
                else if (p.act == (int)Act::PRELU) u = u >= 0.f ? u : u * sl[e];
                else if (p.act == (int)Act::SIGMOID) u = 1.0f / (1.0f + expf(-u));
                v[e] = u;
            }
            const size_t o = (((size_t)b * p.H + oy) * p.W + ox) * C + c4 * 4;
            if (p.res) v += rs[r][x];
            if (p.out1) *reinterpret_cast<v4f*>(p.out1 + o) = v;
            const v4f vb = v * s2 + t2;
            if (p.out2) *reinterpret_cast<v4f*>(p.out2 + o) = vb;
            sink(oy, ox, v, vb);
        }
    }
}

// ================================================================== 3. input phase ===================================================
// Second half: tt[i][c] = (B^T d)[i][c] -> (B^T d B)[i][j] = sum_c tt[i][c] * B^T[j][c] -> optional pack -> store(f = 6 i + j, v4f), for all
// 36 frequencies (a mixed kernel's store drops those its class does not have).
template <bool MIXED, class Store>
__device__ __forceinline__ void wino_input_rows(const v4f (&tt)[6][6], const bool cF2, const int pack, Store store) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        v4f o[6], o2[6];
        wino_bt(tt[i], o);
        if constexpr (MIXED) wino_bt2s(tt[i], o2);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const v4f v = MIXED && cF2 ? o2[j] : o[j];
            store(i * 6 + j, pack ? wino_pack_bf16x2(v) : v);
        }
    }
}

// Tile (ty, tx) of an H x W map: the 6x6 patch of rows / columns 4t - 1 .. 4t + 4.  pixel(iy, ix) -> v4f is called for in-map coordinates
// only; outside the map the patch is zero by a select.
template <bool MIXED, class Pixel, class Store>
__device__ __forceinline__ void wino_input_phase(const int H, const int W, const int ty, const int tx, const bool rF2, const bool cF2,
                                                 const int pack, Pixel pixel, Store store) {
    const int iy0 = 4 * ty - 1, ix0 = 4 * tx - 1;
    v4f tt[6][6];                                            // columns of the patch first
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int ix = ix0 + c;
        v4f d[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int iy = iy0 + r;
            const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            d[r] = ok ? pixel(iy, ix) : v4f{0.f, 0.f, 0.f, 0.f};
        }
        v4f tc[6];
        wino_bt(d, tc);
        if constexpr (MIXED) {
            v4f t2s[6];
            wino_bt2s(d, t2s);
#pragma unroll
            for (int i = 0; i < 6; ++i) tc[i] = rF2 ? t2s[i] : tc[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) tt[i][c] = tc[i];
    }
    wino_input_rows<MIXED>(tt, cF2, pack, store);
}

}  // namespace fh
