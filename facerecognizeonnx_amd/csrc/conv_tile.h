// conv_tile.h — the pieces the direct-convolution kernels of conv_mfma.hip share (conv_igemm_kernel, conv_tall_kernel, conv_pw_kernel,
// conv_fixup_kernel): the tile shape, the activation, the epilogue's per-channel vectors, the stream-K slab layout and the epilogue
// with its four forms.  Plain __forceinline__ functions; the kernels keep what is their own — the loaders, the two K loops (fragment
// ring / per-lane tap select: scheduled around different things) and the stream-K roles.
//
// conv_igemm_kernel is at the limit of the scalar register file in every instantiation (106 SGPRs, 8-139 more spilled to VGPR lanes), and
// how the code around its K loop is WRITTEN decides whether a few VGPRs go to scratch memory.  Each piece below was tried in it alone
// (profiles/conv_tile_refactor.md has the table); it takes those that leave registers, scratch and K loops as they were — conv_epilogue
// with conv_out_pixel, xcd_tile, conv_sk_nparts, the slab address rule conv_slab / conv_slab_at, ConvEpVec's constants — and keeps
// written out what does not: ConvEpVec's two loops (as a struct: 8-32 B of scratch in four instantiations; as free functions: other
// s_waitcnt counts in three K loops), the loops over a slab's blocks (8-12 B in five), and conv_epilogue as ONE function (its four
// forms as functions of their own: 8 B in three).  Change them only with the ISA comparison of that note at hand.
#pragma once
#include "conv_plan.h"
#include "gemm_tile.h"
#include "kernels.h"
#include "plan.h"

namespace fh {

template <int BM, int BN, int WM, int WN>
struct Tile {
    static constexpr int T = WM * WN * 64;
    static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static constexpr int RP = T / 8;                    // tile rows filled per loader pass
    static constexpr int AL = BM / RP, BL = BN / RP;
    static constexpr int SLAB = BM * BN;                // floats per accumulator slab
    static_assert(TM >= 1 && TN >= 1 && AL >= 1 && BL >= 1 && RP % 16 == 0, "tile shape");
};

// ---- activation.  act_c: the activation a compile-time constant; with_act switches ONCE per tile instead of running a branch tree per
// element — inlined 16 times per 32 x 32 block it made the epilogue thousands of basic blocks (phase stamps of conv_pw_kernel,
// scripts/pw_ablate.sh: first block in LDS -> last store issued 7.7 -> 5.8 us of a 37 us tile).  apply_act is the same switch per
// element, for the forms whose activation differs per channel (merged siblings) or that are not hot (plain).
template <int A>
__device__ __forceinline__ float act_c(float v, float slope) {
    if constexpr (A == (int)Act::RELU) return v > 0.f ? v : 0.f;
    else if constexpr (A == (int)Act::PRELU) return v >= 0.f ? v : v * slope;
    else if constexpr (A == (int)Act::SIGMOID) return 1.0f / (1.0f + expf(-v));
    else return v;
}
template <int A> struct ActC { static constexpr int value = A; };
template <class F>
__device__ __forceinline__ void with_act(int act, F&& f) {
    if (act == (int)Act::RELU) f(ActC<(int)Act::RELU>{});
    else if (act == (int)Act::PRELU) f(ActC<(int)Act::PRELU>{});
    else if (act == (int)Act::SIGMOID) f(ActC<(int)Act::SIGMOID>{});
    else f(ActC<(int)Act::NONE>{});
}
__device__ __forceinline__ float apply_act(float v, int act, float slope) {
    with_act(act, [&](auto AC) { v = act_c<decltype(AC)::value>(v, slope); });
    return v;
}

// ---- output row m -> pixel (n, oy, ox), and what the epilogue derives from it
struct ConvPixel {
    int n, oy, ox;
    // border class 3 cy + cx of a 3x3 pad-1 convolution with a BatchNorm shift folded into its bias (ConvArgs::bias_cls): taps that fall
    // on the zero padding contribute none of it
    __device__ __forceinline__ int border_class(const ConvArgs& p) const {
        return 3 * (oy == 0 ? 0 : oy == p.Ho - 1 ? 2 : 1) + (ox == 0 ? 0 : ox == p.Wo - 1 ? 2 : 1);
    }
    // first element of this pixel's row in a residual that is added through a 2x nearest up-sampling (ResMode::UP2X)
    __device__ __forceinline__ size_t up2x_row(const ConvArgs& p) const {
        return ((size_t)(n * (p.Ho >> 1) + (oy >> 1)) * (p.Wo >> 1) + (ox >> 1)) * p.Cout;
    }
};
__device__ __forceinline__ ConvPixel conv_out_pixel(const ConvArgs& p, const int m) {
    const int HoWo = p.Ho * p.Wo;
    const int n = m / HoWo, rem = m - n * HoWo, oy = rem / p.Wo;
    return ConvPixel{n, oy, rem - oy * p.Wo};
}

// ---- the epilogue's per-channel vectors of one tile: float [EP_ROWS][BN] in LDS — rows EP_BIAS .. EP_BIAS + 8 = bias (one per border
// class when bias_cls, else row 0), EP_SLOPE = PReLU slope, EP_S2 / EP_T2 = scale / shift of the second output; channels >= Cout hold
// 0.  With it the epilogue issues NO global load between its stores: on this ISA loads and stores share one in-order counter (vmcnt), so
// a load issued after a store can only be waited for together with that store's acknowledgement — bias / slope loads interleaved with
// the stores turned the epilogue into a chain of store round trips (16 per 256x64 tile, a third of the tile's time).
// fetch() runs before the K loop, into a few registers; park() after it, into LDS the loop has released (the caller's barrier follows).
// conv_tall_kernel and conv_pw_kernel use it; conv_igemm_kernel holds the same two loops written out (see the top of this file).
constexpr int EP_BIAS = 0, EP_SLOPE = 9, EP_S2 = 10, EP_T2 = 11, EP_ROWS = 12;
template <int BN, int THREADS>
struct ConvEpVec {
    static constexpr int FLOATS = EP_ROWS * BN, N = (FLOATS + THREADS - 1) / THREADS;
    float v[N];
    __device__ __forceinline__ void fetch(const ConvArgs& p, const int n0, const int tid, const bool live) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int e = tid + k * THREADS, a = e / BN, c = e - a * BN, co = n0 + c;
            float x = 0.f;
            if (live && a < EP_ROWS && co < p.Cout) {
                if (a < EP_SLOPE) { if (p.bias && (a == 0 || p.bias_cls)) x = p.bias[a * p.Cout + co]; }
                else if (a == EP_SLOPE) { if (p.act == (int)Act::PRELU) x = p.slope[co]; }
                else if (p.out2) x = a == EP_S2 ? p.s2[co] : p.t2[co];
            }
            v[k] = x;
        }
    }
    __device__ __forceinline__ void park(float* const ep, const int tid) const {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int e = tid + k * THREADS;
            if (e < FLOATS) ep[e] = v[k];
        }
    }
};

// ---- stream-K slabs: the raw accumulators of one K segment of remainder tile r, slot `part` of that tile's sk_maxp.  A thread's float4
// g of 32 x 32 block (i, j) sits at ((i TN + j) 4 + g) T + tid float4s: every store and load is a wave's 1 KB of consecutive bytes.
// (how many slots of a tile are filled: conv_sk_nparts, conv_plan.h)
template <class TL>
__device__ __forceinline__ float* conv_slab(const ConvArgs& p, const int r, const int part) { return p.slabs + ((size_t)r * p.sk_maxp + part) * TL::SLAB; }
template <class TL>
__device__ __forceinline__ size_t conv_slab_at(const int blk, const int g, const int tid) { return ((size_t)(blk * 4 + g) * TL::T + tid) * 4; }
// one 32 x 32 block of a slab added to a block of accumulators (conv_fixup_kernel; the owner's and the helper's loops over all blocks
// are written out in conv_igemm_kernel over conv_slab / conv_slab_at)
template <class TL>
__device__ __forceinline__ void conv_slab_add(const float* __restrict__ slab, v16f& sum, const int blk, const int tid) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const v4f v = *reinterpret_cast<const v4f*>(slab + conv_slab_at<TL>(blk, g, tid));
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[4 * g + c] += v[c];
    }
}

// ---- the epilogue: bias -> activation -> (+ residual, optionally through a 2x nearest up-sampling) -> store, plus an optional second
// output  y * s2 + t2.  C/D map of the 32x32 MFMA: column (= pixel here) = lane & 31, row (= channel) = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
// Four forms, the same arithmetic per element in each, each a block of conv_epilogue behind its condition:
//   EP_MERGED  merged sibling convolutions (n_outs > 0): per-channel-range destination and activation, scalar stores;
//   EP_LINES   ep and tr given, Cout % 4 == 0: whole 128-byte lines through a wave-private turn-around scratch (carries the
//              FACEHIP_PW_ABL stamps of the diagnostic build, see conv_pw_kernel);
//   EP_QUADS   ep given, Cout % 4 == 0: per accumulator quad, vectors from LDS;
//   EP_PLAIN   everything else: vectors from global memory, float4 or scalar; only_i / only_j >= 0 = that block alone (conv_fixup_kernel).
// ep: the tile's parked ConvEpVec; tr: the whole-line scratch behind it (conv_ep_wants_lines).  FORMS: the forms a caller can reach;
// the others are not instantiated for it (a launch that reached one would leave its tile unwritten: the launchers' conditions and
// these sets say the same thing — conv_pw_bn excludes n_outs and Cout % 4, conv_tall_plan Cout % 4 without n_outs, conv_fixup_kernel
// passes no ep; launch_pw and launch_cfg check it again on the host).
__device__ __forceinline__ bool conv_ep_wants_lines(const ConvArgs& p) { return p.ep_direct == 0 ? (p.Cout & 31) == 0 : p.ep_direct == 3; }
enum : unsigned { EP_MERGED = 1, EP_LINES = 2, EP_QUADS = 4, EP_PLAIN = 8, EP_ALL = 15 };
template <int BM, int BN, int WM, int WN, unsigned FORMS = EP_ALL>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& p, v16f (&acc)[BM / WM / 32][BN / WN / 32], int m0, int n0,
                                              int wm, int wn, int lane, int only_i = -1, int only_j = -1, const float* ep = nullptr,
                                              float* tr = nullptr) {
    using TL = Tile<BM, BN, WM, WN>;
    const int fr = lane & 31, fh2 = lane >> 5;
    const int HoWo = p.Ho * p.Wo;
    const int M = p.B * HoWo;
    const float* __restrict__ res = p.res;
    float* __restrict__ out1 = p.out1;
    float* __restrict__ out2 = p.out2;
    const bool vec = (p.Cout & 3) == 0;
    if (p.n_outs > 0) {                                  // merged sibling convs: per-channel-range destination
        if constexpr ((FORMS & EP_MERGED) != 0) {
#pragma unroll
        for (int i = 0; i < TL::TM; ++i) {
            const int m = m0 + (wm * TL::TM + i) * 32 + fr;
            if (m >= M || (only_i >= 0 && i != only_i)) continue;
#pragma unroll
            for (int j = 0; j < TL::TN; ++j) {
                if (only_j >= 0 && j != only_j) continue;
                const int cb = n0 + (wn * TL::TN + j) * 32 + 4 * fh2;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int co = cb + 8 * (e >> 2) + (e & 3);
                    if (co >= p.Cout) continue;
                    const int g = co >= p.oc0[2] && p.n_outs > 2 ? 2 : co >= p.oc0[1] ? 1 : 0;
                    const int cg = p.oc0[g + 1] - p.oc0[g];
                    const float v = apply_act(acc[i][j][e] + p.bias[co], p.oact[g], 0.f);
                    p.outs[g][(size_t)m * cg + (co - p.oc0[g])] = v;
                }
            }
        }
        }
        return;
    }
    if (ep && vec && tr && only_i < 0 && only_j < 0) {
        if constexpr ((FORMS & EP_LINES) != 0) {
        // Whole-line form (round 4).  A lane's accumulators are 4-channel pieces of ITS pixel row: written straight from registers, one
        // store instruction puts 32 bytes into each of 32 rows — a quarter of a 128-byte line per row, 8 instructions (and 8 residual
        // reads) per line.  Here each 32 x 32 block is turned around in a wave-private LDS scratch (tr: [waves][32 rows][36 floats], the
        // 16 lanes of a b128 phase hit different banks on the write side) and a lane takes float4 column cq of rows rr, rr + 8, rr + 16,
        // rr + 24: one instruction then moves 8 rows x ONE whole line, for stores and residual reads alike, and the per-channel vectors of
        // a block are the same for all four of a lane's rows (whole lines when Cout % 32 == 0, whole 128-byte runs otherwise).  Same arithmetic
        // per element: bit-identical results.
        float* const blk = tr + (wm * WN + wn) * (32 * 36);
        const int rr = lane >> 3, cq = lane & 7;
#ifdef FACEHIP_PW_ABL
        const unsigned long long est0 = wall_clock64();
        unsigned long long est1 = 0, est2 = 0, est3 = 0;
#endif
        // Loads and stores share ONE in-order counter (vmcnt): a wait for a residual load that sits behind a store in program order is a
        // wait for that store's acknowledgement (~0.36 us; with the residual a run-time flag the compiler kept such a wait in front of every
        // row group even when there was no residual).  So the residual is a compile-time flag here, a block's residual reads are issued
        // first and consumed two row groups at a time BEFORE those groups' stores.  (What remains between blocks is the compiler's
        // vmcnt(0) in front of the next block's LDS stores — it protects the registers the pending global stores read; giving every stored
        // value a register of its own removed it and changed nothing: the tile's 48 KB leave at the chip's ~5 TB/s write rate together
        // with every other workgroup's, scripts/pw_phases.py.)
        auto body = [&](auto AC, auto RC) {
        constexpr int A = decltype(AC)::value;
        constexpr bool R = decltype(RC)::value != 0;
#pragma unroll
        for (int i = 0; i < TL::TM; ++i) {
            const int mb = m0 + (wm * TL::TM + i) * 32 + rr;               // this lane's rows: mb + 8 k
            int cls4 = 0;                                                   // border class of row k in bits 4k .. 4k+3
            if (p.bias_cls) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    cls4 |= conv_out_pixel(p, min(mb + 8 * k, M - 1)).border_class(p) << (4 * k);
                }
            }
            auto res_row = [&](int m) -> size_t {
                return p.res_mode != (int)ResMode::UP2X ? (size_t)m * p.Cout : conv_out_pixel(p, m).up2x_row(p);
            };
#pragma unroll
            for (int j = 0; j < TL::TN; ++j) {
                const int cl = (wn * TL::TN + j) * 32 + 4 * cq;            // channel within the tile
                const int co = n0 + cl;
                if (n0 + (wn * TL::TN + j) * 32 >= p.Cout) continue;       // (a padded column block; wave-uniform)
                const bool cok = co < p.Cout;                              // (the last block of a Cout that is not a multiple of 32: its tail lanes idle)
                v4f r4[4];
                if constexpr (R) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) r4[k] = cok ? *reinterpret_cast<const v4f*>(res + res_row(min(mb + 8 * k, M - 1)) + co) : v4f{0.f, 0.f, 0.f, 0.f};
                }
                wave_lds_order();                                            // (the previous block's scratch reads lie above these writes)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<v4f*>(blk + fr * 36 + 8 * g + 4 * fh2) = v4f{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                wave_lds_order();                                            // (lane (rr, cq) reads rows other lanes wrote)
                v4f sl = {0.f, 0.f, 0.f, 0.f}, s2 = sl, t2 = sl;
                if constexpr (A == (int)Act::PRELU) sl = *reinterpret_cast<const v4f*>(ep + EP_SLOPE * BN + cl);
                if (out2) { s2 = *reinterpret_cast<const v4f*>(ep + EP_S2 * BN + cl); t2 = *reinterpret_cast<const v4f*>(ep + EP_T2 * BN + cl); }
#ifdef FACEHIP_PW_ABL
                if (i == 0 && j == 0) est1 = wall_clock64();                // first block's accumulators written to LDS (issued)
#endif
                // (two row groups at a time: their arithmetic, then their stores — four at a time spill in the 128-register instantiations)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    v4f vk[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int k = 2 * h + q;
                        const v4f a4 = *reinterpret_cast<const v4f*>(blk + (rr + 8 * k) * 36 + 4 * cq);
                        const v4f b4 = *reinterpret_cast<const v4f*>(ep + ((cls4 >> (4 * k)) & 15) * BN + cl);
#pragma unroll
                        for (int c = 0; c < 4; ++c) vk[q][c] = act_c<A>(a4[c] + b4[c], sl[c]);
                        if constexpr (R) vk[q] += r4[k];
                    }
#if defined(__HIP_DEVICE_COMPILE__)
                    __builtin_amdgcn_sched_barrier(0);                      // (every wait of this half lies above its stores)
#endif
#ifdef FACEHIP_PW_ABL
                    if (i == 0 && j == 0 && h == 0) est2 = wall_clock64();  // first block's first values ready
#endif
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int m = mb + 8 * (2 * h + q);
#ifdef FACEHIP_PW_ABL
                        if ((p.sk_test_drop & 16) && lane != 0) continue;  // (diagnostic: every instruction of the epilogue but 63 of 64 lanes' stores)
#endif
                        if (m < M && cok) {
                            const size_t row = (size_t)m * p.Cout + co;
                            if (out1) *reinterpret_cast<v4f*>(out1 + row) = vk[q];
                            if (out2) *reinterpret_cast<v4f*>(out2 + row) = vk[q] * s2 + t2;
                        }
                    }
                }
#ifdef FACEHIP_PW_ABL
                if (i == 0 && j == 0) est3 = wall_clock64();                // first block's four stores issued
#endif
            }
        }
        };
        with_act(p.act, [&](auto AC) {
            if (p.res_mode != (int)ResMode::NONE) body(AC, ActC<1>{}); else body(AC, ActC<0>{});
        });
#ifdef FACEHIP_PW_ABL
        if (threadIdx.x == 0 && p.slabs && p.Cout == 288 && p.Cin == 288) {   // (phase stamps of conv_pw_kernel, second half: see there)
            unsigned long long* o = reinterpret_cast<unsigned long long*>(p.slabs) + 8192 + (size_t)blockIdx.x * 4;
            o[0] = est0; o[1] = est1; o[2] = wall_clock64();
            unsigned long long* o2 = reinterpret_cast<unsigned long long*>(p.slabs) + 16384 + (size_t)blockIdx.x * 2;
            o2[0] = est2; o2[1] = est3;
        }
#endif
        }
        return;
    }
    if (ep && vec) {
        if constexpr ((FORMS & EP_QUADS) != 0) {
        // per 32-pixel row block: its TN*4 residual float4s first, then per accumulator quad vectors from LDS, arithmetic, stores
        // (all TM row blocks' residuals up front would not fit the register file of the large tiles)
        with_act(p.act, [&](auto AC) {
        constexpr int A = decltype(AC)::value;
#pragma unroll
        for (int i = 0; i < TL::TM; ++i) {
            const int m = m0 + (wm * TL::TM + i) * 32 + fr;
            if (m >= M) continue;
            const size_t row = (size_t)m * p.Cout;
            int cls = 0;
            size_t rrow = row;
            if (p.bias_cls || p.res_mode == (int)ResMode::UP2X) {
                const ConvPixel px = conv_out_pixel(p, m);
                if (p.bias_cls) cls = px.border_class(p);
                if (p.res_mode == (int)ResMode::UP2X) rrow = px.up2x_row(p);
            }
            v4f r4[TL::TN][4];
            if (p.res_mode != (int)ResMode::NONE) {
#pragma unroll
                for (int j = 0; j < TL::TN; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int co = n0 + (wn * TL::TN + j) * 32 + 4 * fh2 + 8 * g;
                        r4[j][g] = co < p.Cout ? *reinterpret_cast<const v4f*>(res + rrow + co) : v4f{0.f, 0.f, 0.f, 0.f};
                    }
            }
#pragma unroll
            for (int j = 0; j < TL::TN; ++j) {
                const int cl = (wn * TL::TN + j) * 32 + 4 * fh2;           // channel within the tile
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = n0 + cl + 8 * g;
                    if (co >= p.Cout) continue;
                    const v4f b4 = *reinterpret_cast<const v4f*>(ep + cls * BN + cl + 8 * g);
                    v4f sl = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (A == (int)Act::PRELU) sl = *reinterpret_cast<const v4f*>(ep + EP_SLOPE * BN + cl + 8 * g);
                    v4f v;
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = act_c<A>(acc[i][j][4 * g + c] + b4[c], sl[c]);
                    if (p.res_mode != (int)ResMode::NONE) v += r4[j][g];
                    if (out1) *reinterpret_cast<v4f*>(out1 + row + co) = v;
                    if (out2) {
                        const v4f s2 = *reinterpret_cast<const v4f*>(ep + EP_S2 * BN + cl + 8 * g), t2 = *reinterpret_cast<const v4f*>(ep + EP_T2 * BN + cl + 8 * g);
                        *reinterpret_cast<v4f*>(out2 + row + co) = v * s2 + t2;
                    }
                }
            }
        }
        });
        }
        return;
    }
    if constexpr ((FORMS & EP_PLAIN) != 0) {
#pragma unroll
    for (int i = 0; i < TL::TM; ++i) {
        const int m = m0 + (wm * TL::TM + i) * 32 + fr;
        if (m >= M || (only_i >= 0 && i != only_i)) continue;
        const size_t row = (size_t)m * p.Cout;
        size_t rrow = row;
        const float* __restrict__ bias = p.bias;
        if (p.bias_cls) bias += conv_out_pixel(p, m).border_class(p) * p.Cout;
        if (p.res_mode == (int)ResMode::UP2X) rrow = conv_out_pixel(p, m).up2x_row(p);
#pragma unroll
        for (int j = 0; j < TL::TN; ++j) {
            if (only_j >= 0 && j != only_j) continue;
            const int cb = n0 + (wn * TL::TN + j) * 32 + 4 * fh2;
            if (vec) {
                v4f r4[4];
                if (p.res_mode != (int)ResMode::NONE) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int co = cb + 8 * g;
                        r4[g] = co < p.Cout ? *reinterpret_cast<const v4f*>(res + rrow + co) : v4f{0.f, 0.f, 0.f, 0.f};
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = cb + 8 * g;
                    if (co >= p.Cout) continue;
                    const v4f b4 = bias ? *reinterpret_cast<const v4f*>(bias + co) : v4f{0.f, 0.f, 0.f, 0.f};
                    v4f sl = {0.f, 0.f, 0.f, 0.f};
                    if (p.act == (int)Act::PRELU) sl = *reinterpret_cast<const v4f*>(p.slope + co);
                    v4f v;
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = apply_act(acc[i][j][4 * g + c] + b4[c], p.act, sl[c]);
                    if (p.res_mode != (int)ResMode::NONE) v += r4[g];
                    if (out1) *reinterpret_cast<v4f*>(out1 + row + co) = v;
                    if (out2) {
                        const v4f s2 = *reinterpret_cast<const v4f*>(p.s2 + co), t2 = *reinterpret_cast<const v4f*>(p.t2 + co);
                        *reinterpret_cast<v4f*>(out2 + row + co) = v * s2 + t2;
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int co = cb + 8 * (e >> 2) + (e & 3);
                    if (co >= p.Cout) continue;
                    float v = apply_act(acc[i][j][e] + (bias ? bias[co] : 0.f), p.act, p.slope ? p.slope[co] : 0.f);
                    if (p.res_mode != (int)ResMode::NONE) v += res[rrow + co];
                    if (out1) out1[row + co] = v;
                    if (out2) out2[row + co] = v * p.s2[co] + p.t2[co];
                }
            }
        }
    }
    }
}

}  // namespace fh
