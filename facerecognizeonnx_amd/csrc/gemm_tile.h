// gemm_tile.h — the "lean GEMM" tile: ONE loader, ONE K-chunk body and ONE turn-around store, shared by wino_gemm_kernel,
// wino_gemm_pers_kernel, wino_gemm_bf16x2_kernel, wino_gemm_x3_kernel (winograd.hip), conv_pw_kernel and conv_pw_x3_kernel (conv_mfma.hip); with it the vector typedefs, the
// LDS-DMA wrapper and the XCD-contiguous tile order every .hip file of the library uses.
//
// The tile: 128 rows of the "pixel" operand (V / the activations) x BN rows of the weight operand, both with contiguous rows of K
// floats, K cut into 32-deep chunks.  256 threads = 4 waves; wave `wid` owns pixel rows 32 wid .. 32 wid + 31 and all BN columns.
//   * global -> LDS directly (LDS-DMA, 16 bytes per lane), double buffered: buffer = [128 + BN rows][8 float4 columns], the 16-byte
//     column XOR-swizzled by (row >> 1) & 7 ON THE SOURCE SIDE (lane (lrow, column) fetches source column lqs), which makes the
//     ds_read_b128 fragment reads of 32 different rows conflict-free;
//   * one ds_read_b128 feeds 4 MFMAs (f32) or half of one 16-deep step (split-bf16); the weights are the MFMA's A operand, so a lane
//     ends up with ONE pixel row and, per accumulator quad, 4 consecutive output columns;
//   * one barrier per chunk: the chunk after the current one is requested, the current one multiplied, then everyone meets.
// The kernels keep what is their own: where the operands come from (per-tile weight pointer, zero line behind K), the schedule
// around the loop (several tiles per workgroup, counted waits, phase stamps) and the epilogue.  The pieces are plain
// __forceinline__ functions over the kernel's own `__shared__ v4f lds[2][(128 + BN) * 8]`: every kernel keeps its name, its LDS size
// and the register budget of the loop written out in place.
// conv_igemm_kernel / conv_tall_kernel (2 x 2 wave tiles, fragment ring, per-lane tap masks; their shared pieces and the epilogue all
// three convolution kernels run are in conv_tile.h, which includes this header) and the halo kernels take only the typedefs, lds_dma16
// and xcd_tile from here.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace fh {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// global -> LDS without a register round trip (global_load_lds_dwordx4).  The global address is per lane; the LDS address is the
// WAVE-UNIFORM `dst` + 16 * lane.  (The builtin only exists in the device pass; the host pass just needs the kernel body to parse.)
__device__ __forceinline__ void lds_dma16(const float* src, void* dst) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
#else
    (void)src; (void)dst;
#endif
}

// XCD-contiguous tile order.  Workgroups are dealt round-robin over the 8 XCDs (block % 8), each with its own L2: workgroup `block` of
// `nblocks` takes the tile that gives every XCD one CONTIGUOUS run of tiles, so neighbouring tiles (same rows, shared halo) share an L2.
// (I: blockIdx.x as it is, or the int virtual block index of a kernel that walks several tiles.)
template <typename I>
__device__ __forceinline__ int xcd_tile(const I block, const int nblocks) {
    const int q = nblocks >> 3, r8 = nblocks & 7, x = block & 7;
    return x * q + min(x, r8) + (int)(block >> 3);
}

constexpr int GEMM_BM = 128;                                    // pixel rows per tile
template <int BN> constexpr int gemm_buf_slots() { return (GEMM_BM + BN) * 8; }      // float4 slots per tile buffer
template <int BN> using GemmLds = v4f[2][gemm_buf_slots<BN>()];                       // the kernel's LDS: two tile buffers

// Where a thread stands in the tile.  Fragment side: lane (fr, fh2) multiplies row fr of its 32-row block with k-half fh2 of every
// 8-deep step, fsw = that row's column swizzle.  Loader side: thread (lrow, tid & 7) fills LDS column tid & 7 of rows lrow + 32 i from
// source column lqs.
struct GemmLane {
    int tid, lane, wid, fr, fh2, fsw;
    __device__ __forceinline__ int lrow() const { return tid >> 3; }
    __device__ __forceinline__ int lqs() const { return (tid & 7) ^ ((lrow() >> 1) & 7); }      // source k-column (swizzle on the source side)
};
__device__ __forceinline__ GemmLane gemm_lane() {
    GemmLane l;
    l.tid = threadIdx.x; l.lane = l.tid & 63;
    l.wid = __builtin_amdgcn_readfirstlane(l.tid >> 6);
    l.fr = l.lane & 31; l.fh2 = l.lane >> 5; l.fsw = (l.fr >> 1) & 7;
    return l;
}

// A thread's part in filling the tile buffers: its float4 of row lrow of each operand (`a32` / `b32` floats from one 32-row pass to
// the next), and where its wave's 64 float4s of a pass land in buffer 0.
struct GemmSrc {
    const float* a;
    const float* b;
    size_t a32, b32;
    v4f* dA;
    v4f* dB;
};
// ... for the tile at row m0 of A [rows][lda] and row n0 of B [rows][ldb]
template <int BN>
__device__ __forceinline__ GemmSrc gemm_src(GemmLds<BN>& lds, const float* A, const int m0, const int lda, const float* B, const int n0, const int ldb,
                                            const GemmLane& l) {
    const int lrow = l.lrow(), lqs = l.lqs();
    return GemmSrc{A + (size_t)(m0 + lrow) * lda + lqs * 4, B + (size_t)(n0 + lrow) * ldb + lqs * 4, (size_t)32 * lda, (size_t)32 * ldb,
                   &lds[0][l.wid * 64], &lds[0][GEMM_BM * 8 + l.wid * 64]};
}

// One 32-deep chunk of both operands -> buffer `buf`; both sources advance by 32 floats.  a_live = false sends this thread's pixel
// pieces to `a_dead` instead (conv_pw_kernel: the float4 columns behind K in the last chunk come from a zero line) — chosen by the
// source ADDRESS, never by a branch around the request or a multiply: the LDS image is always written in full.
template <int BN>
__device__ __forceinline__ void gemm_load_chunk(GemmSrc& s, const int buf, const bool a_live = true, const float* const a_dead = nullptr) {
    v4f* const dA = s.dA + buf * gemm_buf_slots<BN>();
    v4f* const dB = s.dB + buf * gemm_buf_slots<BN>();
#pragma unroll
    for (int i = 0; i < GEMM_BM / 32; ++i) lds_dma16(a_live ? s.a + i * s.a32 : a_dead, dA + i * 32 * 8);
#pragma unroll
    for (int i = 0; i < BN / 32; ++i) lds_dma16(s.b + i * s.b32, dB + i * 32 * 8);
    s.a += 32; s.b += 32;
}

// A lane's fragments of one k-step (ablation builds: held in registers instead of read in the loop)
template <int TN>
struct GemmFrag {
    v4f x, w[TN];
};
template <int TN>
__device__ __forceinline__ GemmFrag<TN> gemm_frag(const v4f* const tile, const GemmLane& l, const int s) {
    const v4f* const X = tile + l.wid * (32 * 8) + l.fr * 8;
    const v4f* const Wt = tile + GEMM_BM * 8 + l.fr * 8;
    const int col = (2 * s + l.fh2) ^ l.fsw;
    GemmFrag<TN> f;
    f.x = X[col];
#pragma unroll
    for (int j = 0; j < TN; ++j) f.w[j] = Wt[j * 32 * 8 + col];
    return f;
}

// ---- the K-chunk body, f32: request the next chunk, 4 steps x 4 x TN v_mfma_f32_32x32x2_f32 on the current one, barrier.
// Per output the products are added s outer, e inner (and j innermost between the outputs) — every kernel on this body gives a dot
// product the same bits.  `tile_buf` holds the current chunk, `more` says whether another follows (it goes to the other buffer).
// ABL (diagnostic instantiations only — scripts/wino_gemm_ablate.sh, scripts/pw_ablate.sh; results are garbage): 1 = no loads in the loop
// (the first chunk, in buffer 0, is computed over and over), 2 = no LDS reads (the operands `held` stay in registers), 4 = no barrier.
template <int BN, int ABL = 0>
__device__ __forceinline__ void gemm_chunk_f32(v16f (&acc)[BN / 32], GemmLds<BN>& lds, const int tile_buf, const bool more, GemmSrc& src,
                                               const GemmLane& l, const bool a_live = true, const float* const a_dead = nullptr,
                                               const GemmFrag<BN / 32>* const held = nullptr) {
    constexpr int TN = BN / 32;
    const int buf = (ABL & 1) ? 0 : tile_buf;
    if ((ABL & 1) == 0 && more) gemm_load_chunk<BN>(src, buf ^ 1, a_live, a_dead);
    const v4f* const tile = lds[buf];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        GemmFrag<TN> f;
        if constexpr ((ABL & 2) != 0) {
            f = *held;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(f.x));                     // (opaque: the compiler must not fold the steps together)
#endif
        } else {
            f = gemm_frag<TN>(tile, l, s);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.w[j][e], f.x[e], acc[j], 0, 0, 0);
    }
    if constexpr ((ABL & 4) == 0) __syncthreads();
}

// ---- the MMA steps of one chunk, split-bf16: the operands hold (hi, mid) bf16 pairs in 32-bit words.  A lane takes 8 consecutive k of
// its row per 16-deep step (two ds_read_b128; lane half fh2 owns k = 8 fh2 .. 8 fh2 + 7), separates the hi and the mid halves with
// v_perm_b32 and issues v_mfma_f32_32x32x16_bf16 three times: mid*hi + hi*mid + hi*hi (the dropped mid*mid term is 2^-32 relative).
// Order of additions per output: ks, then the three products.
__device__ __forceinline__ void gemm_split_bf16(const v4u lo4, const v4u hi4, bf16x8& h, bf16x8& m) {     // 8 packed words -> 8 hi halves, 8 mid halves
    const v4u hh = {__builtin_amdgcn_perm(lo4[1], lo4[0], 0x05040100u), __builtin_amdgcn_perm(lo4[3], lo4[2], 0x05040100u),
                    __builtin_amdgcn_perm(hi4[1], hi4[0], 0x05040100u), __builtin_amdgcn_perm(hi4[3], hi4[2], 0x05040100u)};
    const v4u mm = {__builtin_amdgcn_perm(lo4[1], lo4[0], 0x07060302u), __builtin_amdgcn_perm(lo4[3], lo4[2], 0x07060302u),
                    __builtin_amdgcn_perm(hi4[1], hi4[0], 0x07060302u), __builtin_amdgcn_perm(hi4[3], hi4[2], 0x07060302u)};
    h = __builtin_bit_cast(bf16x8, hh); m = __builtin_bit_cast(bf16x8, mm);
}
template <int TN>
__device__ __forceinline__ void gemm_mma_bf16x2(v16f (&acc)[TN], const v4f* const tile, const GemmLane& l) {
    const v4u* const X = reinterpret_cast<const v4u*>(tile) + l.wid * (32 * 8) + l.fr * 8;
    const v4u* const Wt = reinterpret_cast<const v4u*>(tile) + GEMM_BM * 8 + l.fr * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int c0 = (4 * ks + 2 * l.fh2) ^ l.fsw, c1 = (4 * ks + 2 * l.fh2 + 1) ^ l.fsw;
        bf16x8 xh, xm;
        gemm_split_bf16(X[c0], X[c1], xh, xm);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bf16x8 wh, wm;
            gemm_split_bf16(Wt[j * 32 * 8 + c0], Wt[j * 32 * 8 + c1], wh, wm);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xh, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xm, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh, acc[j], 0, 0, 0);
        }
    }
}

// ---- the three-piece bf16 form ("x3"): fp32 products from six bf16 MFMAs.  V stays plain fp32 in memory and in LDS and is split in
// registers; U was split once (wino_pack_x3_kernel, winograd.hip) into three bf16 planes stored as the LDS image itself.
// THE SPLIT RULE (one rule for both operands; tests/wino_x3_model.py states the same):
//     h = x with its low 16 bits cleared (truncation: never overflows, a finite x gives a finite h)
//     m = bf16_rne(x - h)          (x - h is exact in fp32; |x - h| < 2^-7 |x|, so the rounding cannot overflow either)
//     l = bf16_rne(x - h - m)      (exact in fp32, and a multiple of x's last bit with at most 8 significant bits: the rounding is exact)
// so x = h + m + l exactly for every finite x whose pieces are zero or bf16-normal, with |m| <= 2^-7 |x| and |l| <= 2^-16 |x|.  +-Inf
// gives (Inf, NaN, NaN), NaN gives (NaN or Inf, NaN, NaN): a non-finite operand always leaves a NaN piece that meets every product.
// THE PRODUCT ORDER, per output and 16-deep step (w = weight piece, x = pixel piece), smallest first:
//     w_l x_h,  w_h x_l,  w_m x_m,  w_m x_h,  w_h x_m,  w_h x_h        (dropped: m l, l m, l l <= 2^-23 + 2^-23 + 2^-32 of |w x|)
// Order of additions per output: ks (two 16-deep steps per chunk), then the six products in this order.
typedef float v2f_ __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gemm_split3(const v4f lo4, const v4f hi4, bf16x8& h, bf16x8& m, bf16x8& l) {   // 8 fp32 -> 8 h, 8 m, 8 l
    v4u hw, mw, lw;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float a = p < 2 ? lo4[2 * p] : hi4[2 * p - 4], b = p < 2 ? lo4[2 * p + 1] : hi4[2 * p - 3];
        const unsigned ab = __builtin_bit_cast(unsigned, a), bb = __builtin_bit_cast(unsigned, b);
        hw[p] = __builtin_amdgcn_perm(bb, ab, 0x07060302u);                                               // (a's high half, b's high half)
        const v2f_ r = {a - __builtin_bit_cast(float, ab & 0xffff0000u), b - __builtin_bit_cast(float, bb & 0xffff0000u)};
        mw[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_));                       // v_cvt_pk_bf16_f32
        const v2f_ q = {r[0] - __builtin_bit_cast(float, mw[p] << 16), r[1] - __builtin_bit_cast(float, mw[p] & 0xffff0000u)};
        lw[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(q, bf16x2_));
    }
    h = __builtin_bit_cast(bf16x8, hw); m = __builtin_bit_cast(bf16x8, mw); l = __builtin_bit_cast(bf16x8, lw);
}

// The x3 tile buffer: the fp32 pixel image of the f32 tile ([128 rows][8 float4 columns], same swizzle), then three weight planes h, m, l
// of [BN rows][4 slots of 8 bf16] — slot q of row n holds k = 8 q .. 8 q + 7 of the 32-deep chunk and sits at column q ^ ((n >> 2) & 3):
// the 16 lanes of a ds_read_b128 group (rows of one residue mod 4 with four different n >> 2 & 3) then hit 64 different banks.
// 6 bytes per weight element: 128 x 64 tiles 28 KB per buffer (56 KB), 128 x 128 tiles 40 KB (80 KB: two workgroups fill a CU's 160 KB).
// The global x3 image of U is this layout for whole [rows][32 k] chunks: [frequency][plane][chunk][row][4 slots], so a wave's LDS-DMA
// request reads 1 KB of consecutive bytes.
template <int BN> constexpr int gemm_buf_slots_x3() { return GEMM_BM * 8 + 3 * BN * 4; }
template <int BN> using GemmLdsX3 = v4f[2][gemm_buf_slots_x3<BN>()];
struct GemmSrcX3 {
    const float* a;
    const v4f* b;             // this thread's 16 bytes of plane h, pass 0, current chunk
    size_t a32, bplane, bchunk;     // floats between 32-row passes of V; float4s between planes / chunks of U
    v4f* dA;
    v4f* dB;
};
// ... for the tile at row m0 of A [rows][lda] and row n0 of the x3 image B3 (one frequency) of `brows` rows and `chunks` chunks
template <int BN>
__device__ __forceinline__ GemmSrcX3 gemm_src_x3(GemmLdsX3<BN>& lds, const float* A, const int m0, const int lda, const float* B3, const int n0,
                                                 const int brows, const int chunks, const GemmLane& l) {
    return GemmSrcX3{A + (size_t)(m0 + l.lrow()) * lda + l.lqs() * 4, reinterpret_cast<const v4f*>(B3) + (size_t)n0 * 4 + l.tid, (size_t)32 * lda,
                     (size_t)chunks * brows * 4, (size_t)brows * 4, &lds[0][l.wid * 64], &lds[0][GEMM_BM * 8 + l.wid * 64]};
}
// a_live / a_dead: as gemm_load_chunk (conv_pw_x3_kernel's zero line behind K — by source address; a zero fp32 splits into three zero
// pieces).  A plane moves in passes of 64 rows (256 threads x 16 bytes); BN % 64 == 32 leaves a half pass of 32 rows, 128 float4s, which the
// waves with b_half set (the caller's wave-uniform wid < 2) request: 96-wide tiles are 18 wave requests of 1 KB per chunk, 32-wide ones 6.
template <int BN>
__device__ __forceinline__ void gemm_load_chunk_x3(GemmSrcX3& s, const int buf, const bool a_live = true, const float* const a_dead = nullptr,
                                                   const bool b_half = false) {
    v4f* const dA = s.dA + buf * gemm_buf_slots_x3<BN>();
    v4f* const dB = s.dB + buf * gemm_buf_slots_x3<BN>();
#pragma unroll
    for (int i = 0; i < GEMM_BM / 32; ++i) lds_dma16(a_live ? s.a + i * s.a32 : a_dead, dA + i * 32 * 8);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < BN / 64; ++i) lds_dma16(reinterpret_cast<const float*>(s.b + p * s.bplane + i * 256), dB + p * BN * 4 + i * 256);
        if constexpr (BN % 64 != 0) {
            if (b_half) lds_dma16(reinterpret_cast<const float*>(s.b + p * s.bplane + (BN / 64) * 256), dB + p * BN * 4 + (BN / 64) * 256);
        }
    }
    s.a += 32; s.b += s.bchunk;
}
template <int TN>
__device__ __forceinline__ void gemm_mma_x3(v16f (&acc)[TN], const v4f* const tile, const GemmLane& l) {
    constexpr int PL = TN * 32 * 4;                                          // float4 slots per weight plane
    const v4f* const X = tile + l.wid * (32 * 8) + l.fr * 8;
    const v4f* const Wt = tile + GEMM_BM * 8 + l.fr * 4;
    const int wsw = (l.fr >> 2) & 3;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int c0 = (4 * ks + 2 * l.fh2) ^ l.fsw, c1 = (4 * ks + 2 * l.fh2 + 1) ^ l.fsw;
        const int wc = (2 * ks + l.fh2) ^ wsw;
        bf16x8 xh, xm, xl, wh[TN], wm[TN], wl[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            wh[j] = __builtin_bit_cast(bf16x8, Wt[j * 32 * 4 + wc]);
            wm[j] = __builtin_bit_cast(bf16x8, Wt[PL + j * 32 * 4 + wc]);
            wl[j] = __builtin_bit_cast(bf16x8, Wt[2 * PL + j * 32 * 4 + wc]);
        }
        gemm_split3(X[c0], X[c1], xh, xm, xl);
        // (product outer, j inner: consecutive MFMAs write different accumulators; per accumulator the order is the documented one)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[j], xh, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], xl, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm[j], xm, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm[j], xh, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], xm, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[j], xh, acc[j], 0, 0, 0);
    }
}
// the K-chunk body: request the next chunk, multiply the current one, barrier (as gemm_chunk_f32)
template <int BN>
__device__ __forceinline__ void gemm_chunk_x3(v16f (&acc)[BN / 32], GemmLdsX3<BN>& lds, const int buf, const bool more, GemmSrcX3& src, const GemmLane& l) {
    if (more) gemm_load_chunk_x3<BN>(src, buf ^ 1);
    gemm_mma_x3<BN / 32>(acc, lds[buf], l);
    __syncthreads();
}

// ---- stores: a wave's 32 x (32 TN) accumulator block -> M [rows][N] as whole lines.  A lane's accumulators are 4-column pieces of
// ITS row: stored straight from registers, one instruction would write 32 bytes to each of 32 rows (a quarter of a 128-byte line
// each).  Instead the wave turns its block around in its own region of `scratch` (tile buffers the K loop's last barrier has freed;
// row pitch W + 4 floats: the 16 lanes of a b128 phase hit 64 different banks), JB 32-column blocks at a time, and stores whole rows:
// 64 / (W / 4) rows x W * 4 contiguous bytes per instruction.  The caller asserts that BYTES of scratch exist.
template <int TN, int JB>
struct GemmStore {
    static constexpr int W = JB * 32, PITCH = W + 4, RPI = 64 / (W / 4);    // columns at a time; floats per LDS row; rows per store instruction
    static constexpr int NSTORE = (TN / JB) * (32 / RPI);                   // global store instructions per wave and tile
    static constexpr size_t BYTES = 4 * 32 * PITCH * sizeof(float);
    static_assert(TN % JB == 0, "store scratch");
};
template <int TN, int JB>
__device__ __forceinline__ void gemm_store_lines(const v16f (&acc)[TN], float* const scratch, float* __restrict__ M, const int N, const int m0,
                                                 const int n0, const int wid, const int lane) {
    using S = GemmStore<TN, JB>;
    const int fr = lane & 31, fh2 = lane >> 5;
    float* const blk = scratch + wid * 32 * S::PITCH;
    const int rr = lane / (S::W / 4), cq = lane % (S::W / 4);
#pragma unroll
    for (int h = 0; h < TN / JB; ++h) {
        wave_lds_order();                                                   // (the previous round's scratch reads lie above these writes)
#pragma unroll
        for (int jj = 0; jj < JB; ++jj)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int j = h * JB + jj;
                *reinterpret_cast<v4f*>(blk + fr * S::PITCH + jj * 32 + 8 * g + 4 * fh2) = v4f{acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
            }
        wave_lds_order();                                                   // (lane (rr, cq) reads rows other lanes wrote)
        float* const obase = M + (size_t)(m0 + wid * 32 + rr) * N + n0 + h * S::W + 4 * cq;
#pragma unroll
        for (int i = 0; i < 32 / S::RPI; ++i)
            *reinterpret_cast<v4f*>(obase + (size_t)i * S::RPI * N) = *reinterpret_cast<const v4f*>(blk + (rr + i * S::RPI) * S::PITCH + 4 * cq);
    }
}

}  // namespace fh
