// conv_mfma.hip — dense convolution (3x3 / 1x1, stride 1|2) and the final FC as an implicit GEMM
// on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 (gfx950 / CDNA4).
//
// What it replaces: the Conv / Gemm nodes ONNX Runtime executes inside `session_->Run`
// (reference src/face_recognizer.cpp:279-283, src/face_detector.cpp:179-183), with the
// following BatchNormalization / PRelu / Relu / Sigmoid / Add nodes fused into the epilogue.
//
// GEMM view:  M = B*Ho*Wo pixels, N = Cout, K = ks*ks*Cin with k = tap*Cin + ci.
// Activations are channels-last, so a K-chunk of 32 consecutive k is 128 contiguous bytes of
// one input pixel: every global load is a full 16-byte lane access and 8 lanes cover one line.
//
// Tile anatomy (256 threads = 4 waves, >= 2 workgroups per CU):
//   * global -> LDS directly (LDS-DMA, global_load_lds_dwordx4: no staging registers, no
//     ds_write), double buffered; one barrier per 32-deep K chunk.  Padding, ragged M and ragged
//     K are resolved by redirecting the lane's source address to a zero line (no branches).
//   * LDS image [row][32 k] with the 16-byte column XOR-swizzled by (row>>1)&7, which makes the
//     ds_read_b128 fragment reads of 32 different rows conflict-free (MI355X_MICROARCH.md §LDS).
//   * each lane fetches 4 consecutive k of its row with ONE ds_read_b128 and feeds 4 MFMAs; the
//     k-order inside a chunk is therefore permuted identically for both operands, which a dot
//     product does not care about.  A wave tile of 64x64 needs 4 ds_read_b128 per 16 MFMAs;
//     the fragments of the next 8-deep step are fetched while the current 16 MFMAs issue.
//   * the MFMA's A operand is the WEIGHT fragment and B the PIXEL fragment, so a lane ends up
//     with one pixel and, per accumulator quad, 4 consecutive output channels: the epilogue
//     moves float4s (residual in, output out, second output out).
//   * epilogue: bias -> activation -> (+ residual, optionally through a 2x nearest up-sampling)
//     -> store, plus an optional second output  y*s2 + t2  (the next block's pre-conv BN).
//
// Work distribution ("stream-K remainder"): with T tiles and S workgroups resident on the chip,
// the first floor(T/S)*S tiles are computed one per workgroup.  The remaining R < S tiles would
// leave S-R slots idle, so their K range is cut: R OWNER workgroups compute the first q_o chunks
// of their tile, H <= S-R HELPER workgroups (lower block indices, so they are dispatched first)
// share the other chunks evenly, each covering a contiguous run that may span several tiles.
// A helper stores its raw accumulators to a slab and publishes it (agent-scope release + one
// counter add per tile); the owner polls its tile's counter, acquires, adds the <= 3 slabs in K
// order and runs the epilogue — deterministic, no float atomics, no second kernel.  When a tile
// would need more than 3 slabs (the 25088-deep FC as split-K, tiny remainders) there are no
// owners: every segment goes to a slab and conv_fixup_kernel sums them in a second launch.
//
// Where the pieces live: conv_tile.h — tile shape, activation, the epilogue's vectors (ConvEpVec), the slab address rule and the
// epilogue with its four forms (and why conv_igemm_kernel keeps some of it written out); conv_plan.h — every launch decision (stream-K split, conv_tall_kernel / conv_pw_kernel take-over, tile
// config, environment switches) as host arithmetic.  This file: the kernels' loaders, K loops and stream-K roles, and the launchers.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "conv_tile.h"
#include "kernels.h"

namespace fh {

// GRP: grouped form (several GEMMs stacked along M with one weight matrix each, see ConvArgs::wt_group_rows) — a separate
// instantiation, so that the ungrouped convolutions keep their register allocation.
// SC: with the folded-shortcut tap (ConvArgs::sc_in) — its own instantiation for the same reason.
// X3: the K loop on three bf16 pieces and six v_mfma_f32_32x32x16_bf16 per 16-deep step (gemm_tile.h, "x3": fp32 products, 0.375 of the
// f32 instruction's matrix-pipe cycles) — its own instantiations again.  The tile is the x3 GEMM's: 128 x BN, four waves of 32 pixel rows
// x BN channels (Tile<128, BN, 4, 1>), so gemm_mma_x3 and GemmLane apply as they are.  The pixel operand is the fp32 LDS image below,
// filled by the same tap_setup / load_chunk (zero line, tenth tap) and split in registers; p.wt is the x3 image of the [rows][Kpad]
// weights (launch_pack_x3 with one frequency: [plane][chunk][row][4 slots], rows = conv_wt_rows(Cout)), fetched as gemm_load_chunk_x3
// fetches U.  Everything around the K loop — roles, slabs, hand-off, epilogue — is the f32 kernel's.
// Order of additions per output: chunks in K order (tap-major, the shortcut tap last), then the two 16-deep steps of a chunk, then the
// six products in gemm_tile.h's order; with stream-K the owner's chunks first, then the helpers' slabs in K order.  Deterministic.
template <int BM, int BN, int WM, int WN, int OCC, bool FAST, bool GRP, bool SC = false, bool X3 = false>
__global__ __launch_bounds__(WM * WN * 64, OCC) void conv_igemm_kernel(const ConvArgs p_by_value, const int tiles_n, const int chunks) {
    static_assert(!X3 || (FAST && !GRP && BM == GEMM_BM && WM == 4 && WN == 1 && BN % 64 == 0), "x3 K loop: the x3 GEMM's tile only");
    // The argument block is read where it already lies — the kernarg segment (constant address space, scalar loads) — instead of
    // through the by-value parameter: clang materialises that one as a private copy which the optimiser usually removes again, and when
    // it does not (it stopped doing so when this kernel grew the folded-shortcut tap) all 384 bytes live in scratch memory and every
    // field access becomes a scratch load: -25 % on every convolution.
    // (the instantiations without that tap keep the by-value form: there the copy is optimised away and the fields sit in SGPRs)
    // (the x3 instantiations read it there too, with or without the tap: by value the one without spilled 141 SGPRs instead of 65)
    const ConvArgs& p = SC || X3 ? *(const ConvArgs*)__builtin_amdgcn_kernarg_segment_ptr() : p_by_value;      // first explicit argument = offset 0
    using TL = Tile<BM, BN, WM, WN>;
    constexpr int TM = TL::TM, TN = TL::TN, RP = TL::RP, AL = TL::AL, BL = TL::BL;
    constexpr int BUF = X3 ? gemm_buf_slots_x3<BN>() : (BM + BN) * 8;      // float4 slots per tile buffer
    __shared__ v4f lds[2][BUF];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform by construction: keep it scalar
    const int wm = wid / WN, wn = wid % WN;
    const int HoWo = p.Ho * p.Wo;
    const int M = p.B * HoWo;
    const int Ktot = p.ks * p.ks * p.Cin;
    const int lrow = tid >> 3;
    const int lqs = (tid & 7) ^ ((lrow >> 1) & 7);      // source k-column of this lane (swizzle on the source side)
    const int fr = lane & 31, fh2 = lane >> 5;
    const int fsw = (fr >> 1) & 7;

    // ---- which tile(s) and which K range: plain tiles first, then helpers, then owners — each group in XCD-contiguous order (xcd_tile),
    // so that the tiles_n workgroups that read the same pixels (and the neighbours that share their halo rows) hit the same L2
    enum { PLAIN = 0, HELPER = 1, OWNER = 2 };
    int role = PLAIN, tile = 0, c_begin = 0, c_end = chunks;
    int hu = 0, hu_end = 0, helper_id = 0;                  // helper: its run of units [hu, hu_end)
    const int Kh = chunks - p.sk_owner_chunks;              // chunks per remainder tile that helpers compute
    if ((int)blockIdx.x < p.sk_full) {
        tile = xcd_tile((int)blockIdx.x, p.sk_full);
    } else if ((int)blockIdx.x < p.sk_full + p.sk_helpers) {
        role = HELPER;
        helper_id = xcd_tile((int)blockIdx.x - p.sk_full, p.sk_helpers);
        hu = helper_id * p.sk_q;
        hu_end = min(p.sk_units, hu + p.sk_q);
    } else {
        role = OWNER;
        tile = p.sk_full + xcd_tile((int)blockIdx.x - p.sk_full - p.sk_helpers, p.sk_rem);
        c_end = p.sk_owner_chunks;
    }
    unsigned* const sk_counters = reinterpret_cast<unsigned*>(p.slabs + SK_SLAB_FLOATS);
    // stream-K owner: "my hand-off wait timed out" flag.  The LAST word of the LDS images (free once the K loop is over, and beyond the
    // 12 * BN floats the epilogue parks there) — a variable of its own would cost the 256x64 / 128x32 tiles a workgroup per CU
    // (their images fill 80 / 40 KB exactly).
    volatile int* const sk_gave_up = reinterpret_cast<volatile int*>(&lds[1][0]) + (BUF * 4 - 1);

    do {
        int part = 0;
        if (role == HELPER) {                               // next segment of this helper's run
            const int r = hu / Kh, off = hu - r * Kh;
            const int len = min(Kh - off, hu_end - hu);
            tile = p.sk_full + r;
            c_begin = p.sk_owner_chunks + off; c_end = c_begin + len;
            part = helper_id - (r * Kh) / p.sk_q;           // position among the helpers that touch this tile
            hu += len;
        }
        const int gtile = tile + p.tile0;                   // (tile0 > 0: the first tiles of this convolution ran in conv_tall_kernel)
        const int tile_n = gtile % tiles_n, tile_m = gtile / tiles_n;
        const int m0 = tile_m * BM, n0 = tile_n * BN;
        // grouped form (Winograd's 36 GEMMs stacked along M, wt_group_rows rows each, a multiple of BM): only the weight
        // matrix depends on the group — inputs and outputs are one tall matrix
        const float* g_wt = p.wt;
        if (GRP && p.wt_group_rows > 0) g_wt += (size_t)(m0 / p.wt_group_rows) * p.wt_gs;

        // ---- loader bookkeeping.  LDS-DMA (global_load_lds_dwordx4) writes lane l of a wave at
        // wave-uniform base + 16*l, i.e. pass i of wave `wid` fills rows i*RP + wid*8 + (l>>3), 16-byte
        // column l&7 — the LDS image stays lane-linear and the XOR swizzle is applied to the SOURCE:
        // the lane fetches k-column (l&7) ^ ((row>>1)&7)  (cdna_hip_programming.md §5.4 rule 21).
        // (x3: the register file is full — a row's pixel is kept as a 32-bit element offset, launch_conv bounds the tensors to 2^31
        //  elements, and the shortcut's pixel is worked out again from the row index when the tenth tap begins, once per tile)
        const float* a_ptr[X3 ? 1 : AL];
        int a_off[X3 ? AL : 1];                             // (x3: float offset of the row's first input pixel from p.in, swizzled column included)
        const float* sc_ptr[X3 ? 1 : AL];                   // folded shortcut (ConvArgs::sc_in): this row's pixel of the 1x1 convolution's input
        unsigned a_mask[AL];
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int m = m0 + lrow + i * RP;
            a_ptr[X3 ? 0 : i] = p.zeros; a_off[X3 ? i : 0] = 0; a_mask[i] = 0; sc_ptr[X3 ? 0 : i] = p.zeros;
            if (p.ks == 1 && p.stride == 1) {               // plain GEMM rows (1x1 convs, FC, gallery): no pixel arithmetic at all
                if (m < M) { a_ptr[X3 ? 0 : i] = p.in + (long)m * p.Cin + lqs * 4; a_off[X3 ? i : 0] = m * p.Cin + lqs * 4; a_mask[i] = 1u; }
            } else if (m < M) {
                const int n = m / HoWo, rem = m - n * HoWo;
                const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
                const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
                a_ptr[X3 ? 0 : i] = p.in + (long)(((n * p.H + iy0) * p.W + ix0) * p.Cin) + lqs * 4;
                a_off[X3 ? i : 0] = ((n * p.H + iy0) * p.W + ix0) * p.Cin + lqs * 4;
                if (SC && !X3) sc_ptr[i] = p.sc_in + (long)(((n * p.sc_H + oy * p.sc_stride) * p.sc_W + ox * p.sc_stride) * p.sc_C) + lqs * 4;
                unsigned mk = 0;
                if (p.ks == 3) {
#pragma unroll
                    for (int t = 0; t < 9; ++t)
                        if ((unsigned)(iy0 + t / 3) < (unsigned)p.H && (unsigned)(ix0 + t % 3) < (unsigned)p.W) mk |= 1u << t;
                } else {
                    mk = 1u;
                }
                a_mask[i] = mk;
            }
        }
        // weights: wave-uniform base that advances 128 B per chunk + a constant 32-bit lane offset
        // (lets the loads use the scalar-base addressing form: no per-chunk vector pointer math)
        const char* w_base = reinterpret_cast<const char*>(g_wt) + ((size_t)n0 * p.Kpad + (size_t)c_begin * 32) * 4;
        unsigned w_off[BL];
#pragma unroll
        for (int i = 0; i < BL; ++i) w_off[i] = (unsigned)(((lrow + i * RP) * p.Kpad + lqs * 4) * 4);
        // x3: this thread's 16 bytes of plane h of the current chunk (a plane of one chunk and tile is BN * 64 consecutive bytes)
        const int w3_rows = X3 ? (p.Cout + 127) / 128 * 128 : 0;                          // (= conv_wt_rows(Cout), the image's row count)
        const v4f* w3 = reinterpret_cast<const v4f*>(g_wt) + ((size_t)c_begin * w3_rows + n0) * 4 + tid;
        const size_t w3_plane = (size_t)chunks * w3_rows * 4, w3_chunk = (size_t)w3_rows * 4;

        const unsigned long long zero_addr = (unsigned long long)p.zeros + (unsigned long long)(lane & 0) ;
        v4f* const dstA = &lds[0][wid * 64];               // + buf*(BM+BN)*8 + i*RP*8; the hardware adds 16*lane
        v4f* const dstB = &lds[0][BM * 8 + wid * 64];
        // FAST path (Cin % 32 == 0): a chunk never straddles a tap, so tap / channel position are
        // scalars that advance incrementally and the per-row source pointers are only rebuilt
        // (valid tap -> real address, padded tap -> zero line) when the tap changes.
        int ld_tap = 0, ld_ci = 0;
        const float* cur[AL];
        int adv[AL];                                        // floats a row's pointer advances per chunk: 32, or 0 while it reads the zero line
        // (loop-carried uses of the argument block go through locals: `p` lives in memory and every barrier / asm memory clobber in
        //  the K loop would otherwise re-fetch the field — an s_load + lgkmcnt wait per chunk)
        const int Cin = p.Cin, ksz = p.ks, inW = p.W;
        const int taps = ksz * ksz;
        auto tap_setup = [&]() __attribute__((always_inline)) {                            // (a dead row of the 25 088-deep FC would otherwise walk 100 KB past the 8 KiB of zeros)
            if (ld_tap >= taps) {                           // past the own taps: the folded shortcut's pixels (ConvArgs::sc_in)
                if (!SC) return;
#pragma unroll
                for (int i = 0; i < AL; ++i) {
                    const bool on = a_mask[i] != 0;
                    const float* sp = sc_ptr[X3 ? 0 : i];
                    if constexpr (X3) {                     // (a_mask != 0: the row is a real pixel, m < M)
                        const int m = m0 + lrow + i * RP;
                        const int n = m / HoWo, rem = m - n * HoWo, oy = rem / p.Wo, ox = rem - oy * p.Wo;
                        sp = p.sc_in + (long)(((n * p.sc_H + oy * p.sc_stride) * p.sc_W + ox * p.sc_stride) * p.sc_C) + lqs * 4;
                    }
                    cur[i] = (const float*)(on ? (unsigned long long)(sp + ld_ci) : zero_addr);
                    adv[i] = on ? 32 : 0;
                }
                return;
            }
            const int ky = ld_tap / 3, kx = ld_tap - ky * 3;
            const int toff = (ksz == 3 ? (ky * inW + kx) * Cin : 0) + ld_ci;
#pragma unroll
            for (int i = 0; i < AL; ++i) {
                const unsigned long long real = (unsigned long long)(X3 ? p.in + (a_off[X3 ? i : 0] + toff) : a_ptr[X3 ? 0 : i] + toff);
                const bool on = ((a_mask[i] >> ld_tap) & 1u) != 0;
                cur[i] = (const float*)(on ? real : zero_addr);
                adv[i] = on ? 32 : 0;
            }
        };
        if (FAST) {
            ld_tap = min((c_begin * 32) / Cin, taps);
            ld_ci = c_begin * 32 - ld_tap * Cin;
            tap_setup();
        }
        auto load_chunk = [&](int kc, int buf) __attribute__((always_inline)) {
            v4f* const dA = dstA + buf * BUF;
            v4f* const dB = dstB + buf * BUF;
            if (FAST) {
#pragma unroll
                for (int i = 0; i < AL; ++i) { lds_dma16(cur[i], dA + i * RP * 8); cur[i] += adv[i]; }
                if constexpr (X3) {                         // (as gemm_load_chunk_x3)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                        for (int i = 0; i < BN / 64; ++i) lds_dma16(reinterpret_cast<const float*>(w3 + pl * w3_plane + i * 256), dB + pl * BN * 4 + i * 256);
                    w3 += w3_chunk;
                } else {
#pragma unroll
                for (int i = 0; i < BL; ++i) lds_dma16(reinterpret_cast<const float*>(w_base + w_off[i]), dB + i * RP * 8);
                w_base += 128;
                }
                ld_ci += 32;
                if (ld_ci >= Cin && ld_tap < taps) { ld_ci = 0; ++ld_tap; tap_setup(); }      // wave-uniform branch
                return;
            }
            const int kb = kc * 32;
            int tap, toff;                               // toff: float offset of this lane's 4 channels from a_ptr
            if (ksz == 1) { tap = 0; toff = kb; }
            else {
                const int k4 = kb + lqs * 4;
                tap = k4 / Cin;
                const int ci = k4 - tap * Cin;
                const int ky = tap / 3, kx = tap - ky * 3;
                toff = (ky * inW + kx) * Cin + ci - lqs * 4;
            }
            const bool kvalid = kb + lqs * 4 < Ktot;
#pragma unroll
            for (int i = 0; i < AL; ++i) {
                // integer select (v_cndmask), not a branch: border lanes read the zero line
                const unsigned long long real = (unsigned long long)(a_ptr[X3 ? 0 : i] + toff);
                const unsigned long long sel = (kvalid && ((a_mask[i] >> tap) & 1u)) ? real : zero_addr;
                lds_dma16((const float*)sel, dA + i * RP * 8);
            }
#pragma unroll
            for (int i = 0; i < BL; ++i) lds_dma16(reinterpret_cast<const float*>(w_base + w_off[i]), dB + i * RP * 8);
            w_base += 128;
        };

        v16f acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        // the epilogue's per-channel vectors: no global read is left for the epilogue to wait on
        const bool use_ep = role != HELPER && p.n_outs == 0 && (p.Cout & 3) == 0;
        using EpVec = ConvEpVec<BN, TL::T>;                  // (its layout; the two loops are written out here, see conv_tile.h)
        float epv[EpVec::N];
#pragma unroll
        for (int k = 0; k < EpVec::N; ++k) {
            const int e = tid + k * TL::T, a = e / BN, c = e - a * BN, co = n0 + c;
            float v = 0.f;
            if (use_ep && a < EP_ROWS && co < p.Cout) {
                if (a < EP_SLOPE) { if (p.bias && (a == 0 || p.bias_cls)) v = p.bias[a * p.Cout + co]; }
                else if (a == EP_SLOPE) { if (p.act == (int)Act::PRELU) v = p.slope[co]; }
                else if (p.out2) v = a == EP_S2 ? p.s2[co] : p.t2[co];
            }
            epv[k] = v;
        }

        auto compute = [&](int buf) {
            if constexpr (X3) {
                gemm_mma_x3<TN>(acc[0], lds[buf], GemmLane{tid, lane, wid, fr, fh2, fsw});
                return;
            }
            const v4f* X = lds[buf] + (wm * TM * 32 + fr) * 8;
            const v4f* Wt = lds[buf] + BM * 8 + (wn * TN * 32 + fr) * 8;
            v4f x[2][TM], w[2][TN];
            {
                const int col = fh2 ^ fsw;
#pragma unroll
                for (int i = 0; i < TM; ++i) x[0][i] = X[i * 32 * 8 + col];
#pragma unroll
                for (int j = 0; j < TN; ++j) w[0][j] = Wt[j * 32 * 8 + col];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int cur = s & 1, nxt = cur ^ 1;
                if (s < 3) {
                    const int col = (2 * (s + 1) + fh2) ^ fsw;
#pragma unroll
                    for (int i = 0; i < TM; ++i) x[nxt][i] = X[i * 32 * 8 + col];
#pragma unroll
                    for (int j = 0; j < TN; ++j) w[nxt][j] = Wt[j * 32 * 8 + col];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cur][j][e], x[cur][i][e], acc[i][j], 0, 0, 0);
            }
        };

        if (c_begin < c_end) {
            load_chunk(c_begin, 0);
            __syncthreads();                              // (drains vmcnt: the DMA of chunk 0 has landed)
            for (int kc = c_begin, it = 0; kc < c_end; ++kc, ++it) {
                const int buf = it & 1;
                if (kc + 1 < c_end) load_chunk(kc + 1, buf ^ 1);
                compute(buf);
                __syncthreads();                          // all reads of `buf` done, DMA into buf^1 landed
            }
        }

        if (role == HELPER) {
            const int r = tile - p.sk_full;
            float* __restrict__ slab = conv_slab<TL>(p, r, part);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        v4f v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                        *reinterpret_cast<v4f*>(slab + conv_slab_at<TL>(i * TN + j, g, tid)) = v;
                    }
            if (p.sk_owner_chunks > 0) {
                // publish (cdna_hip_programming.md Guideline 16, counter form): every wave drains its stores,
                // barrier, ONE lane releases at agent scope, waits, then bumps the tile's counter
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0 && !p.sk_test_drop) {          // (sk_test_drop: the watchdog test's lost publication)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_fetch_add(sk_counters + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            continue;
        }
        if (role == OWNER) {
            const int r = tile - p.sk_full;
            const int nparts = conv_sk_nparts(r, Kh, p.sk_q);
            if (tid == 0) {                              // ONE lane polls relaxed, then ONE acquire
                // Bounded wait: forward progress rests on helpers (lower block indices) being dispatched before owners, which HIP
                // does not promise.  Past sk_timeout (default 2 s of the constant 100 MHz clock — five orders of magnitude beyond any
                // real wait) the owner gives up: it reports (tile, arrivals seen, arrivals expected) through its Net's host-visible
                // error record, leaves its tile unwritten and exits, so that the launch drains and the next call on that handle
                // returns FH_ERR_DEVICE instead of the process hanging with the GPU lease.
                const unsigned long long t0 = wall_clock64();
                unsigned seen, spins = 0;
                bool arrived = true;
                while ((seen = __hip_atomic_load(sk_counters + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != (unsigned)nparts) {
                    __builtin_amdgcn_s_sleep(4);
                    if ((++spins & 255u) == 0 && ((wall_clock64() - t0) >> 16) > (unsigned long long)p.sk_timeout) { arrived = false; break; }
                }
                if (arrived) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(sk_counters + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
                } else if (p.sk_err) {
                    __hip_atomic_store(p.sk_err + 1, (unsigned)tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(p.sk_err + 2, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(p.sk_err + 3, (unsigned)nparts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(p.sk_err + 0, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                *sk_gave_up = arrived ? 0 : 1;
            }
            __syncthreads();
            if (*sk_gave_up) return;                        // (workgroup-uniform; an owner runs exactly one tile)
            for (int q = 0; q < nparts; ++q) {              // K order: own chunks first, then the helpers' runs
                const float* slab = conv_slab<TL>(p, r, q);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const v4f v = *reinterpret_cast<const v4f*>(slab + conv_slab_at<TL>(i * TN + j, g, tid));
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[i][j][4 * g + c] += v[c];
                        }
            }
        }
        float* const ep = reinterpret_cast<float*>(&lds[0][0]);            // (every wave is past the K loop's last barrier: LDS is free)
        if (use_ep) {
#pragma unroll
            for (int k = 0; k < EpVec::N; ++k) {
                const int e = tid + k * TL::T;
                if (e < EpVec::FLOATS) ep[e] = epv[k];
            }
            __syncthreads();
        }
        // (the transposition scratch of the whole-line epilogue sits behind the vectors: both fit the tile buffers of every shape)
        static_assert((EpVec::FLOATS + WM * WN * 32 * 36) * sizeof(float) <= sizeof(lds), "epilogue scratch");
        // (x3: launch_conv_x3 admits Cout % 64 == 0 without merged outputs and launch_cfg pins ep_direct to 0 — the whole-line form alone)
        conv_epilogue<BM, BN, WM, WN, X3 ? EP_LINES : EP_ALL>(p, acc, m0, n0, wm, wn, lane, -1, -1, use_ep ? ep : nullptr,
                                                             use_ep && conv_ep_wants_lines(p) ? ep + EpVec::FLOATS : nullptr);
    } while (role == HELPER && hu < hu_end);
}

// Owner-less form: sums the slabs of one remainder tile in K order and applies the epilogue.  One workgroup
// per (tile, 32x32 accumulator block of each wave): TM*TN times more workgroups than tiles, because this
// kernel is pure streaming and R < #CUs*2 tiles alone would leave most of the chip's load queues empty.
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void conv_fixup_kernel(const ConvArgs p, const int tiles_n, const int chunks) {
    using TL = Tile<BM, BN, WM, WN>;
    constexpr int TM = TL::TM, TN = TL::TN;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int r = blockIdx.x / (TM * TN);               // remainder tile index
    const int sub = blockIdx.x - r * (TM * TN);
    const int si = sub / TN, sj = sub - si * TN;
    const int tile = p.sk_full + r;
    const int nparts = conv_sk_nparts(r, chunks, p.sk_q);   // (no owners: the helpers compute all of a tile's chunks)
    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    v16f sum;
#pragma unroll
    for (int e = 0; e < 16; ++e) sum[e] = 0.f;
    for (int q = 0; q < nparts; ++q) conv_slab_add<TL>(conv_slab<TL>(p, r, q), sum, si * TN + sj, tid);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
            if (i == si && j == sj) acc[i][j] = sum;
    const int gtile = tile + p.tile0;                       // (see conv_igemm_kernel)
    const int tile_n = gtile % tiles_n, tile_m = gtile / tiles_n;
    conv_epilogue<BM, BN, WM, WN, EP_MERGED | EP_PLAIN>(p, acc, tile_m * BM, tile_n * BN, wm, wn, lane, si, sj);
}

int conv_wt_rows(int Cout) { return (Cout + 127) / 128 * 128; }

// Packs plan-layout weights w[Cout][taps][Cin] into the kernel's [rows][Kpad] image, k = tap*Cin + ci.
// (A tap-inner order, k = (ci/32)*288 + tap*32 + ci%32, was measured: it turns the 9x input re-read
// into L1/L2 hits but needs the per-row source pointers rebuilt every chunk instead of every
// Cin/32 chunks, and those extra VALU instructions cost more than the cache hits gain: -3 %.)
void conv_pack_weights(const float* w, int Cout, int Cin, int ks, float* dst) {
    const int taps = ks * ks, Ktot = taps * Cin, Kpad = conv_kpad(Ktot);
    for (int co = 0; co < Cout; ++co)
        for (int k = 0; k < Ktot; ++k) dst[(size_t)co * Kpad + k] = w[(size_t)co * Ktot + k];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// conv_tall_kernel (round 3) — 3x3 stride-1 pad-1 convolutions with Cin % 32 == 0 on maps up to 112 wide: ONE LDS image per 32-channel
// chunk serves all nine taps.
//
// conv_igemm_kernel gathers a fresh A tile per (tap, chunk): 256 rows x 128 B nine times per 32 channels, although the nine tiles are
// the same pixels shifted — for the row-linear tile [m0, m0 + BM) tap (ky, kx) reads pixel m + (ky - 1) W + (kx - 1).  What that costs is
// not bytes (they come from L2) but ISSUE: each 1 KB LDS-DMA piece takes its wave 60-185 cycles, 40 pieces per 64 MFMAs and wave for the
// 256x64 tile — the kernel that runs IResNet's stage 1 (Cin = 64: 2.2 ms of the 12.8 ms step) at 105-112 TFLOP/s where the 128x128
// tile of the wider layers reaches 117-123.  Here the A image holds the BM + 2 W + 2 consecutive pixels m0 - W - 1 .. m0 + BM + W of
// ONE 32-channel chunk (482 rows = 61.7 KB at W = 112, beside the 16 KB weight double buffer: still two workgroups per CU) and the nine
// taps are nine row-shifted views of it: fragment row = tile row + ky W + kx.  A traffic / 4.8, LDS-DMA pieces per MFMA / 2.6.
//   * K order: chunk-major (for each 32-channel chunk: nine taps); the weight chunk of (chunk c, tap t) sits at k = t Cin + 32 c of the
//     packed row, so only an address changes.
//   * a shifted view reads a REAL neighbour where the convolution pads with zero (left / right image border, first / last row, and the
//     pixels of the neighbouring image across a batch boundary): every lane carries a 9-bit validity mask of its fragment pixel per
//     32-row block and zeroes the fragment with v_cndmask (a select, not a multiply: the neighbour may hold anything).  Image rows
//     outside the tensor come from the zero line.
//   * swizzle: 16-byte column ^ ((LDS row >> 1) & 7), on the source side as in conv_igemm_kernel; a view's key is that of its shifted row.
//   * tiles are row-linear as in conv_igemm_kernel, so conv_epilogue (9 bias classes, PReLU, residual, second output) is shared and
//     nothing is wasted on maps that are no multiple of a spatial tile (56 = 3.5 x 16).
//   * no stream-K here: launch_cfg gives this kernel the whole ROUNDS of tiles and the remainder (tile0 = the first one) to
//     conv_igemm_kernel, whose owner / helper hand-off cuts those few tiles' K range over the whole chip.
template <int BM, int BN, int WM, int WN, int OCC>
__global__ __launch_bounds__(WM * WN * 64, OCC) void conv_tall_kernel(const ConvArgs p, const int tiles_n, const int rows_a) {
    using TL = Tile<BM, BN, WM, WN>;
    constexpr int TM = TL::TM, TN = TL::TN, RP = TL::RP, BL = TL::BL;
    constexpr int NPMAX = (BM + 2 * 112 + 2 + RP - 1) / RP;                // loader passes of the tallest image (W = 112)
    extern __shared__ v4f tsm[];
    v4f* const As = tsm;                                                   // [rows_a][8 float4], rows_a = whole loader passes
    v4f* const Bs = tsm + (size_t)rows_a * 8;                              // [2][BN][8]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;
    const int W = p.W, HW = p.H * p.W, Cin = p.Cin;
    const int M = p.B * HW;
    const int lrow = tid >> 3;
    const int lqs = (tid & 7) ^ ((lrow >> 1) & 7);                         // (RP % 16 == 0: the key of row i * RP + lrow is that of lrow)
    const int fr = lane & 31, fh2 = lane >> 5;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tile_n = tile % tiles_n, tile_m = tile / tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int np = rows_a / RP;

    // ---- A image loader: pass i fills LDS rows i * RP + lrow <- pixel m0 - W - 1 + row (all of one 32-channel chunk, this lane's column)
    const float* a_ptr[NPMAX];
#pragma unroll
    for (int i = 0; i < NPMAX; ++i) {
        const long q = (long)m0 - W - 1 + i * RP + lrow;
        a_ptr[i] = (i < np && q >= 0 && q < M) ? p.in + q * Cin + lqs * 4 : p.zeros;
    }
    int a_adv[NPMAX];
#pragma unroll
    for (int i = 0; i < NPMAX; ++i) a_adv[i] = a_ptr[i] == p.zeros ? 0 : 32;      // (rows that read the zero line do not walk off it)
    const char* w_tile = reinterpret_cast<const char*>(p.wt) + (size_t)n0 * p.Kpad * 4;
    unsigned w_off[BL];
#pragma unroll
    for (int i = 0; i < BL; ++i) w_off[i] = (unsigned)(((lrow + i * RP) * p.Kpad + lqs * 4) * 4);
    v4f* const dstA = As + wid * 64;
    v4f* const dstB = Bs + wid * 64;
    auto load_b = [&](int c, int tap, int buf) __attribute__((always_inline)) {
        const char* wb = w_tile + (size_t)(tap * Cin + c * 32) * 4;
#pragma unroll
        for (int i = 0; i < BL; ++i) lds_dma16(reinterpret_cast<const float*>(wb + w_off[i]), dstB + buf * (BN * 8) + i * RP * 8);
    };

    // ---- fragment views: block i of this wave = tile rows (wm TM + i) 32 + fr; validity of the nine taps of that pixel
    unsigned vmask[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + (wm * TM + i) * 32 + fr;
        unsigned mk = 0;
        if (m < M) {
            const int rem = m % HW, oy = rem / W, ox = rem - oy * W;
#pragma unroll
            for (int t = 0; t < 9; ++t)
                if ((unsigned)(oy + t / 3 - 1) < (unsigned)p.H && (unsigned)(ox + t % 3 - 1) < (unsigned)W) mk |= 1u << t;
        }
        vmask[i] = mk;
    }
    v16f acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    ConvEpVec<BN, TL::T> epv;                                              // the epilogue's per-channel vectors, parked in LDS after the K loop
    epv.fetch(p, n0, tid, true);

    const int NC = Cin >> 5;
    const int rbase = (wm * TM * 32 + fr);                                 // this lane's row in the tile (block 0)
    for (int c = 0; c < NC; ++c) {
        __syncthreads();                                                   // every wave is done with the previous chunk's image and weight buffers
        for (int i = 0; i < np; ++i) { lds_dma16(a_ptr[i < NPMAX ? i : 0], dstA + i * RP * 8); }
#pragma unroll
        for (int i = 0; i < NPMAX; ++i) a_ptr[i] += a_adv[i];
        load_b(c, 0, 0);
        __syncthreads();                                                   // (drains vmcnt: image + first weight chunk have landed)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int buf = tap & 1;
            if (tap + 1 < 9) load_b(c, tap + 1, buf ^ 1);
            const int shift = (tap / 3) * W + tap % 3;
            const int r0 = rbase + shift;                                  // LDS row of block 0's fragment pixel under this tap
            const int key = (r0 >> 1) & 7;                                 // (block i adds 32 i rows: same key)
            const v4f* X = As + r0 * 8;
            const v4f* Wt = Bs + buf * (BN * 8) + (wn * TN * 32 + fr) * 8;
            const int wkey = (fr >> 1) & 7;
            bool ok[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) ok[i] = (vmask[i] >> tap) & 1u;
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                v4f x[TM], w[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    x[i] = X[i * 32 * 8 + ((2 * s2 + fh2) ^ key)];
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[i][e] = ok[i] ? x[i][e] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) w[j] = Wt[j * 32 * 8 + ((2 * s2 + fh2) ^ wkey)];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j][e], x[i][e], acc[i][j], 0, 0, 0);
            }
            if (tap + 1 < 9) __syncthreads();                              // next weight chunk landed; everyone done with this one
        }
    }
    __syncthreads();                                                       // K loop over: LDS is free
    float* const ep = reinterpret_cast<float*>(Bs);
    epv.park(ep, tid);
    __syncthreads();
    conv_epilogue<BM, BN, WM, WN, EP_MERGED | EP_QUADS>(p, acc, m0, n0, wm, wn, lane, -1, -1, ep);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// conv_pw_kernel (round 3) — 1x1 stride-1 convolutions as the plain GEMM they are: out [M][N] = in [M][K] * W^T.
// conv_igemm_kernel spends ~650 vector + ~490 scalar instructions per wave on tap / padding / index bookkeeping around the MFMAs of a
// short-K tile (that is why the Winograd GEMMs got wino_gemm_kernel); SCRFD's 1x1 convolutions (K = 72 / 152 / 288, 0.8 ms of the
// detector at B = 128) and MobileFaceNet's ran at 65-88 TFLOP/s in it.  Here: the lean GEMM tile of gemm_tile.h — rows are contiguous, a lane's
// source address only advances by 32 floats per chunk — with a zero-line source for the float4 columns behind K in the last chunk
// (K % 4 == 0, any remainder), 128 x BN tiles with BN = 96 (N = 288: three exact column tiles) / 64 / 32, and the shared
// conv_epilogue (bias, ReLU / PReLU, residual incl. the FPN's 2x upsampled one, second output) with its vectors parked in LDS.
// M % 128 == 0 (whole tiles) and at least one tile per CU, else launch_conv keeps the generic kernel and its stream-K.
#ifdef FACEHIP_PW_ABL
// Diagnostic build (scripts/pw_ablate.sh, scripts/pw_phases.py; an ablated run's results are garbage).  ABL = the loop masks of
// gemm_chunk_f32 (1 = no loads in the K loop, 2 = no LDS reads, 4 = no barriers in the K loop), chosen by launch_pw_cfg from the low bits
// of FACEHIP_PW_ABL; the higher bits stay run-time, in p.sk_test_drop: 8 = no epilogue, 16 = epilogue stores from one lane only,
// 32 = the CU's second workgroup starts (bits 8..) x 0.64 us late, 64 = wait for the stores' acknowledgement before the last stamp.
// Phase stamps (100 MHz ticks) of the 20x20x288 layers go to the stream-K workspace: [workgroup][entry, first chunk landed, K loop
// done, epilogue done] and, from 8192 on, [workgroup][epilogue entry, first block in LDS, last store issued, ep vectors parked].
// (Only this build has the third parameter: the kernel's name in the production build is what the profiles and scripts key on.)
template <int BN, int OCC, int ABL = 0>
#else
template <int BN, int OCC>
#endif
__global__ __launch_bounds__(256, OCC) void conv_pw_kernel(const ConvArgs p, const int tiles_n, const int chunks) {
    constexpr int BM = GEMM_BM, TN = BN / 32;
#ifndef FACEHIP_PW_ABL
    constexpr int ABL = 0;
#endif
    __shared__ v4f lds[2][(BM + BN) * 8];
    const GemmLane l = gemm_lane();
    const int tid = l.tid;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tile_n = tile % tiles_n, tile_m = tile / tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int K = p.Cin;

    GemmSrc src = gemm_src<BN>(lds, p.in, m0, K, p.wt, n0, p.Kpad, l);
    const float* const zsrc = p.zeros + l.lqs() * 4;
    int kleft = K - l.lqs() * 4;                                            // > 0: this lane's float4 of the current chunk lies inside a row
    v16f acc[1][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][j][e] = 0.f;

    using EpVec = ConvEpVec<BN, 256>;                                       // the epilogue's per-channel vectors, parked in LDS after the K loop
    EpVec epv;
    epv.fetch(p, n0, tid, true);

#ifdef FACEHIP_PW_ABL
    const int abl = p.sk_test_drop;
    const unsigned long long ts0 = wall_clock64();
    if ((abl & 32) && blockIdx.x >= 256u && blockIdx.x < 512u)
        while (wall_clock64() - ts0 < (unsigned long long)(abl >> 8) * 64ull) __builtin_amdgcn_s_sleep(32);
#endif
    gemm_load_chunk<BN>(src, 0, kleft > 0, zsrc);
    kleft -= 32;
    __syncthreads();
#ifdef FACEHIP_PW_ABL
    const unsigned long long ts1 = wall_clock64();
#endif
    GemmFrag<TN> held{};
    if constexpr ((ABL & 2) != 0) held = gemm_frag<TN>(lds[0], l, 0);
    for (int kc = 0; kc < chunks; ++kc) {
        gemm_chunk_f32<BN, ABL>(acc[0], lds, kc & 1, kc + 1 < chunks, src, l, kleft > 0, zsrc, &held);
        kleft -= 32;
    }
#ifdef FACEHIP_PW_ABL
    __syncthreads();
    const unsigned long long ts2 = wall_clock64();
    if ((abl & 8) && acc[0][0][0] != 123.456f) return;
#endif
    float* const ep = reinterpret_cast<float*>(&lds[0][0]);
    epv.park(ep, tid);
    __syncthreads();
    static_assert((EpVec::FLOATS + 4 * 32 * 36) * sizeof(float) <= sizeof(lds), "epilogue scratch");
#ifdef FACEHIP_PW_ABL
    const bool stamp = tid == 0 && p.slabs && p.Cout == 288 && p.Cin == 288;
    if (stamp) reinterpret_cast<unsigned long long*>(p.slabs)[8192 + (size_t)blockIdx.x * 4 + 3] = wall_clock64();
#endif
    conv_epilogue<BM, BN, 4, 1, EP_LINES | EP_QUADS>(p, acc, m0, n0, l.wid, 0, l.lane, -1, -1, ep, conv_ep_wants_lines(p) ? ep + EpVec::FLOATS : nullptr);
#ifdef FACEHIP_PW_ABL
    if (stamp) {
        const unsigned long long ts3 = wall_clock64();                  // stores issued
        if (abl & 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... and acknowledged
        unsigned long long* o = reinterpret_cast<unsigned long long*>(p.slabs) + (size_t)blockIdx.x * 5;
        o[0] = ts0; o[1] = ts1; o[2] = ts2; o[3] = (abl & 64) ? (unsigned long long)wall_clock64() : ts3; o[4] = 1;
    }
#endif
}

// conv_pw_x3_kernel — the same GEMM with its K loop on three bf16 pieces and six v_mfma_f32_32x32x16_bf16 per 16-deep step (gemm_tile.h,
// "x3": fp32 products, 0.375 of the f32 instruction's matrix-pipe cycles).  The pixel operand stays the fp32 LDS image of conv_pw_kernel
// (same swizzle, same zero line behind K, chosen by source address) and is split in registers by gemm_mma_x3; p.wt is the x3 image of the
// [conv_wt_rows(Cout)][Kpad] weights (launch_pack_x3 with one frequency: [plane][chunk][row][4 slots]; rows behind Cout and columns behind
// K are zero in all three planes because they are zero in the f32 image).  BN = 96 / 64 / 32 (conv_pw_x3_bn); the 32-row remainder of a
// 96- or 32-wide plane is a half pass of the loader that waves 0 and 1 request.  LDS per workgroup: 68 / 56 / 44 KB.
// Order of additions per output: chunks in K order, the two 16-deep steps of a chunk, the six products in gemm_tile.h's order.
template <int BN, int OCC>
__global__ __launch_bounds__(256, OCC) void conv_pw_x3_kernel(const ConvArgs p, const int tiles_n, const int chunks) {
    constexpr int BM = GEMM_BM, TN = BN / 32;
    __shared__ v4f lds[2][gemm_buf_slots_x3<BN>()];
    const GemmLane l = gemm_lane();
    const int tid = l.tid;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tile_n = tile % tiles_n, tile_m = tile / tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int K = p.Cin;

    GemmSrcX3 src = gemm_src_x3<BN>(lds, p.in, m0, K, p.wt, n0, (p.Cout + 127) / 128 * 128, chunks, l);   // (rows = conv_wt_rows(Cout))
    const float* const zsrc = p.zeros + l.lqs() * 4;
    int kleft = K - l.lqs() * 4;                                            // > 0: this lane's float4 of the current chunk lies inside a row
    const bool b_half = l.wid < 2;                                          // (wave-uniform)
    v16f acc[1][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[0][j][e] = 0.f;

    using EpVec = ConvEpVec<BN, 256>;
    EpVec epv;
    epv.fetch(p, n0, tid, true);

    gemm_load_chunk_x3<BN>(src, 0, kleft > 0, zsrc, b_half);
    kleft -= 32;
    __syncthreads();
    for (int kc = 0; kc < chunks; ++kc) {
        if (kc + 1 < chunks) gemm_load_chunk_x3<BN>(src, (kc & 1) ^ 1, kleft > 0, zsrc, b_half);
        gemm_mma_x3<TN>(acc[0], lds[kc & 1], l);
        __syncthreads();
        kleft -= 32;
    }
    float* const ep = reinterpret_cast<float*>(&lds[0][0]);
    epv.park(ep, tid);
    __syncthreads();
    static_assert((EpVec::FLOATS + 4 * 32 * 36) * sizeof(float) <= sizeof(GemmLdsX3<BN>), "epilogue scratch");
    conv_epilogue<BM, BN, 4, 1, EP_LINES | EP_QUADS>(p, acc, m0, n0, l.wid, 0, l.lane, -1, -1, ep, conv_ep_wants_lines(p) ? ep + EpVec::FLOATS : nullptr);
}

template <int BN, int OCC>
static void launch_pw_x3_cfg(const ConvArgs& a, long M, hipStream_t s) {
    const int tiles_n = (a.Cout + BN - 1) / BN;
    KernelTimer& timer = KernelTimer::get();
    timer.begin(s);
    hipLaunchKernelGGL((conv_pw_x3_kernel<BN, OCC>), dim3((unsigned)((M / 128) * tiles_n)), dim3(256), 0, s, a, tiles_n, a.Kpad / 32);
    timer.end(s, 11, a.t_flops, a.t_bytes);       // (booked where the f32 launch is, with the same f32-equivalent FLOPs)
}

template <int BN, int OCC>
static void launch_pw_cfg(const ConvArgs& a, long M, hipStream_t s) {
    const int tiles_n = (a.Cout + BN - 1) / BN;
    KernelTimer& timer = KernelTimer::get();
    timer.begin(s);
    const dim3 grid((unsigned)((M / 128) * tiles_n));
#ifdef FACEHIP_PW_ABL
#define PWABL(X) case X: hipLaunchKernelGGL((conv_pw_kernel<BN, OCC, X>), grid, dim3(256), 0, s, a, tiles_n, a.Kpad / 32); break;
    switch (a.sk_test_drop & 7) { PWABL(1) PWABL(2) PWABL(4) PWABL(7)                   // (the loop masks scripts/pw_ablate.sh uses)
        default: hipLaunchKernelGGL((conv_pw_kernel<BN, OCC>), grid, dim3(256), 0, s, a, tiles_n, a.Kpad / 32); }
#undef PWABL
#else
    hipLaunchKernelGGL((conv_pw_kernel<BN, OCC>), grid, dim3(256), 0, s, a, tiles_n, a.Kpad / 32);
#endif
    timer.end(s, 11, a.t_flops, a.t_bytes);
}

static ConvGeom conv_geom(const ConvArgs& a) {        // what the predicates of conv_plan.h look at
    return ConvGeom{(long)a.B * a.Ho * a.Wo, a.H, a.W, a.Cin, a.Ho, a.Wo, a.Cout, a.ks, a.stride, a.pad, a.Kpad, a.n_outs,
                    a.wt_group_rows > 0, a.sc_in != nullptr, a.res_mode == (int)ResMode::UP2X, a.no_pw != 0};
}

// true = launched (eligibility and tile width: conv_pw_bn)
static bool launch_pw(ConvArgs a, hipStream_t s) {
    const ConvGeom g = conv_geom(a);
    const int bn = conv_pw_bn(g, a.cus > 0 ? a.cus : conv_num_cus(), conv_knobs());
    if (!bn) return false;
    // conv_pw_kernel instantiates the whole-line and per-quad epilogues only (EP_LINES | EP_QUADS): hold the predicate to that
    if (a.n_outs > 0 || (a.Cout & 3)) throw std::logic_error("conv_pw_bn admitted a layer conv_pw_kernel has no epilogue form for");
    a.zeros = conv_zero_line();
    a.ep_direct = conv_knobs().ep_direct;
#ifdef FACEHIP_PW_ABL
    { static const int abl = [] { const char* e = getenv("FACEHIP_PW_ABL"); return e ? atoi(e) : 0; }(); a.sk_test_drop = abl; }
#endif
    if (bn == 96) launch_pw_cfg<96, 2>(a, g.M, s);
    else if (bn == 64) launch_pw_cfg<64, 3>(a, g.M, s);
    else launch_pw_cfg<32, 4>(a, g.M, s);
    return true;
}

// The three-piece bf16 form of a 1x1 stride-1 layer: wt3 = the x3 image of its [conv_wt_rows(Cout)][Kpad] weights (a.wt, the f32 image, is
// what the launch falls back on).  true = launched on conv_pw_x3_kernel; false = the layer has no such form at this batch (conv_pw_x3_bn) or,
// unless `force`, the form does not pay for the launch (conv_pw_x3_pays) — the caller then runs launch_conv.
static void conv_check(const ConvArgs& a, long M);
bool launch_conv_pw_x3(ConvArgs a, const float* wt3, bool force, hipStream_t s) {
    const long M = (long)a.B * a.Ho * a.Wo;
    if (M <= 0 || !wt3) return false;
    const ConvGeom g = conv_geom(a);
    const int cus = a.cus > 0 ? a.cus : conv_num_cus();
    const int bn = conv_pw_x3_bn(g, cus, conv_knobs());
    if (!bn) return false;
    const int tiles_n = (a.Cout + bn - 1) / bn;
    if (!force && !conv_pw_x3_pays((M / 128) * tiles_n, a.Kpad, a.Cout, cus, conv_knobs())) return false;
    conv_check(a, M);
    // (the kernel's epilogue forms and the rows its loader reads of the image: hold the predicate to them)
    if (a.n_outs > 0 || (a.Cout & 3) || tiles_n * bn > conv_wt_rows(a.Cout))
        throw std::logic_error("conv_pw_x3_bn admitted a layer conv_pw_x3_kernel has no form for");
    a.wt = wt3;
    a.zeros = conv_zero_line();
    a.ep_direct = conv_knobs().ep_direct;
    if (bn == 96) launch_pw_x3_cfg<96, 2>(a, M, s);
    else if (bn == 64) launch_pw_x3_cfg<64, 2>(a, M, s);
    else launch_pw_x3_cfg<32, 3>(a, M, s);
    return true;
}

static int g_num_cus = 0;
static const float* g_zeros = nullptr;
static int num_cus() {
    if (!g_num_cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        g_num_cus = n;
    }
    return g_num_cus;
}
int conv_num_cus() { return num_cus(); }
const float* conv_zero_line() {                      // 8 KiB of zeros: a padded tap streams up to Cin*4 bytes from it
    if (!g_zeros) {
        void* p = nullptr;
        if (hipMalloc(&p, 8192) == hipSuccess) { (void)hipMemset(p, 0, 8192); g_zeros = (const float*)p; }
    }
    return g_zeros;
}

size_t conv_slab_floats() { return SK_SLAB_FLOATS + SK_COUNTERS; }   // slabs + one counter word per remainder tile
void conv_workspace_init(float* ws) { (void)hipMemset(ws + SK_SLAB_FLOATS, 0, SK_COUNTERS * sizeof(unsigned)); }
void conv_workspace_reset_async(float* ws, hipStream_t s) { (void)hipMemsetAsync(ws + SK_SLAB_FLOATS, 0, SK_COUNTERS * sizeof(unsigned), s); }

// ---- stream-K watchdog, host state (records, generations, the test hook conv_debug_streamk): a host-mapped (pinned, device-visible)
// record an owner writes when its hand-off wait times out
static unsigned* g_sk_err = nullptr;
static std::atomic<unsigned> g_sk_generation{0};      // (handles may be driven from different host threads)
static unsigned g_sk_timeout = (unsigned)((2000ull * 100000ull) >> 16);      // 2 s in units of 2^16 ticks of the 100 MHz wall clock
static int g_sk_test_drop = 0;
unsigned* conv_error_words() {
    if (!g_sk_err) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) { memset(p, 0, 64); g_sk_err = (unsigned*)p; }
    }
    return g_sk_err;
}
// One record per Net (allocated with its workspace) so that a time-out is reported by a call on the handle whose launch was abandoned;
// launches without one (the single-kernel test entry points) share the process-wide record above.  Records are never freed while the
// device may still write them: a Net parks its record on a free list at destruction.
static std::vector<unsigned*> g_sk_free;
static std::mutex g_sk_mu;
unsigned* conv_error_record_new() {
    {
        std::lock_guard<std::mutex> lk(g_sk_mu);
        if (!g_sk_free.empty()) { unsigned* r = g_sk_free.back(); g_sk_free.pop_back(); memset(r, 0, 64); return r; }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
    memset(p, 0, 64);
    return (unsigned*)p;
}
void conv_error_record_release(unsigned* r) {
    if (!r) return;
    std::lock_guard<std::mutex> lk(g_sk_mu);
    g_sk_free.push_back(r);
}
bool conv_error_pending(const unsigned* rec) {
    const volatile unsigned* e = rec;
    return e && e[0];
}
bool conv_take_error(std::string& msg, unsigned* rec) {
    volatile unsigned* e = rec;
    if (!e || !e[0]) return false;
    char buf[256];
    snprintf(buf, sizeof buf, "HIP error: stream-K hand-off timed out (remainder tile %u saw %u of %u helper arrivals): the launch was "
             "abandoned, its outputs are incomplete", e[1], e[2], e[3]);
    msg = buf;
    e[0] = 0;
    g_sk_generation.fetch_add(1, std::memory_order_relaxed);                                   // every workspace's counters are suspect: owners re-zero them before their next run
    return true;
}
unsigned conv_error_generation() { return g_sk_generation.load(std::memory_order_relaxed); }
static std::atomic<unsigned> g_sk_debug_gen{0};
unsigned conv_debug_generation() { return g_sk_debug_gen.load(std::memory_order_relaxed); }
void conv_debug_streamk(int drop_publish, int timeout_ms) {
    g_sk_debug_gen.fetch_add(1, std::memory_order_relaxed);
    g_sk_test_drop = drop_publish;
    g_sk_timeout = (unsigned)(((unsigned long long)(timeout_ms > 0 ? timeout_ms : 2000) * 100000ull) >> 16);
}

// One tile config: conv_tall_kernel for the whole rounds it takes (conv_tall_plan), then conv_igemm_kernel for the tiles from tile0 on,
// cut as conv_streamk_plan says, then conv_fixup_kernel if the plan has no owners.
// (conv_tall_kernel, 256x64: IResNet's stage 1 / 2.  128x32: SCRFD's merged 64 -> 30 head convolutions at B = 128 — 340 -> 330 us on
// 80x80, 98 -> 91 on 40x40: a small gain, because with three phase-locked workgroups per CU the image load at the top of each of the two
// chunks stays exposed; a three-deep weight ring (two taps ahead, barrier with vmcnt(1)) changed nothing: 306 against 307 us)
// X3: conv_igemm_kernel's three-piece bf16 instantiations (a.wt = the x3 weight image; launch_conv_x3 checked the layer's form).
template <int BM, int BN, int WM, int WN, int OCC, bool X3 = false>
static void launch_cfg(ConvArgs a, int resident_per_cu, int cfg_tag, hipStream_t s) {
    using TL = Tile<BM, BN, WM, WN>;
    const ConvGeom g = conv_geom(a);
    const int tiles_n = (a.Cout + BN - 1) / BN, tiles = (int)((g.M + BM - 1) / BM) * tiles_n;
    const int cus = a.cus > 0 ? a.cus : num_cus();
    a.zeros = conv_zero_line();
    a.tile0 = 0;
    if constexpr (!X3 && ((BM == 256 && BN == 64) || (BM == 128 && BN == 32))) {
        constexpr int TOCC = BM == 256 ? 2 : 3;                             // (= conv_tall_plan's occ)
        const ConvTallPlan t = conv_tall_plan(g, BM, BN, TL::RP, tiles, tiles_n, cus, conv_knobs());
        if (t.tiles > 0) {
            // conv_tall_kernel instantiates the merged and per-quad epilogues only (EP_MERGED | EP_QUADS): hold the predicate to that
            if (a.n_outs == 0 && (a.Cout & 3)) throw std::logic_error("conv_tall_plan admitted a layer conv_tall_kernel has no epilogue form for");
            static bool attr_set = false;
            if (!attr_set) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_tall_kernel<BM, BN, WM, WN, TOCC>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
                attr_set = true;
            }
            const double part = (double)t.tiles / tiles;
            KernelTimer& tt = KernelTimer::get();
            tt.begin(s);
            hipLaunchKernelGGL((conv_tall_kernel<BM, BN, WM, WN, TOCC>), dim3((unsigned)t.tiles), dim3(TL::T), t.lds, s, a, tiles_n, t.rows_a);
            tt.end(s, 10, a.t_flops * part, a.t_bytes * part);
            a.t_flops *= (double)(tiles - t.tiles) / tiles; a.t_bytes *= (double)(tiles - t.tiles) / tiles;
            a.tile0 = t.tiles;
            if (t.tiles == tiles) return;
        }
    }
    const int chunks = a.Kpad / 32;
    const ConvSkPlan pl = conv_streamk_plan(tiles - a.tile0, cus * resident_per_cu, chunks, TL::SLAB, cus, a.Kpad, a.tile0, a.slabs && a.sk_enable, conv_knobs());
    a.sk_full = pl.full; a.sk_helpers = pl.helpers; a.sk_rem = pl.rem;
    a.sk_units = pl.units; a.sk_q = pl.q; a.sk_owner_chunks = pl.owner_chunks; a.sk_maxp = pl.maxp;
    a.sk_err = pl.owners ? (a.sk_err ? a.sk_err : conv_error_words()) : nullptr; a.sk_timeout = g_sk_timeout; a.sk_test_drop = g_sk_test_drop;
    a.ep_direct = X3 ? 0 : conv_knobs().ep_direct;             // (the x3 instantiations hold the whole-line epilogue only)
    KernelTimer& timer = KernelTimer::get();
    timer.begin(s);
    const dim3 grid((unsigned)(pl.full + pl.helpers + pl.owners));
    if constexpr (X3) {
        if (a.sc_in) hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, OCC, true, false, true, true>), grid, dim3(TL::T), 0, s, a, tiles_n, chunks);
        else hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, OCC, true, false, false, true>), grid, dim3(TL::T), 0, s, a, tiles_n, chunks);
    } else if (g.grouped) {                                    // (wt_group_rows % BM == 0 and Cin % 32 == 0: the caller's contract)
        hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, OCC, true, true>), grid, dim3(TL::T), 0, s, a, tiles_n, chunks);
    } else if (a.sc_in)                                        // (launch_conv checked Cin % 32 == 0)
        hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, OCC, true, false, true>), grid, dim3(TL::T), 0, s, a, tiles_n, chunks);
    else if ((a.Cin & 31) == 0)
        hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, OCC, true, false>), grid, dim3(TL::T), 0, s, a, tiles_n, chunks);
    else
        hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, OCC, false, false>), grid, dim3(TL::T), 0, s, a, tiles_n, chunks);
    timer.end(s, g.grouped ? 7 : cfg_tag, a.t_flops, a.t_bytes);   // (grouped = Winograd GEMM: its own tag)
    if (pl.fixup) {
        timer.begin(s);
        hipLaunchKernelGGL((conv_fixup_kernel<BM, BN, WM, WN>), dim3((unsigned)(pl.rem * TL::TM * TL::TN)), dim3(TL::T), 0, s, a, tiles_n, chunks);
        timer.end(s, 6, 0.0, 0.0);
    }
}

static void conv_check(const ConvArgs& a, long M) {
    // the loader and the epilogue index pixels and tensor elements with 32-bit integers
    if ((long)a.B * a.H * a.W * a.Cin >= (1L << 31) || M * a.Cout >= (1L << 31))
        throw std::runtime_error("conv: tensor too large for the 32-bit element offsets of one launch (split the batch)");
    if (a.sc_in && (a.ks != 3 || a.Cin % 32 != 0 || a.sc_C % 32 != 0 || a.Kpad != 9 * a.Cin + a.sc_C || a.wt_group_rows > 0 ||
                    (long)a.B * a.sc_H * a.sc_W * a.sc_C >= (1L << 31)))
        throw std::runtime_error("conv: folded shortcut needs a 3x3 convolution with Cin % 32 == 0, sc_C % 32 == 0 and Kpad = 9*Cin + sc_C");
}

// The three-piece bf16 form of one layer: a.wt = the x3 image of its [conv_wt_rows(Cout)][Kpad] weights.  tag: the timer tag the layer's
// f32 launch would carry (the launch is booked there, with the same f32-equivalent FLOPs).
void launch_conv_x3(const ConvArgs& a, int tag, hipStream_t s) {
    const long M = (long)a.B * a.Ho * a.Wo;
    if (M <= 0) return;
    conv_check(a, M);
    if (!conv_x3_ok(a.Cin, a.Cout) || a.wt_group_rows > 0 || a.Kpad % 32 || a.n_outs > 0 || (a.ks != 1 && a.ks != 3) ||
        a.Kpad != a.ks * a.ks * a.Cin + (a.sc_in ? a.sc_C : 0))
        throw std::runtime_error("conv: this layer has no three-piece bf16 form (it needs Cin % 32 == 0, Cout % 64 == 0, one group)");
    if (conv_x3_bn(a.Cout) == 128) launch_cfg<128, 128, 4, 1, 2, true>(a, 2, tag, s);
    else launch_cfg<128, 64, 4, 1, 2, true>(a, 2, tag, s);
}
bool conv_x3_ok(int Cin, int Cout) { return Cin > 0 && Cin % 32 == 0 && conv_x3_bn(Cout) != 0; }

void launch_conv(const ConvArgs& a, int cfg, hipStream_t s) {
    const long M = (long)a.B * a.Ho * a.Wo;
    if (M <= 0) return;
    conv_check(a, M);
    if (launch_pw(a, s)) return;
    if (cfg < 0) cfg = conv_pick_cfg(M, a.Cout);
    switch (cfg) {
        case 0: launch_cfg<128, 128, 2, 2, 2>(a, 2, 0, s); break;
        case 1: launch_cfg<256, 64, 4, 1, 2>(a, 2, 1, s); break;
        case 2: launch_cfg<128, 32, 4, 1, 4>(a, 4, 2, s); break;
        default: launch_cfg<64, 64, 2, 2, 4>(a, 5, 3, s); break;
    }
}

}  // namespace fh
