// conv_wino2.hip — 3x3 stride-1 pad-1 convolutions with 64 input channels (IResNet-50's stage 1 and the stage-2 entry, SCRFD's merged
// 64 -> 30 head convolutions) as ONE fused Winograd F(2x2, 3x3) kernel on v_mfma_f32_16x16x4_f32 (gfx950 / CDNA4).
//
// What it replaces: Conv nodes inside `session_->Run` (reference src/face_recognizer.cpp:279-283, src/face_detector.cpp:179-183) —
// 112x112x64 -> 64, 4 x 56x56x64 -> 64, 56x56x64 -> 128: 2.7 ms of the 12.1 ms step at B = 128 in the direct form (conv_tall_kernel,
// 113-115 TFLOP/s = 0.73 of the f32 MFMA peak: at its ceiling).  Y = A^T [ (G g G^T) (.) (B^T d B) ] A on 2x2 output tiles needs 16
// multiplies per 4 outputs and input channel instead of 36: 2.25x less matrix-core work.  The unfused form (transform kernel -> GEMM ->
// transform kernel, as winograd.hip does for Cin >= 128) moves 4x the activation through memory twice around a K = 64 GEMM that is all
// prologue; here nothing but the layer's input and output touches memory:
//
//   * ONE WAVE per workgroup owns a 4 x 4 tile group (8 x 8 outputs = the 16 MFMA columns: lane = tile) and ALL 16 CB output channels
//     of its column tile (CB = 4: 64 channels; CB = 2: the <= 32 channels of merged sibling convolutions);
//   * the whole 64-channel halo of the group (10 x 10 pixels x 256 B = 25.6 KB) comes in once by LDS-DMA, de-interleaved into the four
//     (row parity, column parity) planes of 5 x 5 pixels — tile (tr, tc) reads patch pixel (dy, dx) from plane (dy & 1, dx & 1) at
//     pixel (tr + dy/2, tc + dx/2), so the lanes of one ds_read_b128 touch neighbouring rows of a [pixel][16 x float4] image whose
//     16-byte column is XOR-swizzled by 2 ((pc + 4 (pr & 1)) & 7): conflict-free (scripts/wino2_banks.py enumerates every read; with
//     interleaved pixels every lane's address has the same parity and no swizzle avoids a 2-way conflict).  A wave only reads what it
//     loaded itself: NO barrier anywhere in the kernel; six independent waves per CU (LDS-bound);
//   * for each of the 16 frequencies f = (i, j) in turn: lane (tile n = lane & 15, kq = lane >> 4) forms V_f = (B^T d B)[i][j] of ITS
//     tile for channels 16 g + 4 kq + e of k-step group g from four ds_read_b128 and three adds (B^T has two +-1 entries per row) — a
//     float4 that is exactly the B fragment the MFMA wants from that lane and feeds 4 (e) x CB MFMAs; U_f = G g G^T (fp64 at load time,
//     carrying the block's folded BatchNorm) is pre-arranged [f][g][cb][lane][4] and goes global -> registers a few steps ahead;
//     M_f accumulates in 4 CB registers and is added into the four output accumulators Y[a][b] with A^T's {0, +-1} coefficients (1, 2 or
//     4 adds per register) in the shadow of the NEXT frequency's MFMAs;
//   * epilogue on the 2x2 pixels of the lane's tile: bias (9 border classes when the block's BatchNorm is folded in, engine.cpp) ->
//     ReLU / PReLU -> + residual -> store (+ second output); or, CB = 2, per-channel-range destinations and activations (merged heads).
//
// A 32-column form of the same algorithm (v_mfma_f32_32x32x2_f32: 4 x 7 | 8 tiles per wave, two tile groups x two 32-channel halves per
// 4-wave workgroup, 32-channel halo chunks, weights through an LDS stage or registers, persistent or not) was built first and measured
// equal: 185-197 us on 56x56x64 -> 64 at B = 128 for every variant, against 285 us direct (docs/kernels.md 3.1l has the ablation that says why:
// the costs ADD — the kernel behaves like one bound by energy, not by any one pipe).  This form is kept: exact fit on 56 / 112 / 80 / 40-wide
// maps, V formed once per tile instead of once per channel half, no barrier, and the merged-output epilogue.
//
// Numerics: the interpolation points of F(2x2, 3x3) are {0, 1, -1, inf}; G has entries 1 and 1/2 — rounding stays within ~3x of the
// direct fp32 form (tests/test_gpu_round4.py bars single layers at 5e-5 abs on O(1) outputs; winograd.hip's F(4x4) needs 2e-4).
//
// Layout of this file: THE TILE BODY (walk, halo, patch addresses, patch reads and V, the A^T fold, the plain epilogue — each stated once
// with its design note), then wino2_kernel (products on f32 MFMAs; also the merged-sibling epilogue and the diagnostic switches) and
// wino2_x3_kernel (products on six bf16 MFMAs), which differ in their weight ring and K loop alone; then one launcher (launch_w2) and
// the two weight packers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "gemm_tile.h"
#include "kernels.h"
#include "plan.h"

namespace fh {

namespace {

// NONE / ReLU / PReLU without a branch per element: sl = 1 (none) or the PReLU slope; relu is wave-uniform
__device__ __forceinline__ float act1(float v, bool relu, float sl) {
    const float a = v >= 0.f ? v : v * sl;
    return relu ? fmaxf(v, 0.f) : a;
}

// B^T of F(2x2, 3x3): row i has two non-zero entries, at patch rows YA[i] (sign +1) and YB[i] (sign SB[i])
//   [ 1  0 -1  0 ]   [ 0  1  1  0 ]   [ 0 -1  1  0 ]   [ 0  1  0 -1 ]
constexpr int kYA[4] = {0, 1, 2, 1}, kYB[4] = {2, 2, 1, 3};
constexpr int kSA[4] = {1, 1, 1, 1}, kSB[4] = {-1, 1, -1, -1};
// A^T = [ 1 1 1 0 ; 0 1 -1 -1 ]: coefficient of frequency row i in output row a
constexpr int kAT[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};

template <int V> struct IC { static constexpr int value = V; };          // compile-time integers: the loop over the 16 frequencies is a fold over
                                                                          // 16 instantiations (`#pragma unroll` gives up on a body of this size, and a
                                                                          // run-time f turns every B^T / A^T coefficient into a branch)

// ====================================================================================================================================
// THE TILE BODY: everything wino2_kernel and wino2_x3_kernel have in common, each piece stated once.  What a kernel keeps for itself is
// its weight ring, its K loop (step / stage) and, for wino2_kernel, the merged-sibling epilogue and the diagnostic switches.
// Both kernels are ONE basic block without scratch: the pins (asm volatile "+v"), the sched_barrier(0) brackets around the MFMA block and
// the opaque scalars ("+s") below and in the kernels are part of the register budget, not decoration (docs/kernels.md 3.1l).  The pieces
// take the kernel's by-value ConvArgs by const reference and are always inlined: .private_segment_fixed_size must stay 0
// (profiles/wino2_tile_refactor.md has every instantiation's figures).

// Walk.  Workgroup -> (column tile, image, tile group) in XCD-contiguous order, column tile fastest: the tiles_n workgroups around one
// halo are neighbours on one L2.  Lane -> tile (tr, tc) of the 4 x 4 group and k quarter kq.
struct W2Walk { int tile_n, gn, gy, gx, kq, tr, tc; };
__device__ __forceinline__ W2Walk w2_walk(const int lane, const int tiles_n, const int tgx, const int tgy) {
    const int blk = xcd_tile(blockIdx.x, (int)gridDim.x);
    const int tile_n = blk % tiles_n, tg = blk / tiles_n;
    const int per_img = tgx * tgy;
    const int gn = tg / per_img, rem = tg - gn * per_img;
    const int gy = rem / tgx, gx = rem - gy * tgx;
    const int tn = lane & 15;
    return {tile_n, gn, gy, gx, lane >> 4, tn >> 2, tn & 3};
}

// Halo.  The swizzle key of plane pixel (pr, pc): XORed into the 16-byte column on the way in (source side) and on the way out (rb[]).
__device__ __forceinline__ constexpr int w2_key(int pr, int pc) { return 2 * ((pc + 4 * (pr & 1)) & 7); }

// The 64-channel halo of tile group (gn, gy, gx) -> LDS: 25 pieces of 4 LDS rows x 16 columns.  LDS row 4 i + pl holds pixel i = 5 pr + pc
// of parity plane pl, so piece i is the same plane pixel of the four planes: its lanes' plane is lane >> 4 (computed once), its (pr, pc)
// and swizzle key are compile-time constants — ~10 VALU per piece instead of ~30 with plane-major rows (the bank a read hits does not
// depend on its row: a row is all 64 banks).  The NW waves of a workgroup take alternate pieces.
template <int NW>
__device__ __forceinline__ void w2_load_halo(const ConvArgs& p, char* const halo, const int lane, const int wv, const int gn, const int gy, const int gx) {
    const int H = p.H, W = p.W;
    const int col = lane & 15, pl = lane >> 4;
    const int y0 = 8 * gy - 1 + (pl >> 1), x0 = 8 * gx - 1 + (pl & 1);
    const float* const img = p.in + ((size_t)gn * H * W + (size_t)y0 * W + x0) * 64;   // (may point in front of the image: only dereferenced when in range)
#pragma unroll
    for (int i = 0; i < 25; ++i) {
        const int pr = i / 5, pc = i - 5 * pr;
        const int y = y0 + 2 * pr, x = x0 + 2 * pc;
        const bool ok = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        if (NW > 1 && (i % NW) != wv) continue;                            // (wave-uniform)
        lds_dma16(ok ? img + ((long)2 * pr * W + 2 * pc) * 64 + ((col ^ w2_key(pr, pc)) << 2) : p.zeros, halo + i * 1024);
    }
}

// Patch addresses.  rb[4 dy + dx] = the ABSOLUTE LDS byte address of patch pixel (dy, dx) of tile (tr, tc), column kq of k-step group 0:
// plane (dy & 1, dx & 1), plane pixel (tr + dy / 2, tc + dx / 2).  Group g is rb[] ^ (g << 6) — valid while the halo sits at a 256-byte
// aligned LDS address, which launch_w2 checks.
__device__ __forceinline__ void w2_patch_addrs(unsigned (&rb)[16], const char* const halo, const int tr, const int tc, const int kq) {
    const unsigned halo_base = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)halo;
#pragma unroll
    for (int dy = 0; dy < 4; ++dy)
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
            const int pl = (dy & 1) * 2 + (dx & 1), pr = tr + (dy >> 1), pc = tc + (dx >> 1);
            rb[dy * 4 + dx] = halo_base + (unsigned)((4 * (pr * 5 + pc) + pl) * 256 + ((w2_key(pr, pc) ^ kq) << 4));
        }
}

// Patch reads.  The four patch pixels frequency F = (i, j) needs — rows (kYA[i], kYB[i]) x columns (kYA[j], kYB[j]) — of k-step group g
// (columns 4 g .. 4 g + 3).  The group offset is an opaque scalar: a compile-time XOR is hoisted out of the unrolled loop — 48 addresses
// in registers; for g = 0 too: reads that depend on nothing float stages ahead.
template <int F>
__device__ __forceinline__ void w2_read_patch(v4f* const d, const unsigned (&rb)[16], const int g) {
    typedef const __attribute__((address_space(3))) v4f* lds_v4f;
    constexpr int ya = kYA[F >> 2], yb = kYB[F >> 2], xa = kYA[F & 3], xb = kYB[F & 3];
    unsigned gxr = g << 6;
    asm volatile("" : "+s"(gxr));
    d[0] = *reinterpret_cast<lds_v4f>((size_t)(rb[ya * 4 + xa] ^ gxr));
    d[1] = *reinterpret_cast<lds_v4f>((size_t)(rb[ya * 4 + xb] ^ gxr));
    d[2] = *reinterpret_cast<lds_v4f>((size_t)(rb[yb * 4 + xa] ^ gxr));
    d[3] = *reinterpret_cast<lds_v4f>((size_t)(rb[yb * 4 + xb] ^ gxr));
}

// V.  V_F = (B^T d B)[i][j] from the four values of w2_read_patch<F>: three signed adds, in this order (tests/wino2_x3_model.py states
// the same), for the N k-step groups of a step at once: chain n reads d[4 n .. 4 n + 3], and each add is written for all chains before the
// next one (chain after chain, the x3 kernel's K loop gains 27 s_waitcnt).  The caller pins the result in front of its MFMAs.
template <int F, int N>
__device__ __forceinline__ void w2_form_v(v4f (&v)[N], const v4f* const d) {
    constexpr int fi = F >> 2, fj = F & 3;
    constexpr int sab = kSA[fi] * kSB[fj], sba = kSB[fi] * kSA[fj], sbb = kSB[fi] * kSB[fj];
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = d[4 * n];
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = sab > 0 ? v[n] + d[4 * n + 1] : v[n] - d[4 * n + 1];
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = sba > 0 ? v[n] + d[4 * n + 2] : v[n] - d[4 * n + 2];
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = sbb > 0 ? v[n] + d[4 * n + 3] : v[n] - d[4 * n + 3];
}

// A^T fold.  M of frequency F -> the four output accumulators with A^T's {0, +-1} coefficients.
template <int F, int CB>
__device__ __forceinline__ void w2_y_update(v4f (&Y)[2][2][CB], const v4f (&M)[CB]) {
    constexpr int i = F >> 2, j = F & 3;
    constexpr int c00 = kAT[0][i] * kAT[0][j], c01 = kAT[0][i] * kAT[1][j], c10 = kAT[1][i] * kAT[0][j], c11 = kAT[1][i] * kAT[1][j];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        if constexpr (c00 > 0) Y[0][0][cb] += M[cb]; else if constexpr (c00 < 0) Y[0][0][cb] -= M[cb];
        if constexpr (c01 > 0) Y[0][1][cb] += M[cb]; else if constexpr (c01 < 0) Y[0][1][cb] -= M[cb];
        if constexpr (c10 > 0) Y[1][0][cb] += M[cb]; else if constexpr (c10 < 0) Y[1][0][cb] -= M[cb];
        if constexpr (c11 > 0) Y[1][1][cb] += M[cb]; else if constexpr (c11 < 0) Y[1][1][cb] -= M[cb];
        // pinned here: pure arithmetic floats freely in this barrier-free kernel, and left alone the scheduler defers the updates —
        // every deferred frequency keeps its 4 CB accumulator registers alive (256 registers + spills by the tenth frequency)
        if constexpr (c00 != 0) asm volatile("" : "+v"(Y[0][0][cb]));
        if constexpr (c01 != 0) asm volatile("" : "+v"(Y[0][1][cb]));
        if constexpr (c10 != 0) asm volatile("" : "+v"(Y[1][0][cb]));
        if constexpr (c11 != 0) asm volatile("" : "+v"(Y[1][1][cb]));
    }
}

// The fold over the 16 frequencies (see IC)
template <class Stage>
__device__ __forceinline__ void w2_each_freq(Stage&& stage) {
    stage(IC<0>{}); stage(IC<1>{}); stage(IC<2>{}); stage(IC<3>{}); stage(IC<4>{}); stage(IC<5>{}); stage(IC<6>{}); stage(IC<7>{});
    stage(IC<8>{}); stage(IC<9>{}); stage(IC<10>{}); stage(IC<11>{}); stage(IC<12>{}); stage(IC<13>{}); stage(IC<14>{}); stage(IC<15>{});
}

// Plain epilogue on the 2x2 pixels at (oy0, ox0) of image gn, channels n0 + 16 cb + e (n0 includes the lane's 4 kq): bias (its pixel's
// border class when the block's BatchNorm is folded in) -> ReLU / PReLU -> + residual -> store (+ second output).
// Every load goes out BEFORE the first store: bias, slope, residual — 36 float4 per lane in flight together, ONE global-memory latency.
// (Per pixel "load, wait, compute, store" was four latencies in a row: with the stores masked to one lane of 64 the epilogue still cost
// 33 of the layer's 195 us — it was never the traffic.)  The caller fences it off from the K loop: the kernel is one basic block, and
// unfenced these loads are scheduled in front of the K loop and their ~80 destination registers spilled through it.
template <int CB>
__device__ __forceinline__ void w2_store_plain(const ConvArgs& p, const v4f (&Y)[2][2][CB], const int gn, const int oy0, const int ox0, const int n0) {
    const int Cout = p.Cout;
    const float* __restrict__ res = p.res;
    float* __restrict__ out1 = p.out1;
    float* __restrict__ out2 = p.out2;
    const bool relu = p.act == (int)Act::RELU, prelu = p.act == (int)Act::PRELU;
    bool live[4]; size_t row[4]; v4f b4[4][CB], r4[4][CB], sl[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) sl[cb] = prelu ? *reinterpret_cast<const v4f*>(p.slope + n0 + 16 * cb) : v4f{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int oy = oy0 + (q >> 1), ox = ox0 + (q & 1);
        live[q] = oy < p.Ho && ox < p.Wo;
        const int oyc = min(oy, p.Ho - 1), oxc = min(ox, p.Wo - 1);         // (clamped: dead pixels load a neighbour's vectors and store nothing)
        row[q] = (((size_t)gn * p.Ho + oyc) * p.Wo + oxc) * Cout + n0;
        const int cls = p.bias_cls ? 3 * (oyc == 0 ? 0 : oyc == p.Ho - 1 ? 2 : 1) + (oxc == 0 ? 0 : oxc == p.Wo - 1 ? 2 : 1) : 0;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            b4[q][cb] = p.bias ? *reinterpret_cast<const v4f*>(p.bias + cls * Cout + n0 + 16 * cb) : v4f{0.f, 0.f, 0.f, 0.f};
            if (p.res_mode != (int)ResMode::NONE) r4[q][cb] = *reinterpret_cast<const v4f*>(res + row[q] + 16 * cb);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!live[q]) continue;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            v4f v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act1(Y[q >> 1][q & 1][cb][e] + b4[q][cb][e], relu, sl[cb][e]);
            if (p.res_mode != (int)ResMode::NONE) v += r4[q][cb];
            if (out1) *reinterpret_cast<v4f*>(out1 + row[q] + 16 * cb) = v;
            if (out2) {
                const v4f s2 = *reinterpret_cast<const v4f*>(p.s2 + n0 + 16 * cb), t2 = *reinterpret_cast<const v4f*>(p.t2 + n0 + 16 * cb);
                *reinterpret_cast<v4f*>(out2 + row[q] + 16 * cb) = v * s2 + t2;
            }
        }
    }
}

// ====================================================================================================================================
// NW = waves per workgroup that share ONE halo: wave w computes the 16 CB channels [16 CB w, 16 CB (w + 1)) of the workgroup's 16 CB NW-channel
// column tile (NW = 1: the original one-wave form).  MERGED selects the merged-sibling epilogue (per-channel-range destinations).
// NW = 2, CB = 2 on the plain 64-channel layers: the 25.6 KB halo limits a CU to six workgroups either way, so six waves of 226 registers
// (1.5 per SIMD: two SIMDs carry two waves, two carry one) become twelve of 112 (three per SIMD) — DESIGN.md 3.1.
template <int CB, int NW, bool MERGED>
__global__ __launch_bounds__(64 * NW, NW == 1 ? 2 : 3) void wino2_kernel(const ConvArgs p, const int tiles_n, const int tgx, const int tgy) {
    extern __shared__ v4f w2sm[];
    char* const halo = reinterpret_cast<char*>(w2sm);                      // [5][5] plane pixels x [4 parity planes] x 16 x 16 B
    const int lane = threadIdx.x & 63;
    const int wv = NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    constexpr int CBT = CB * NW;                                           // 16-channel blocks per column tile in the weight image
#ifdef FACEHIP_W2_PROF
    const long long prof_c0 = __builtin_readcyclecounter(), prof_r0 = __builtin_amdgcn_s_memrealtime();   // shader clock vs the constant 100 MHz counter
#endif
    const W2Walk t = w2_walk(lane, tiles_n, tgx, tgy);
    w2_load_halo<NW>(p, halo, lane, wv, t.gn, t.gy, t.gx);
    unsigned rb[16];
    w2_patch_addrs(rb, halo, t.tr, t.tc, t.kq);
    // weights of this column tile: step (f, j) = CB KB at ((f * 4 + j) * CB) * 256 floats; cb-th fragment + cb * 256
    // (a wave-uniform running pointer + the lane's 16-byte offset: with compile-time step offsets the 64 step addresses are hoisted out of
    //  the loop into 128 registers)
    const char* wstep = reinterpret_cast<const char*>(p.wt + ((size_t)t.tile_n * 64 * CBT + (size_t)wv * CB) * 256);
    const unsigned wlane = lane * 16;
    constexpr int WD = 2;                                                  // weight ring: fragments are requested WD - 1 steps (512 MFMA cycles each) ahead
    v4f wr[WD][CB] = {};                                                   // (WD = 4 measured the same: 196.0 vs 194.6 us on 56x56x64, and costs 32 registers)
#ifdef FACEHIP_W2_PROF
    const bool abl_w = p.sk_test_drop & 4, abl_d = p.sk_test_drop & 8, abl_y = p.sk_test_drop & 16, abl_st = p.sk_test_drop & 2;   // ablations (wrong results)
#else
    constexpr bool abl_w = false, abl_d = false, abl_y = false, abl_st = false;
#endif
    auto fetch_w = [&](bool advance, int buf) __attribute__((always_inline)) {
        if (abl_w) return;
        unsigned adv = advance ? CBT * 1024 : 0;
        asm volatile("" : "+s"(adv));
        wstep += adv;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) wr[buf][cb] = *reinterpret_cast<const v4f*>(wstep + wlane + cb * 1024);
    };
    v4f Y[2][2][CB], Mp[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        Mp[cb] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) Y[a >> 1][a & 1][cb] = v4f{0.f, 0.f, 0.f, 0.f};
    }
    auto y_update = [&](auto fc, const v4f (&M)[CB]) __attribute__((always_inline)) {
        constexpr int f = decltype(fc)::value;
        if (abl_y && f != 5) return;
        w2_y_update<f, CB>(Y, M);
    };
    v4f d[2][4] = {};                                                      // the patch values of two steps: a double buffer
    auto fetch_d = [&](auto fc, auto jc, auto bc) __attribute__((always_inline)) {
        if (abl_d) return;
        w2_read_patch<decltype(fc)::value>(d[decltype(bc)::value], rb, decltype(jc)::value);   // k-step group j
    };
    auto stage = [&](auto fc) __attribute__((always_inline)) {
        constexpr int f = decltype(fc)::value;
        v4f M[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) M[cb] = v4f{0.f, 0.f, 0.f, 0.f};
        auto step = [&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value, k = f * 4 + j;
            fetch_w(k + WD - 1 < 64, (k + WD - 1) % WD);                    // fragments of step k + WD - 1 (past the end: a harmless re-fetch)
            if constexpr (j < 3) fetch_d(IC<f>{}, IC<j + 1>{}, IC<(k + 1) & 1>{});
            else if constexpr (f < 15) fetch_d(IC<f + 1>{}, IC<0>{}, IC<(k + 1) & 1>{});
            __builtin_amdgcn_sched_barrier(0);
            v4f v[1];
            w2_form_v<f>(v, d[k & 1]);
            asm volatile("" : "+v"(v[0]));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[k % WD][cb][e], v[0][e], M[cb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        };
        step(IC<0>{}); step(IC<1>{});
        y_update(IC<(f + 15) & 15>{}, Mp);                                 // the previous frequency's result -> the outputs, in the shadow of this one's MFMAs
        step(IC<2>{}); step(IC<3>{});
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) Mp[cb] = M[cb];
        __builtin_amdgcn_sched_barrier(0);
    };
    fetch_w(false, 0);
#pragma unroll
    for (int q = 1; q < WD - 1; ++q) fetch_w(true, q);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the halo has landed: LDS-DMA is ordered for its own wave by vmcnt alone
    if constexpr (NW > 1) __syncthreads();                                 // ... and for the sibling wave's pieces by the workgroup's only barrier
    fetch_d(IC<0>{}, IC<0>{}, IC<0>{});
    w2_each_freq(stage);
    y_update(IC<15>{}, Mp);

    // ---- epilogue: lane = tile (tr, tc), accumulator block cb = channels 16 cb + 4 kq .. + 3 of the column tile (fenced: w2_store_plain)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (abl_st && lane != 0) return;                                       // (lane 0 goes on to the clock stamp; 63 of 64 lanes' stores are gone)
    const int oy0 = 2 * (4 * t.gy + t.tr), ox0 = 2 * (4 * t.gx + t.tc);
    const int n0 = (t.tile_n * NW + wv) * 16 * CB;
    if constexpr (!MERGED) {
        w2_store_plain<CB>(p, Y, t.gn, oy0, ox0, n0 + 4 * t.kq);
    } else {                                                               // merged sibling convolutions: per-channel-range destination and activation
        const int kq = t.kq, Cout = p.Cout;
        float bm[CB][4];                                                   // this lane's 8 bias values, fetched once (no load between the stores)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const int co = n0 + 16 * cb + 4 * kq + e; bm[cb][e] = co < Cout ? p.bias[co] : 0.f; }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int oy = oy0 + a, ox = ox0 + b;
                if (oy >= p.Ho || ox >= p.Wo) continue;
                const size_t pix = ((size_t)t.gn * p.Ho + oy) * p.Wo + ox;  // (merged convolutions carry no folded BatchNorm: wino2_ok)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {                       // channel pairs: one 8-byte store where both land in one destination, aligned
                        const int co = n0 + 16 * cb + 4 * kq + e;
                        if (co >= Cout) continue;
                        const int g = co >= p.oc0[2] && p.n_outs > 2 ? 2 : co >= p.oc0[1] ? 1 : 0;
                        const int cg = p.oc0[g + 1] - p.oc0[g], ga = p.oact[g];
                        auto fin = [&](float v) { return ga == (int)Act::RELU ? fmaxf(v, 0.f) : ga == (int)Act::SIGMOID ? 1.0f / (1.0f + expf(-v)) : v; };
                        float* const dst = p.outs[g] + pix * cg + (co - p.oc0[g]);
                        const float v0 = fin(Y[a][b][cb][e] + bm[cb][e]);
                        if (co + 1 < p.oc0[g + 1] && !((cg | (co - p.oc0[g])) & 1)) {
                            *reinterpret_cast<float2*>(dst) = float2{v0, fin(Y[a][b][cb][e + 1] + bm[cb][e + 1])};
                        } else {
                            dst[0] = v0;
                            if (co + 1 < Cout) {                          // the pair straddles two destinations (or is unaligned): scalar stores
                                const int g1 = co + 1 >= p.oc0[2] && p.n_outs > 2 ? 2 : co + 1 >= p.oc0[1] ? 1 : 0;
                                const int cg1 = p.oc0[g1 + 1] - p.oc0[g1], ga1 = p.oact[g1];
                                float v1 = Y[a][b][cb][e + 1] + bm[cb][e + 1];
                                v1 = ga1 == (int)Act::RELU ? fmaxf(v1, 0.f) : ga1 == (int)Act::SIGMOID ? 1.0f / (1.0f + expf(-v1)) : v1;
                                p.outs[g1][pix * cg1 + (co + 1 - p.oc0[g1])] = v1;
                            }
                        }
                    }
            }
    }
#ifdef FACEHIP_W2_PROF
    if (lane == 0 && p.slabs && blockIdx.x < (1u << 17)) {                 // this wave's mean shader clock in MHz x 10 -> the diagnostic buffer (never an output)
        const long long dc = __builtin_readcyclecounter() - prof_c0, dr = (long long)__builtin_amdgcn_s_memrealtime() - prof_r0;
        reinterpret_cast<float*>(p.slabs)[blockIdx.x] = (float)(dc * 1000 / (dr + 1));
    }
#endif
}

// ------------------------------------------------------------------------------------------------------------------------------------
// wino2_x3_kernel — the same algorithm with its products on v_mfma_f32_16x16x32_bf16: fp32 products from three bf16 pieces per operand
// and six MFMAs per 32-deep step (gemm_tile.h: THE SPLIT RULE, THE PRODUCT ORDER), 0.375 of the f32 instruction's matrix-pipe cycles.
// Plain layers only (Cout % 64 == 0, no merged outputs).  What differs from wino2_kernel is the K loop and the weight image alone:
//   * the bf16 instruction's C layout (col = lane & 15, row = 4 (lane >> 4) + reg) is the f32 one's, so lane = tile, accumulator block
//     cb = channels 16 cb + 4 kq + e, and the whole tile body above applies unchanged;
//   * K ORDER BY PERMUTATION: a sum over K does not care which eight channels a lane holds as long as A and B agree.  The patch reads stay
//     w2_read_patch's (the same rb[], the same swizzle, column 4 g + kq: conflict-free, scripts/wino2_banks.py); step s in {0, 1}
//     of a frequency takes the groups g = 2 s and 2 s + 1, so B element j of lane (tn, kq) is channel 16 (2 s + (j >> 2)) + 4 kq + (j & 3)
//     and the weight image (wino2_pack_weights_x3) carries the same permutation;
//   * per step: 8 ds_read_b128 -> two float4 of V (w2_form_v) -> gemm_split3 on the pair -> 6 CB MFMAs,
//     product-outer, cb-inner: l h, h l, m m, m h, h m, h h (weight piece first);
//   * REGISTERS: ONE patch buffer — the next step's eight reads go out as soon as V is formed and land under the split and the MFMAs
//     (32 registers instead of the 64 of wino2_kernel's double buffer); the weight ring stays two steps deep (2 x 3 x CB x 4 registers).
// <CB = 2, NW = 2> is the one instantiation: 160 registers, three waves per SIMD — the six workgroups per CU the halo allows.  <4, 1> at one
// wave per SIMD (238 + 32 registers, four workgroups per CU) measured 0.85-0.93 of the f32 kernel where this one has 0.75-0.89
// (profiles/wino2_x3.md); at two waves per SIMD it would spill.
template <int CB, int NW>
__global__ __launch_bounds__(64 * NW, 3) void wino2_x3_kernel(const ConvArgs p, const int tiles_n, const int tgx, const int tgy) {
    extern __shared__ v4f w2sm[];
    char* const halo = reinterpret_cast<char*>(w2sm);                      // [5][5] plane pixels x [4 parity planes] x 16 x 16 B
    const int lane = threadIdx.x & 63;
    const int wv = NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const W2Walk t = w2_walk(lane, tiles_n, tgx, tgy);
    w2_load_halo<NW>(p, halo, lane, wv, t.gn, t.gy, t.gx);
    unsigned rb[16];
    w2_patch_addrs(rb, halo, t.tr, t.tc, t.kq);
    // weights of this column tile and wave: step k = 2 f + s is 3 planes x CB fragments of 1 KB (64 lanes x 8 bf16), the waves' steps
    // interleaved: [16 f][2 s][NW][3][CB][64][8].  A wave-uniform running pointer + the lane's 16-byte offset, as in wino2_kernel.
    constexpr unsigned WSTEP = 3 * CB * 1024;
    const char* wstep = reinterpret_cast<const char*>(p.wt) + ((size_t)t.tile_n * 32 * NW + (size_t)wv) * WSTEP;
    const unsigned wlane = lane * 16;
    bf16x8 wr[2][3][CB] = {};                                              // [ring][plane h, m, l][cb]
    auto fetch_w = [&](bool advance, int buf) __attribute__((always_inline)) {
        unsigned adv = advance ? NW * WSTEP : 0;
        asm volatile("" : "+s"(adv));
        wstep += adv;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) wr[buf][pl][cb] = *reinterpret_cast<const bf16x8*>(wstep + wlane + (pl * CB + cb) * 1024);
    };
    v4f Y[2][2][CB], Mp[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        Mp[cb] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) Y[a >> 1][a & 1][cb] = v4f{0.f, 0.f, 0.f, 0.f};
    }
    v4f d[8] = {};                                                         // the patch values of ONE step: groups g = 2 s (0..3) and 2 s + 1 (4..7)
    auto fetch_d = [&](auto fc, auto sc) __attribute__((always_inline)) {
        constexpr int f = decltype(fc)::value, s = decltype(sc)::value;
        w2_read_patch<f>(d, rb, 2 * s);
        w2_read_patch<f>(d + 4, rb, 2 * s + 1);
    };
    auto stage = [&](auto fc) __attribute__((always_inline)) {
        constexpr int f = decltype(fc)::value;
        v4f M[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) M[cb] = v4f{0.f, 0.f, 0.f, 0.f};
        auto step = [&](auto sc) __attribute__((always_inline)) {
            constexpr int s = decltype(sc)::value, k = f * 2 + s;
            fetch_w(k + 1 < 32, (k + 1) & 1);                              // fragments of step k + 1 (past the end: a harmless re-fetch)
            __builtin_amdgcn_sched_barrier(0);
            v4f v[2];
            w2_form_v<f>(v, d);
            asm volatile("" : "+v"(v[0]), "+v"(v[1]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (s == 0) fetch_d(IC<f>{}, IC<1>{});               // the patch buffer is free: the next step's reads land under the MFMAs
            else if constexpr (f < 15) fetch_d(IC<f + 1>{}, IC<0>{});
            bf16x8 vh, vm, vl;
            gemm_split3(v[0], v[1], vh, vm, vl);
            asm volatile("" : "+v"(vh), "+v"(vm), "+v"(vl));
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8 (&w)[3][CB] = wr[k & 1];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[2][cb], vh, M[cb], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0][cb], vl, M[cb], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1][cb], vm, M[cb], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[1][cb], vh, M[cb], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0][cb], vm, M[cb], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) M[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[0][cb], vh, M[cb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        };
        step(IC<0>{});
        w2_y_update<(f + 15) & 15, CB>(Y, Mp);                             // the previous frequency's result -> the outputs, in the shadow of this one's MFMAs
        step(IC<1>{});                                                     // (for f = 0, Mp = 0 is added: exact, and +0 stays +0)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) Mp[cb] = M[cb];
        __builtin_amdgcn_sched_barrier(0);
    };
    fetch_w(false, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // the halo has landed: LDS-DMA is ordered for its own wave by vmcnt alone
    if constexpr (NW > 1) __syncthreads();                                 // ... and for the sibling wave's pieces by the workgroup's only barrier
    fetch_d(IC<0>{}, IC<0>{});
    w2_each_freq(stage);
    w2_y_update<15, CB>(Y, Mp);
    asm volatile("" ::: "memory");                                         // (fenced: w2_store_plain)
    __builtin_amdgcn_sched_barrier(0);
    w2_store_plain<CB>(p, Y, t.gn, 2 * (4 * t.gy + t.tr), 2 * (4 * t.gx + t.tc), (t.tile_n * NW + wv) * 16 * CB + 4 * t.kq);
}

bool shape_ok(int Cin, int Cout) { return Cin == 64 && (Cout % 64 == 0 || Cout <= 32); }   // (<= 32: merged outputs only, see wino2_ok)

constexpr int w2_groups(int extent) { return ((extent + 1) / 2 + 3) / 4; }   // 4 x 4 tile groups (8 x 8 outputs) along a map side

// One workgroup of NW waves per (tile group, column tile of COLS channels); KERNEL(args, tiles_n, tgx, tgy) with 25.6 KB of dynamic LDS.
template <auto KERNEL, int COLS, int NW>
void launch_w2(const ConvArgs& a, hipStream_t s) {
    const int tgy = w2_groups(a.H), tgx = w2_groups(a.W);
    const long n_tg = (long)a.B * tgy * tgx;
    const int tiles_n = (a.Cout + COLS - 1) / COLS;
    // The kernels XOR swizzle keys into ABSOLUTE LDS addresses (w2_patch_addrs, w2_read_patch): that equals base + (offset ^ key) only while
    // the dynamic LDS base is 256-byte aligned, i.e. 0 — true as long as the kernel declares no static __shared__ object.  Checked once per
    // instantiation.
    static const bool lds_ok = [] {
        hipFuncAttributes fa{};
        FH_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(KERNEL)));
        return fa.sharedSizeBytes % 256 == 0;
    }();
    if (!lds_ok) throw std::runtime_error("wino2: static LDS moved the halo off its 256-byte alignment (see the address XOR in w2_read_patch)");
    KernelTimer& timer = KernelTimer::get();
    timer.begin(s);
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)(n_tg * tiles_n)), dim3(64 * NW), 25600, s, a, tiles_n, tgx, tgy);
    // booked with the FLOPs the matrix cores EXECUTE (padded tiles / channels included); bytes slot: the layer's direct-form FLOPs, as tag 7
    timer.end(s, 12, 2.0 * 16 * 16.0 * (double)n_tg * a.Cin * ((double)COLS * tiles_n), a.t_flops);
}

}  // namespace

// The two packers below each keep their own fp64 G g G^T loop and the x3 packer its own statement of THE SPLIT RULE: one shared U function
// and a named host split (byte-identical images) changed the packers' speed, and scripts/wino2_bench.py, which packs on the host in front
// of every launch, then measured 56x56x64 -> 128 4-7 % slower on BOTH kernels with the kernels' code unchanged
// (profiles/wino2_tile_refactor.md 3: new kernels + these packers run at the parent's level, the parent's kernels + shared packers do not).
// U_f = G g G^T per (output channel, input channel) in fp64, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], in the order the kernel streams it:
// [column tile][16 f][4 g][CB blocks of 16 channels][64 lanes (m = lane & 15, kq = lane >> 4)][4 floats],
// element = U_f[cout = 16 CB tn + 16 cb + m][cin = 16 g + 4 kq + e]; channels >= Cout are zero rows.  w = [Cout][9 taps][Cin] (the engine's layout).
size_t wino2_weight_floats(int Cin, int Cout) { return (size_t)16 * Cin * (Cout <= 32 ? 32 : Cout); }
void wino2_pack_weights(const float* w, int Cout, int Cin, float* dst) {
    static const double Gm[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    if (!shape_ok(Cin, Cout)) throw std::runtime_error("wino2_pack_weights: layer shape not supported");
    const int CB = Cout <= 32 ? 2 : 4;
    memset(dst, 0, wino2_weight_floats(Cin, Cout) * sizeof(float));
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            double g[3][3], t[4][3];
            for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = w[((size_t)co * 9 + k) * Cin + ci];
            for (int i = 0; i < 4; ++i)
                for (int x = 0; x < 3; ++x) t[i][x] = Gm[i][0] * g[0][x] + Gm[i][1] * g[1][x] + Gm[i][2] * g[2][x];
            const int tn = co / (16 * CB), cb = (co % (16 * CB)) / 16, m = co % 16;
            const int j = ci / 16, kq = (ci % 16) / 4, e = ci % 4;
            for (int i = 0; i < 4; ++i)
                for (int jj = 0; jj < 4; ++jj) {
                    const double u = t[i][0] * Gm[jj][0] + t[i][1] * Gm[jj][1] + t[i][2] * Gm[jj][2];
                    const size_t step = ((size_t)tn * 16 + (i * 4 + jj)) * 4 + j;
                    dst[(step * CB + cb) * 256 + (kq * 16 + m) * 4 + e] = (float)u;
                }
        }
}

// The three-piece bf16 image of the same U for wino2_x3_kernel: U_f in fp64, rounded to fp32, split by THE SPLIT RULE (gemm_tile.h) on the
// host.  [column tile of 64][16 f][2 s][2 waves][3 planes h, m, l][2 cb][64 lanes (m = lane & 15, kq = lane >> 4)][8 bf16];
// element j of lane (m, kq) in step s = U_f[cout = 64 tn + 32 wave + 16 cb + m][cin = 16 (2 s + (j >> 2)) + 4 kq + (j & 3)] — the
// K permutation of the kernel's patch reads.  6 bytes per element.
bool wino2_x3_shape_ok(int Cin, int Cout) { return Cin == 64 && Cout > 0 && Cout % 64 == 0; }
size_t wino2_x3_weight_floats(int Cin, int Cout) { return (size_t)16 * Cin * Cout * 3 / 2; }
void wino2_pack_weights_x3(const float* w, int Cout, int Cin, unsigned short* dst) {
    static const double Gm[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    if (!wino2_x3_shape_ok(Cin, Cout)) throw std::runtime_error("wino2_pack_weights_x3: layer shape not supported");
    constexpr int CB = 2, nw = 2;                                          // wino2_x3_kernel<2, 2>
    auto bits = [](float x) { unsigned u; memcpy(&u, &x, 4); return u; };
    auto flt = [](unsigned u) { float x; memcpy(&x, &u, 4); return x; };
    auto rne = [&](float x) { const unsigned u = bits(x); return (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u; };   // finite x: bf16, nearest even
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            double g[3][3], t[4][3];
            for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = w[((size_t)co * 9 + k) * Cin + ci];
            for (int i = 0; i < 4; ++i)
                for (int x = 0; x < 3; ++x) t[i][x] = Gm[i][0] * g[0][x] + Gm[i][1] * g[1][x] + Gm[i][2] * g[2][x];
            const int tn = co / 64, wave = (co % 64) / (16 * CB), cb = (co % (16 * CB)) / 16, m = co % 16;
            const int gq = ci / 16, kq = (ci % 16) / 4, e = ci % 4, st = gq >> 1, j = 4 * (gq & 1) + e;
            for (int f = 0; f < 16; ++f) {
                const int i = f >> 2, jj = f & 3;
                const volatile float u = (float)(t[i][0] * Gm[jj][0] + t[i][1] * Gm[jj][1] + t[i][2] * Gm[jj][2]);
                const unsigned hb = bits(u) & 0xffff0000u;
                const volatile float r = u - flt(hb);
                const unsigned mb = rne(r);
                const volatile float q = r - flt(mb);
                const unsigned pieces[3] = {hb, mb, rne(q)};
                const size_t step = (((size_t)tn * 16 + f) * 2 + st) * nw + wave;
                for (int pl = 0; pl < 3; ++pl) dst[(((step * 3 + pl) * CB + cb) * 64 + kq * 16 + m) * 8 + j] = (unsigned short)(pieces[pl] >> 16);
            }
        }
}

bool wino2_ok(const ConvArgs& a) {
    if (!(a.ks == 3 && a.stride == 1 && a.pad == 1 && a.H == a.Ho && a.W == a.Wo && a.H >= 2 && a.W >= 2 && shape_ok(a.Cin, a.Cout) &&
          a.act != (int)Act::SIGMOID && !a.sc_in && !a.dw_w && !a.u8_src && a.wt_group_rows == 0 &&
          (a.res_mode == (int)ResMode::NONE || a.res_mode == (int)ResMode::SAME)))
        return false;
    if (a.n_outs > 0)                                                      // merged sibling convolutions: per-range destinations, no residual / second output
        return a.Cout <= 32 && a.res_mode == (int)ResMode::NONE && !a.out2 && !a.bias_cls;
    return a.Cout % 64 == 0;                                               // plain layers: whole 64-channel column tiles
}

// diagnostic runs (FACEHIP_W2_ABLATE set, diagnostic build): per-workgroup shader-clock stamps land in a 512 KB device buffer; returns their
// median in MHz (0 in production builds, which never write it)
static float* g_w2_clock = nullptr;
double wino2_debug_clock_mhz() {
    if (!g_w2_clock) return 0.0;
    std::vector<float> h(1 << 17);
    if (hipMemcpy(h.data(), g_w2_clock, h.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 0.0;
    std::vector<float> v;
    for (float x : h) if (x > 0.f) v.push_back(x);
    if (v.empty()) return 0.0;
    std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
    return v[v.size() / 2] / 10.0;
}

// one-wave workgroups of the launch, in units of four (= the 256-thread workgroups the engine's cross-over is expressed in)
long wino2_blocks(const ConvArgs& a) {
    return (long)a.B * w2_groups(a.H) * w2_groups(a.W) * ((a.Cout + 63) / 64) / 4;
}

// a.wt = wino2_pack_weights' image of the filter; everything else as for launch_conv
void launch_wino2(const ConvArgs& a_in, hipStream_t s) {
    if (!wino2_ok(a_in)) throw std::runtime_error("launch_wino2: layer shape not supported");
    ConvArgs a = a_in;
    a.zeros = conv_zero_line();
    static const int ablate = [] { const char* e = getenv("FACEHIP_W2_ABLATE"); return e ? atoi(e) : -1; }();
    a.sk_test_drop = ablate < 0 ? 0 : ablate;                              // (read by diagnostic builds only: scripts/wino2_prof.sh)
    if (ablate >= 0 && !g_w2_clock) { void* q = nullptr; if (hipMalloc(&q, sizeof(float) << 17) == hipSuccess) g_w2_clock = (float*)q; }
    if (g_w2_clock) (void)hipMemsetAsync(g_w2_clock, 0, sizeof(float) << 17, s);
    a.slabs = g_w2_clock;
    // plain 64-channel column tiles: two waves of 32 channels around one halo (FACEHIP_WINO2_NW=1: the one-wave form of round 4, for A / B timing)
    static const int nw = [] { const char* e = getenv("FACEHIP_WINO2_NW"); return e ? atoi(e) : 2; }();
    if (a.Cout <= 32) launch_w2<wino2_kernel<2, 1, true>, 32, 1>(a, s);
    else if (nw == 2) launch_w2<wino2_kernel<2, 2, false>, 64, 2>(a, s);
    else launch_w2<wino2_kernel<4, 1, false>, 64, 1>(a, s);
}

// The same layer on wino2_x3_kernel: a.wt = wino2_pack_weights_x3's image.  Plain layers only.
bool wino2_x3_ok(const ConvArgs& a) { return wino2_ok(a) && a.n_outs == 0 && wino2_x3_shape_ok(a.Cin, a.Cout); }
long wino2_x3_workgroups(const ConvArgs& a) { return (long)a.B * w2_groups(a.H) * w2_groups(a.W) * (a.Cout / 64); }
void launch_wino2_x3(const ConvArgs& a_in, hipStream_t s) {
    if (!wino2_x3_ok(a_in)) throw std::runtime_error("launch_wino2_x3: layer shape not supported");
    ConvArgs a = a_in;
    a.zeros = conv_zero_line();
    launch_w2<wino2_x3_kernel<2, 2>, 64, 2>(a, s);
}

}  // namespace fh
