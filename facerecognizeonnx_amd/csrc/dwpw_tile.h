// dwpw_tile.h — the tile body of the PERSISTENT depthwise 3x3 -> pointwise 1x1 kernels, each piece once: dwpw_reg_kernel,
// dwpw_reg2_kernel and front_kernel (dwpw_mfma.hip) are composed from it; stem_mfma_kernel (stem.hip) takes the walk.
//
// The tile: 8 x 16 output pixels, 256 threads = 4 waves.  A wave owns 32 pixels for the whole K loop, lane = (pixel r = lane & 31, half
// h = lane >> 5).  For the 8-channel step j the lane evaluates the depthwise 3x3 (+bias +ReLU) of channels 8j + 4h .. + 3 of ITS pixel
// straight from the halo image in LDS — a float4 that is exactly the B fragment v_mfma_f32_32x32x2_f32 wants from that lane — so the
// depthwise result goes from the vector ALU into the matrix core without touching LDS and no wave waits for another inside a tile.
//   1. walk      the LDS-only barrier, the priority rotation, the XCD-contiguous run of a workgroup and the division-free tile advance;
//   2. K steps   the hand-scheduled loop: one MFMA per slot, the next step's depthwise behind it;
//   3. halo      next tile's halo global -> registers (buffer loads, zero fill in hardware), registers -> LDS;
//   4. prologue / epilogue   constants -> LDS, the lane's pixel and fragment addresses, accumulators from the bias, floor + float4 stores;
//   5. launch    grid of a persistent kernel, one-time LDS opt-in, the priority switch;
//   6. stamps    the six phase sums of a -DFACEHIP_DWPW_PROF build.
// The kernels keep what is their own: their names, template parameters, __launch_bounds__ and LDS sizes, the order of the phases of a
// tile (one halo image or two parts taking turns in one buffer, a stem in front) and the depth of the tap ring (RA / RING), which is
// what each kernel's register budget allows.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "gemm_tile.h"
#include "kernels.h"

namespace fh {

constexpr int DP_TH = 8, DP_TW = 16, DP_BM = DP_TH * DP_TW;            // 128 output pixels per tile
constexpr int DP_HW = DP_TW + 2, DP_HALO = (DP_TH + 2) * DP_HW;         // 10 x 18 = 180 halo pixels (stride 1)

// ================================================================== 1. walk ==========================================================
// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, which would make every barrier of a tile loop wait
// for the NEXT tile's prefetched loads
__device__ __forceinline__ void lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// Wave priority by tile count.  A SIMD's instruction arbiter prefers its OLDEST wave: with several persistent workgroups per CU and a
// static share of tiles each, the first-launched workgroup runs at full speed and the last-launched one on what is left (front_kernel's
// phase stamps: a workgroup's loop took 586 k / 690 k / 811 k / 936 k cycles by launch order on its CU) — the kernel ends with the slowest
// while the fast ones' slots idle.  s_setprio beats age, so every workgroup takes each level in turn.
__device__ __forceinline__ void rotate_wave_priority(int it) {
    switch (it & 3) {                                                      // (s_setprio takes an immediate)
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// Tiles of a persistent workgroup.  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8), each with its own L2: XCD x owns the
// CONTIGUOUS run [run0, run1) of the tiles_total tiles, and its wgs workgroups walk it side by side — workgroup wg takes run0 + wg,
// run0 + wg + wgs, ... — so neighbouring tiles (shared halo / window rows) are in flight on one L2 at the same time.
// (gridDim.x is a multiple of 8.)
struct XcdRun {
    int run0, run1, wg, wgs;
};
__device__ __forceinline__ XcdRun xcd_run(const int tiles_total) {
    const int xcd = blockIdx.x & 7, wg = blockIdx.x >> 3, wgs = gridDim.x >> 3;
    const int q8 = tiles_total >> 3, r8 = tiles_total & 7;
    const int run0 = xcd * q8 + min(xcd, r8), run1 = run0 + q8 + (xcd < r8 ? 1 : 0);
    return XcdRun{run0, run1, wg, wgs};
}

// Tile t = (n * tiles_y + tyi) * tiles_x + txi moved on by the same `stride` tiles every time: the coordinates advance by the same three
// steps, no division in the loop.
struct TileWalk {
    int n, tyi, txi;
    int d_n, d_ty, d_tx, tiles_x, tiles_y;
    __device__ __forceinline__ TileWalk(const int t, const int stride, const int tiles_x_, const int tiles_y_)
        : n(t / (tiles_x_ * tiles_y_)), tyi((t / tiles_x_) % tiles_y_), txi(t % tiles_x_),
          d_n(stride / (tiles_x_ * tiles_y_)), d_ty((stride / tiles_x_) % tiles_y_), d_tx(stride % tiles_x_), tiles_x(tiles_x_), tiles_y(tiles_y_) {}
    __device__ __forceinline__ void advance() {
        txi += d_tx; if (txi >= tiles_x) { txi -= tiles_x; ++tyi; }
        tyi += d_ty; if (tyi >= tiles_y) { tyi -= tiles_y; ++n; }
        n += d_n;
    }
};

// ================================================================== 3. halo (geometry first: the K steps index it) ===================
// Halo of an 8 x 16 output tile under a depthwise stride DS: rows DS oy - 1 .. DS oy + 1 -> (8 - 1) DS + 3 rows, same for the columns:
// 10 x 18 = 180 pixels (DS = 1), 17 x 33 = 561 (DS = 2).  In LDS a pixel is CQ float4 of channels at a pitch of PQ = CQ + 1 float4: odd, so
// the 16-byte reads of neighbouring pixels spread over all banks.
template <int DS>
struct DwpwHalo {
    static constexpr int HH = (DP_TH - 1) * DS + 3, HWD = (DP_TW - 1) * DS + 3, HALO = HH * HWD;
    static constexpr int HW2 = (HWD + 1) / 2;
    // LDS slot of halo pixel hp = hy * HWD + hx.  Stride 1: hp itself.  Stride 2: a row's EVEN columns first, then its odd ones — lane =
    // output pixel reads input column 2 px + kx, i.e. slot px + (kx >> 1) of plane kx & 1: neighbouring lanes are ONE pixel pitch (odd in
    // float4) apart.  With interleaved columns they were two apart: every halo index of an instruction had the same parity, 8 bank quads
    // for the 16 lanes of a ds_read_b128 group, a 2-way conflict on every tap (SQ_LDS_BANK_CONFLICT 0.34 of the LDS cycles).
    static __device__ __forceinline__ constexpr int slot(const int hp) {
        if (DS == 1) return hp;
        const int hy = hp / HWD, hx = hp - hy * HWD;
        return hy * HWD + (hx & 1) * HW2 + (hx >> 1);
    }
    // ... and of tap (ky, kx) relative to the slot of the lane's own pixel (py * DS * HWD + px)
    static __device__ __forceinline__ constexpr int tapoff(const int ky, const int kx) {
        return DS == 1 ? ky * HWD + kx : ky * HWD + (kx & 1) * HW2 + (kx >> 1);
    }
};

// One part of a tile's halo on its way global -> registers -> LDS: CQP float4 columns per pixel starting at column Q0 of the block's
// CQ (the whole pixel: CQP = CQ, Q0 = 0; dwpw_reg2_kernel: two parts that take turns in one LDS buffer).  The NEXT tile's part is
// fetched while this tile computes — no second halo buffer, so the occupancy stays — and parked between two LDS-only barriers.
// It comes in through BUFFER loads with a per-image descriptor: rows above / below the image are out of range and read as zero in
// hardware, columns left / right of it are pushed out of range by one select (first / last tile column only) — no per-item bounds
// arithmetic, no branches, and the loads of a tile issue back to back.  Per thread and item the byte offset relative to the tile's halo
// origin is tile-invariant (voff); per tile: one add each.
template <int DS, int CQ, int CQP, int Q0>
struct DwpwHaloPart {
    using H = DwpwHalo<DS>;
    static constexpr int ITEMS = H::HALO * CQP, NP = (ITEMS + 255) / 256;  // float4 of the part, per thread
    v4f pf[NP];
    int voff[NP];

    __device__ __forceinline__ void init(const ConvArgs& p, const int tid) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = min(tid + 256 * k, ITEMS - 1);
            const int hp = i / CQP, q = i - hp * CQP;
            const int hy = hp / H::HWD, hx = hp - hy * H::HWD;
            voff[k] = ((hy * p.W + hx) * (CQ * 4) + 4 * (Q0 + q)) * 4;
        }
    }
    // tile t -> registers (issued, not waited for)
    __device__ __forceinline__ void prefetch(const ConvArgs& p, const int img_bytes, const int t, const int per_img, const int tiles_x, const int tid) {
        constexpr int C = CQ * 4;
        const int n = t / per_img, rem = t - n * per_img;
        const int tyi = rem / tiles_x, txi = rem - tyi * tiles_x;
        const int y0 = tyi * DP_TH * DS - 1, x0 = txi * DP_TW * DS - 1;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in + (size_t)n * p.H * p.W * C), 0, img_bytes, 0x00020000);
        const int tile_off = (y0 * p.W + x0) * C * 4;                       // (negative on the first tile row / column: wraps out of range)
        int vo[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) vo[k] = tile_off + voff[k];
        if (x0 < 0 || x0 + H::HWD > p.W) {                                  // wave-uniform: only the first / last tile column
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int i = min(tid + 256 * k, ITEMS - 1);
                const int hx = (i / CQP) % H::HWD;
                vo[k] = (unsigned)(x0 + hx) < (unsigned)p.W ? vo[k] : (int)0x80000000;
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) pf[k] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo[k], 0, 0));
    }
    // registers -> halo image of pixel pitch PQ (waits for the loads issued a whole tile ago)
    template <int PQ>
    __device__ __forceinline__ void park(v4f* const halo, const int tid) const {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = tid + 256 * k;
            if (i < ITEMS) { const int hp = i / CQP; halo[H::slot(hp) * PQ + (i - hp * CQP)] = pf[k]; }
        }
    }
};

// ================================================================== 2. K steps ======================================================
// Where a lane reads its A fragments (pointwise weights: row = output column n, 4 k of half h) of column group jn: float4 index into
// Wl [STEPS][2][Cout], the fragment-order image of dwpw_reg_kernel / dwpw_reg2_kernel — step j's fragment is at 2 j Cout + wrow[jn].
template <int TN>
__device__ __forceinline__ void dwpw_wrows(int (&wrow)[TN], const int Cout, const int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) wrow[jn] = h * Cout + min(32 * jn + r, Cout - 1);   // rows >= Cout: any valid address (their columns are never stored)
}

// Steps [J0, J1) of the block's K loop (a step = 8 channels) on the halo image now in LDS, whose float4 columns 2 (j - J0) + h hold step
// j's channels; TN 32-column groups of accumulators.  hbase = the lane's pixel in the halo (+ h), pixel pitch PQ; dbase = the depthwise
// taps + bias [10][CQ] (+ h).  The A fragments come from W, one of two images:
//   SWZ = false  Wl in fragment order, step j at W[2 j Cout + wrow[jn]], double-buffered through wq[2] one group (= four slots) ahead;
//   SWZ = true   front_kernel's Wt [32 rows][8 float4], filled by LDS-DMA and XOR-swizzled like a lean-GEMM tile (gemm_tile.h): wrow[0] = the
//                lane's row, TN = 1, one float4 per step, read at the step.
// Hand-scheduled.  Left to itself the compiler emits, per step, nine times (2 ds_read, wait, 2 FMA) and only then the step's MFMAs
// (ds_read, wait, 4 MFMA): every LDS latency exposed, nothing beside the matrix pipe.  So the order is written out: one MFMA per SLOT;
// behind it the slot's share of the NEXT step's depthwise — each tap's two LDS reads are issued RA tap-slots ahead of their FMAs (ring
// registers hv / dv, RING = RA + 1 deep: as deep as the kernel's register budget allows) — and a sched_barrier(0) pins the slot.  The
// counted lgkmcnt waits the compiler inserts are then exact (LDS returns in order).  The first step's depthwise has nothing to hide
// behind.  ReLU (floor 0) or none (floor -inf) is one v_max: a branch per step would end the basic block and with it the overlap.
// (W, Cout and wrow are plain arguments on purpose: handed over as a policy object or a functor, the same expressions came out of the
// compiler with up to 16 more VGPRs and a second spill — profiles/dwpw_tile_refactor.md.)
template <int J0, int J1, int TN, int RA, int RING, int DS, int PQ, int CQ, bool SWZ>
__device__ __forceinline__ void dwpw_k_steps(v16f (&acc)[TN], const v4f* const hbase, const v4f* const dbase, const float dw_floor, const v4f* const W,
                                             const int Cout, const int (&wrow)[TN]) {
    static_assert(!SWZ || TN == 1, "the swizzled image holds one 32-column group");
    constexpr int NJ = J1 - J0;
    constexpr int NS = 4 * TN;                                              // MFMA slots per 8-channel step
    constexpr int NT = 10;                                                  // tap-slots per step: the depthwise bias, then the 9 taps
    constexpr int AHEAD = SWZ ? 0 : 1;
    v4f hv[RING], dv[RING], wq[2];
    auto issue = [&](int G) __attribute__((always_inline)) {               // LDS reads of tap-slot G = NT * (step - J0) + t
        const int jl = G / NT, tt = G % NT;
        if (jl >= NJ) return;
        dv[G % RING] = dbase[(tt == 0 ? 9 : tt - 1) * CQ + 2 * (J0 + jl)];
        if (tt > 0) hv[G % RING] = hbase[DwpwHalo<DS>::tapoff((tt - 1) / 3, (tt - 1) % 3) * PQ + 2 * jl];
    };
    v4f an;
    auto consume = [&](int G) __attribute__((always_inline)) {
        if (G / NT >= NJ) return;
        if (G % NT == 0) an = dv[G % RING]; else an += hv[G % RING] * dv[G % RING];
    };
    auto wfrag = [&](int grp) __attribute__((always_inline)) {             // A fragment of (step J0 + grp / TN, column group grp % TN)
        if (grp >= NJ * TN) return;
        if constexpr (SWZ) {
            const int lane = threadIdx.x & 63;
            wq[grp & 1] = W[wrow[0] + ((2 * (J0 + grp) + (lane >> 5)) ^ (((lane & 31) >> 1) & 7))];
        } else {
            wq[grp & 1] = W[2 * (J0 + grp / TN) * Cout + wrow[grp % TN]];
        }
    };
    if (AHEAD) wfrag(0);
#pragma unroll
    for (int G = 0; G < RA; ++G) issue(G);
#pragma unroll
    for (int G = 0; G < NT; ++G) { issue(G + RA); consume(G); }
    v4f a;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = fmaxf(an[e], dw_floor);
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            const int grp = j * TN + sl / 4;
            if (sl % 4 == 0) wfrag(grp + AHEAD);
            acc[sl / 4] = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[grp & 1][sl % 4], a[sl % 4], acc[sl / 4], 0, 0, 0);
#pragma unroll
            for (int G = NT * (j + 1) + sl * NT / NS; G < NT * (j + 1) + (sl + 1) * NT / NS; ++G) { issue(G + RA); consume(G); }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ================================================================== 4. prologue and epilogue ========================================
// once per workgroup: the block's constants -> LDS, resident for the kernel's lifetime behind the halo image (visible after the next barrier):
// dwl [10][CQ] the 9 depthwise taps + bias, Wl [STEPS][2][Cout] the pointwise weights as A fragments (n = row, 4 k of half h), pwb [32 * TN] the
// pointwise bias (zero behind Cout)
template <int CQ, int TN>
__device__ __forceinline__ void dwpw_fill_constants(v4f* const dwl, v4f* const Wl, float* const pwb, const ConvArgs& p, const int tid) {
    constexpr int C = CQ * 4, STEPS = C / 8;
    const int Cout = p.Cout;
    for (int i = tid; i < 10 * CQ; i += 256) {
        const int k = i / CQ, q = i - k * CQ;
        dwl[i] = *reinterpret_cast<const v4f*>(k < 9 ? p.dw_w + (size_t)k * C + 4 * q : p.dw_b + 4 * q);
    }
    for (int i = tid; i < STEPS * 2 * Cout; i += 256) {
        const int n = i % Cout, jh = i / Cout;                             // jh = 2 j + h
        Wl[i] = *reinterpret_cast<const v4f*>(p.wt + (size_t)n * p.Kpad + 4 * jh);
    }
    for (int i = tid; i < 32 * TN; i += 256) pwb[i] = i < Cout ? p.bias[i] : 0.f;
}

// A lane's pixel (py, px) of the tile and its fragment addresses (float4 units): hbase + tapoff(ky, kx) * PQ + 2 (j - first step of the
// part), dbase + tap * CQ + 2 j.
// The wave's second pixel row takes its columns rotated by 2.  A ds_read_b128 serves lanes {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}
// together; with an odd pixel pitch the 16 addresses fall into 16 different bank quads iff the pixels' linear halo indices differ mod 16,
// and a halo row is 18 = 16 + 2 pixels: unrotated, lanes 12 / 13 collide with lanes 26 / 27 and lanes 4 / 5 with lanes 18 / 19 — every
// fragment read took 8 LDS cycles instead of 4 (SQ_LDS_BANK_CONFLICT = 27-34 % of SQ_LDS_IDX_ACTIVE).  Stride 2 with its column planes
// (px indexes a plane): consecutive slots again and a row pitch of 2 * 33 = 66 = 64 + 2 slots — the same rotation.
struct DwpwLane {
    int py, px;
    const v4f* hbase;
    const v4f* dbase;
};
template <int DS, int PQ>
__device__ __forceinline__ DwpwLane dwpw_lane(const v4f* const halo, const v4f* const dwl, const int wid, const int lane) {
    const int r = lane & 31, h = lane >> 5;
    const int pix = wid * 32 + r, py = pix / DP_TW, px = (py & 1) ? (pix - py * DP_TW - 2) & (DP_TW - 1) : pix - py * DP_TW;
    return DwpwLane{py, px, halo + (py * DS * DwpwHalo<DS>::HWD + px) * PQ + h, dwl + h};
}

// accumulators start from the pointwise bias pwb [32 * TN]: lane half h holds columns 32 jn + 8 g + 4 h .. + 3 in quad g
template <int TN>
__device__ __forceinline__ void dwpw_acc_from_bias(v16f (&acc)[TN], const float* const pwb, const int h) {
#pragma unroll
    for (int jn = 0; jn < TN; ++jn)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4f b = *reinterpret_cast<const v4f*>(pwb + 32 * jn + 8 * g + 4 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[jn][4 * g + c] = b[c];
        }
}
// epilogue: lane = pixel (oy, ox) of image n, accumulator quads = 4 consecutive channels; ReLU or none as a floor, float4 stores.
// (Stride-2 form, 320x320x16 -> 160x160x40: the phase stamps show stores 6.3 k + next prefetch's issue 4.1 k of 16.4 k cycles per tile —
// queueing behind the memory pipeline.  Parking the wave's pixels in the halo rows it owns exclusively and writing them back as whole
// lines changed nothing (296 vs 301 us, stores still 5.9 k): it is the 4.6 TB/s of mixed read / write traffic itself, not the 16-byte
// pieces, that the block waits for.)
template <int TN>
__device__ __forceinline__ void dwpw_store(const v16f (&acc)[TN], const ConvArgs& p, const int n, const int oy, const int ox, const int h, const float out_floor) {
    const int Cout = p.Cout;
    if (oy < p.Ho && ox < p.Wo) {
        float* __restrict__ orow = p.out1 + (((size_t)n * p.Ho + oy) * p.Wo + ox) * Cout;
#pragma unroll
        for (int jn = 0; jn < TN; ++jn)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = 32 * jn + 8 * g + 4 * h;
                if (co >= Cout) continue;
                v4f v;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = fmaxf(acc[jn][4 * g + c], out_floor);
                *reinterpret_cast<v4f*>(orow + co) = v;
            }
    }
}

// ================================================================== 6. stamps =======================================================
// -DFACEHIP_DWPW_PROF (scripts/dwpw_prof.sh): every wave sums the shader cycles of six phases of its tile loop, DWPW_STAMP(i) closing
// phase i, and leaves them in p.slabs as [workgroup][wave][8]: 6 phase sums, tile count, shader MHz x 10.
#ifdef FACEHIP_DWPW_PROF
struct DwpwStamps {
    long long ph[6] = {0, 0, 0, 0, 0, 0}, st0;
    int ntiles = 0;
    const long long clk0 = __builtin_readcyclecounter(), rt0 = __builtin_amdgcn_s_memrealtime();   // shader clock vs the constant 100 MHz counter
    __device__ __forceinline__ void tile() { st0 = __builtin_readcyclecounter(); ++ntiles; }
    __device__ __forceinline__ void stamp(const int i) { const long long now_ = __builtin_readcyclecounter(); ph[i] += now_ - st0; st0 = now_; }
    __device__ __forceinline__ void write(float* const slabs, const int wid, const int lane) const {
        if (lane == 0 && slabs) {
            long long* o = reinterpret_cast<long long*>(slabs) + ((size_t)blockIdx.x * 4 + wid) * 8;
            for (int i = 0; i < 6; ++i) o[i] = ph[i];
            o[6] = ntiles;
            o[7] = (__builtin_readcyclecounter() - clk0) * 1000 / ((long long)__builtin_amdgcn_s_memrealtime() - rt0 + 1);   // shader cycles per 100 MHz tick x 1000 = MHz x 10
        }
    }
};
#define DWPW_STAMP(i) stamps.stamp(i);
#else
struct DwpwStamps {
    __device__ __forceinline__ void tile() {}
    __device__ __forceinline__ void write(const float*, int, int) const {}
};
#define DWPW_STAMP(i)
#endif

// ================================================================== 5. launch =======================================================
static inline size_t dwpw_reg_lds(int CQ, int Cout, int TN, int DS, int CQH) {      // CQH = float4 columns per pixel of the halo image (pitch CQH + 1)
    const int halo = ((DP_TH - 1) * DS + 3) * ((DP_TW - 1) * DS + 3);
    return ((size_t)halo * (CQH + 1) + 10 * CQ + (size_t)(CQ / 2) * 2 * Cout) * 16 + (size_t)32 * TN * 4;
}
// A persistent kernel of OCC workgroups per CU over the 8 x 16 tiles of a.B x a.Ho x a.Wo: as many workgroups as fit the device (a.cus > 0:
// as if it had that many CUs — the tile-walk tests), a multiple of 8 (XCDs), never more than there are tiles rounded up to 8.
// FACEHIP_DWPW_PRIO=0: no priority rotation (A / B timing).
template <auto KERNEL, int OCC>
static void launch_dwpw_persistent(const ConvArgs& a, const size_t lds, hipStream_t s) {
    const int tiles_x = (a.Wo + DP_TW - 1) / DP_TW, tiles_y = (a.Ho + DP_TH - 1) / DP_TH;
    const int tiles_total = a.B * tiles_y * tiles_x;
    const int cus = a.cus > 0 ? a.cus : conv_num_cus();
    static bool attr_set = false;                                          // (per instantiation) dynamic LDS beyond the 64 KB default needs the opt-in
    if (!attr_set) {
        FH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    int grid = std::min((tiles_total + 7) / 8 * 8, cus * OCC);
    grid = std::max(8, grid / 8 * 8);
    ConvArgs ap = a;
    { static int pr = -1; if (pr < 0) { const char* e = getenv("FACEHIP_DWPW_PRIO"); pr = e ? atoi(e) : 1; } ap.no_prio = pr ? 0 : 1; }
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(256), lds, s, ap, tiles_x, tiles_y, tiles_total);
}

}  // namespace fh
