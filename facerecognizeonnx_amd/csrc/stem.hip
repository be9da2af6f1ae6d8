// stem.hip — the graph's first convolution (3x3, Cin = 3) fused with the image preprocess (FaceDetector::preprocess
// src/face_detector.cpp:120-136 / FaceRecognizer::preprocess src/face_recognizer.cpp:135-150): the BGR u8 frame is read once (1 byte
// per sample instead of a 4-byte float written and read back).  Letterbox area (inside the net input, outside the pasted image) = u8 0
// = -0.99609375 after normalisation; outside the net input = the conv's zero padding.  Three forms, chosen by launch_stem from the
// channel count: an LDS tile on the vector ALU, a thread per pixel with the weights in SGPRs plus a literal kernel for the frame around
// its interior (16 / 32 channels), the matrix cores (48 / 64).  Their shared pieces are stem_tile.h's; stem_pack_wfrag is at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "dwpw_tile.h"
#include "kernels.h"
#include "stem_fma.h"
#include "stem_tile.h"

namespace fh {

constexpr int STEM_TILE = 16;

// ---- LDS-tile form ----------------------------------------------------------------------------------------------------------
// Normalises a (TILE-1)*STRIDE+3 square of the frame into LDS and runs the 27-tap stencil on the vector ALU.  Thread = 4 output
// channels x its share of the tile's pixels; weights live in registers; persistent blocks.
template <int STRIDE>
__global__ __launch_bounds__(256) void stem_conv_u8_kernel(const StemArgs a, const int Ho, const int Wo, const int ntiles) {
    constexpr int IT = (STEM_TILE - 1) * STRIDE + 3;                 // input tile edge
    __shared__ float tile[IT * IT * 3];
    const int tid = threadIdx.x;
    const int tiles_x = (Wo + STEM_TILE - 1) / STEM_TILE, tiles_y = (Ho + STEM_TILE - 1) / STEM_TILE;
    const int Cout = a.Cout, G = Cout >> 2;                          // channel groups of 4
    const int c4 = tid % G;
    const int pix_per_pass = 256 / G;
    v4f w[27];                                                       // [tap][ci] for this thread's 4 channels, loaded ONCE per block
#pragma unroll
    for (int k = 0; k < 27; ++k) w[k] = *reinterpret_cast<const v4f*>(a.w27 + (size_t)k * Cout + c4 * 4);
    const v4f b4 = *reinterpret_cast<const v4f*>(a.bias + c4 * 4);
    v4f sl = {0.f, 0.f, 0.f, 0.f}, sc2 = {0.f, 0.f, 0.f, 0.f}, sh2 = {0.f, 0.f, 0.f, 0.f};
    if (a.slope) sl = *reinterpret_cast<const v4f*>(a.slope + c4 * 4);
    if (a.out2) { sc2 = *reinterpret_cast<const v4f*>(a.s2 + c4 * 4); sh2 = *reinterpret_cast<const v4f*>(a.t2 + c4 * 4); }
    // persistent blocks: each walks over many tiles, so the 27 weight vectors are fetched once
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int b = tl / (tiles_x * tiles_y);
        const int t = tl - b * tiles_x * tiles_y;
        const int oy0 = (t / tiles_x) * STEM_TILE, ox0 = (t % tiles_x) * STEM_TILE;
        const int iy0 = oy0 * STRIDE - 1, ix0 = ox0 * STRIDE - 1;
        const uint8_t* img = a.src + (size_t)b * a.img_stride;
        __syncthreads();                                             // previous tile fully consumed
        for (int i = tid; i < IT * IT; i += 256) {
            const int ty = i / IT, tx = i - ty * IT;
            const StemBytes<3> px = stem_byte<3>(img, a.step, iy0 + ty, ix0 + tx, 0, a.inH, a.inW, a.srcH, a.srcW);
            float r = 0.f, g = 0.f, bl = 0.f;
            if (px.at != StemAt::PAD) { r = (px.v[2] - 127.5f) / 128.0f; g = (px.v[1] - 127.5f) / 128.0f; bl = (px.v[0] - 127.5f) / 128.0f; }
            tile[i * 3 + 0] = r; tile[i * 3 + 1] = g; tile[i * 3 + 2] = bl;   // RGB order = graph channel order
        }
        __syncthreads();
        if (tid >= G * pix_per_pass) continue;
        for (int p = tid / G; p < STEM_TILE * STEM_TILE; p += pix_per_pass) {
            const int py = p / STEM_TILE, px = p - py * STEM_TILE;
            const int oy = oy0 + py, ox = ox0 + px;
            if (oy >= Ho || ox >= Wo) continue;
            v4f acc = b4;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float* tp = tile + ((py * STRIDE + ky) * IT + px * STRIDE + kx) * 3;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) acc += w[(ky * 3 + kx) * 3 + ci] * tp[ci];
                }
            stem_epilogue(acc, a.act, &sl, a.out1, a.out2, (((size_t)b * Ho + oy) * Wo + ox) * Cout + c4 * 4, &sc2, &sh2);
        }
    }
}

// ---- thread-per-pixel form ------------------------------------------------------------------------------------------------
// One thread = one output pixel x ALL output channels.  The 27 input bytes of the pixel's 3x3 window are fetched as 3 aligned dwords
// per image row straight from the u8 frame (neighbouring lanes overlap: L1 / L2 serve the re-reads, each byte leaves HBM once),
// converted with v_cvt_f32_ubyteN, and multiplied by weights that live in SGPRs (every lane uses the same 27 x COUT weights: uniform
// loads through the scalar cache, one SGPR operand per v_fmac).  No LDS, no barrier, ~60 VGPRs: 8 waves per SIMD hide the loads.
// The normalisation (v - 127.5) / 128 is folded into the weights on the host: wf = w / 128 (a power of two: exact) in BYTE order
// (B, G, R per pixel), biasf = bias - 127.5/128 * sum(w).  That only works where all nine taps are real image pixels, so this kernel
// covers the INTERIOR of the output map (stem_interior); the thin frame of pixels whose window touches the zero padding, the letterbox
// canvas or the first / last pixel of a row goes to stem_conv_border_kernel (literal arithmetic, per-tap bounds).
typedef const unsigned __attribute__((address_space(1))) gmem_u32;
template <int STRIDE, int COUT>
__global__ __launch_bounds__(256) void stem_conv_px_kernel(const uint8_t* __restrict__ src, long img_stride, int step, int Ho, int Wo, int x0,
                                                           int y0, int nx, int ny, int B, const float* __restrict__ wf,
                                                           const float* __restrict__ biasf, const float* __restrict__ slope, int act,
                                                           float* __restrict__ out1, float* __restrict__ out2, const float* __restrict__ s2,
                                                           const float* __restrict__ t2) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * ny * nx) return;
    const int ox = x0 + idx % nx;
    const int r0 = idx / nx;
    const int oy = y0 + r0 % ny, b = r0 / ny;
    const uint8_t* p = src + (size_t)b * img_stride + (size_t)(oy * STRIDE - 1) * step + (size_t)(ox * STRIDE - 1) * 3;
    float v[27];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const unsigned long long ad = (unsigned long long)(p + (size_t)r * step);
        const unsigned sh = (unsigned)ad & 3u;
        const gmem_u32* q = (const gmem_u32*)(ad - sh);                      // (explicit global address space: no flat loads)
        stem_unpack<9>(q[0], q[1], q[2], sh, v + r * 9);
    }
    float acc[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) acc[c] = biasf[c];
    // weights in SGPRs, packed FMAs: see stem_fma.h.  One asm block per image row (9 taps) and 16-channel group.
#pragma unroll
    for (int g = 0; g < COUT / 16; ++g) {
        fh_v2f a2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a2[i] = fh_v2f{acc[g * 16 + 2 * i], acc[g * 16 + 2 * i + 1]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float* wrow = wf + (size_t)(r * 9) * COUT + g * 16;
            fh_v2f xp[5];
#pragma unroll
            for (int i = 0; i < 4; ++i) xp[i] = fh_v2f{v[r * 9 + 2 * i], v[r * 9 + 2 * i + 1]};
            xp[4] = fh_v2f{v[r * 9 + 8], 0.f};
#if defined(__HIP_DEVICE_COMPILE__)
            FH_STEM_ROW_FMA(a2, xp, wrow, COUT * 4);
#else
            (void)wrow; (void)xp;
#endif
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) { acc[g * 16 + 2 * i] = a2[i][0]; acc[g * 16 + 2 * i + 1] = a2[i][1]; }
    }
    const size_t o = (((size_t)b * Ho + oy) * Wo + ox) * COUT;
#pragma unroll
    for (int c4 = 0; c4 < COUT / 4; ++c4)
        stem_epilogue(v4f{acc[c4 * 4], acc[c4 * 4 + 1], acc[c4 * 4 + 2], acc[c4 * 4 + 3]}, act, reinterpret_cast<const v4f*>(slope) + c4, out1, out2,
                      o + c4 * 4, reinterpret_cast<const v4f*>(s2) + c4, reinterpret_cast<const v4f*>(t2) + c4);
}

// Frame of the output map around the interior [x0, x0+nx) x [y0, y0+ny): one thread per pixel and 4 channels, literal arithmetic, w27 in the graph's RGB order.
__global__ __launch_bounds__(256) void stem_conv_border_kernel(const StemArgs a, const int Ho, const int Wo, const int x0, const int y0, const int nx,
                                                               const int ny) {
    const int Cout = a.Cout, stride = a.stride, G = Cout >> 2;
    const int top = y0 * Wo, bottom = (Ho - y0 - ny) * Wo, side = Wo - nx;      // pixels above / below the interior rows, and per interior row beside it
    const int per_img = top + bottom + ny * side;
    const long total = (long)a.B * per_img * G;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(t % G);
        const long pi = t / G;
        const int b = (int)(pi / per_img);
        int q = (int)(pi - (long)b * per_img), ox, oy;
        if (q < top) { oy = q / Wo; ox = q - oy * Wo; }
        else if (q < top + bottom) { q -= top; oy = y0 + ny + q / Wo; ox = q % Wo; }
        else { q -= top + bottom; oy = y0 + q / side; const int j = q % side; ox = j < x0 ? j : j + nx; }
        const uint8_t* img = a.src + (size_t)b * a.img_stride;
        v4f acc = *reinterpret_cast<const v4f*>(a.bias + c4 * 4);
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const StemBytes<3> px = stem_byte<3>(img, a.step, oy * stride - 1 + ky, ox * stride - 1 + kx, 0, a.inH, a.inW, a.srcH, a.srcW);
                if (px.at == StemAt::PAD) continue;
                const float x3[3] = {(px.v[2] - 127.5f) / 128.0f, (px.v[1] - 127.5f) / 128.0f, (px.v[0] - 127.5f) / 128.0f};
                for (int ci = 0; ci < 3; ++ci) acc += *reinterpret_cast<const v4f*>(a.w27 + (size_t)((ky * 3 + kx) * 3 + ci) * Cout + c4 * 4) * x3[ci];
            }
        v4f sl = {0.f, 0.f, 0.f, 0.f};
        if (a.slope) sl = *reinterpret_cast<const v4f*>(a.slope + c4 * 4);
        stem_epilogue(acc, a.act, &sl, a.out1, a.out2, (((size_t)b * Ho + oy) * Wo + ox) * Cout + c4 * 4, reinterpret_cast<const v4f*>(a.s2 + c4 * 4),
                      reinterpret_cast<const v4f*>(a.t2 + c4 * 4));
    }
}

template <int STRIDE, int COUT>
static void launch_stem_px(const StemArgs& a, int Ho, int Wo, hipStream_t s) {
    StemRect in = stem_interior(STRIDE, a.srcH, a.srcW, Ho, Wo);
    if (in.empty()) in = StemRect{0, 0, -1, -1};
    const int x0 = in.x0, y0 = in.y0, nx = in.x1 - x0 + 1, ny = in.y1 - y0 + 1;
    const long inner = (long)a.B * ny * nx;
    if (inner >= (1L << 31)) throw std::runtime_error("stem conv: batch too large for the 32-bit pixel index (split the batch)");
    if (inner > 0)
        hipLaunchKernelGGL((stem_conv_px_kernel<STRIDE, COUT>), dim3((unsigned)((inner + 255) / 256)), dim3(256), 0, s, a.src, a.img_stride, a.step, Ho, Wo,
                           x0, y0, nx, ny, a.B, a.wf, a.biasf, a.slope, a.act, a.out1, a.out2, a.s2, a.t2);
    const long frame = ((long)a.B * Ho * Wo - inner) * (COUT / 4);
    if (frame > 0)
        hipLaunchKernelGGL(stem_conv_border_kernel, dim3((unsigned)std::min((frame + 255) / 256, 256L * 16)), dim3(256), 0, s, a, Ho, Wo, x0, y0, nx, ny);
}

// ---- matrix-core form for stems of 48 / 64 output channels (IResNet: 64) -----------------------------------------------------------
// The LDS-tile kernel above is bound by its 27 x Cout scalar-operand FMAs and LDS reads (155 us for 128 faces, 411 MB written: 0.33 of
// HBM).  Same construction as front_kernel's stem (dwpw_mfma.hip): per 16 output pixels one v_mfma_f32_16x16x32_bf16 shape per 16
// output channels — rows = channels (A = weights as three bf16 terms whose sum is the fp32 weight exactly), columns = pixels (B = the 27
// u8 taps of the 3 x 9-byte window, exact in bf16, 127.5 for the conv padding), fp32 accumulate; the result of the MFMA is pixel x 4
// consecutive channels = one 16-byte store.  Persistent workgroups, a tile = 16 x 16 output pixels, its u8 window prefetched one tile
// ahead into registers and parked in LDS, one LDS-only barrier per tile; per-channel vectors (bias, slope, s2, t2) in LDS so that no
// global load sits between the stores.  Border tiles run a second, per-byte pass for the pixels whose window leaves the frame.
// The walk — XCD-contiguous run, division-free advance, LDS-only barrier — is dwpw_tile.h's.
// (Scalar parameters, like stem_conv_px_kernel: only a const __restrict__ pointer that is a kernel ARGUMENT counts as read-only memory
//  for the compiler — through StemArgs the px kernel's per-channel scalar loads became vector loads and this kernel gained a s_waitcnt.)
template <int STRIDE, int CB>
__global__ __launch_bounds__(256, 3) void stem_mfma_kernel(const uint8_t* __restrict__ src, long img_stride, int srcH, int srcW, int step, int inH,
                                                           int inW, int Ho, int Wo, const unsigned* __restrict__ wfrag, const float* __restrict__ biasf,
                                                           const float* __restrict__ slope, int act, float* __restrict__ out1,
                                                           float* __restrict__ out2, const float* __restrict__ s2, const float* __restrict__ t2,
                                                           int tiles_x, int tiles_y, int tiles_total) {
    constexpr int S = STRIDE, T = STEM_TILE, COUT = CB * 16;
    constexpr int ROWS = (T - 1) * S + 3;                                  // staged window rows
    constexpr int PITCH = S == 1 ? 16 : 32;                                // dwords per staged row: ((T-1)*S + 3) * 3 + 3 bytes
    constexpr int SLOTS = (ROWS * PITCH + 255) / 256;
    static_assert(((T - 1) * S + 3) * 3 + 3 <= PITCH * 4, "staged row too narrow");
    __shared__ unsigned stage[2][ROWS * PITCH];
    __shared__ float cst[4][COUT];                                          // bias (folded), slope, s2, t2
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, lp = lane & 15;
    const int row_bytes = srcW * 3;
    if (tid < COUT) {
        cst[0][tid] = biasf[tid];
        cst[1][tid] = slope ? slope[tid] : 0.f;
        cst[2][tid] = out2 ? s2[tid] : 0.f;
        cst[3][tid] = out2 ? t2[tid] : 0.f;
    }
    v4u wq[CB][3];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int q = 0; q < 3; ++q) wq[cb][q] = reinterpret_cast<const v4u*>(wfrag)[(cb * 3 + q) * 64 + lane];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) asm volatile("" ::"v"(wq[cb][0]), "v"(wq[cb][1]), "v"(wq[cb][2]));   // (the compiler's own wait for these loads: here)
#endif
    const StemRect in = stem_interior(S, srcH, srcW, Ho, Wo);           // the FAST pass's pixels

    const XcdRun run = xcd_run(tiles_total);
    const int run1 = run.run1, wgs = run.wgs;
    int t = run.run0 + run.wg;
    TileWalk tw(t, wgs, tiles_x, tiles_y);                                 // the tile being PREFETCHED
    unsigned pf[SLOTS];
    const int pr = tid / PITCH, pd4 = (tid % PITCH) * 4;
    auto prefetch = [&]() __attribute__((always_inline)) {
        const uint8_t* frame = src + (size_t)tw.n * img_stride;
        const int sy0 = tw.tyi * T * S - 1, sx3 = (tw.txi * T * S - 1) * 3;
        const unsigned base_lo = (unsigned)(unsigned long long)frame + (unsigned)(sy0 * step + sx3);
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
            const int r = pr + (256 / PITCH) * k;
            const unsigned shr = (base_lo + (unsigned)(r * step)) & 3u;
            const int rel = sx3 - (int)shr + pd4;
            const bool ok = r < ROWS && (unsigned)(sy0 + r) < (unsigned)srcH && rel >= 0 && rel + 4 <= row_bytes;
            pf[k] = ok ? *(const gmem_u32*)(frame + (unsigned)((sy0 + r) * step + rel)) : 0u;
        }
    };
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    lds_barrier();
    if (t < run1) prefetch();
    int buf = 0;
    for (; t < run1; t += wgs, buf ^= 1) {
        const int cn = tw.n, ty0 = tw.tyi * T, tx0 = tw.txi * T;
        const uint8_t* frame = src + (size_t)cn * img_stride;
        const int sy0 = ty0 * S - 1, sx0 = tx0 * S - 1;
        const unsigned base_lo = (unsigned)(unsigned long long)frame + (unsigned)(sy0 * step + sx0 * 3);
#pragma unroll
        for (int k = 0; k < SLOTS; ++k)
            if (tid + 256 * k < ROWS * PITCH) stage[buf][tid + 256 * k] = pf[k];
        tw.advance();
        if (t + wgs < run1) prefetch();
        lds_barrier();
        const unsigned* st = stage[buf];
        const bool tile_inside = in.has_tile(tx0, ty0, T);
        auto finish = [&](const float (&f)[8], bool store, int oy, int ox) __attribute__((always_inline)) {
            const size_t o = (((size_t)cn * Ho + oy) * Wo + ox) * COUT + 4 * g;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const int c = cb * 16 + 4 * g;
                const v4f a4 = stem_mfma3(f, *reinterpret_cast<const v4f*>(&cst[0][c]), wq[cb][2], wq[cb][1], wq[cb][0]);
                if (store)
                    stem_epilogue(a4, act, reinterpret_cast<const v4f*>(&cst[1][c]), out1, out2, o + cb * 16,
                                  reinterpret_cast<const v4f*>(&cst[2][c]), reinterpret_cast<const v4f*>(&cst[3][c]));
            }
        };
        // FAST pass: wave w takes the tile rows w, w + 4, ...; lane = pixel lp of the row, K block g
#pragma unroll
        for (int i = 0; i < T / 4; ++i) {
            const int py = wid + 4 * i;
            const int oy = ty0 + py, ox = tx0 + lp;
            const bool live = oy < Ho && ox < Wo;
            const bool fast = live && (tile_inside || in.has(ox, oy));
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = 0.f;
            if (fast) {
                const int cb3 = lp * S * 3;                                 // window's first byte relative to the staged row's first byte
                if (g < 3) {
                    const int rr = py * S + g;
                    const unsigned pos = ((base_lo + (unsigned)(rr * step)) & 3u) + (unsigned)cb3;
                    const unsigned* q = st + rr * PITCH + (pos >> 2);
                    stem_unpack<8>(q[0], q[1], q[2], pos & 3u, f);
                } else {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const int rr = py * S + r;
                        const unsigned pos = ((base_lo + (unsigned)(rr * step)) & 3u) + (unsigned)(cb3 + 8);
                        f[r] = (float)((st[rr * PITCH + (pos >> 2)] >> (8u * (pos & 3u))) & 255u);
                    }
                }
            }
            finish(f, fast, oy, ox);
        }
        if (!tile_inside) {
            // BORDER pass: live pixels the FAST pass skipped — per byte (stem_byte), the conv padding as 127.5: it cancels against the folded bias
#pragma unroll 1
            for (int i = 0; i < T / 4; ++i) {
                const int py = wid + 4 * i;
                const int oy = ty0 + py, ox = tx0 + lp;
                const bool live = oy < Ho && ox < Wo;
                const bool slow = live && !in.has(ox, oy);
                const int iy0 = oy * S - 1, ix0 = ox * S - 1;
                float f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = 0.f;
                if (slow) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int r = g < 3 ? g : j, rb = g < 3 ? j : 8;
                        if (g == 3 && j >= 3) continue;
                        const StemBytes<1> px = stem_byte<1>(frame, step, iy0 + r, ix0 + rb / 3, rb % 3, inH, inW, srcH, srcW);
                        f[j] = px.at == StemAt::PAD ? 127.5f : px.v[0];
                    }
                }
                finish(f, slow, oy, ox);
            }
        }
    }
}

template <int STRIDE>
static bool launch_stem_mfma(const StemArgs& a, int Ho, int Wo, hipStream_t s) {
    const int tiles_x = (Wo + STEM_TILE - 1) / STEM_TILE, tiles_y = (Ho + STEM_TILE - 1) / STEM_TILE;
    const int tiles_total = a.B * tiles_x * tiles_y;
    if ((long)a.srcH * a.step >= (1L << 31)) return false;
    const int grid = std::max(8, std::min((tiles_total + 7) / 8 * 8, (a.cus > 0 ? a.cus : conv_num_cus()) * 3) / 8 * 8);
#define FH_STEM_MFMA(CB)                                                                                                              \
    hipLaunchKernelGGL((stem_mfma_kernel<STRIDE, CB>), dim3(grid), dim3(256), 0, s, a.src, a.img_stride, a.srcH, a.srcW, a.step, a.inH, a.inW, Ho, \
                       Wo, a.wfrag, a.biasf, a.slope, a.act, a.out1, a.out2, a.s2, a.t2, tiles_x, tiles_y, tiles_total)
    switch (a.Cout) {
        case 48: FH_STEM_MFMA(3); return true;
        case 64: FH_STEM_MFMA(4); return true;
        default: return false;
    }
#undef FH_STEM_MFMA
}

void launch_stem(const StemArgs& a, hipStream_t s) {
    static const bool mfma_on = !(getenv("FACEHIP_STEM_MFMA") && atoi(getenv("FACEHIP_STEM_MFMA")) == 0);       // A/B switch
    const int Ho = (a.inH + 2 - 3) / a.stride + 1, Wo = (a.inW + 2 - 3) / a.stride + 1;
    if (a.wfrag && a.biasf && mfma_on && a.Cout > 32) {            // (16 / 32 channels: the thread-per-pixel kernel below is at its output-write bound)
        if (a.stride == 1 ? launch_stem_mfma<1>(a, Ho, Wo, s) : launch_stem_mfma<2>(a, Ho, Wo, s)) return;
    }
    if (a.wf && (a.Cout == 16 || a.Cout == 32) && (a.stride == 1 || a.stride == 2)) {
        // (Cout = 64, IResNet's stem: 64 accumulators + 108 scalar loads per thread — measured 545 us against 176 us for the LDS-tile
        //  kernel below at B = 128, whose 4-channels-per-thread layout also writes whole 256-byte pixel rows per wave)
        if (a.stride == 2) a.Cout == 16 ? launch_stem_px<2, 16>(a, Ho, Wo, s) : launch_stem_px<2, 32>(a, Ho, Wo, s);
        else a.Cout == 16 ? launch_stem_px<1, 16>(a, Ho, Wo, s) : launch_stem_px<1, 32>(a, Ho, Wo, s);
        return;
    }
    const int ntiles = a.B * ((Wo + STEM_TILE - 1) / STEM_TILE) * ((Ho + STEM_TILE - 1) / STEM_TILE);
    const int blocks = std::min(ntiles, (a.cus > 0 ? a.cus : 256) * 8);
    if (a.stride == 1) hipLaunchKernelGGL(stem_conv_u8_kernel<1>, dim3(blocks), dim3(256), 0, s, a, Ho, Wo, ntiles);
    else hipLaunchKernelGGL(stem_conv_u8_kernel<2>, dim3(blocks), dim3(256), 0, s, a, Ho, Wo, ntiles);
}

// Folded stem weights wf [27][Cout] (tap-major: (ky*9 + kx*3 + byte) x channel) as the A fragments of v_mfma_f32_16x16x32_bf16: three
// bf16 terms (hi, mid, lo — their sum is the fp32 weight exactly), lane l = channel l & 15, K block l >> 4; K index 8g + j = byte j of
// window row g (g < 3), 24 + r = byte 8 of row r, 27..31 = 0.  One [3][64][4]-dword block per 16 output channels.
void stem_pack_wfrag(const float* wf, int Cout, unsigned* out) {             // Cout % 16 == 0; out: [Cout / 16][3][64][4] dwords
    auto bf = [](float x) {                                                // round to nearest even, as bits
        unsigned u; memcpy(&u, &x, 4);
        u += 0x7fffu + ((u >> 16) & 1u);
        return u >> 16;
    };
    auto fl = [](unsigned b) { unsigned u = b << 16; float x; memcpy(&x, &u, 4); return x; };
    for (int cb = 0; cb < Cout / 16; ++cb)
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int co = cb * 16 + (l & 15), k = 8 * (l >> 4) + j;
                float w = 0.f;
                if (k < 24) w = wf[((k >> 3) * 9 + (k & 7)) * Cout + co];
                else if (k < 27) w = wf[((k - 24) * 9 + 8) * Cout + co];
                const unsigned hi = bf(w); const float r1 = w - fl(hi);
                const unsigned mid = bf(r1); const float r2 = r1 - fl(mid);
                const unsigned t[3] = {hi, mid, bf(r2)};
                for (int q = 0; q < 3; ++q) {
                    unsigned& d = out[((cb * 3 + q) * 64 + l) * 4 + (j >> 1)];
                    d = (j & 1) ? (d | (t[q] << 16)) : t[q];
                }
            }
}

}  // namespace fh
