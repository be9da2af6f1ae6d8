// conv_plan.h — the launch arithmetic of the direct convolutions (conv_mfma.hip), the ONE place it lives.  Plain integers in, plain
// integers out, no HIP: launch_conv copies the answers into ConvArgs and launches, api.cpp exposes them (fh_debug_conv_plan) and
// tests/test_conv_plan_cpu.py holds them to the properties the kernels rely on, without a GPU.
#pragma once
#include <cstddef>
#include <cstdlib>

#if defined(__HIPCC__)
#define FH_CONV_HD __host__ __device__
#else
#define FH_CONV_HD
#endif

namespace fh {

// stream-K workspace: accumulator slabs followed by one counter word per remainder tile
constexpr size_t SK_SLAB_FLOATS = (size_t)2 * 1280 * 128 * 128;
constexpr size_t SK_COUNTERS = 4096;

// The tuning / A-B switches of this file's launchers, read from the environment once.
struct ConvKnobs {
    int sk_b_ratio = 4;      // FACEHIP_SK_B_RATIO: fix-up form only when a tile is cut into >= ratio/2 pieces
    int sk_min_owner = 12;   // FACEHIP_SK_MIN_OWNER: chunks of its own an owner needs next to its ~8 us hand-off (fence, poll, slab reads)
    int sk_margin2 = 3;      // FACEHIP_SK_MARGIN: the helpers' head start over the owners, in half chunks
    int tall_tail_q = 3;     // FACEHIP_TALL_TAIL_Q: segment length of the few tiles conv_tall_kernel leaves over
    int conv_pw = 1;         // FACEHIP_CONV_PW / FACEHIP_CONV_TALL: 0 = conv_igemm_kernel everywhere (A / B timing)
    int conv_tall = 1;
    int ep_direct = 0;       // FACEHIP_EP_DIRECT: see ConvArgs::ep_direct
    int conv_x3 = 1;         // FACEHIP_CONV_X3: 0 = the folded-shortcut layers stay on the f32 MFMA even where the handle's x3 switch is on,
                             // 2 = x3 wherever the layer has the form, whatever conv_x3_pays would say (A / B timing)
    int pw_x3 = 1;           // FACEHIP_PW_X3: the same three values for the 1x1 stride-1 layers (conv_pw_x3_pays)
    int pw_x3_bn = 0;        // FACEHIP_PW_X3_BN: 64 = 64-wide x3 tiles where the rule would take 32-wide ones (A / B timing)
    int wino2_x3 = 1;        // FACEHIP_WINO2_X3: the same three values for the fused F(2x2) Winograd layers (wino2_x3_pays)
};
inline const ConvKnobs& conv_knobs() {
    static const ConvKnobs k = [] {
        ConvKnobs v;
        auto env = [](const char* name, int& x) { if (const char* e = getenv(name)) x = atoi(e); };
        env("FACEHIP_SK_B_RATIO", v.sk_b_ratio); env("FACEHIP_SK_MIN_OWNER", v.sk_min_owner); env("FACEHIP_SK_MARGIN", v.sk_margin2);
        env("FACEHIP_TALL_TAIL_Q", v.tall_tail_q); env("FACEHIP_CONV_PW", v.conv_pw); env("FACEHIP_CONV_TALL", v.conv_tall);
        env("FACEHIP_EP_DIRECT", v.ep_direct); env("FACEHIP_CONV_X3", v.conv_x3); env("FACEHIP_PW_X3", v.pw_x3); env("FACEHIP_PW_X3_BN", v.pw_x3_bn);
        env("FACEHIP_WINO2_X3", v.wino2_x3);
        return v;
    }();
    return k;
}

// What the predicates below need of a ConvArgs.
struct ConvGeom {
    long M;                  // B * Ho * Wo
    int H, W, Cin, Ho, Wo, Cout, ks, stride, pad, Kpad, n_outs;
    bool grouped, sc, up2x, no_pw;
};

// Tile config of conv_igemm_kernel: 0 = 128x128, 1 = 256x64, 2 = 128x32, 3 = 64x64.
inline int conv_pick_cfg(long M, int Cout) {
    // padded-column waste per candidate tile width; prefer the wider tile when it costs <= 10 % more
    auto cols = [&](int bn) { return (Cout + bn - 1) / bn * bn; };
    int bn = 32;
    if (cols(64) * 10 <= cols(32) * 11) bn = 64;
    if (cols(128) * 10 <= cols(bn) * 11) bn = 128;
    if (bn == 128) return 0;
    if (bn == 64) return (M / 256) * (cols(64) / 64) >= 1024 ? 1 : 3;
    return 2;
}

// The three-piece bf16 K loop of conv_igemm_kernel ("x3", gemm_tile.h) exists for 128 x BN tiles of four 32-row waves, BN = 128 where
// Cout % 128 == 0 and 64 where Cout % 64 == 0; 0 = the layer has no such form (it also needs Cin % 32 == 0 and no groups: the caller's part).
inline int conv_x3_bn(int Cout) { return Cout <= 0 ? 0 : Cout % 128 == 0 ? 128 : Cout % 64 == 0 ? 64 : 0; }
// Does the x3 K loop pay for a launch of `tiles` 128 x conv_x3_bn(Cout) tiles of depth Kpad on `cus` CUs?  Measured on IResNet-50's four
// folded-shortcut layers (Kpad 640 / 1216 / 2432 / 4864) at B = 8, 32, 64, 128, 256, f32 against x3 in one session (profiles/conv_x3.md):
// every layer gains at every batch, 0.61-0.69 of the f32 time from B = 64 up and still 0.68-0.95 at B = 8, where the smallest launch is
// 16 tiles on 256 CUs cut by stream-K.  So the form is on from there up — one tile per 16 CUs, 20 chunks — and what lies below, which
// nothing measured, stays on the f32 kernel.  Monotone in `tiles` and in Kpad.
inline bool conv_x3_pays(long tiles, int Kpad, int Cout, int cus, const ConvKnobs& k) {
    if (!k.conv_x3 || !conv_x3_bn(Cout) || Kpad % 32 || cus <= 0) return false;
    if (k.conv_x3 == 2) return true;
    return tiles * 16 >= (long)cus && Kpad >= 640;
}

// One tile's time on one CU's matrix cores (~110 TFLOP/s over 256 CUs).  A matrix-core-bound launch takes as long as its busiest CU
// has tiles (measured on the Winograd GEMMs), not whole chip-wide rounds: both rules below weigh that against a launch.
inline double conv_tile_us(long tile_floats, int Kpad) { return 2.0 * tile_floats * (double)Kpad / 0.43e6; }

// conv_pw_kernel (1x1 stride-1 as the plain GEMM): the tile width it runs the layer with (96 / 64 / 32), or 0 = not eligible.
// Whole 128-row tiles, float4 rows on both sides, no merged outputs, and at least one tile per CU: with fewer the generic kernel cuts K
// over the chip.
inline int conv_pw_bn(const ConvGeom& g, int cus, const ConvKnobs& k) {
    if (!k.conv_pw || g.no_pw || g.ks != 1 || g.stride != 1 || g.pad != 0 || g.grouped || g.sc || g.n_outs > 0 || (g.Cin & 3) || (g.Cout & 3) ||
        (g.M & 127) || g.H != g.Ho || g.W != g.Wo || g.Kpad % 32 || g.Kpad < g.Cin)
        return 0;
    auto cols = [&](int bn) { return (g.Cout + bn - 1) / bn * bn; };
    // widest tile whose padded columns cost <= 7 %; the 32-wide one otherwise (the generic kernel pads the same way)
    int bn = 32;
    if (cols(64) * 100 <= g.Cout * 107) bn = 64;
    if (cols(96) * 100 <= g.Cout * 107 && cols(96) <= cols(64)) bn = 96;
    return (g.M / 128) * (cols(bn) / bn) < (long)cus ? 0 : bn;
}

// conv_pw_x3_kernel (the same GEMM on three bf16 pieces): the tile width it runs the layer with, or 0 = no such form — never a form where
// conv_pw_bn has none.  96 where the f32 kernel takes 96 (N = 288: three exact tiles; the padded columns then never exceed the weight
// image's conv_wt_rows), 64 where 64-wide tiles pad <= 7 %, else the narrow width: 32 (N = 152: 160 columns) unless FACEHIP_PW_X3_BN = 64
// asks for 64 (192 columns, two accumulator blocks per pixel split) for A / B timing.  At least one tile per CU, as conv_pw_bn.
inline int conv_pw_x3_bn(const ConvGeom& g, int cus, const ConvKnobs& k) {
    if (!conv_pw_bn(g, cus, k)) return 0;
    auto cols = [&](int bn) { return (g.Cout + bn - 1) / bn * bn; };
    int bn = k.pw_x3_bn == 64 ? 64 : 32;
    if (cols(64) * 100 <= g.Cout * 107) bn = 64;
    if (cols(96) * 100 <= g.Cout * 107 && cols(96) <= cols(64)) bn = 96;
    return (g.M / 128) * (cols(bn) / bn) < (long)cus ? 0 : bn;
}
// Does the x3 form pay for a launch of `tiles` 128 x conv_pw_x3_bn tiles of depth Kpad on `cus` CUs?  FACEHIP_PW_X3: 0 = never (the 1x1s
// stay on conv_pw_kernel with the handle's switch on), 2 = wherever the form exists (A / B timing), 1 = the measured rule below.
// Measured on SCRFD det_500m's thirteen conv_pw launches at B = 64, 128, 256, f32 against x3 in three alternating runs on 256 CUs
// (profiles/pw_x3.md; us at B = 128, min-max): 20x20x288 -> 288 84-89 -> 55-64, 20x20x152 -> 288 56-59 -> 41-43, 40x40x152 -> 152 112-114 ->
// 90-93, 40x40x72 -> 152 92.1-92.5 -> 86.8-87.4 (three chunks: the smallest gain of a deep class, 6 %, still ten times the f32 side's
// spread), 80x80x72 -> 16 79-80 -> 74, 40x40x152 -> 16 36.6-36.9 -> 35.7-36.2, 20x20x64 -> 64 15.4-15.6 -> 14.0-14.1; the same classes
// gain at B = 64 and 256.  Two classes do not: one chunk (20x20x16 -> 64: 14.6-14.8 against 14.6-14.7) — so Kpad >= 64 — and a 16-channel
// lateral with under two tiles per CU (20x20x288 -> 16, 400 half-empty 32-wide tiles at B = 128: 16.8 -> 17.3-17.7; at B = 256, 800 tiles,
// 28.0-29.0 -> 26.7-27.0) — so Cout < 32 asks for two tiles per CU.  Monotone in `tiles` and in Kpad.
constexpr int PW_X3_MIN_KPAD = 64;
inline bool conv_pw_x3_pays(long tiles, int Kpad, int Cout, int cus, const ConvKnobs& k) {
    if (!k.pw_x3 || Cout <= 0 || (Cout & 3) || Kpad <= 0 || Kpad % 32 || cus <= 0) return false;
    if (k.pw_x3 == 2) return true;
    return tiles >= (long)cus * (Cout < 32 ? 2 : 1) && Kpad >= PW_X3_MIN_KPAD;
}

// wino2_x3_kernel (conv_wino2.hip: the fused F(2x2) Winograd layer on three bf16 pieces): does it pay for a launch of `workgroups`
// (tile groups x 64-channel column tiles) on `cus` CUs?  FACEHIP_WINO2_X3: 0 = never, 2 = wherever the form exists (A / B timing),
// 1 = the measured rule.  Measured on 56x56x64 -> 64 / 128, 112x112x64 -> 64 and 80x80x64 -> 64 at B = 8, 64, 128, 256, f32 against x3 in
// three alternating runs on 256 CUs (profiles/wino2_x3.md): every launch gains, 0.75-0.89 of the f32 time, the smallest one too (B = 8 on
// 56 x 56: 392 workgroups, 29.6 -> 24.7 us).  So the form is on from there up — three workgroups per two CUs — and what lies below, which
// nothing measured, stays on the f32 kernel.  Monotone in `workgroups`.  Whether the layer runs on the fused form at all is decided before
// this, by wino2_blocks (engine.cpp).
inline bool wino2_x3_pays(long workgroups, int cus, const ConvKnobs& k) {
    if (!k.wino2_x3 || workgroups <= 0 || cus <= 0) return false;
    if (k.wino2_x3 == 2) return true;
    return workgroups * 2 >= (long)cus * 3;
}

// conv_tall_kernel's take-over of a 3x3 stride-1 pad-1 layer with Cin % 32 == 0 on a map up to 112 wide, for the 256x64 and 128x32
// tiles (rp = Tile::RP): it takes the whole ROUNDS of the T tiles (whole tile rows) and leaves the rest to conv_igemm_kernel with
// tile0 = tiles.  When that rest is at most one more tile per CU and a tile is short (< ~30 us), running it here too costs less than
// the second launch + fix-up of the split (SCRFD's 80x80 head convolution: 6 400 tiles = 25 per CU exactly: 329 + 38 us -> 343 us);
// IResNet's 256x64 tiles (44 us each) keep the split.  tiles = 0: not taken (not eligible, under one round, or the image exceeds LDS).
struct ConvTallPlan { int tiles, rows_a; size_t lds; };
inline ConvTallPlan conv_tall_plan(const ConvGeom& g, int BM, int BN, int rp, int T, int tiles_n, int cus, const ConvKnobs& k) {
    const int occ = BM == 256 ? 2 : 3;                                  // resident workgroups per CU of the tall form (LDS)
    const int St = cus * occ;
    ConvTallPlan t{0, 0, 0};
    if (!k.conv_tall || g.grouped || g.sc || g.ks != 3 || g.stride != 1 || g.pad != 1 || (g.Cin & 31) || g.H != g.Ho || g.W != g.Wo || g.W > 112 ||
        !(BN == 32 ? g.n_outs > 0 || (g.Cout & 3) == 0 : g.n_outs == 0 && (g.Cout & 3) == 0) || g.up2x || T < St)
        return t;
    t.rows_a = (BM + 2 * g.W + 2 + rp - 1) / rp * rp;
    t.lds = ((size_t)t.rows_a * 8 + 2 * BN * 8) * 16;
    t.tiles = (T / St) * St;
    t.tiles -= t.tiles % tiles_n;
    if (t.tiles > 0 && T - t.tiles <= cus && conv_tile_us((long)BM * BN, g.Kpad) < 30.0) t.tiles = T;
    if (t.lds > (size_t)(160 / occ) * 1024) t.tiles = 0;
    return t;
}

// Slabs a remainder tile r is cut into when every tile has Kh chunks for the helpers and a helper's run is q chunks: the runs that
// overlap [r Kh, (r + 1) Kh).  The owner / conv_fixup_kernel sum exactly this many; the plan sizes a tile's slab slots (maxp) for it.
FH_CONV_HD inline int conv_sk_nparts(int r, int Kh, int q) { return ((r + 1) * Kh - 1) / q - (r * Kh) / q + 1; }

// Stream-K remainder of T tiles on S resident workgroup slots (`chunks` 32-deep K chunks per tile of tile_floats accumulators; tile0 > 0:
// the tiles before it ran in conv_tall_kernel; slabs_ok: a workspace exists and stream-K is allowed).  The first `full` tiles run
// whole; the `rem` behind them are cut into `units` chunks dealt q at a time to `helpers` workgroups, either
//   owners > 0:  each remainder tile has an owner that computes its first owner_chunks chunks and adds the helpers' <= maxp - 1 slabs, or
//   fixup:       every segment goes to a slab and conv_fixup_kernel sums them in a second launch (owner_chunks = 0),
// or nothing is cut (helpers = 0, full = T).  maxp = slab slots per remainder tile.
struct ConvSkPlan { int full, rem, helpers, owners, fixup, units, q, owner_chunks, maxp; };
inline ConvSkPlan conv_streamk_plan(int T, int S, int chunks, long tile_floats, int cus, int Kpad, int tile0, bool slabs_ok, const ConvKnobs& k) {
    ConvSkPlan pl{(T / S) * S, 0, 0, 0, 0, 0, 1, 0, 1};
    const int R = T - pl.full;
    // (leaving R remainder tiles whole costs (ceil(R / CUs) - R / CUs) tile times of imbalance; cutting them over the chip costs a fix-up
    //  launch (10-17 us).  Short tiles — SCRFD's 20x20 head convolutions, 11 us — stay whole: 31 + 17 us -> 25 us; IResNet's 44 us
    //  tiles keep the split.)
    const bool cheap_whole = ((R + cus - 1) / cus - (double)R / cus) * conv_tile_us(tile_floats, Kpad) < 10.0;
    if (R > 0 && R * 10 <= S * 9 && slabs_ok && !cheap_whole) {          // worth it only if the last round is <= 90 % full
        // (1) owners + helpers inside the launch
        const int H = S - R;
        const int q_o = (int)(((long)R * chunks + (long)H * k.sk_margin2 / 2 + S - 1) / S);
        const int Kh = chunks - q_o;
        if (Kh >= 1 && q_o >= k.sk_min_owner && R <= (int)SK_COUNTERS) {
            const long U = (long)R * Kh;
            const int q_h = (int)((U + H - 1) / H);
            const int maxp = (Kh + q_h - 1) / q_h + 1;
            if (maxp <= 3 && (size_t)R * maxp * tile_floats <= SK_SLAB_FLOATS) {
                pl.units = (int)U; pl.q = q_h; pl.owner_chunks = q_o; pl.maxp = maxp;
                pl.helpers = (int)((U + q_h - 1) / q_h); pl.owners = R;
            }
        }
        // (2) otherwise: every segment to a slab, reduced by the fix-up kernel
        if (!pl.owners) {
            const long U = (long)R * chunks;
            int q = (int)((U + S - 1) / S);
            // do not cut segments shorter than 8 chunks — 24 for very deep K (the 25 088-deep FC: 61 slabs per tile made the fix-up kernel,
            // 16 workgroups summing them one after the other, take 35 of the layer's 80 us; 21 slabs: 48 + 20 us)
            // (the tail of a convolution whose whole rounds ran in conv_tall_kernel is a few tiles on an otherwise empty chip: cut them finer)
            const int min_q = tile0 > 0 ? (chunks < k.tall_tail_q ? chunks : k.tall_tail_q) : chunks < 8 ? chunks : chunks >= 256 ? 24 : 8;
            if (q < min_q) q = min_q;
            const int maxp = (chunks + q - 1) / q + 1;
            if (q * k.sk_b_ratio <= chunks * 2 && q < chunks && (size_t)R * maxp * tile_floats <= SK_SLAB_FLOATS) {
                pl.units = (int)U; pl.q = q; pl.maxp = maxp;
                pl.helpers = (int)((U + q - 1) / q); pl.fixup = 1;
            }
        }
    }
    if (pl.helpers) pl.rem = R; else pl.full = T;
    return pl;
}

}  // namespace fh
