// kernels.h — host-side launch interface of the gfx950 kernels (device pointers only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include <vector>

#include "conv_plan.h"

namespace fh {

void hip_check(hipError_t e, const char* what);
#define FH_HIP(x) ::fh::hip_check((x), #x)

// Orders one wave's own LDS stores before its own later LDS loads of bytes OTHER lanes stored (the per-wave turn-around scratch of the
// whole-line epilogues) and those loads before the next round's stores.  LDS operations of one wave execute in issue order, so no
// instruction is needed; this only keeps the COMPILER from moving an access across one it cannot prove disjoint (wavefront-scope fence +
// wave barrier: no code is emitted).
#if defined(__HIPCC__)
__device__ __forceinline__ void wave_lds_order() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#endif
}
#endif

// Optional per-launch HIP-event timing of the network kernels (bench.py's roofline leg).
// Tags: 0..3 = conv_igemm tile configs, 4 = depthwise conv, 5 = other graph ops, 6 = conv stream-K fix-up.
struct KernelTimer {
    static constexpr int kTags = 13;     // 0-3 conv tile configs, 4 dw / dwpw, 5 other, 6 fix-up, 7 Winograd GEMM, 8 Winograd transforms, 9 halo conv, 10 conv_tall_kernel, 11 conv_pw_kernel, 12 wino2_kernel
    bool enabled = false;
    void begin(hipStream_t s);
    void end(hipStream_t s, int tag, double flops, double bytes);
    // synchronises, aggregates elapsed ms / flops / bytes / launches per tag, then resets
    void collect(double* ms, double* flops, double* bytes, long long* launches);
    // un-aggregated variant (tuning): one entry per recorded launch, in launch order
    int collect_ops(double* ms, double* flops, int* tag, int cap);
    static KernelTimer& get();

  private:
    struct Rec { hipEvent_t a, b; int tag; double flops, bytes; };
    std::vector<Rec> recs_;
    std::vector<hipEvent_t> pool_;
    hipEvent_t cur_ = nullptr;
    hipEvent_t take();
};


// --------------------------------------------------------------------------------------------
// Dense convolution / FC as implicit GEMM on v_mfma_f32_32x32x2_f32 (conv_mfma.hip)
//   M = B*Ho*Wo output pixels, N = Cout, K = ks*ks*Cin (k = tap*Cin + ci), all fp32, NHWC.
// --------------------------------------------------------------------------------------------
struct ConvArgs {
    const float* in;        // [B,H,W,Cin]
    const float* wt;        // packed [CoutPad][Kpad], rows >= Cout and cols >= Ktot are zero
    const float* bias;      // [Cout] — or, with bias_cls != 0, [9][Cout]: one vector per border class of the output pixel
                            // (3 * (oy == 0 ? 0 : oy == Ho-1 ? 2 : 1) + same for ox): a pre-conv BatchNorm folded into this 3x3 pad-1 conv
    const float* slope;     // [Cout] (PReLU) or null
    const float* res;       // residual [B,Ho,Wo,Cout] (SAME) / [B,Ho/2,Wo/2,Cout] (UP2X) or null
    float* out1;            // [B,Ho,Wo,Cout] or null
    float* out2;            // second output  out*s2 + t2, or null
    const float* s2;
    const float* t2;
    float* slabs;           // stream-K accumulator slabs (conv_slab_floats() floats) or null = plain tiles only
    const float* zeros;     // >= 16 zero bytes (filled in by launch_conv)
    int B, H, W, Cin, Ho, Wo, Cout;
    int ks, stride, pad;
    int Kpad;               // multiple of 32
    int bias_cls;           // see bias
    // folded shortcut (sc_in != null; needs ks == 3, Cin % 32 == 0, sc_C % 32 == 0): a 1x1 stride-sc_stride convolution of sc_in
    // [B,sc_H,sc_W,sc_C] on the same output grid runs as a tenth tap of the K loop — wt holds its sc_C columns after the 9*Cin
    // own ones (Kpad = 9*Cin + sc_C), bias the sum of both biases
    const float* sc_in;
    int sc_H, sc_W, sc_C, sc_stride;
    int act;                // fh::Act
    int res_mode;           // fh::ResMode
    const float* dw_w;      // fused depthwise 3x3 front end (launch_dwpw): weights [9][Cin], bias [Cin], activation
    const float* dw_b;
    int dw_act;
    int dw_stride;          // 1 | 2
    // fused u8 stem in FRONT of the depthwise part (launch_dwpw with u8_src != null): `in` is not read — the workgroup computes the
    // stem convolution (3x3, 3 -> 16 channels, stride u8_stride, preprocess folded into stem_wf / stem_bf as StemArgs::wf / biasf)
    // for its halo pixels straight from the BGR u8 frames.  H x W = the stem's output grid = the depthwise input.
    const uint8_t* u8_src;
    long u8_img_stride;
    int u8_step, u8_srcH, u8_srcW, u8_inH, u8_inW, u8_stride, stem_act;
    const float* stem_wf;
    const float* stem_bf;
    const unsigned* stem_wfrag;   // launch_dwpw's fused stem: stem_wf as bf16 MFMA fragments (stem_pack_wfrag)
    int no_prio;            // 1: the persistent depthwise kernels do not rotate their wave priority (dwpw_tile.h rotate_wave_priority: A / B switch)
    int no_pw;              // 1: keep conv_igemm_kernel even where conv_pw_kernel (the lean 1x1 form) would take the layer (forced-cfg runs)
    int n_outs;             // > 0: merged sibling convs — channels [oc0[g], oc0[g+1]) go to outs[g] with act oact[g]
    float* outs[3];
    int oc0[4];
    int oact[3];
    int sk_enable;          // allow the stream-K remainder wave
    int cus;                // CUs this launch can occupy (0 = the whole device); sizes the stream-K remainder round
    // grouped GEMM (Winograd: 36 independent [rows x K] x [K x N] products stacked along M in one launch): rows
    // [g*wt_group_rows, (g+1)*wt_group_rows) use the weight matrix wt + g*wt_gs (floats).  wt_group_rows = 0: off;
    // otherwise a multiple of the tile height (128 covers every configuration but the 256-row one).
    int wt_group_rows;
    long wt_gs;
    double t_flops, t_bytes; // algorithmic work of this launch (only used by the optional KernelTimer)
    // filled in by launch_conv: #plain tiles, K-chunk units dealt to helpers, units per helper, #helpers, #remainder
    // tiles, chunks each owner computes itself (0 = no owners: fix-up kernel), slab slots per remainder tile
    int sk_full, sk_units, sk_q, sk_helpers, sk_rem, sk_owner_chunks, sk_maxp;
    // stream-K watchdog (filled in by launch_conv): host-visible error record, the owners' wait bound in 2^16 ticks of the 100 MHz
    // wall clock, and the test hook that makes helpers "lose" their publication
    unsigned* sk_err;
    int ep_direct;                  // tuning hook (FACEHIP_EP_DIRECT): 1 = epilogue stores straight from the accumulator registers, 3 = whole-line form for every Cout % 4 == 0
    unsigned sk_timeout;
    int sk_test_drop;
    int tile0;              // filled in by launch_conv: first tile conv_igemm_kernel computes (the tiles before it ran in conv_tall_kernel)
};

// cfg: 0 = 128x128 tile, 1 = 256x64, 2 = 128x32, 3 = 64x64 (256 threads each); -1 = choose (conv_pick_cfg).  Which kernels a layer
// gets and how its remainder tiles are cut is host arithmetic in conv_plan.h; the kernels' shared device pieces are in conv_tile.h.
void launch_conv(const ConvArgs& a, int cfg, hipStream_t s);
// The same layer on conv_igemm_kernel's three-piece bf16 K loop ("x3", gemm_tile.h: fp32 products from six bf16 MFMAs; 128 x 128 or 128 x 64
// tiles): a.wt = launch_pack_x3(weights [conv_wt_rows(Cout)][Kpad], ..., freqs = 1).  conv_x3_ok: the layer has the form (Cin % 32 == 0,
// Cout % 64 == 0; ungrouped, Kpad = ks*ks*Cin + sc_C: checked by the launcher).  tag: the timer tag to book the launch under.  Whether the
// form pays for a launch is conv_x3_pays (conv_plan.h).
void launch_conv_x3(const ConvArgs& a, int tag, hipStream_t s);
bool conv_x3_ok(int Cin, int Cout);
// A 1x1 stride-1 layer on conv_pw_x3_kernel (conv_pw_kernel's GEMM with the x3 K loop): wt3 = launch_pack_x3(a.wt = the f32 image
// [conv_wt_rows(Cout)][Kpad], ..., freqs = 1).  false = not launched: the layer has no such form at this batch (conv_pw_x3_bn, conv_plan.h)
// or — unless force — the form does not pay for the launch (conv_pw_x3_pays); the caller then runs launch_conv.  Booked under tag 11.
bool launch_conv_pw_x3(ConvArgs a, const float* wt3, bool force, hipStream_t s);
void conv_workspace_init(float* ws);          // zero the counter words of a freshly allocated stream-K workspace
void conv_workspace_reset_async(float* ws, hipStream_t s);   // the same, stream-ordered (after a reported hand-off time-out)
// Stream-K watchdog.  An owner workgroup whose helpers never arrive gives up after a bounded wait and reports through a host-mapped
// record of the launching Net's own; conv_take_error(msg, rec) — called with the records of the handles an API call works on — returns
// true once for that handle (with a message starting "HIP error") and bumps conv_error_generation(), after which
// every Net re-zeroes its hand-off counters before its next run.  conv_debug_streamk(drop, ms): test hook — helpers skip their
// publication / the owners' wait bound in milliseconds (0 = the 2 s default).
unsigned* conv_error_words();                 // the process-wide record (launches whose ConvArgs::sk_err is null: the single-kernel test entry points)
unsigned* conv_error_record_new();            // a record of a Net's own (host-mapped, 64 B); ConvArgs::sk_err of its launches
void conv_error_record_release(unsigned* r);
bool conv_take_error(std::string& msg, unsigned* rec);   // consumes THIS record's report, if any
bool conv_error_pending(const unsigned* rec); // a reported time-out has not been consumed yet
unsigned conv_error_generation();
void conv_debug_streamk(int drop_publish, int timeout_ms);
unsigned conv_debug_generation();             // bumped by conv_debug_streamk (its settings are kernel arguments: captured graphs hold them)
// Fused Winograd F(2x2, 3x3) for 3x3 stride-1 pad-1 convolutions with Cin = 64 and Cout % 64 == 0 (or <= 32 with merged outputs) (conv_wino2.hip): a.wt = the
// wino2_pack_weights image of the filter [Cout][9][Cin]; epilogue fields (bias / bias_cls, act, slope, res, out1, out2) as for launch_conv
size_t wino2_weight_floats(int Cin, int Cout);
void wino2_pack_weights(const float* w_ohwi, int Cout, int Cin, float* dst);
bool wino2_ok(const ConvArgs& a);
void launch_wino2(const ConvArgs& a, hipStream_t s);
long wino2_blocks(const ConvArgs& a);          // workgroups the launch would have
// ... and its three-piece bf16 form (wino2_x3_kernel: fp32 products on six bf16 MFMAs), plain layers with Cout % 64 == 0 only: a.wt =
// the wino2_pack_weights_x3 image (wino2_x3_weight_floats floats, built on the host).  Whether a
// launch of `workgroups` gains from it is wino2_x3_pays' question (conv_plan.h).  Booked under tag 12 like the f32 form.
bool wino2_x3_shape_ok(int Cin, int Cout);
size_t wino2_x3_weight_floats(int Cin, int Cout);
void wino2_pack_weights_x3(const float* w_ohwi, int Cout, int Cin, unsigned short* dst);
bool wino2_x3_ok(const ConvArgs& a);
long wino2_x3_workgroups(const ConvArgs& a);
void launch_wino2_x3(const ConvArgs& a, hipStream_t s);
double wino2_debug_clock_mhz();              // diagnostic builds (scripts/wino2_prof.sh): median in-kernel shader clock of the last launch
const float* conv_zero_line();                // 8 KiB of device zeros (target of padded / dead loads)
int conv_num_cus();                           // compute units of the current device
// dense 3x3 stride-1 convolutions with 16 input channels and <= 64 output channels on an 8x16 spatial tile with an LDS halo
// (conv_halo.hip); wfrag = conv_halo_pack_weights' image of the filter
bool conv_halo_ok(const ConvArgs& a);
size_t conv_halo_wfrag_floats(int Cin, int Cout);
void conv_halo_pack_weights(const float* w_ohwi, int Cout, int Cin, float* dst);
void launch_conv_halo(const ConvArgs& a, const float* wfrag, hipStream_t s);
// depthwise 3x3 stride 1 (+bias +act) fused with the 1x1 conv that consumes it (dwpw_mfma.hip)
bool front_fused_ok(int Cin, int Cout, int dw_stride);   // the opening block (u8 stem + depthwise + pointwise) has a one-kernel form
void launch_dwpw(const ConvArgs& a, hipStream_t s);
// Winograd F(4x4,3x3) form of a 3x3 stride-1 pad-1 convolution (winograd.hip): a = the convolution's arguments,
// wt36 = U[36][conv_wt_rows(Cout)][Cin], V / M = workspaces of 36 * tiles * max(Cin, Cout) floats each
// in_scale / in_shift (optional): per-input-channel affine applied to in-image pixels by the input transform
// prec: 0 = native f32; 1 = the split-bf16 operand format below (wt36 already packed; the input transform packs V); 2 = the three-piece
// bf16 GEMM (wt36 = the launch_pack_x3 image; V stays fp32)
void launch_conv_winograd(const ConvArgs& a, const float* wt36, float* V, float* M, int cfg, const float* in_scale, const float* in_shift,
                          hipStream_t s, int prec = 0);
// the three stages separately, and stage 3 of one convolution fused with stage 1 of the next (same map, C = Cout = next Cin)
// pack / bf16x2 / pack_next: the opt-in split-bf16 operand format (V and U as (hi, mid) bf16 pairs in 32-bit words, see winograd.hip)
struct WinoPlanes;
void launch_wino_input(const ConvArgs& a, float* V, const float* in_scale, const float* in_shift, bool pack, hipStream_t s);
void launch_wino_gemm(const ConvArgs& a, const float* wt36, const float* V, float* M, int cfg, int prec, hipStream_t s,
                      const WinoPlanes* mix = nullptr);   // mix: V / M in the mixed-tiling layout (lean kernel only); prec as above
bool wino_gemm_ok_bf16x2(int Cin, int Cout);              // ... which also says whether the layer has the three-piece (x3) form
// Three-piece bf16 GEMM ("x3", gemm_tile.h): fp32 U [36][rows][K] -> its x3 image of 36 * wino_x3_floats(rows, K) floats; whether a handle's
// fp32 path uses it by default (FACEHIP_WINO_X3, read once); whether it pays for a launch of row_tiles 128-row tiles
// (freqs: matrices in `in`; 1 = one [rows][K] weight matrix of a direct convolution, launch_conv_x3)
void launch_pack_x3(const float* in, float* out, int rows, int K, hipStream_t s, int freqs = 36);
inline size_t wino_x3_floats(int rows, int K) { return (size_t)rows * K * 3 / 2; }
bool wino_x3_default();
bool wino_x3_pays(long row_tiles, int Cin, int Cout);
void launch_wino_output(const ConvArgs& a, const float* M, hipStream_t s);
bool wino_can_fuse(int H, int W, int C, bool touches_memory);
void launch_wino_fused(const ConvArgs& a, const float* M, float* Vnext, int feed_aff, bool pack_next, hipStream_t s);
void launch_pack_bf16x2(const float* in, float* out, long n, hipStream_t s);      // fp32 -> split-bf16 words, n % 4 == 0
// Mixed F(4x4) / F(2x2) tiling (round 3) for maps whose side is 4 k + 2 or 4 k + 1 (IResNet's 14x14): the last tile row / column is an
// F(2x2, 3x3) tile instead of an F(4x4) tile hanging over the border — 484 instead of 576 GEMM rows per 14x14 image.  Tiles fall into
// four classes (rows F4 | F2) x (columns F4 | F2) with 36 / 24 / 24 / 16 frequency planes; the F(2) interpolation points {0, +-1, inf}
// are a subset of F(4)'s, so the planes multiply the SAME 36 weight matrices (plane (i, j) of an F(2) direction uses frequency
// {0, 1, 2, 5}[i] with the row scales {4, -3, -3, 1} folded into the input transform).
struct WinoPlanes {
    int e[4];                // first 128-row GEMM tile of class c (classes stored one after the other, plane-major inside a class)
    int t[4];                // 128-row GEMM tiles per plane
    int nfc[4];              // frequencies along a patch row: 6 (F4 columns) or 4 (F2 columns)
    int f2[4];               // bit 0: columns are F(2), bit 1: rows are F(2)
    int n[4];                // tiles per image
    int rows[4];             // rows per plane (B * n rounded up to 128)
    int base[4];             // first row of the class's first plane
    int total_tiles;         // 128-row GEMM tiles over all planes
    int planes;              // 36 + 24 + 24 + 16 (classes with n = 0 contribute none)
};
// layout of the mixed tiling for B images of H x W; false: this map / batch keeps the uniform tiling
bool wino_mix_layout(int B, int H, int W, int Cin, int Cout, WinoPlanes* out);
// one kernel for the three transform roles of a mixed-tiling convolution `a` (whole images x 64 channels per workgroup):
//   M != null: Y = A^T M A of convolution `a` (+bias, activation, residual; out1 / out2 written when non-null), else the image comes from
//              a.in (per-channel affine in_scale / in_shift on in-image pixels when non-null);
//   Vnext != null: V = B^T d B for the next convolution (= `a` itself when M is null) from that image (feed_aff: through a.s2 / a.t2).
void launch_wino_mix(const ConvArgs& a, const WinoPlanes& pl, const float* M, float* Vnext, int feed_aff, const float* in_scale,
                     const float* in_shift, bool pack_next, hipStream_t s);
void wino_filter_transform(const double g[9], double u[36]);     // host: G g G^T of one 3x3 filter
void wino_debug_slots(int slots);            // test hook: workgroup slots the multi-tile Winograd GEMM sizes its grid for (0 = the device)
long wino_rows(long tiles);                  // rows per frequency plane of the V / M workspaces (tiles rounded up to 256)
int conv_wt_rows(int Cout);                   // packed weight rows (Cout rounded up to 128)
size_t conv_slab_floats();                    // size of the stream-K slab workspace
// host: plan-layout weights [Cout][ks*ks][Cin] -> packed [conv_wt_rows(Cout)][conv_kpad(ks*ks*Cin)] (dst pre-zeroed)
void conv_pack_weights(const float* w, int Cout, int Cin, int ks, float* dst);
inline int conv_kpad(int Ktot) { return (Ktot + 31) / 32 * 32; }

// --------------------------------------------------------------------------------------------
// Bandwidth-bound graph ops (ops_misc.hip)
// --------------------------------------------------------------------------------------------
// depthwise 3x3 pad 1 (+bias, ReLU / PReLU with per-channel slope); w9c = [9][C]
void launch_dwconv3x3(const float* in, const float* w9c, const float* bias, float* out, int B, int H, int W,
                      int C, int stride, int act, const float* slope, hipStream_t s);
// depthwise k x k VALID over a k x k map -> [B, C] (taps = k*k, w = [taps][C])
void launch_dwglobal(const float* in, const float* w, const float* bias, float* out, int B, int taps, int C, int act, const float* slope,
                     hipStream_t s);
// grouped 3x3 pad 1 with G = 2 | 4 channels per group on both sides; w = [9][C][G]
void launch_gconv3x3(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int C, int G, int stride, int act,
                     const float* slope, hipStream_t s);
void launch_affine(const float* in, const float* sc, const float* sh, float* out, long pixels, int C, hipStream_t s);
void launch_act(const float* in, const float* slope, float* out, long pixels, int C, int act, hipStream_t s);
void launch_add(const float* a, const float* b, float* out, long n, hipStream_t s);
void launch_upsample2x(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);

// --------------------------------------------------------------------------------------------
// Non-NN kernels of the face path (face_kernels.hip)
// --------------------------------------------------------------------------------------------
struct FaceRec {            // POD mirror of reference struct FaceBox (src/face_detector.h:8-12), 60 B
    int32_t x, y, w, h;
    float score;
    float lm[10];
};

// FaceDetector::preprocess (src/face_detector.cpp:92-137) → NHWC4 fp32 [B,inH,inW,4]
//   frames: B images, each rows x cols BGR u8 with row pitch `step` bytes and image pitch `img_stride`.
void launch_det_preprocess(const uint8_t* frames, long img_stride, int rows, int cols, int step, int B,
                           int inH, int inW, int newH, int newW, float* out, hipStream_t s);
// FaceRecognizer::preprocess (src/face_recognizer.cpp:135-150) on aligned crops → NHWC4
void launch_rec_preprocess(const uint8_t* crops, int n, int H, int W, float* out, hipStream_t s);

// ---- the graph's first Conv 3x3 (Cin = 3, pad 1) fused with the u8 preprocess (stem.hip): BGR u8 frames -> [B,Ho,Wo,Cout] fp32 ----
struct StemArgs {
    const uint8_t* src;         // B frames of srcH x srcW BGR pixels, row pitch `step` bytes, frame pitch img_stride, pasted at the origin of
    long img_stride;            // the inH x inW net input (the rest of it is the letterbox canvas, u8 0)
    int srcH, srcW, step, B;
    int inH, inW, stride, Cout; // Cout % 4 == 0
    const float *w27, *bias;    // the literal form: [27][Cout], k = (ky*3+kx)*3 + ci (ci in RGB order), and [Cout]
    const float *wf, *biasf;    // (optional) the normalisation folded in: wf[tap*3 + j][Cout] = w27[tap*3 + (2-j)] / 128 (j = byte of the BGR
                                // pixel), biasf = bias - 127.5/128 * sum_k w27[k]: the thread-per-pixel kernel (16 | 32 channels)
    const unsigned* wfrag;      // (optional, Cout % 16 == 0) wf as bf16 MFMA fragments (stem_pack_wfrag): the matrix-core kernel (48 | 64)
    const float* slope;         // [Cout] (PReLU) or null
    int act;                    // fh::Act
    float *out1, *out2;         // [B,Ho,Wo,Cout] or null; out2 = out1 * s2 + t2
    const float *s2, *t2;
    int cus;                    // compute units the persistent grids are sized for (0 = the whole device), as ConvArgs::cus
};
void launch_stem(const StemArgs& a, hipStream_t s);
void stem_pack_wfrag(const float* wf, int Cout, unsigned* out);   // wf [27][Cout] -> [Cout/16][3][64][4] dwords

// ---- detector post-process: decode / threshold per VIEW, one NMS per FRAME (flat, ragged and tiled calls alike) ---------------------
// A call's frames are cut into views; every view went through the network (or arrives as caller's rows) as one row block.  A flat or
// ragged call is the case of one view per frame and needs no tables; a tiled call (include/facehip.h: fh_det_detect_tiled_dev) brings
// both.
// One row per VIEW of a call, in plan order (the views of frame 0, then of frame 1, ...): the frame it belongs to, its index among the
// frame's views, its rectangle in the frame, its interior-edge mask (fh_view::edges; 0 for view 0) and its letterbox scale
// (fh_letterbox_plan of h x w; 0 = a dead view, which emits nothing).
struct ViewDesc {
    int32_t frame, local, x, y, w, h, edges;
    float scale;
};
static_assert(sizeof(ViewDesc) == 32, "ViewDesc is a 32-byte table row");
// One row per FRAME: its views are rows [first_view, first_view + views) of the view table, its keys and suppression flags live in
// [key_off, key_off + seg_cap) of the key / flag buffers, seg_cap = the power of two >= views * cap (the in-place sort pads up to it).
struct FrameSeg {
    int32_t first_view, views, key_off, seg_cap;
};
struct PostArgs {
    // the candidates: SCRFD heads (launch_scrfd_decode) ...
    const float* score[3];      // per stride [V, gh*gw*2]
    const float* bbox[3];       // [V, gh*gw*2, 4]
    const float* kps[3];        // [V, gh*gw*2, 10]
    int inH, inW;
    // ... or the reference's own layout (launch_rows_threshold): [V][n_rows][feat >= 15] = x1,y1,x2,y2,score,kps
    const float* rows;
    int n_rows, feat;
    // the views: both tables (a tiled call) or neither
    const ViewDesc* views;      // [V], or null: view b is frame b, whole and at the origin, with scale scales ? scales[b] : scale
    const FrameSeg* segs;       // [n_frames], or null: frame b owns payload block b and the key / flag segment [b * cap, (b + 1) * cap)
    const float* scales;        // (views == null) [V] per-frame letterbox scale of a ragged call, or null
    float scale;                // a view or frame whose scale is not > 0 (a dead one) emits nothing
    int V, cap, border;         // cap: candidates per view, a power of two; border < 0: the border rule is off
    float thr;
    FaceRec* cand;              // [V][cap] payload, one block per view
    unsigned long long* keys;   // per-frame segments; key = (score desc, local_view * cap + index asc)
    int* count;                 // [n_frames]
};
// Per candidate with score > thr: the reference's row arithmetic in VIEW coordinates, the border rule (a box within `border` pixels of
// an interior edge of its tile is dropped), the shift into frame coordinates, the payload store and the key appended to the FRAME's list
void launch_scrfd_decode(const PostArgs& a, hipStream_t s);
void launch_rows_threshold(const PostArgs& a, hipStream_t s);
// sort by key + greedy integer-IoU NMS (src/face_detector.cpp:340-384), one workgroup per frame over the frame's segment (segs, or
// null = the identity segment as PostArgs::segs); writes survivors (score-descending) to out[n_frames][max_out], counts to out_count[n_frames].
void launch_sort_nms(const FaceRec* cand, unsigned long long* keys, const int* count, const FrameSeg* segs, int cap, int n_frames,
                     float nms_thr, FaceRec* out, int* out_count, int max_out, int* order_ws, hipStream_t s);

// FaceRecognizer::alignFace (src/face_recognizer.cpp:93-133): similarity estimate + warpAffine
//   faces[n] with frame index frame_of[n]; writes crops [n,112,112,3] BGR u8 and ok[n].
void launch_align(const uint8_t* frames, long img_stride, int rows, int cols, int step, const FaceRec* faces,
                  const int* frame_of, int n, int outH, int outW, uint8_t* crops, int* ok, hipStream_t s);
// Mixed-size batches: one row per frame of the device table the ragged entry points build (engine.cpp FrameTable).  bgr = device pixels
// (any alignment), step = row pitch in bytes; new_h x new_w = the letterbox plan (fh_letterbox_plan), 0 x 0 for a dead frame.
struct FrameDesc {
    const uint8_t* bgr;
    int32_t rows, cols, step, new_h, new_w, pad_;
};
static_assert(sizeof(FrameDesc) == 32, "FrameDesc is a 32-byte table row");
// FaceDetector::preprocess' resize + paste (src/face_detector.cpp:101-121) for n frames of different sizes in one launch: canvas
// [n][inH][inW][3] u8 (4-byte aligned, inW % 4 == 0) = the frame resized to new_h x new_w (resize_px, bit for bit) top-left on zeros
void launch_letterbox_ragged(const FrameDesc* table, int n, int inH, int inW, uint8_t* canvas, hipStream_t s);
// launch_align with per-face frame geometry: face i lies on table[frame_of ? frame_of[i] : i] (an index outside [0, n_frames) or a dead
// frame gives the empty result, ok = 0)
void launch_align_ragged(const FrameDesc* table, int n_frames, const FaceRec* faces, const int* frame_of, int n, int outH, int outW,
                         uint8_t* crops, int* ok, hipStream_t s);
void launch_resize_u8c3(const uint8_t* src, long src_stride, int sh, int sw, int sstep, uint8_t* dst, long dst_stride,
                        int dh, int dw, int dstep, int n, hipStream_t s);

// FaceRecognizer::normalize (src/face_recognizer.cpp:306-318), one wave per row
void launch_l2_normalize(const float* in, float* out, int n, int dim, hipStream_t s);

// compareFaces generalised to 1:N (src/face_recognizer.cpp:320-334): top-k of (dot+1)/2 ranked (score desc, gallery index asc).
// gallery.hip: ONE streaming pass — gallery rows x queries on the matrix cores, per-workgroup top-k lists [gallery_parts][Q][k] kept in
// LDS while the rows go by (no G x Q matrix in memory); then launch_topk_merge.  The scans' launcher speaks of their argument struct
// and sits beside it: launch_gallery_scan, gallery_scan.h.
int gallery_parts(long G, int Q, int* tiles_per_part);
void launch_label(const float* best_score, const int* best_idx, int n, float thr, int* labels, hipStream_t s);
void launch_topk_merge(const float* part_score, const int* part_idx, int nparts, int Q, int k, float* out_score,
                       int* out_idx, hipStream_t s, const int* qcount = nullptr);     // qcount (device, optional): queries >= *qcount skipped
void launch_topk_merge_strided(const float* part_score, const int* part_idx, int nparts, int Q, int k, long part_stride, float* out_score,
                               int* out_idx, hipStream_t s, const int* qcount = nullptr);

// gallery_ids.hip — the labelled gallery: every row carries an identity id >= 0, a query is answered with its best k IDENTITIES, each
// represented by its best row (score desc, global row index asc).  Same streaming scan (gallery_scan.h), lists of (score, row, id) with
// at most one entry per identity, and an id plane beside the part / seed planes.
// [nparts][Q][k] identity lists (each list: distinct ids, -1 rows = empty) -> the identity top-k of their union; out_idx may be null
void launch_topk_merge_ids(const float* part_score, const int* part_id, const int* part_idx, int nparts, int Q, int k, float* out_score,
                           int* out_id, int* out_idx, hipStream_t s, const int* qcount = nullptr);
// out_id[i] = ids[idx[i] - idx_base] for idx[i] >= 0 (and, with use_thr, score[i] > thr), else -1
void launch_ids_of_rows(const float* score, const int* idx, int n, const int* ids, long idx_base, float thr, bool use_thr, int* out_id,
                        hipStream_t s);
// stable compaction: dst row j = src row map[j] (rows of row_bytes, a multiple of 16; 16-byte aligned buffers), j < m
void launch_gather_rows(const void* src, void* dst, const int* map, long m, size_t row_bytes, hipStream_t s);
void launch_gather_ids(const int* src, int* dst, const int* map, long m, hipStream_t s);

// gallery_tags.hip — watchlists: a 32-bit tag per row, a 32-bit mask per query, row r admitted for query q iff (tags[r] & qmask[q]) != 0;
// the answer is the exact top-k of the query's admitted rows or of their identities, global indices kept.  Same streaming scan, same
// part / seed planes, same merges.  tile_or[t] = OR of the tags of rows [128 t, 128 t + 128) by position; tag_ctr [2] (device) counts
// the (workgroup, tile) visits multiplied / skipped.
constexpr int GAL_TAG_TILE = 128;                            // rows per tile_or entry = the scan's row tile
void gallery_debug_tag_skip(int on);                         // 0: tagged scans multiply every tile (same answer); gallery.hip
// rebuilds tile_or for the tiles that rows [first, first + n) of a gallery of G rows touch
void launch_tag_tile_or(const unsigned* tags, long G, long first, long n, unsigned* tile_or, hipStream_t s);
// dst_tags[j] = OR of src_tags[order[i]], starts[j] <= i < starts[j + 1] (the inverted index of fh_gallery_group_ids), j < m
void launch_fuse_tags(const unsigned* src_tags, const int* order, const long long* starts, long m, unsigned* dst_tags, hipStream_t s);

// gallery_fuse.hip — template pooling (fh_gallery_fuse_ids): one wave per work item sums the rows src[order[begin + i]], i < count,
// strictly in that order (p = row0; p = p + row1; ...), into row `out` of dst (final != 0; L2-normalised when `unit` and count > 1: a
// one-row list is copied verbatim) or of the scratch `part` (final == 0: a chunk's partial sum, never normalised).  order == nullptr:
// the list is the consecutive rows begin .. begin + count of src (an identity's partials, added in chunk order by a second launch).
struct FuseItem { int begin, count, out, final; };
void launch_gallery_fuse_sum(const float* src, const int* order, const FuseItem* items, long n_items, int dim, float* dst, float* part,
                             bool unit, hipStream_t s);
// out[r] = (dot(src row r, the tmpl row whose id is src_ids[r]) + 1) / 2, or -1 when tmpl_ids (ascending, distinct, m of them) lacks it
void launch_gallery_self_scores(const float* src, const int* src_ids, long n, const float* tmpl, const int* tmpl_ids, long m, int dim,
                                float* out, hipStream_t s);

// gallery_cluster.hip — exact DBSCAN over the gallery's own rows (fh_gallery_cluster_dev; the rule: cluster_plan.h): init, degree pass
// (min_pts > 1), link pass and flatten on s.  deg / parent [G] and best [G] are scratch; labels [G] and info [4] (may be null) the result.
void launch_gallery_cluster(const float* gal, long G, int dim, float thr, int min_pts, bool noise_self, int* deg, int* parent,
                            unsigned long long* best, int* labels, int* info, hipStream_t s);
void cluster_debug_tiles(int tiles_per_wg);   // test hook: A tiles per workgroup run of the pair passes (0 = automatic)
// The same pair pass with the histogram epilogue (fh_gallery_pair_hist_dev; the bin rule: roc_plan.h): hist [2][kHistBins] (genuine,
// impostor) and nan [2] (may be null) are overwritten with the counts over all pairs row < col < G; scratch holds
// gallery_pair_hist_scratch_bytes() and is cleared on s first.  G <= 0 launches nothing.
void launch_gallery_pair_hist(const float* gal, const int* ids, long G, int dim, unsigned long long* scratch, unsigned long long* hist,
                              unsigned long long* nan, hipStream_t s);
size_t gallery_pair_hist_scratch_bytes();
void cluster_debug_hist_copies(int copies);   // measurement hook: privatised histogram copies the workgroups flush into (0 = default)
// The pair audit (fh_gallery_pairs_dev; the rule: pairs_plan.h): the pair pass with the count epilogue, the cut, the pair pass with the
// collect epilogue, the select kernel — all on s.  info [4] = {count, nan, returned, complete}; out_s [cap], out_rows / out_ids [cap][2]
// (each may be null; out_ids needs ids) = the first `returned` pairs of the ordered list, (-1.0f, -1, -1) behind them.  ids may be null
// for class "any".  scratch holds gallery_pairs_scratch_bytes(cap); its head is cleared on s first.  G <= 0 launches nothing.
constexpr int kPairsSlots = 2048 + 1;         // 64-bit words of the scratch: selected pairs by rank, then the class's NaN-scored pairs
constexpr int kPairsHead = kPairsSlots + 3;   // ... {int cut, unsigned slot counter}, {returned}, one word of padding: candidates 16-byte aligned
constexpr long kPairsRoom = 65536;            // candidates held at most (16 bytes each)
void launch_gallery_pairs(const float* gal, const int* ids, long G, int dim, int cls, int side, float thr, int cap,
                          unsigned long long* scratch, unsigned long long* info, float* out_s, int* out_rows, int* out_ids, hipStream_t s);
long gallery_pairs_room(int cap);             // max(the room in force, cap)
size_t gallery_pairs_scratch_bytes(int cap);
void pairs_debug_room(long room);             // test hook: the candidate room (0 = kPairsRoom)
// gallery_pairs.hip — the one-workgroup kernels of the audit.  cut: pairs_cut over the scratch's counters -> info, and the last rank to
// collect + `returned` into the scratch.  select: the best `cap` candidates under pairs_before (bitonic sort in LDS, a batch at a time),
// the three lists and their padding.  empty: info = {0, 0, 0, 1} and empty lists (an empty gallery).
void launch_pairs_cut(unsigned long long* scratch, int cap, long room, unsigned long long* info, hipStream_t s);
void launch_pairs_select(const unsigned long long* scratch, long room, int side, int cap, const int* ids, float* out_s, int* out_rows,
                         int* out_ids, hipStream_t s);
void launch_pairs_empty(int cap, unsigned long long* info, float* out_s, int* out_rows, int* out_ids, hipStream_t s);

// gallery_f16.hip — the opt-in F16_RERANK scan (fh_gallery_set_scan): an fp16 copy of the rows is scanned for the top GAL16_KC candidates
// per query, the candidates are re-scored from the fp32 rows exactly as gallery_topk_kernel scores them, and a per-query certificate
// proves that no other row can reach the top-k; uncertified queries are compacted on the device (fb_count / fb_idx) for the fp32 scan.
constexpr int GAL16_KC = 32;
// f32 -> f16 (round to nearest even) of n rows; stats[0..2] = float bits of max ||g||, max ||g^||, max ||g - g^|| (rounded up, atomicMax
// into what is there), stats[3] |= 1 when a value is non-finite or |x| > 65504
void launch_gallery16_convert(const float* rows, uint16_t* rows16, long n, int dim, unsigned* stats, hipStream_t s);
int gallery16_parts(long G, int Q, int* tiles_per_part);
// queries [Q][dim] f32 -> q16 [ceil64(Q)][dim] -> fp16 scan + merge: cand_* = [Q][GAL16_KC] (fp16 mapped score, global index; -1 = none)
// part_*: [gallery16_parts][Q][GAL16_KC], seed_*: [Q][GAL16_KC]
void launch_gallery16_candidates(const uint16_t* rows16, long G, int dim, const float* q, uint16_t* q16, int Q, long idx_base, float* part_score,
                                 int* part_idx, float* seed_score, int* seed_idx, float* cand_score, int* cand_idx, hipStream_t s);
// exact fp32 re-score of the candidates + top-k + certificate (bounds = max ||g||, max ||g^||, max ||g - g^||); certified queries are
// written to out_*, the others appended to fb_idx (fb_count must be 0 before); counters[0] += certified, counters[1] += fallback
void launch_gallery16_rescore(const float* rows, long G, int dim, const float* q, int Q, int k, long idx_base, const float* cand_score,
                              const int* cand_idx, float gn, float ghn, float dn, float* out_score, int* out_idx, int* fb_count, int* fb_idx,
                              unsigned long long* counters, hipStream_t s);
// qpacked [ceil64(Q)][dim]: row r < *fb_count = q[fb_idx[r]], zero behind; then the fp32 answers fb_* [*fb_count][k] back to rows fb_idx
void launch_gallery16_gather(const float* q, int Q, int dim, const int* fb_count, const int* fb_idx, float* qpacked, hipStream_t s);
void launch_gallery16_scatter(const float* fb_score, const int* fb_idx_out, int Q, int k, const int* fb_count, const int* fb_idx, float* out_score,
                              int* out_idx, hipStream_t s);

// gallery_range.hip — exact threshold search (fh_gallery_range_dev; the rule: range_plan.h): the scan of gallery_scan.h with the hit
// bitmap as its epilogue, popcounts, then per query the best `cap` hits re-scored from the fp32 rows and sorted.  qpacked
// [ceil64(Q)][dim], zero rows behind Q; masks (device [Q]) with tags (device [G]), or both null; hits / unit_cnt: scratch of
// gallery_range_hits_bytes / gallery_range_units_bytes (G, Q), written before they are read: never cleared.  counts [Q]; out_* [Q][cap],
// each may be null — all three null: counts only, no row is gathered; ids (needed with out_d): the id of every row.  G == 0: zero counts,
// empty lists.  Q <= 0 launches nothing.
constexpr int GAL_RANGE_UNIT = 256;                          // 32-row blocks per unit of the count planes (8192 rows)
size_t gallery_range_hits_bytes(long G, int Q);
size_t gallery_range_units_bytes(long G, int Q);
void launch_gallery_range(const float* rows, long G, int dim, const float* qpacked, const unsigned* tags, const unsigned* masks, int Q,
                          long idx_base, float thr, int cap, unsigned* hits, int* unit_cnt, const int* ids, long long* counts, float* out_s,
                          int* out_i, int* out_d, hipStream_t s);

// gallery_deep.hip — exact top-k of 1 <= k <= GAL_DEEP_MAX rows per query (fh_gallery_topk_deep_dev; the rule and the block rule:
// deep_plan.h): the scan of gallery_scan.h with the maximum per (32-row block, query) as its epilogue, then per query the best k blocks
// by that maximum, their rows re-scored from the fp32 rows and the best k of those.  qpacked, tags / masks, ids, out_* [Q][k] as for
// launch_gallery_range; bmax / bmax_t (the maxima by block and by query), chosen (the chosen blocks [Q][k]) and cand (their rows' scores
// [Q][k][32]): scratch of gallery_deep_*_bytes, each written before it is read: never cleared.  G == 0: empty lists.  Q <= 0 launches
// nothing.
constexpr int GAL_DEEP_MAX = 1024;
size_t gallery_deep_bmax_bytes(long G, int Q);
size_t gallery_deep_bmax_t_bytes(long G, int Q);
size_t gallery_deep_chosen_bytes(int Q, int k);
size_t gallery_deep_cand_bytes(int Q, int k);
void launch_gallery_deep(const float* rows, long G, int dim, const float* qpacked, const unsigned* tags, const unsigned* masks, int Q,
                         long idx_base, int k, float* bmax, float* bmax_t, int* chosen, float* cand, const int* ids, float* out_s,
                         int* out_i, int* out_d, hipStream_t s);

// detect -> embed hand-off: first min(count,F) faces per frame, densely packed (n <= 4096 frames)
void launch_select_faces(const FaceRec* det, const int* counts, int n, int per_frame, int F, FaceRec* faces, int* frame_of,
                         int* total, hipStream_t s);

// --------------------------------------------------------------------------------------------
// Face tracker (track.hip; the contract is in include/facehip.h)
// --------------------------------------------------------------------------------------------
struct TrackState {         // layout of fh_track_state, 32 B; id = -1: a free slot
    int32_t id, x, y, w, h, last_seen, last_embed, hits;
};
constexpr TrackState kFreeTrack{-1, 0, 0, 0, 0, 0, 0, 0};
struct TrackParams {
    int max_tracks;         // 1 .. 64 slots per stream (one lane each)
    float iou_thr;
    int max_missed, refresh;
    int bs_num, bs_den, bs_gap;     // the best-shot rule: re-embed when q * den > best_q * num and min_gap frames have passed
};
// One wave per stream walks starts[s] .. starts[s + 1] of `order` (track_plan.h).  heads = [streams][2] (frame_no, next_id), slots =
// [streams][max_tracks].  det = [n][per_frame] records, counts = [n]; track / embed = [n][per_frame] are written entirely, and so is
// slot (the lane of the detection's track, else -1) unless it is null.  quality = [n][per_frame] and best_q = [streams][max_tracks]:
// both non-null = the best-shot policy is on for this call; either null = the update without it, bit for bit.
void launch_track_update(int* heads, TrackState* slots, int streams, TrackParams p, const FaceRec* det, const int* counts, int per_frame,
                         const int* order, const int* starts, int* track, int* embed, int* slot, const int* quality, int* best_q,
                         hipStream_t s);
// face_quality.hip: quality[n][per_frame] = the score of face_quality.h for the entries below each frame's count, 0 behind it.  table ==
// nullptr: frame f = frames + f * stride (rows x cols, row pitch step); otherwise the ragged table's row f (frames etc. unused).
void launch_face_quality(const uint8_t* frames, long stride, int rows, int cols, int step, const FrameDesc* table, int n, const FaceRec* det,
                         const int* counts, int per_frame, int* quality, hipStream_t s);
// the flagged twin of launch_select_faces: the records with embed != 0, densely in (frame, slot) order, with frame index and track id
void launch_track_select(const FaceRec* det, const int* embed, const int* track, int n, int per_frame, FaceRec* faces, int* frame_of,
                         int* track_of, int* total, hipStream_t s);

// Per-track identity (track_ident.hip).  One TrackIdent (layout of fh_track_ident, 16 B) and one fp32 sum row [dim] per (stream, slot).
struct TrackIdent {
    int32_t owner, n_emb, label;    // owner = the track id the entry belongs to, -1: none
    float score;
};
constexpr TrackIdent kFreeIdent{-1, 0, -1, -1.0f};
constexpr int kTrackPoolLast = 0, kTrackPoolSum = 1, kTrackPoolWeighted = 2;     // enum fh_track_pool
struct TrackIdentState {
    TrackIdent* ident;      // [streams][max_tracks]
    float* sums;            // [streams][max_tracks][dim]
    int streams, max_tracks, dim, pool;
};
// One identify call (Tracker::identify_dev) as its kernels see it: what the update wrote, the stream plan (track_plan.h), the ranks.
struct TrackCall {
    const int *track, *slot, *embed;    // [n][per_frame], the update's outputs
    const int* quality;                 // [n][per_frame], read only by kTrackPoolWeighted (which needs it); else may be null
    int* frame_off;                     // [n + 1] = the flags before each frame, written by launch_track_ranks: rank = frame_off[f] + those before it in f
    const int *order, *starts;          // [n], [streams + 1], on the device
    int n, per_frame, total;            // total = the embeddings given: a flagged entry of rank >= total is nobody's
};
void launch_track_ranks(const TrackCall& c, hipStream_t s);
// stage A: one wave per (stream, slot), one more per stream for the untracked faces; emb [total][dim] -> queries[min(total, flags)][dim]
void launch_track_pool(const TrackIdentState& st, const TrackCall& c, const float* emb, float* queries, hipStream_t s);
// stage C: one wave per stream; ans_label / ans_score = [total] answers of the queries; label / score = [n][per_frame], written entirely
void launch_track_propagate(const TrackIdentState& st, const TrackCall& c, const int* ans_label, const float* ans_score, int* label,
                            float* score, hipStream_t s);
// gallery_tags.hip, the tracker's watchlist per camera: qmask[j] = stream_mask[stream of the frame that query j belongs to], j < c.total
void launch_track_query_masks(const unsigned* stream_mask, int streams, const TrackCall& c, unsigned* qmask, hipStream_t s);

// Track re-linking (track_ident.hip; include/facehip.h, "track re-linking").  Per stream a table of max_tracks + memory records: rows
// below max_tracks belong to the slots (their sums are the identity's `sums`), the rest is the memory of lost tracks (`msums`).
struct TrackLink {          // layout of fh_track_link, 32 B; owner = -1: a free row
    int32_t owner, root, n_emb, label;
    float score;
    int32_t last_seen, links, pad;
};
constexpr TrackLink kFreeLink{-1, -1, 0, -1, -1.0f, 0, 0, 0};
constexpr int kTrackLinkMemory = 256;                                            // memory rows per stream, at most
struct TrackLinkParams {
    int memory;             // 0 .. kTrackLinkMemory
    float link_thr;
    int max_missed, max_age;
};
// stage A with re-linking on: one workgroup per stream; heads = the tracker's [streams][2] (frame_no, next_id) after the update.
// Writes queries as launch_track_pool does (the untracked faces' copies included) and root[n][per_frame] entirely.
void launch_track_link(const TrackIdentState& st, TrackLink* links, float* msums, const int* heads, TrackLinkParams lp, const TrackCall& c,
                       const float* emb, float* queries, int* root, hipStream_t s);
// re-linking off: root[i] = track[i] where slot[i] >= 0, else -1 (entries = n * per_frame)
void launch_track_roots(const int* track, const int* slot, long entries, int* root, hipStream_t s);

}  // namespace fh
