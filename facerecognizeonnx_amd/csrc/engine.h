// engine.h — device-side owner of one loaded graph (weights + activation arena + launch
// sequence) and the detector / recognizer / gallery objects built on it.  These are the
// objects behind the opaque C handles of include/facehip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"
#include "plan.h"
#include "tile_plan.h"

namespace fh {


struct DevBuf {                // owning hipMalloc buffer
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf();
    void ensure(size_t n);     // grow-only (re)allocation
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    void grow(size_t n, size_t keep) {   // ensure(n) that keeps the first `keep` bytes: a second buffer takes them, the old one is freed
        if (n <= bytes) return;
        if (keep == 0) return ensure(n);
        DevBuf bigger;
        bigger.ensure(n);
        FH_HIP(hipMemcpy(bigger.p, p, keep, hipMemcpyDeviceToDevice));
        swap(bigger);
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

unsigned long long layout_epoch();   // bumped by every DevBuf (re)allocation / release in the process (key of captured graphs)

// One ONNX graph planned for a fixed input size, resident on the current device.
class Net {
  public:
    Net(const std::string& onnx_path, int default_h, int default_w);
    void reserve(int max_batch);                          // arena + split-K slabs for this batch
    float* input() const { return arena_.as<float>() + plan_.tensors[plan_.input].offset * (size_t)cap_; }
    float* output(int i) const { return tensor_ptr(plan_.outputs[i].tensor); }
    void run(int batch, hipStream_t s, int first_op = 0);
    // preprocess (+ first conv when it can be fused) straight from BGR u8 images, then the rest of the graph.
    // srcH x srcW = pasted image (<= net input; the remainder is the zero letterbox canvas)
    void run_u8(const uint8_t* src, long img_stride, int srcH, int srcW, int step, int batch, hipStream_t s);
    bool fuse_stem = true;                                // tuning / test hook: keep the preprocessed input tensor
    bool fuse_front = true;                               // tuning / test hook: stem conv inside the first depthwise -> pointwise kernel
    const Plan& plan() const { return plan_; }
    int in_h() const { return plan_.inH; }
    int in_w() const { return plan_.inW; }
    int capacity() const { return cap_; }
    bool winograd = true;                                 // Winograd F(4x4,3x3) for the deep 3x3 convs (false: direct form everywhere)
    bool halo_conv = true;                                // tuning / test hook: spatial-tile kernel for the thin 3x3 convolutions
    bool fold_shortcut = true;                            // tuning / test hook: a block's strided 1x1 shortcut as a tenth tap of the 3x3 it is added to
    bool fuse_wino = true;                                // tuning / test hook: fused output+input transform between consecutive Winograd layers
    // opt-in precision mode (fh_rec_set_precision): the Winograd GEMMs take split-bf16 operands (hi + mid bf16 per value, three bf16 MFMAs,
    // f32 accumulate); transforms, epilogues and every other layer stay fp32.  Returns the number of layers that switch.
    int set_bf16x2(bool on, hipStream_t s);
    bool bf16x2() const { return bf16x2_; }
    // the fp32 mode's Winograd GEMMs as six bf16 MFMAs on three-piece operands (fp32 results, not bit-identical to the f32 MFMA; gemm_tile.h):
    // the recogniser's default (fh_rec_set_wino_x3, FACEHIP_WINO_X3), off for every other Net.  on: the weights are split once, on the
    // device, into a second image of 1.5 x the f32 one's bytes.  Returns the number of layers that have the form.
    int set_wino_x3(bool on, hipStream_t s);
    bool wino_x3() const { return wino_x3_; }
    // The same switch governs the direct convolutions with a folded shortcut (IResNet's stride-2 3x3 layers): their K loop on three bf16
    // pieces (conv_mfma.hip, X3) where conv_x3_pays says the launch gains.  Number of layers that have the form while the switch is on.
    int conv_x3_layers() const { return conv_x3_ ? conv_x3_n_ : 0; }
    // ... and, with a switch of their own underneath, the 1x1 stride-1 convolutions (conv_pw_x3_kernel, where conv_pw_x3_bn / conv_pw_x3_pays
    // admit the launch).  set_wino_x3 sets it too (MobileFaceNet's 1x1s ride on the recogniser's switch); the detector sets it alone
    // (fh_det_set_x3, FACEHIP_DET_X3).  Returns / reports the number of layers that have the 1x1 form while it is on.
    int set_pw_x3(bool on, hipStream_t s);
    int pw_x3_layers() const { return pw_x3_ ? pw_x3_n_ : 0; }
    // ... and the fused F(2x2) Winograd layers (wino2_x3_kernel, where wino2_x3_pays admits the launch; their image is built at load time).
    int wino2_x3_layers() const { return wino2_x3_ ? wino2_x3_n_ : 0; }
    int cus = 0;                                          // CUs of the stream this net runs on when it is CU-masked (0 = all)
    int force_cfg = -1;                                   // tuning hook: conv tile config override
    bool sk_enable = true;                                // tuning hook: stream-K remainder wave
    // every switch above that changes which kernels run or with which arguments, as one word: part of the key of a captured
    // batch-1 graph (api.cpp), so a setter between two calls can never be answered by a replay of the old launch sequence
    long long config_word() const {
        return (long long)fuse_stem | (long long)fuse_front << 1 | (long long)winograd << 2 | (long long)halo_conv << 3 |
               (long long)fold_shortcut << 4 | (long long)fuse_wino << 5 | (long long)bf16x2_ << 6 | (long long)sk_enable << 7 |
               (long long)(cus & 0xffff) << 8 | (long long)((force_cfg + 1) & 0xff) << 24 | (long long)wino_x3_ << 32 | (long long)conv_x3_ << 33 |
               (long long)pw_x3_ << 34 | (long long)wino2_x3_ << 35;
    }

  private:
    struct DevOp {
        size_t wt = 0, bias = 0, slope = 0, s2 = 0, t2 = 0;   // float offsets into params_
        bool has_slope = false, has_aff = false;
        size_t w27 = 0;                                       // stem layout [27][Cout] (op 0 only)
        size_t wfr = 0;                                       // ... and wf as bf16 MFMA fragments (stem_pack_wfrag), 16-channel stems
        size_t wf = 0, bf = 0;                                // ... and with the u8 normalisation folded in (byte order, w / 128; adjusted bias)
        size_t dww = 0, dwb = 0;                              // fused depthwise front end (DWPW)
        size_t w36 = 0;                                       // Winograd F(4,3) weights U[36][rows][Cin]
        size_t w36n = 0, w36p = 0;                            // ... their float count; offset of the split-bf16 copy in w36_bf_ (bf2 layers)
        size_t w36x = 0;                                      // ... offset of the three-piece (x3) image in w36_x3_ (bf2 layers)
        int w36k = 0;                                         // ... Cin
        bool bf2 = false;                                     // this layer's GEMM has a split-bf16 (and a three-piece) form
        size_t wfrag = 0;                                     // halo-conv weights in MFMA fragment order (conv_halo.hip)
        bool halo = false;                                    // eligible for the spatial-tile 3x3 kernel
        bool wino = false;                                    // eligible: 3x3 stride 1 pad 1, Cin >= 128
        size_t w2 = 0;                                        // fused Winograd F(2x2,3x3) image of the filter (conv_wino2.hip): 3x3 stride 1 pad 1,
        bool w2ok = false;                                    //   32 <= Cin < 128, Cout % 64 == 0 (IResNet's 64-channel stages)
        size_t w2x = 0;                                       // ... its three-piece (x3) image (wino2_pack_weights_x3) ...
        bool w2x_ok = false;                                  // ... which exists (plain layers: Cout % 64 == 0, no merged outputs)
        int aff_src = -1;                                     // Winograd op whose input is op[aff_src]'s second (BatchNorm) output and its only
                                                              // consumer: the transform reads op[aff_src].out and applies that affine itself
        int aff_dst = -1;                                     // ... and the producer's side of the same link
        int bn_fold_src = -1;                                 // direct 3x3 conv with its block's BatchNorm folded in (weights * s, 9-class bias):
                                                              // reads op[bn_fold_src].out, whose second output is then never written
        bool bn_fold_dst = false;                             // ... and the producer's side: skip out2
        int sc_src = -1;                                      // 3x3 conv that can take op[sc_src] (1x1 shortcut) into its K loop ...
        size_t wt_sc = 0, bias_sc = 0;                        // ... weights [rows][9*Cin + sc_C] and summed bias for that form
        int Kpad_sc = 0;
        size_t wt_sc_x3 = 0;                                  // ... offset of that form's three-piece (x3) weight image in wsc_x3_
        bool sc_x3 = false;                                   // ... which exists (Cin % 32 == 0, Cout % 64 == 0)
        size_t wt_pw_x3 = 0;                                  // 1x1 stride-1 convolution: offset of its three-piece (x3) weight image in wpw_x3_ ...
        bool pw_x3 = false;                                   // ... which exists (plain CONV, Cin % 4 == 0, Cout % 4 == 0, Kpad % 32 == 0, one output)
        bool sc_dst = false;                                  // ... and the shortcut's side: skipped when its consumer folds it
        bool fuse_next = false;                               // Winograd op followed by another on the same small map: fused transform kernel
        bool fuse_feed_aff = false;                           //   the next conv sees out * s2 + t2 (its block's BatchNorm) instead of out
        bool fuse_keep_out1 = true;                           //   something else reads the plain output too (e.g. a later residual): write it
        int Kpad = 0;
    };
  public:
    float* workspace() const { return partial_.as<float>(); }   // stream-K slabs (diagnostic builds of dwpw_mfma.hip park phase stamps there)
    unsigned* error_record() const { return sk_rec_.p; }        // this Net's stream-K watchdog record (null before reserve)
  private:
    float* tensor_ptr(int t) const { return arena_.as<float>() + plan_.tensors[t].offset * (size_t)cap_; }
    Plan plan_;
    std::vector<DevOp> dev_;
    DevBuf params_, arena_, partial_, wino_v_, wino_m_, w36_bf_, w36_x3_, wsc_x3_, wpw_x3_;
    bool bf16x2_ = false, wino_x3_ = false, conv_x3_ = false, pw_x3_ = false, wino2_x3_ = false;
    int conv_x3_n_ = 0, pw_x3_n_ = 0, wino2_x3_n_ = 0;
    size_t wino_maxc_ = 0;
    size_t wino_elems_ = 0;                                   // per image: 36 * tiles * max(Cin, Cout) of the largest Winograd op
    int cap_ = 0;
    struct SkRecord {                                         // host-mapped; parked on a free list at destruction (the device may still write it)
        unsigned* p = nullptr;
        int device = -1;                                      // the device whose launches write it (set with p)
        SkRecord() = default;
        SkRecord(const SkRecord&) = delete;
        SkRecord& operator=(const SkRecord&) = delete;
        ~SkRecord();
    } sk_rec_;
    unsigned sk_gen_ = 0;                                     // conv_error_generation() this Net's hand-off counters were last zeroed under
    bool stem_ok_ = false;
    bool front_ok_ = false;                                   // ops 0 + 1 = stem conv (16 channels) -> DW+PW: one kernel
};

// FaceDetector::preprocess' letterbox arithmetic (src/face_detector.cpp:101-113), the ONE place it lives: scale = min((float)in_w / cols,
// (float)in_h / rows), new_w = (int)((float)cols * scale), new_h likewise.  Returns 1 for a live frame; 0 — with scale = 0 and a 0 x 0
// plan — for an empty image (:94-98) or "Invalid resize dimensions" (:109-113).  Host code (fh_letterbox_plan).
int letterbox_plan(int rows, int cols, int in_w, int in_h, int* new_w, int* new_h, float* scale);

// One frame of a mixed-size batch as the caller describes it (layout of fh_frame, include/facehip.h): bgr = DEVICE pixels.
struct FrameIn {
    const uint8_t* bgr;
    int32_t rows, cols, step;
};
inline bool frame_empty(const FrameIn& f) { return !f.bgr || f.rows <= 0 || f.cols <= 0; }     // the reference's empty image

// A small host-built table sent to the device with ONE asynchronous copy on the caller's stream.  The copy's source must outlive it, and
// the next call on the handle may follow at once with another table, so the pinned staging memory is a RING of kSlots buffers, each with
// an event recorded behind its copy: stage() takes the next slot and — only when the ring has wrapped round to a slot whose copy may
// still be pending — waits for that slot's event before the caller rewrites it.  (The device side needs no ring: it is rewritten in
// stream order.)
class StagedTable {
  public:
    StagedTable() = default;
    StagedTable(const StagedTable&) = delete;
    StagedTable& operator=(const StagedTable&) = delete;
    ~StagedTable();
    void* stage(size_t bytes);                       // pinned host memory for the next table
    void* send(size_t bytes, hipStream_t s);         // the staged bytes -> the device buffer (returned), asynchronously on s
    void* dev() const { return dev_.p; }

  private:
    static constexpr int kSlots = 4;
    struct Slot { void* p = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool pending = false; } slot_[kSlots];
    int next_ = 0, cur_ = 0;
    DevBuf dev_;
};

// The device image of a call's frame descriptors: [n] FrameDesc rows followed by [n] float scales, built on the host from the caller's
// descriptors and letterbox_plan (StagedTable).
class FrameTable {
  public:
    // in_w / in_h > 0: plan the letterbox of every frame; 0: geometry only (the recogniser's align).  Returns the device table.
    const FrameDesc* upload(const FrameIn* frames, int n, int in_w, int in_h, hipStream_t s);
    const FrameDesc* table() const { return static_cast<const FrameDesc*>(st_.dev()); }
    const float* scales() const { return reinterpret_cast<const float*>(table() + n_); }
    int size() const { return n_; }

  private:
    int n_ = 0;
    StagedTable st_;
};

// The tables of one tiled call, planned on the host (tile_plan.h): the views as plain frames (what the ragged letterbox + network run
// on), one ViewDesc per view and one FrameSeg per frame.  plan() returns the total view count, or -1 when it exceeds max_views (nothing
// is changed then); cap = the per-view candidate capacity (a power of two).
struct TilePlan {
    std::vector<FrameIn> view_frames;
    std::vector<ViewDesc> views;
    std::vector<FrameSeg> segs;
    size_t key_total = 0;                            // sum of the frames' seg_cap
    int plan(const FrameIn* frames, int n, const Tiling& t, int in_w, int in_h, int cap, int max_views);
};
constexpr int kTileMaxViews = 256;                   // FH_TILE_MAX_VIEWS

// the device image of a TilePlan's views + segs
class TileTable {
  public:
    void upload(const TilePlan& p, hipStream_t s);
    const ViewDesc* views() const { return static_cast<const ViewDesc*>(st_.dev()); }
    const FrameSeg* segs() const { return reinterpret_cast<const FrameSeg*>(views() + V_); }

  private:
    int V_ = 0;
    StagedTable st_;
};

// The detector's post-process on the a.V views of n_frames frames: zero the counts, decode (a.rows == nullptr: the SCRFD heads) or
// threshold (a.rows: pre-decoded rows [V][n_rows][feat]), then one NMS per frame.  The caller fills the candidate source, thr, cap, V
// and the buffers.  tab == nullptr: a flat or ragged call, one view per frame (V == n_frames) with a.scale / a.scales; else the tables
// of a tiled call, whose a.border applies.  counts of frames without views are 0.  sup: the NMS' flags, sized as a.keys.
void postprocess_views(PostArgs a, int n_frames, const TileTable* tab, float nms_thr, int* sup, FaceRec* out, int max_out, int* counts,
                       hipStream_t s);

bool det_x3_default();   // the detector's 1x1 convolutions on three bf16 pieces unless FACEHIP_DET_X3=0 (read once)

class Detector {
  public:
    explicit Detector(const std::string& onnx_path);
    // frames: device pointer, n images of rows x cols BGR u8 (row pitch `step`, image pitch `stride`)
    // out: device [n][max_out] FaceRec, counts: device [n].  Asynchronous on stream s.
    void detect_dev(const uint8_t* frames, int n, int rows, int cols, int step, long stride, float score_thr, float nms_thr,
                    FaceRec* out, int max_out, int* counts, hipStream_t s);
    // network + decode only, for tests: rows15 = device [n][N][15]? not needed — outputs are read through net()
    Net& net() { return net_; }
    int num_anchors() const { return anchors_; }
    bool predecoded() const { return predecoded_; }
    float last_scale() const { return scale_; }
    // stage hooks used by parity tests (device pointers)
    void run_network_dev(const uint8_t* frames, int n, int rows, int cols, int step, long stride, hipStream_t s);
    void postprocess_dev(int n, float score_thr, float nms_thr, FaceRec* out, int max_out, int* counts, hipStream_t s);
    // input: device [n][inH][inW][4] preprocessed floats (lane 3 = 0) -> copied into net().input(), then every op runs (the path
    // run_u8 takes with the fused stem off, minus the preprocess kernel)
    void run_input_dev(const float* input, int n, hipStream_t s);
    // Mixed-size batches (frames: HOST array of n descriptors of device images).  plan -> table -> letterbox_ragged_kernel -> run_u8 on
    // the canvas, the path a batch of input-sized frames takes; postprocess_dev then divides by the per-frame scales.
    void letterbox_ragged_dev(const FrameIn* frames, int n, uint8_t* canvas, hipStream_t s);        // canvas [n][inH][inW][3], caller's
    void run_network_ragged_dev(const FrameIn* frames, int n, hipStream_t s);
    void detect_ragged_dev(const FrameIn* frames, int n, float score_thr, float nms_thr, FaceRec* out, int max_out, int* counts,
                           hipStream_t s);
    const FrameTable& frame_table() const { return table_; }   // of the last ragged call: handed to the recogniser's align by the pipeline
    // Tiled detection (include/facehip.h): the views of all frames are ONE ragged batch (table_ then holds the VIEWS), decoded with the
    // plan's view table and merged by one NMS per frame.  run_network_tiled_dev returns the total view count (0: only empty frames),
    // or throws std::invalid_argument when the call has more than kTileMaxViews views — before anything is launched.
    int run_network_tiled_dev(const FrameIn* frames, int n, const Tiling& t, hipStream_t s);
    void detect_tiled_dev(const FrameIn* frames, int n, const Tiling& t, float score_thr, float nms_thr, FaceRec* out, int max_out,
                          int* counts, hipStream_t s);
    // the FRAMES of the last tiled call (geometry only): the faces are in frame coordinates, so this — not table_ — is what the
    // pipeline's align reads
    const FrameTable& tiled_frame_table() const { return frames_table_; }

  private:
    void reserve(int n, int rows, int cols);
    PostArgs post_source(int V, float score_thr);         // the network's outputs of V views + this object's buffers, no views yet
    Net net_;
    bool predecoded_ = false;
    int anchors_ = 0, feat_ = 15, cap_ = 0, nb_ = 0;
    float scale_ = 1.f;
    bool ragged_ = false;                                 // the last network run was a ragged one: postprocess_dev reads table_.scales()
    FrameTable table_, frames_table_;
    TilePlan tplan_;
    TileTable ttab_;
    DevBuf resized_, cand_, keys_, count_, ws_;           // resized_: the uniform path's resized frames / the ragged path's canvas
};

class Recognizer {
  public:
    explicit Recognizer(const std::string& onnx_path);
    int dim() const { return dim_; }
    Net& net() { return net_; }
    // aligned crops [n][H][W][3] BGR u8 (device) -> L2-normalised embeddings [n][dim] (device)
    void embed_aligned_dev(const uint8_t* crops, int n, float* out, hipStream_t s, float* raw_out = nullptr);
    // alignFace + embed: faces[n] (device) on frames; ok[n] (device, may be null) 1/2 = produced, 0 = empty
    void embed_faces_dev(const uint8_t* frames, int rows, int cols, int step, long stride, const FaceRec* faces,
                         const int* frame_of, int n, float* out, int* ok, hipStream_t s);
    void align_dev(const uint8_t* frames, int rows, int cols, int step, long stride, const FaceRec* faces, const int* frame_of,
                   int n, uint8_t* crops, int* ok, hipStream_t s);
    void resize_embed_dev(const uint8_t* frames, int n, int rows, int cols, int step, long stride, float* out, hipStream_t s);
    // the same two on a mixed-size batch: face i lies on frame frame_of[i] (null = i) of a device table of n_frames rows — the
    // detector's (pipeline) or, from host descriptors, one this object builds
    void align_table_dev(const FrameDesc* table, int n_frames, const FaceRec* faces, const int* frame_of, int n, uint8_t* crops, int* ok,
                         hipStream_t s);
    void embed_faces_table_dev(const FrameDesc* table, int n_frames, const FaceRec* faces, const int* frame_of, int n, float* out, int* ok,
                               hipStream_t s);
    void align_ragged_dev(const FrameIn* frames, int n_frames, const FaceRec* faces, const int* frame_of, int n, uint8_t* crops, int* ok,
                          hipStream_t s);
    void embed_faces_ragged_dev(const FrameIn* frames, int n_frames, const FaceRec* faces, const int* frame_of, int n, float* out, int* ok,
                                hipStream_t s);
    // input: device [n][H][W][4] preprocessed floats (lane 3 = 0) instead of u8 crops; otherwise embed_aligned_dev
    void embed_input_dev(const float* input, int n, float* out, hipStream_t s, float* raw_out = nullptr);
    int max_chunk = 256;                                 // faces per network pass

  private:
    Net net_;
    int dim_ = 0;
    FrameTable table_;
    DevBuf crops_, ok_, raw_;
};

// The face tracker behind fh_tracker (include/facehip.h): per stream a (frame_no, next_id) head and max_tracks slots, resident on the
// device; one wave per stream updates them (track.hip).  The walk order of a call is planned on the host (track_plan.h) and sent
// through a StagedTable, so the next call may follow at once with another stream_of.  Identity (enable_identity; track_ident.hip): one
// TrackIdent and one fp32 sum row per (stream, slot), pooled, labelled against a gallery and carried forward by identify_dev.  Best
// shot (set_bestshot): one int32 best_q per (stream, slot), kept by the update kernel when it is given the faces' qualities.
// Re-linking (enable_relink): per stream a table of max_tracks + memory TrackLink records — the slots' rows, then a memory of lost
// tracks with sums of its own — through which identify_dev's stage A resumes a lost track when its face comes back.  (tracker.cpp)
class Gallery;
class Tracker {
  public:
    Tracker(int streams, int max_tracks, float iou_thr, int max_missed, int refresh);
    int streams() const { return streams_; }
    int max_tracks() const { return p_.max_tracks; }
    void reset(int stream);                                      // -1: all; synchronous
    // live slots of one stream, ascending, into out[max_tracks] (the rest: id = -1); returns their number; synchronous
    int get_state(int stream, TrackState* out, int* frame_no, int* next_id);
    // stream_of: HOST [n], already checked against [0, streams) (null: all stream 0).  track / embed = device [n][per_frame].
    // slot (optional) = device [n][per_frame]: the lane of each detection's track, else -1.  quality (optional) = device
    // [n][per_frame]: with the best-shot policy on, the update applies it; null or the policy off: the plain update.
    void update_dev(const FaceRec* det, const int* counts, int n, int per_frame, const int* stream_of, int* track, int* embed, int* slot,
                    const int* quality, hipStream_t s);
    // the best-shot policy: 1 <= den <= num <= 32768, min_gap >= 1, checked by the caller; synchronous; clears best_q on every call
    void set_bestshot(bool on, int num, int den, int min_gap);
    bool bestshot() const { return bestshot_; }
    bool has_best_quality() const { return best_.p != nullptr; }     // set_bestshot was called
    // best_q of the live slots, ascending, into out[max_tracks] (the rest: 0); returns their number; synchronous
    int get_quality(int stream, int* out);
    int* quality_scratch(size_t entries) { quality_.ensure(entries * sizeof(int)); return quality_.as<int>(); }   // the pipeline's qualities
    const int* quality() const { return quality_.as<int>(); }
    int* embed_scratch(size_t entries) { embed_.ensure(entries * sizeof(int)); return embed_.as<int>(); }   // the pipeline's flags
    int* slot_scratch(size_t entries) { slot_.ensure(entries * sizeof(int)); return slot_.as<int>(); }      // ... and its slots
    // identity: dim % 64 == 0, 64 <= dim <= 4096, pool 0 (last) / 1 (sum) / 2 (quality-weighted sum), checked by the caller;
    // synchronous; clears on every call
    void enable_identity(int dim, int pool);
    int identity_dim() const { return idim_; }                   // 0: not enabled
    int identity_pool() const { return ipool_; }
    // stages A (pool), B (label through g, chunks of <= 256 queries) and C (propagate) on s; arguments checked by the caller.  quality =
    // device [n][per_frame], needed (and read) by the weighted pool only.
    // root (optional) = device [n][per_frame]: the entries' chain roots (re-linking off: their own track ids).  With re-linking on it
    // is needed, and stage A is the link kernel.
    void identify_dev(Gallery& g, float thr, const int* track, const int* slot, const int* embed, const int* quality, const float* emb,
                      int total, int n, int per_frame, const int* stream_of, int* label, float* score, hipStream_t s, int* root = nullptr);
    // re-linking: 0 <= memory <= kTrackLinkMemory, a finite thr, max_age > max_missed and identity enabled, checked by the caller;
    // synchronous; clears the identity state and the table.  enable_identity switches it off again.
    void enable_relink(int memory, float thr, int max_age);
    bool relink() const { return relink_; }
    int link_rows() const { return p_.max_tracks + lp_.memory; }
    int max_missed() const { return p_.max_missed; }
    // the whole table of one stream by row into out[link_rows()] and its sums into sums_out[link_rows()][dim] (may be null); synchronous
    void get_links(int stream, TrackLink* out, float* sums_out);
    int* roots_scratch(size_t entries) { roots_.ensure(entries * sizeof(int)); return roots_.as<int>(); }     // the pipeline's roots
    const int* roots() const { return roots_.as<int>(); }
    const float* queries() const { return queries_.as<float>(); }   // [total][dim] of the last identify_dev
    // a watchlist per camera: masks_host [streams] (null: off, the default); with masks on, stage B of identify_dev labels every query
    // through the gallery's tagged label call with the mask of its frame's stream.  Synchronous.
    void set_stream_masks(const unsigned* masks_host);
    // the live slots' identities, ascending, into out[max_tracks] (the rest: id = -1) and their sums into sums_out[max_tracks][dim]
    // (may be null); returns their number; synchronous
    int get_identity(int stream, TrackIdent* out, float* sums_out);

  private:
    int* heads() const { return state_.as<int>(); }
    TrackState* slots() const { return reinterpret_cast<TrackState*>(state_.as<int>() + 2 * (size_t)streams_); }
    std::vector<TrackState> slots_of(int stream);                // the slots of one stream, copied to the host; synchronous
    const int* send_plan(StagedTable& table, const int* stream_of, int n, hipStream_t s);    // stream_of's plan through plan_ | iplan_
    int streams_;
    TrackParams p_;
    DevBuf state_, embed_, slot_;                                // [streams][2] heads, then [streams][max_tracks] slots
    bool bestshot_ = false;
    DevBuf best_, quality_;                                      // [streams][max_tracks] best_q / the pipeline's [n][per_frame] qualities
    StagedTable plan_, iplan_;                                   // order[n], starts[streams + 1] of update / identify (a queued update still reads its own)
    void clear_identity(int first, int count);
    int idim_ = 0, ipool_ = 0;
    DevBuf ident_, isum_;                                        // [streams][max_tracks] TrackIdent / [streams][max_tracks][idim_] sums
    DevBuf queries_, ans_label_, ans_score_, frame_off_;         // of one identify_dev: [total][idim_], [total], [total], [n + 1]
    void clear_links(int first, int count);
    bool relink_ = false;
    TrackLinkParams lp_{0, 0.f, 0, 0};
    DevBuf link_, msum_, roots_;                                 // [streams][max_tracks + memory] TrackLink / [streams][memory][idim_] / [n][F]
    bool masks_on_ = false;
    DevBuf smask_, qmask_;                                       // [streams] watchlist masks / [total] per-query masks of one identify_dev
};

class Gallery {
  public:
    explicit Gallery(int dim) : dim_(dim) {}
    // ids == nullptr: an unlabelled row set; otherwise one identity id >= 0 per row (host or device, as the rows) and the gallery is
    // LABELLED.  A gallery is one or the other: the mixed calls throw (FH_ERR_STATE) and change nothing.
    void upload(const float* rows, const int* ids, long n, bool device_src, long index_base);
    long enroll(const float* rows, const int* ids, long n, bool device_src);     // append; returns the global index of the first new row
    // The two queries.  queries [Q][dim] device, Q <= 256, k <= 16; masks (device [Q], may be null): the watchlist form — the same call
    // on the sub-gallery of each query's admitted rows, global indices kept, always the fp32 scan; ids: answer with IDENTITIES
    // (labelled gallery unless empty), each by its best row.
    // topk_dev -> out_score / out_row [Q][k], with ids also out_id [Q][k] (then out_row may be null; without ids out_id is unused).
    // Without masks the rows, and the k == 1 identity (the identity of the best row), are the top-k of the scan mode; an identity
    // list of k > 1 always takes the fp32 scan (32 row candidates cannot certify it).
    void topk_dev(const float* q, const unsigned* masks, int Q, int k, bool ids, float* out_score, int* out_id, int* out_row, hipStream_t s);
    // label_dev -> the best row (ids: its identity) per query if its mapped score > thr, else -1 (main.cpp:229-233); out_score = that
    // best score
    void label_dev(const float* q, const unsigned* masks, int Q, float thr, bool ids, int* out_label, float* out_score, hipStream_t s);
    // Threshold search (gallery_range.hip; the rule: range_plan.h): counts [Q] = the exact number of rows whose mapped score is above
    // thr (admitted rows only with masks), and — each may be null — out_score / out_row / out_id [Q][cap] = the best min(count, cap) of
    // them, (score desc, global row asc), empty slots (-1, -1, -1).  Always the fp32 rows, whatever the scan mode.  out_id needs a
    // labelled gallery unless empty.  Q, cap and thr are checked by the caller.  Asynchronous; the scratch (hit bitmap: 4 bytes per 32
    // rows and query of a whole 64-query tile, at most ceil(size / 32) * 1 KB = 1.6 % of the fp32 rows at dim 512; count planes: 1 / 256
    // of that) lives in the handle and grows, synchronously, with the first call of a larger (Q, size).
    void range_dev(const float* q, const unsigned* masks, int Q, float thr, int cap, long long* counts, float* out_score, int* out_row,
                   int* out_id, hipStream_t s);
    // Deep top-k (gallery_deep.hip; the rule: deep_plan.h): out_score / out_row / out_id [Q][k] — each may be null — = the best
    // min(k, eligible) rows of every query (admitted rows only with masks; a NaN or -inf score is never listed), (score desc, global
    // row asc), empty slots (-1, -1, -1); 1 <= k <= 1024.  Always the fp32 rows, whatever the scan mode; it touches neither the part /
    // seed lists nor the F16_RERANK state.  out_id needs a labelled gallery unless empty.  Q and k are checked by the caller.
    // Asynchronous; the scratch (block maxima, twice the size of range_dev's hit bitmap; the chosen blocks and their rows' scores, 132
    // bytes per list entry) lives in the handle and grows, synchronously, with the first call of a larger (Q, size, k).
    void topk_deep_dev(const float* q, const unsigned* masks, int Q, int k, float* out_score, int* out_row, int* out_id, hipStream_t s);
    // removes every row whose id is listed (stable compaction through a second buffer: transiently the surviving fp32 rows, ids and
    // fp16 rows exist twice, plus 4 bytes per survivor); synchronous; returns the number of rows removed
    long remove_ids(const int* ids_host, long n_ids);
    void get_ids(long first, long n, int* out_host);
    void get_rows(long first, long n, float* out_host);           // fp32 rows by position, either kind of gallery
    // Template pooling (gallery_fuse.hip): THIS gallery is replaced by one row per identity of src, ascending ids, index base 0 — the
    // identity's rows summed in the fixed chunked order (chunks of `chunk` rows), normalised when `unit`.  Synchronous; returns the
    // number of identities.  src must be another gallery of the same dim, labelled unless empty (the caller checks the first two).
    long fuse_from(Gallery& src, bool unit, int chunk);
    bool fused() const { return fused_; }                        // ids distinct and ascending: set by fuse_from, cleared by upload / enroll
    // out[r] = (dot(row r, tmpl's row of row r's id) + 1) / 2, -1 where tmpl has no such id; tmpl.fused() required.  Asynchronous.
    void self_scores_dev(const Gallery& tmpl, float* out, hipStream_t s);
    // Exact DBSCAN over the fp32 rows (gallery_cluster.hip; the rule: cluster_plan.h): labels [size] = positions, info [4] (may be null),
    // both device.  Arguments checked by the caller.  Asynchronous; the scratch (16 bytes per row) is cleared on s at every call.
    void cluster_dev(float thr, int min_pts, bool noise_self, int* labels, int* info, hipStream_t s);
    // Genuine / impostor score histograms over all unordered pairs of the fp32 rows (gallery_cluster.hip; the bin rule: roc_plan.h):
    // hist [2][2048] and nan [2] (may be null), both device, both overwritten.  Needs a labelled gallery unless empty (the caller
    // checks).  Asynchronous; the scratch (the histogram the workgroups flush into) lives in the handle and is cleared on s at every call.
    void pair_hist_dev(unsigned long long* hist, unsigned long long* nan, hipStream_t s);
    // The pair audit (gallery_cluster.hip, gallery_pairs.hip; the rule: pairs_plan.h): info [4] = {count, nan, returned, complete};
    // out_score [cap], out_rows / out_ids [cap][2] — each may be null — = the first `returned` selected pairs, most extreme first,
    // (-1, -1, -1) behind them; positions are 0-based.  cls, side, thr and cap are checked by the caller, as is the labelled state (a
    // class other than "any" and out_ids need ids unless the gallery is empty).  Asynchronous; the scratch (counters by rank, the cut,
    // the slot counter, gallery_pairs_room(cap) candidates of 16 bytes) lives in the handle and its head is cleared on s at every call.
    void pairs_dev(int cls, int side, float thr, int cap, unsigned long long* info, float* out_score, int* out_rows, int* out_ids, hipStream_t s);
    // replaces every row's id by position (host or device list, checked by the caller: none negative); synchronous
    void set_ids(const int* ids, bool device_src);
    bool labelled() const { return ids_.live; }                  // meaningful while size() > 0; an empty gallery takes either kind
    long size() const { return n_; }
    int dim() const { return dim_; }
    // fh_gallery_set_scan: 1 = F16_RERANK (an fp16 copy of the rows beside the fp32 rows, G x dim x 2 bytes; same answer bit for bit),
    // 0 = FP32 (frees the copy).  Synchronous.
    void set_scan(int mode);
    int scan() const { return rows16_.live ? 1 : 0; }
    void scan_stats(long long* certified, long long* fallback);   // waits for the device; resets both
    // Watchlists (gallery_tags.hip): a 32-bit tag per row, a 32-bit mask per query (device [Q]); row r is admitted for query q iff
    // (tag[r] & mask[q]) != 0.  A gallery whose tags were never set (or not since the last upload) has none: it behaves as if every
    // row carried all ones, and the tag buffers come into being with the first set_tags or tagged query.  Arguments checked by the
    // caller except the ranges.  set_tags / get_tags: rows [first, first + n) by position; synchronous.
    void set_tags(long first, long n, const unsigned* tags, bool device_src);
    void get_tags(long first, long n, unsigned* out_host);
    void tag_stats(long long* scanned, long long* skipped);       // waits for the device; resets both

  private:
    // The row set: ONE capacity in rows and the per-row columns that share it.  A live column always holds cap_ rows; a dead one keeps
    // whatever buffer it had and is sized afresh when it comes to life (its contents are then the caller's to fill).
    struct Column {
        size_t row_bytes;
        bool live;
        DevBuf buf;
        template <class T> T* as() const { return buf.as<T>(); }
    };
    void set_live(Column& c, bool on);                           // on: cap_ rows (nothing kept)
    void reserve(long cap);                                      // every live column holds max(cap, cap_) rows, the first n_ kept
    long append(long n);                                         // room for n more rows (grows to max(need, 2 x capacity)); returns n_
    void compact(const int* map, long m);                        // row j <- row map[j] (device, ascending), j < m; capacity = m; synchronous
    void need_tags();                                            // the tags are live (first use: all ones) and their counters exist
    void rebuild_tile_or(long first, long n);                    // tile_or of the tiles rows [first, first + n) touch; synchronous
    void convert16(long first, long n);                          // rows [first, first + n) -> rows16_, bounds + flag (synchronous)
    void topk_f16(const float* q, int Q, int k, float* out_score, int* out_idx, hipStream_t s);
    // the ONE fp32 scan: pack the queries (q == nullptr: qpack_ is filled already), size the lists, launch, merge
    void scan_f32(const float* q, const unsigned* masks, int Q, int k, bool ids, float* out_score, int* out_id, int* out_row, hipStream_t s,
                  const int* qcount);
    void pack_queries(const float* q, int Q, hipStream_t s);     // qpack_ <- q as whole 64-row tiles, zero rows behind Q
    void need_labelled(const std::string& what) const;           // throws on a non-empty unlabelled gallery
    int dim_;
    long n_ = 0, cap_ = 0, base_ = 0;
    bool fused_ = false;
    Column rows_{(size_t)dim_ * sizeof(float), true}, rows16_{(size_t)dim_ * sizeof(uint16_t), false};   // fp32 rows; fp16 rows, live in F16_RERANK
    Column ids_{sizeof(int), false}, tags_{sizeof(unsigned), false};     // identity id per row, live while labelled; tag per row, live once set
    static constexpr int kCols = 4;
    Column* const cols_[kCols] = {&rows_, &rows16_, &ids_, &tags_};
    DevBuf tile_or_, tag_ctr_;                                   // follows the tags: their OR per 128-row tile; [2] visit counters
    DevBuf qpack_, ps_, pi_, pd_, best_i_, seed_s_, seed_i_, seed_d_;    // packed queries; part / seed lists of the fp32 scan (pd_, seed_d_: id planes)
    DevBuf cl_deg_, cl_parent_, cl_best_;                        // cluster_dev: degree, union-find parent, best core neighbour per row
    DevBuf cl_hist_;                                             // pair_hist_dev: the histogram the workgroups flush into
    DevBuf cl_pairs_;                                            // pairs_dev: counters by rank, cut, slot counter, candidates
    DevBuf rg_hits_, rg_units_;                                  // range_dev: hit bitmap [32-row block][query], hits per (8192 rows, query)
    DevBuf dp_bmax_, dp_bmax_t_, dp_chosen_, dp_cand_;           // topk_deep_dev: best eligible score [32-row block][query] and [query][block]; chosen blocks [query][k]; their rows' scores [query][k][32]
    // F16_RERANK state: [max|g|, max|g^|, max|g - g^| (float bits), non-finite / > 65504 flag] on the device and its host copy,
    // per-call scratch, the certified / fallback counters
    bool f16_bad_ = false;
    float gbound_[3] = {0.f, 0.f, 0.f};
    long long host_fallback_ = 0;
    DevBuf gstat_, q16_, ps16_, pi16_, seed16_s_, seed16_i_, cand_s_, cand_i_, fb_cnt_, fb_idx_, fb_s_, fb_i_, ctr_;
};

}  // namespace fh
