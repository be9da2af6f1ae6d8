// api.cpp — the extern "C" boundary declared in include/facehip.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/facehip.h"
#include "cluster_plan.h"
#include "deep_plan.h"
#include "pairs_plan.h"
#include "range_plan.h"
#include "roc_plan.h"
#include "engine.h"
#include "group_ids.h"
#include "jpeg_dev.h"
#include "jpeg_enc.h"
#include "track_plan.h"

static_assert(sizeof(fh_face) == 60 && sizeof(fh::FaceRec) == 60, "FaceBox mirror must stay 60 bytes");
static_assert(sizeof(fh_frame) == 24 && sizeof(fh::FrameIn) == 24 && offsetof(fh_frame, rows) == offsetof(fh::FrameIn, rows) &&
              offsetof(fh_frame, step) == offsetof(fh::FrameIn, step), "fh_frame and the engine's FrameIn are one layout");
static_assert(sizeof(fh_track_state) == sizeof(fh::TrackState) && offsetof(fh_track_state, hits) == offsetof(fh::TrackState, hits) &&
              FH_TRACK_MAX == 64, "fh_track_state mirrors TrackState; one slot per lane of a wave");
static_assert(sizeof(fh_track_ident) == 16 && sizeof(fh::TrackIdent) == 16 && offsetof(fh_track_ident, score) == offsetof(fh::TrackIdent, score),
              "fh_track_ident mirrors TrackIdent");
static_assert(sizeof(fh_track_link) == 32 && sizeof(fh::TrackLink) == 32 && offsetof(fh_track_link, last_seen) == offsetof(fh::TrackLink, last_seen) &&
              FH_TRACK_LINK_MEMORY == fh::kTrackLinkMemory, "fh_track_link mirrors TrackLink");
static_assert(FH_TRACK_POOL_LAST == fh::kTrackPoolLast && FH_TRACK_POOL_SUM == fh::kTrackPoolSum && FH_TRACK_POOL_WEIGHTED == fh::kTrackPoolWeighted,
              "fh_track_pool mirrors the pool kernel's modes");
static_assert(sizeof(fh_tiling) == sizeof(fh::Tiling) && offsetof(fh_tiling, border) == offsetof(fh::Tiling, border) &&
              sizeof(fh_view) == sizeof(fh::View) && offsetof(fh_view, edges) == offsetof(fh::View, edges) &&
              FH_TILE_MAX_VIEWS == fh::kTileMaxViews && FH_ERR_ARG == fh::kTilePlanBadArg, "fh_tiling / fh_view mirror tile_plan.h");

namespace {
thread_local std::string g_err;

// Which handles the running API call works on (set by the entry point before guarded(), cleared when it returns).  Each Net owns its
// stream-K watchdog record, so a hand-off time-out is reported by a call on the handle whose launch was abandoned: a call on another
// handle, or on none, neither sees nor consumes it.  (The single-kernel test entry points share the process-wide record: `shared`.)
struct CallOwners { const fh::Net* net[2] = {nullptr, nullptr}; bool shared = false; };
thread_local CallOwners t_owners;
struct Owns {
    explicit Owns(const fh::Net* a, const fh::Net* b = nullptr) { t_owners.net[0] = a; t_owners.net[1] = b; t_owners.shared = !a && !b; }
    ~Owns() { t_owners = CallOwners{}; }
    Owns(const Owns&) = delete;
    Owns& operator=(const Owns&) = delete;
};
template <class F>
int guarded(F&& f) {
    try {
        const int rc = f();
        // stream-K watchdog (conv_mfma.hip): a launch whose hand-off timed out has reported through its Net's host-mapped record by the
        // time a later call on that handle gets here (the synchronous entry points: in this very call, after their own stream sync)
        for (const fh::Net* n : t_owners.net)
            if (n && fh::conv_take_error(g_err, n->error_record())) return FH_ERR_DEVICE;
        if (t_owners.shared && fh::conv_take_error(g_err, fh::conv_error_words())) return FH_ERR_DEVICE;
        return rc;
    } catch (const std::exception& e) {
        g_err = e.what();
        const bool dev = g_err.rfind("HIP error", 0) == 0;
        return dev ? FH_ERR_DEVICE : (g_err.rfind("onnx", 0) == 0 || g_err.rfind("plan", 0) == 0) ? FH_ERR_MODEL : FH_ERR_STATE;
    } catch (...) {
        g_err = "unknown exception";
        return FH_ERR_STATE;
    }
}
int arg_error(const char* msg) { g_err = msg; return FH_ERR_ARG; }
// bytes a caller's row-strided image (cv::Mat data / step, a numpy column slice, a Mat ROI) really owns: the last row ends after
// cols*3 bytes, not after a whole pitch
size_t host_image_bytes(int rows, int cols, int step) { return (size_t)(rows - 1) * step + (size_t)cols * 3; }
hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
// the descriptor array of a ragged entry point: 1 <= n <= 4096, and a non-empty frame's pitch holds its row (empty frames — the
// reference's empty image, src/face_detector.cpp:148-156 — are legal: they yield nothing).  Null on success, else the complaint.
const char* bad_frames(const fh_frame* frames, int n) {
    if (!frames) return "null frame descriptors";
    if (n <= 0 || n > 4096) return "need 1 <= n <= 4096 frames";
    for (int i = 0; i < n; ++i) {
        const fh_frame& f = frames[i];
        if (f.bgr && f.rows > 0 && f.cols > 0 && (long long)f.step < (long long)f.cols * 3) return "a frame's step is smaller than cols * 3";
    }
    return nullptr;
}
int frames_error(const char* fn, const char* what) { g_err = std::string(fn) + ": " + what; return FH_ERR_ARG; }
const fh::FrameIn* FI(const fh_frame* f) { return reinterpret_cast<const fh::FrameIn*>(f); }
const fh::Tiling& TL(const fh_tiling* t) { return *reinterpret_cast<const fh::Tiling*>(t); }
// the view count of a tiled call (empty frames have none), or -1: a bad tiling or more than FH_TILE_MAX_VIEWS views.  Host arithmetic
// only — every tiled entry point asks this before it launches anything.
int tiled_view_total(const int* rows, const int* cols, const fh_frame* frames, int n, const fh_tiling* t) {
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (frames && !frames[i].bgr) continue;
        const int c = fh::tile_plan(frames ? frames[i].rows : rows[i], frames ? frames[i].cols : cols[i], &TL(t), nullptr, 0);
        if (c < 0) return -1;
        total += c;
        if (total > FH_TILE_MAX_VIEWS) return -1;
    }
    return (int)total;
}
const char* bad_tiling(const fh_tiling* t) {
    if (!t) return "null tiling";
    if (!fh::tiling_ok(&TL(t))) return "need tile_w, tile_h >= 16 and 0 <= overlap < min(tile_w, tile_h)";
    return nullptr;
}
}  // namespace

namespace fh {
void set_error(const std::string& msg) { g_err = msg; }      // for the other translation units of the C ABI
}

// ---------------------------------------------------------------------------------------------------------------------------
// Batch-1 host-pointer calls (fh_det_detect / fh_rec_extract / fh_rec_extract_simple = the reference's own mode: one image per
// call, src/face_detector.cpp:170, src/face_recognizer.cpp:270, callers src/main.cpp:88-104) are ~100 short kernels each: issued
// eagerly they are bound by the host's launch rate (~3.5 us per launch), not by the GPU.  The whole call — H2D of the image from a
// pinned staging buffer, every kernel, D2H of the results into a pinned landing buffer — is therefore captured ONCE per call shape
// into a HIP graph and replayed: one hipGraphLaunch + one stream synchronise per call.  The first call with a new shape runs
// eagerly (it sizes every device buffer: nothing may allocate during capture), the second captures, later ones replay.  Same
// kernels, same order, same arguments: results are bitwise those of the eager path (tests/test_gpu_round3.py).
struct PinnedBuf {
    void* p = nullptr; size_t bytes = 0;
    bool ensure(size_t n) {                                   // returns true when the buffer moved (a captured graph holds the old address)
        if (n <= bytes) return false;
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0;
        FH_HIP(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
        return true;
    }
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};
bool g_graph_replay = [] { const char* e = getenv("FACEHIP_GRAPH"); return !e || atoi(e) != 0; }();
struct GraphCall {
    hipGraph_t g = nullptr; hipGraphExec_t x = nullptr;
    std::vector<long long> key;
    int seen = 0;
    size_t nodes = 0;
    long replays = 0;
    void reset() {
        if (x) (void)hipGraphExecDestroy(x);
        if (g) (void)hipGraphDestroy(g);
        x = nullptr; g = nullptr; seen = 0; nodes = 0;
    }
    ~GraphCall() { reset(); }
    // body(stream) enqueues the whole call on `stream` (async copies + kernels, no host synchronisation, no allocation once warm)
    template <class F>
    void run(const std::vector<long long>& k, hipStream_t s, F&& body) {
        const bool allow = g_graph_replay && !fh::KernelTimer::get().enabled && !getenv("FACEHIP_DEBUG_SYNC");
        if (!allow) { reset(); key.clear(); body(s); return; }
        if (k != key) { reset(); key = k; }
        if (x) { FH_HIP(hipGraphLaunch(x, s)); ++replays; return; }
        if (seen++ == 0) { body(s); return; }
        FH_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
            body(s);
        } catch (...) {
            hipGraph_t dead = nullptr;
            (void)hipStreamEndCapture(s, &dead);
            if (dead) (void)hipGraphDestroy(dead);
            seen = 0;
            throw;
        }
        FH_HIP(hipStreamEndCapture(s, &g));
        FH_HIP(hipGraphInstantiate(&x, g, nullptr, nullptr, 0));
        (void)hipGraphGetNodes(g, nullptr, &nodes);
        FH_HIP(hipGraphLaunch(x, s));
        ++replays;
    }
};
struct CallStream {                                         // the handle's own stream for the host-pointer calls (capture needs a non-null stream)
    hipStream_t s = nullptr;
    hipStream_t get() { if (!s) FH_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return s; }
    ~CallStream() { if (s) (void)hipStreamDestroy(s); }
};
// What a captured call depends on beyond its own arguments: where every internal buffer lives (layout epoch), which kernels the
// handle's switches select (Net::config_word), the stream-K test hook's kernel arguments, and whether a hand-off time-out has been
// reported since (the eager path then re-zeroes the Net's counters — a replay would skip that).
static void graph_env_key(std::vector<long long>& key, const fh::Net& net) {
    key.push_back((long long)fh::layout_epoch());
    key.push_back(net.config_word());
    key.push_back((long long)fh::conv_error_generation() << 32 | fh::conv_debug_generation());
}
constexpr int kGraphFaces = 256;                            // records copied back inside the graph; a call with more fetches the rest eagerly

struct fh_det {
    explicit fh_det(const char* p) : det(p) {}
    fh::Detector det;
    fh::DevBuf img, out, cnt;            // staging for the host-pointer API
    PinnedBuf h_img, h_res;              // pinned source of the image upload / landing zone of [count | first kGraphFaces records]
    GraphCall gcall;                     // (declared after the buffers: destroyed first)
    CallStream cs;
    fh::DevBuf p_det, p_cnt, p_total;    // pipeline scratch
    hipEvent_t ev_sel = nullptr;         // detect -> embed hand-off (face count known / stream_rec may start)
    int* h_total = nullptr;              // pinned landing word of the face count
    PinnedBuf h_arena;                   // fh_pipeline_run_images: the live images packed row by row / their device copy / device results
    fh::DevBuf arena, i_faces, i_fo, i_emb;
    fh::DevBuf t_img, t_out;             // fh_det_detect_tiled: the image on the device / its records + count
    ~fh_det() { if (ev_sel) (void)hipEventDestroy(ev_sel); if (h_total) (void)hipHostFree(h_total); }
};
struct fh_rec {
    explicit fh_rec(const char* p) : rec(p) {}
    fh::Recognizer rec;
    fh::DevBuf img, face, emb;
    PinnedBuf h_img, h_io;               // pinned image source; [fh_face in | ok flag + embedding out]
    GraphCall gcall, gcall_simple;
    CallStream cs;
};
struct fh_gallery {
    explicit fh_gallery(int dim) : g(dim) {}
    fh::Gallery g;
};

extern "C" {

const char* fh_version(void) { return "facehip 0.1 (gfx950)"; }
const char* fh_last_error(void) { return g_err.c_str(); }

int fh_init(int device) {
    return guarded([&] {
        int n = 0;
        FH_HIP(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) throw std::runtime_error("HIP error: no such device");
        FH_HIP(hipSetDevice(device));
        return n;
    });
}

int fh_plan_describe(const char* onnx_path, int default_h, int default_w, char* buf, int cap) {
    if (!onnx_path || !buf || cap <= 0) return arg_error("fh_plan_describe: null argument");
    return guarded([&] {
        fh::OnnxModel m = fh::load_onnx(onnx_path);
        int H = default_h, W = default_w;
        const auto& shp = m.inputs[0].shape;
        if (shp.size() == 4) { if (shp[2] > 0) H = (int)shp[2]; if (shp[3] > 0) W = (int)shp[3]; }
        fh::Plan p = fh::build_plan(m, H, W);
        std::string s = p.describe();
        snprintf(buf, (size_t)cap, "%s", s.c_str());
        return (int)s.size();
    });
}

int fh_onnx_dump(const char* onnx_path, char* buf, int cap) {
    if (!onnx_path || !buf || cap <= 0) return arg_error("fh_onnx_dump: null argument");
    return guarded([&] {
        const fh::OnnxModel m = fh::load_onnx(onnx_path);
        std::string s;
        char tmp[256];
        auto dims = [&](const std::vector<int64_t>& d) { std::string o; for (size_t i = 0; i < d.size(); ++i) { o += (i ? "," : ""); o += std::to_string(d[i]); } return o; };
        for (const auto& v : m.inputs) s += "input " + v.name + " [" + dims(v.shape) + "]\n";
        for (const auto& v : m.outputs) s += "output " + v.name + " [" + dims(v.shape) + "]\n";
        for (const auto& kv : m.inits) {                                   // (std::map: sorted by name)
            const fh::OnnxTensor& t = kv.second;
            double sum = 0, first = 0, last = 0;
            size_t n = 0;
            if (!t.f.empty()) { n = t.f.size(); for (float x : t.f) sum += x; first = t.f.front(); last = t.f.back(); }
            else if (!t.i.empty()) { n = t.i.size(); for (int64_t x : t.i) sum += (double)x; first = (double)t.i.front(); last = (double)t.i.back(); }
            snprintf(tmp, sizeof tmp, " n=%zu sum=%.9g first=%.9g last=%.9g\n", n, sum, first, last);
            s += "init " + kv.first + " dtype=" + std::to_string(t.dtype) + " [" + dims(t.dims) + "]" + tmp;
        }
        for (const auto& nd : m.nodes) {
            s += "node " + nd.op + " in=";
            for (size_t i = 0; i < nd.inputs.size(); ++i) s += (i ? "," : "") + nd.inputs[i];
            s += " out=";
            for (size_t i = 0; i < nd.outputs.size(); ++i) s += (i ? "," : "") + nd.outputs[i];
            for (const auto& av : nd.attrs) {                               // (sorted by name)
                const fh::OnnxAttr& a = av.second;
                s += " " + av.first + "=";
                if (!a.ints.empty()) s += "ints:" + dims(a.ints);
                else if (!a.floats.empty()) { s += "floats:"; for (size_t i = 0; i < a.floats.size(); ++i) { snprintf(tmp, sizeof tmp, "%s%.9g", i ? "," : "", a.floats[i]); s += tmp; } }
                else if (!a.s.empty()) s += "s:" + a.s;
                else if (!a.t.dims.empty() || !a.t.f.empty() || !a.t.i.empty()) s += "t:[" + dims(a.t.dims) + "]";
                else if (a.f != 0.f) { snprintf(tmp, sizeof tmp, "f:%.9g", a.f); s += tmp; }
                else s += "i:" + std::to_string(a.i);
            }
            s += "\n";
        }
        snprintf(buf, (size_t)cap, "%s", s.c_str());
        return (int)std::min<size_t>(s.size(), (size_t)cap - 1);
    });
}

// ---------------------------------------------------------------------------------- detector
fh_det* fh_det_create(const char* onnx_path) {
    if (!onnx_path) { g_err = "fh_det_create: null path"; return nullptr; }
    fh_det* h = nullptr;
    int rc = guarded([&] { h = new fh_det(onnx_path); return 0; });
    return rc == 0 ? h : nullptr;
}
void fh_det_destroy(fh_det* d) { delete d; }
int fh_det_input_size(const fh_det* d, int* w, int* h) {
    if (!d) return arg_error("null handle");
    if (w) *w = const_cast<fh_det*>(d)->det.net().in_w();
    if (h) *h = const_cast<fh_det*>(d)->det.net().in_h();
    return FH_OK;
}
int fh_det_num_anchors(const fh_det* d) { return d ? d->det.num_anchors() : arg_error("null handle"); }
double fh_det_macs_per_frame(const fh_det* d) { return d ? const_cast<fh_det*>(d)->det.net().plan().macs : 0.0; }
double fh_det_act_bytes_per_frame(const fh_det* d) { return d ? const_cast<fh_det*>(d)->det.net().plan().act_bytes : 0.0; }

int fh_det_detect_batch_dev(fh_det* d, const uint8_t* frames, int n, int rows, int cols, int step, long long stride,
                            float score_thr, float nms_thr, fh_face* out, int max_pf, int* counts, void* stream) {
    if (!d || !frames || !out || !counts) return arg_error("fh_det_detect_batch_dev: null argument");
    if (n <= 0 || rows <= 0 || cols <= 0 || step < cols * 3 || max_pf <= 0) return arg_error("fh_det_detect_batch_dev: bad size");
    Owns owns(&d->det.net());
    return guarded([&] {
        d->det.detect_dev(frames, n, rows, cols, step, (long)stride, score_thr, nms_thr, reinterpret_cast<fh::FaceRec*>(out), max_pf,
                          counts, S(stream));
        return n;
    });
}

// ---------------------------------------------------------------------------------- mixed-size batches (detector side)
int fh_letterbox_plan(int rows, int cols, int in_w, int in_h, int* new_w, int* new_h, float* scale) {
    return fh::letterbox_plan(rows, cols, in_w, in_h, new_w, new_h, scale);              // src/face_detector.cpp:94-113
}
int fh_det_letterbox_ragged_dev(fh_det* d, const fh_frame* frames, int n, uint8_t* canvas, void* stream) {
    if (!d || !canvas) return arg_error("fh_det_letterbox_ragged_dev: null argument");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_det_letterbox_ragged_dev", bad);
    if (reinterpret_cast<uintptr_t>(canvas) & 3) return arg_error("fh_det_letterbox_ragged_dev: the canvas must be 4-byte aligned");
    Owns owns(&d->det.net());
    return guarded([&] { d->det.letterbox_ragged_dev(FI(frames), n, canvas, S(stream)); return n; });
}
int fh_det_run_network_ragged_dev(fh_det* d, const fh_frame* frames, int n, void* stream) {
    if (!d) return arg_error("fh_det_run_network_ragged_dev: null handle");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_det_run_network_ragged_dev", bad);
    Owns owns(&d->det.net());
    return guarded([&] { d->det.run_network_ragged_dev(FI(frames), n, S(stream)); return n; });
}
int fh_det_detect_ragged_dev(fh_det* d, const fh_frame* frames, int n, float score_thr, float nms_thr, fh_face* out, int max_pf,
                             int* counts, void* stream) {
    if (!d || !out || !counts) return arg_error("fh_det_detect_ragged_dev: null argument");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_det_detect_ragged_dev", bad);
    if (max_pf <= 0) return arg_error("fh_det_detect_ragged_dev: bad size");
    Owns owns(&d->det.net());
    return guarded([&] {
        d->det.detect_ragged_dev(FI(frames), n, score_thr, nms_thr, reinterpret_cast<fh::FaceRec*>(out), max_pf, counts, S(stream));
        return n;
    });
}

// ---------------------------------------------------------------------------------- tiled detection (detector side)
int fh_tile_plan(int rows, int cols, const fh_tiling* t, fh_view* views, int cap) {
    const int c = fh::tile_plan(rows, cols, reinterpret_cast<const fh::Tiling*>(t), reinterpret_cast<fh::View*>(views), cap);
    if (c < 0) g_err = "fh_tile_plan: bad tiling, or more views than cap";
    return c;
}
int fh_det_run_network_tiled_dev(fh_det* d, const fh_frame* frames, int n, const fh_tiling* t, void* stream) {
    if (!d) return arg_error("fh_det_run_network_tiled_dev: null handle");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_det_run_network_tiled_dev", bad);
    if (const char* bad = bad_tiling(t)) return frames_error("fh_det_run_network_tiled_dev", bad);
    if (tiled_view_total(nullptr, nullptr, frames, n, t) < 0) return arg_error("fh_det_run_network_tiled_dev: more than FH_TILE_MAX_VIEWS views");
    Owns owns(&d->det.net());
    return guarded([&] { return d->det.run_network_tiled_dev(FI(frames), n, TL(t), S(stream)); });
}
int fh_det_detect_tiled_dev(fh_det* d, const fh_frame* frames, int n, const fh_tiling* t, float score_thr, float nms_thr, fh_face* out,
                            int max_pf, int* counts, void* stream) {
    if (!d || !out || !counts) return arg_error("fh_det_detect_tiled_dev: null argument");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_det_detect_tiled_dev", bad);
    if (const char* bad = bad_tiling(t)) return frames_error("fh_det_detect_tiled_dev", bad);
    if (max_pf <= 0) return arg_error("fh_det_detect_tiled_dev: bad size");
    if (tiled_view_total(nullptr, nullptr, frames, n, t) < 0) return arg_error("fh_det_detect_tiled_dev: more than FH_TILE_MAX_VIEWS views");
    Owns owns(&d->det.net());
    return guarded([&] {
        d->det.detect_tiled_dev(FI(frames), n, TL(t), score_thr, nms_thr, reinterpret_cast<fh::FaceRec*>(out), max_pf, counts, S(stream));
        return n;
    });
}
// FaceDetector::detect on ONE host image, tiled: upload, fh_det_detect_tiled_dev with n = 1, fetch.  Blocking and eager.
int fh_det_detect_tiled(fh_det* d, const uint8_t* bgr, int rows, int cols, int step, const fh_tiling* t, float score_thr, float nms_thr,
                        fh_face* out, int max_out) {
    if (!d) return arg_error("Model not loaded!");                       // src/face_detector.cpp:142-145
    if (const char* bad = bad_tiling(t)) return frames_error("fh_det_detect_tiled", bad);
    if (!bgr || rows <= 0 || cols <= 0) return 0;                        // :148-156 -> empty result
    if (!out || max_out <= 0 || step < cols * 3) return arg_error("fh_det_detect_tiled: bad output buffer / step");
    const fh_frame host{bgr, rows, cols, step};
    if (tiled_view_total(nullptr, nullptr, &host, 1, t) < 0) return arg_error("fh_det_detect_tiled: more than FH_TILE_MAX_VIEWS views");
    Owns owns(&d->det.net());
    return guarded([&] {
        const size_t used = host_image_bytes(rows, cols, step);
        hipStream_t s = d->cs.get();
        FH_HIP(hipStreamSynchronize(s));
        d->t_img.ensure(used);
        d->t_out.ensure((size_t)max_out * sizeof(fh_face) + sizeof(int));
        int* const d_cnt = reinterpret_cast<int*>(d->t_out.as<fh_face>() + max_out);
        const fh_frame f{d->t_img.as<uint8_t>(), rows, cols, step};
        FH_HIP(hipMemcpyAsync(d->t_img.p, bgr, used, hipMemcpyHostToDevice, s));
        d->det.detect_tiled_dev(FI(&f), 1, TL(t), score_thr, nms_thr, d->t_out.as<fh::FaceRec>(), max_out, d_cnt, s);
        int c = 0;
        FH_HIP(hipMemcpyAsync(&c, d_cnt, sizeof(int), hipMemcpyDeviceToHost, s));
        FH_HIP(hipStreamSynchronize(s));
        c = c < max_out ? c : max_out;
        if (c > 0) FH_HIP(hipMemcpy(out, d->t_out.p, (size_t)c * sizeof(fh_face), hipMemcpyDeviceToHost));
        return c;
    });
}

int fh_det_detect(fh_det* d, const uint8_t* bgr, int rows, int cols, int step, float score_thr, float nms_thr, fh_face* out,
                  int max_out) {
    if (!d) return arg_error("Model not loaded!");                       // src/face_detector.cpp:142-145
    if (!bgr || rows <= 0 || cols <= 0) return 0;                        // :148-156 -> empty result
    if (!out || max_out <= 0 || step < cols * 3) return arg_error("fh_det_detect: bad output buffer / step");
    Owns owns(&d->det.net());
    return guarded([&] {
        const size_t bytes = (size_t)rows * step, used = host_image_bytes(rows, cols, step);
        const int in_graph = max_out < kGraphFaces ? max_out : kGraphFaces;
        d->img.ensure(bytes);
        d->out.ensure((size_t)max_out * sizeof(fh_face));
        d->cnt.ensure(sizeof(int));
        const bool m1 = d->h_img.ensure(bytes), m2 = d->h_res.ensure(64 + (size_t)kGraphFaces * sizeof(fh_face));
        const bool moved = m1 || m2;
        if (moved) d->gcall.reset();
        memcpy(d->h_img.p, bgr, used);                                        // pageable -> pinned (what hipMemcpy would do internally)
        hipStream_t s = d->cs.get();
        int* const h_cnt = static_cast<int*>(d->h_res.p);
        fh_face* const h_faces = reinterpret_cast<fh_face*>(static_cast<char*>(d->h_res.p) + 64);
        long long kthr, knms;
        { float f = score_thr; int v; memcpy(&v, &f, 4); kthr = v; f = nms_thr; memcpy(&v, &f, 4); knms = v; }
        std::vector<long long> key{rows, cols, step, kthr, knms, max_out, (long long)(size_t)d->img.p, (long long)(size_t)d->out.p};
        graph_env_key(key, d->det.net());
        try {
            d->gcall.run(key, s, [&](hipStream_t st) {
                FH_HIP(hipMemcpyAsync(d->img.p, d->h_img.p, used, hipMemcpyHostToDevice, st));
                d->det.detect_dev(d->img.as<uint8_t>(), 1, rows, cols, step, (long)bytes, score_thr, nms_thr, d->out.as<fh::FaceRec>(),
                                  max_out, d->cnt.as<int>(), st);
                FH_HIP(hipMemcpyAsync(h_cnt, d->cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
                FH_HIP(hipMemcpyAsync(h_faces, d->out.p, (size_t)in_graph * sizeof(fh_face), hipMemcpyDeviceToHost, st));
            });
        } catch (const std::runtime_error& e) {
            if (std::string(e.what()) == "Invalid resize dimensions") return 0;   // :109-113,164-167
            throw;
        }
        FH_HIP(hipStreamSynchronize(s));
        int c = *h_cnt;
        c = c < max_out ? c : max_out;
        const int first = c < in_graph ? c : in_graph;
        if (first > 0) memcpy(out, h_faces, (size_t)first * sizeof(fh_face));
        if (c > first)                                                        // rare: more faces than the graph's landing zone holds
            FH_HIP(hipMemcpy(out + first, d->out.as<fh_face>() + first, (size_t)(c - first) * sizeof(fh_face), hipMemcpyDeviceToHost));
        return c;
    });
}

int fh_det_sync(fh_det* d, void* stream) {
    if (!d) return arg_error("fh_det_sync: null handle");
    Owns owns(&d->det.net());
    return guarded([&] { FH_HIP(hipStreamSynchronize(S(stream))); return (int)FH_OK; });
}
int fh_det_run_network_dev(fh_det* d, const uint8_t* frames, int n, int rows, int cols, int step, long long stride, void* stream) {
    if (!d || !frames || n <= 0) return arg_error("fh_det_run_network_dev: bad argument");
    Owns owns(&d->det.net());
    return guarded([&] { d->det.run_network_dev(frames, n, rows, cols, step, (long)stride, S(stream)); return n; });
}
// Net::run_u8 on frames taken as they are — pasted at the net input's origin, no letterbox resize — for the stem tests
int fh_debug_det_run_pasted_dev(fh_det* d, const uint8_t* frames, int n, int rows, int cols, int step, long long stride, void* stream) {
    if (!d || !frames || n <= 0 || rows <= 0 || cols <= 0 || step < cols * 3 || rows > d->det.net().in_h() || cols > d->det.net().in_w())
        return arg_error("fh_debug_det_run_pasted_dev: bad argument (the frame must fit the net input)");
    Owns owns(&d->det.net());
    return guarded([&] { d->det.net().reserve(n); d->det.net().run_u8(frames, (long)stride, rows, cols, step, n, S(stream)); return n; });
}
int fh_det_run_input_dev(fh_det* d, const float* input, int n, void* stream) {
    if (!d || !input || n <= 0) return arg_error("fh_det_run_input_dev: bad argument");
    if (d->det.net().plan().tensors[d->det.net().plan().input].C != 4) return arg_error("fh_det_run_input_dev: the graph input is not a 3-channel image");
    Owns owns(&d->det.net());
    return guarded([&] { d->det.run_input_dev(input, n, S(stream)); return n; });
}
int fh_det_num_outputs(const fh_det* d) { return d ? (int)const_cast<fh_det*>(d)->det.net().plan().outputs.size() : arg_error("null handle"); }
const float* fh_det_output_dev(fh_det* d, int index, int* rows, int* cols) {
    if (!d || index < 0 || index >= (int)d->det.net().plan().outputs.size()) { g_err = "bad output index"; return nullptr; }
    const auto& o = d->det.net().plan().outputs[index];
    if (rows) *rows = o.rows;
    if (cols) *cols = o.cols;
    return d->det.net().capacity() > 0 ? d->det.net().output(index) : nullptr;
}
const float* fh_det_input_dev(fh_det* d) { return d && d->det.net().capacity() > 0 ? d->det.net().input() : nullptr; }
int fh_det_postprocess_dev(fh_det* d, int n, float score_thr, float nms_thr, fh_face* out, int max_pf, int* counts, void* stream) {
    if (!d || !out || !counts || n <= 0) return arg_error("fh_det_postprocess_dev: bad argument");
    Owns owns(&d->det.net());
    return guarded([&] { d->det.postprocess_dev(n, score_thr, nms_thr, reinterpret_cast<fh::FaceRec*>(out), max_pf, counts, S(stream)); return n; });
}

// Scratch of the two fh_postprocess_rows*_dev entry points: one set per calling thread, and a call on a DIFFERENT stream than the
// previous one first waits for that one's kernels (event), so overlapping calls cannot race on cand / keys / ws / count.  Heap-allocated
// and never destroyed: a static DevBuf's destructor would call hipFree after the HIP runtime has been torn down at process exit.
namespace {
struct RowsScratch {
    fh::DevBuf cand, keys, ws, count;
    fh::TilePlan plan;                                                     // (tiled calls only)
    fh::TileTable tab;
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    void begin(hipStream_t s) {
        if (!done) FH_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (used && last != s) FH_HIP(hipStreamWaitEvent(s, done, 0));
    }
    // threshold + NMS of V views of n frames, cap candidates per view, key_total keys in all; then the fence for the next call
    void run(fh::PostArgs a, int n, size_t key_total, const fh::TileTable* tb, float nms_thr, fh_face* out, int max_pf, int* counts,
             hipStream_t s) {
        cand.ensure((size_t)a.V * a.cap * sizeof(fh::FaceRec));
        keys.ensure(key_total * sizeof(unsigned long long));
        ws.ensure(key_total * sizeof(int));
        count.ensure((size_t)n * sizeof(int));
        a.cand = cand.as<fh::FaceRec>(); a.keys = keys.as<unsigned long long>(); a.count = count.as<int>();
        fh::postprocess_views(a, n, tb, nms_thr, ws.as<int>(), reinterpret_cast<fh::FaceRec*>(out), max_pf, counts, s);
        FH_HIP(hipEventRecord(done, s));
        last = s; used = true;
    }
    static RowsScratch& mine() {
        thread_local RowsScratch* p = new RowsScratch();
        return *p;
    }
};
// caller's rows [V][rows_per_view][feat] with the smallest power-of-two capacity (the in-place bitonic sort needs one)
fh::PostArgs rows_source(const float* rows, int V, int rows_per_view, int feat, float score_thr) {
    fh::PostArgs a{};
    a.rows = rows; a.n_rows = rows_per_view; a.feat = feat; a.V = V; a.thr = score_thr; a.border = -1;
    a.cap = 1;
    while (a.cap < rows_per_view) a.cap <<= 1;
    return a;
}
}  // namespace

// FaceDetector::postprocess + nms on caller-supplied pre-decoded rows (src/face_detector.cpp:224-338,356-384)
int fh_postprocess_rows_dev(const float* rows, int n, int rows_per_frame, int feat, float scale, float score_thr, float nms_thr,
                            fh_face* out, int max_pf, int* counts, void* stream) {
    if (!rows || !out || !counts) return arg_error("fh_postprocess_rows_dev: null argument");
    if (n <= 0 || rows_per_frame <= 0 || max_pf <= 0 || !(scale > 0.f)) return arg_error("fh_postprocess_rows_dev: bad size");
    if ((long)n * rows_per_frame >= (1L << 31) / 16) return arg_error("fh_postprocess_rows_dev: too many rows");
    return guarded([&] {
        hipStream_t s = S(stream);
        if (feat < 15) {                                                   // "Unexpected output shape format" :300-303,326-328 -> no boxes
            FH_HIP(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int), s));
            return n;
        }
        RowsScratch& sc = RowsScratch::mine();
        sc.begin(s);
        fh::PostArgs a = rows_source(rows, n, rows_per_frame, feat, score_thr);
        a.scale = scale;
        sc.run(a, n, (size_t)n * a.cap, nullptr, nms_thr, out, max_pf, counts, s);
        return n;
    });
}

// fh_postprocess_rows_dev on the rows of every view of tiled frames: the plan's view table + one NMS per frame
int fh_postprocess_rows_tiled_dev(const float* rows, const int* frame_rows, const int* frame_cols, int n, const fh_tiling* t, int in_w,
                                  int in_h, int rows_per_view, int feat, float score_thr, float nms_thr, fh_face* out, int max_pf,
                                  int* counts, void* stream) {
    if (!rows || !frame_rows || !frame_cols || !out || !counts) return arg_error("fh_postprocess_rows_tiled_dev: null argument");
    if (const char* bad = bad_tiling(t)) return frames_error("fh_postprocess_rows_tiled_dev", bad);
    if (n <= 0 || n > 4096 || in_w <= 0 || in_h <= 0 || rows_per_view <= 0 || max_pf <= 0) return arg_error("fh_postprocess_rows_tiled_dev: bad size");
    if (rows_per_view > (1 << 21)) return arg_error("fh_postprocess_rows_tiled_dev: too many rows per view");   // 2 * 256 * cap keys < 2^31
    if (tiled_view_total(frame_rows, frame_cols, nullptr, n, t) < 0) return arg_error("fh_postprocess_rows_tiled_dev: more than FH_TILE_MAX_VIEWS views");
    return guarded([&] {
        hipStream_t s = S(stream);
        if (feat < 15) {                                                   // "Unexpected output shape format" :300-303,326-328 -> no boxes
            FH_HIP(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int), s));
            return n;
        }
        RowsScratch& sc = RowsScratch::mine();
        sc.begin(s);
        fh::PostArgs a = rows_source(rows, 0, rows_per_view, feat, score_thr);
        static const uint8_t live = 0;                                     // (the planner only asks whether a frame HAS pixels)
        std::vector<fh::FrameIn> fr((size_t)n);
        for (int i = 0; i < n; ++i) fr[(size_t)i] = fh::FrameIn{&live, frame_rows[i], frame_cols[i], 0};
        a.V = sc.plan.plan(fr.data(), n, TL(t), in_w, in_h, a.cap, FH_TILE_MAX_VIEWS);
        if (a.V <= 0) {
            FH_HIP(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int), s));
            return n;
        }
        sc.tab.upload(sc.plan, s);
        a.border = t->border;
        sc.run(a, n, sc.plan.key_total, &sc.tab, nms_thr, out, max_pf, counts, s);
        return n;
    });
}

// ---------------------------------------------------------------------------------- recognizer
fh_rec* fh_rec_create(const char* onnx_path) {
    if (!onnx_path) { g_err = "fh_rec_create: null path"; return nullptr; }
    fh_rec* h = nullptr;
    int rc = guarded([&] { h = new fh_rec(onnx_path); return 0; });
    return rc == 0 ? h : nullptr;
}
void fh_rec_destroy(fh_rec* r) { delete r; }
int fh_rec_input_size(const fh_rec* r, int* w, int* h) {
    if (!r) return arg_error("null handle");
    if (w) *w = const_cast<fh_rec*>(r)->rec.net().in_w();
    if (h) *h = const_cast<fh_rec*>(r)->rec.net().in_h();
    return FH_OK;
}
int fh_rec_feature_dim(const fh_rec* r) { return r ? r->rec.dim() : arg_error("null handle"); }
double fh_rec_macs_per_face(const fh_rec* r) { return r ? const_cast<fh_rec*>(r)->rec.net().plan().macs : 0.0; }
double fh_rec_act_bytes_per_face(const fh_rec* r) { return r ? const_cast<fh_rec*>(r)->rec.net().plan().act_bytes : 0.0; }
int fh_rec_set_chunk(fh_rec* r, int n) {
    if (!r || n <= 0) return arg_error("fh_rec_set_chunk: bad argument");
    // the kernels index one pass's tensors with 32-bit element offsets: the largest per-face tensor times the chunk must stay < 2^31
    size_t biggest = 1;
    for (const auto& t : r->rec.net().plan().tensors) biggest = std::max(biggest, t.elems());
    const long limit = (long)(((1UL << 31) - 1) / biggest);
    if (n > limit) return arg_error("fh_rec_set_chunk: chunk too large for the 32-bit tensor offsets of one pass");
    r->rec.max_chunk = n;
    return FH_OK;
}
const float* fh_rec_input_dev(fh_rec* r) { return r && r->rec.net().capacity() > 0 ? r->rec.net().input() : nullptr; }

int fh_rec_embed_aligned_dev(fh_rec* r, const uint8_t* crops, int n, float* out, float* raw, void* stream) {
    if (!r || !crops || !out || n <= 0) return arg_error("fh_rec_embed_aligned_dev: bad argument");
    Owns owns(&r->rec.net());
    return guarded([&] { r->rec.embed_aligned_dev(crops, n, out, S(stream), raw); return n; });
}
int fh_rec_run_input_dev(fh_rec* r, const float* input, int n, float* out, float* raw, void* stream) {
    if (!r || !input || !out || n <= 0) return arg_error("fh_rec_run_input_dev: bad argument");
    if (r->rec.net().plan().tensors[r->rec.net().plan().input].C != 4) return arg_error("fh_rec_run_input_dev: the graph input is not a 3-channel image");
    Owns owns(&r->rec.net());
    return guarded([&] { r->rec.embed_input_dev(input, n, out, S(stream), raw); return n; });
}
int fh_rec_sync(fh_rec* r, void* stream) {
    if (!r) return arg_error("fh_rec_sync: null handle");
    Owns owns(&r->rec.net());
    return guarded([&] { FH_HIP(hipStreamSynchronize(S(stream))); return (int)FH_OK; });
}
int fh_rec_align_dev(fh_rec* r, const uint8_t* frames, int rows, int cols, int step, long long stride, const fh_face* faces,
                     const int* frame_of, int n, uint8_t* crops, int* ok, void* stream) {
    if (!r || !frames || !faces || !crops || !ok || n <= 0 || rows <= 0 || cols <= 0) return arg_error("fh_rec_align_dev: bad argument");
    Owns owns(&r->rec.net());
    return guarded([&] {
        r->rec.align_dev(frames, rows, cols, step, (long)stride, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, n, crops, ok, S(stream));
        return n;
    });
}
int fh_rec_embed_faces_dev(fh_rec* r, const uint8_t* frames, int rows, int cols, int step, long long stride, const fh_face* faces,
                           const int* frame_of, int n, float* out, int* ok, void* stream) {
    if (!r || !frames || !faces || !out || n <= 0 || rows <= 0 || cols <= 0) return arg_error("fh_rec_embed_faces_dev: bad argument");
    Owns owns(&r->rec.net());
    return guarded([&] {
        r->rec.embed_faces_dev(frames, rows, cols, step, (long)stride, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, n, out, ok, S(stream));
        return n;
    });
}

int fh_rec_align_ragged_dev(fh_rec* r, const fh_frame* frames, int n_frames, const fh_face* faces, const int* frame_of, int n,
                            uint8_t* crops, int* ok, void* stream) {
    if (!r || !faces || !crops || !ok) return arg_error("fh_rec_align_ragged_dev: null argument");
    if (const char* bad = bad_frames(frames, n_frames)) return frames_error("fh_rec_align_ragged_dev", bad);
    if (n <= 0 || (!frame_of && n > n_frames)) return arg_error("fh_rec_align_ragged_dev: bad size");
    Owns owns(&r->rec.net());
    return guarded([&] {
        r->rec.align_ragged_dev(FI(frames), n_frames, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, n, crops, ok, S(stream));
        return n;
    });
}
int fh_rec_embed_faces_ragged_dev(fh_rec* r, const fh_frame* frames, int n_frames, const fh_face* faces, const int* frame_of, int n,
                                  float* out, int* ok, void* stream) {
    if (!r || !faces || !out) return arg_error("fh_rec_embed_faces_ragged_dev: null argument");
    if (const char* bad = bad_frames(frames, n_frames)) return frames_error("fh_rec_embed_faces_ragged_dev", bad);
    if (n <= 0 || (!frame_of && n > n_frames)) return arg_error("fh_rec_embed_faces_ragged_dev: bad size");
    Owns owns(&r->rec.net());
    return guarded([&] {
        r->rec.embed_faces_ragged_dev(FI(frames), n_frames, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, n, out, ok, S(stream));
        return n;
    });
}

int fh_rec_extract(fh_rec* r, const uint8_t* bgr, int rows, int cols, int step, const fh_face* face, float* out, int out_cap) {
    if (!r) return arg_error("Model not loaded!");                        // src/face_recognizer.cpp:239-242
    if (!bgr || rows <= 0 || cols <= 0) return 0;                         // :245-248 -> empty vector
    if (!face || !out || step < cols * 3) return arg_error("fh_rec_extract: bad argument");
    if (out_cap < r->rec.dim()) return arg_error("fh_rec_extract: output buffer too small");
    Owns owns(&r->rec.net());
    return guarded([&] {
        const size_t bytes = (size_t)rows * step, used = host_image_bytes(rows, cols, step);
        const size_t dimb = (size_t)r->rec.dim() * sizeof(float);
        r->img.ensure(bytes);
        r->face.ensure(sizeof(fh_face) + sizeof(int));
        r->emb.ensure(dimb);
        const bool m1 = r->h_img.ensure(bytes), m2 = r->h_io.ensure(128 + dimb);
        const bool moved = m1 || m2;
        if (moved) { r->gcall.reset(); r->gcall_simple.reset(); }
        char* const io = static_cast<char*>(r->h_io.p);                     // [0,60) face in | [64,68) ok out | [128, ...) embedding out
        memcpy(r->h_img.p, bgr, used);
        memcpy(io, face, sizeof(fh_face));
        int* okp = reinterpret_cast<int*>(r->face.as<uint8_t>() + sizeof(fh_face));
        hipStream_t s = r->cs.get();
        std::vector<long long> key{rows, cols, step, (long long)(size_t)r->img.p, (long long)(size_t)r->emb.p, (long long)(size_t)r->face.p};
        graph_env_key(key, r->rec.net());
        r->gcall.run(key, s, [&](hipStream_t st) {
            FH_HIP(hipMemcpyAsync(r->img.p, r->h_img.p, used, hipMemcpyHostToDevice, st));
            FH_HIP(hipMemcpyAsync(r->face.p, io, sizeof(fh_face), hipMemcpyHostToDevice, st));
            r->rec.embed_faces_dev(r->img.as<uint8_t>(), rows, cols, step, (long)bytes, r->face.as<fh::FaceRec>(), nullptr, 1, r->emb.as<float>(), okp, st);
            FH_HIP(hipMemcpyAsync(io + 64, okp, sizeof(int), hipMemcpyDeviceToHost, st));
            FH_HIP(hipMemcpyAsync(io + 128, r->emb.p, dimb, hipMemcpyDeviceToHost, st));
        });
        FH_HIP(hipStreamSynchronize(s));
        if (!*reinterpret_cast<int*>(io + 64)) return 0;                    // "Face alignment failed!" :254-257
        memcpy(out, io + 128, dimb);
        return r->rec.dim();
    });
}

int fh_rec_extract_simple(fh_rec* r, const uint8_t* bgr, int rows, int cols, int step, float* out, int out_cap) {
    if (!r) return arg_error("Model not loaded!");
    if (!bgr || rows <= 0 || cols <= 0) return 0;
    if (!out || step < cols * 3) return arg_error("fh_rec_extract_simple: bad argument");
    if (out_cap < r->rec.dim()) return arg_error("fh_rec_extract_simple: output buffer too small");
    Owns owns(&r->rec.net());
    return guarded([&] {
        const size_t bytes = (size_t)rows * step, used = host_image_bytes(rows, cols, step);
        const size_t dimb = (size_t)r->rec.dim() * sizeof(float);
        r->img.ensure(bytes);
        r->emb.ensure(dimb);
        const bool m1 = r->h_img.ensure(bytes), m2 = r->h_io.ensure(128 + dimb);
        const bool moved = m1 || m2;
        if (moved) { r->gcall.reset(); r->gcall_simple.reset(); }
        char* const io = static_cast<char*>(r->h_io.p);
        memcpy(r->h_img.p, bgr, used);
        hipStream_t s = r->cs.get();
        std::vector<long long> key{rows, cols, step, (long long)(size_t)r->img.p, (long long)(size_t)r->emb.p};
        graph_env_key(key, r->rec.net());
        r->gcall_simple.run(key, s, [&](hipStream_t st) {
            FH_HIP(hipMemcpyAsync(r->img.p, r->h_img.p, used, hipMemcpyHostToDevice, st));
            r->rec.resize_embed_dev(r->img.as<uint8_t>(), 1, rows, cols, step, (long)bytes, r->emb.as<float>(), st);
            FH_HIP(hipMemcpyAsync(io + 128, r->emb.p, dimb, hipMemcpyDeviceToHost, st));
        });
        FH_HIP(hipStreamSynchronize(s));
        memcpy(out, io + 128, dimb);
        return r->rec.dim();
    });
}

// FaceRecognizer::compareFaces (src/face_recognizer.cpp:320-334) — 1 024 FLOP, stays on the host.
float fh_compare(const float* f1, int n1, const float* f2, int n2) {
    if (n1 != n2 || n1 <= 0 || !f1 || !f2) return 0.0f;
    float dot = 0.0f;
    for (int i = 0; i < n1; ++i) dot += f1[i] * f2[i];
    return (dot + 1.0f) / 2.0f;
}

// ---------------------------------------------------------------------------------- pipeline
namespace {
// detect + decode + NMS + face selection on stream sd, then the ONE host hand-off of the pipeline: the number of live faces
// (4 bytes through pinned memory, behind an event on sd).  Everything after it — align + embed — is sized by that count, so
// the recogniser never runs on empty slots (the reference embeds "for every face", src/main.cpp:221-238: 0..F per frame).
// (detect(out, max_per_frame, counts) runs the detector of the caller's kind — uniform or ragged — on sd)
int count_handoff(fh_det* d, const int* dt, hipStream_t sd) {
    FH_HIP(hipMemcpyAsync(d->h_total, dt, sizeof(int), hipMemcpyDeviceToHost, sd));
    FH_HIP(hipEventRecord(d->ev_sel, sd));
    FH_HIP(hipEventSynchronize(d->ev_sel));               // waits for the DETECTOR of this batch only; a recogniser queued earlier on another stream keeps running
    return *d->h_total;
}
extern "C++" template <class Detect>
int detect_select_count_with(fh_det* d, int n, int F, fh_face* faces, int* frame_of, int* d_total, hipStream_t sd, Detect&& detect) {
    d->p_det.ensure((size_t)n * F * sizeof(fh_face));
    d->p_cnt.ensure((size_t)n * sizeof(int));
    d->p_total.ensure(sizeof(int));
    if (!d->ev_sel) FH_HIP(hipEventCreateWithFlags(&d->ev_sel, hipEventDisableTiming));
    if (!d->h_total) FH_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->h_total), sizeof(int), hipHostMallocDefault));
    int* dt = d_total ? d_total : d->p_total.as<int>();
    detect(d->p_det.as<fh::FaceRec>(), F, d->p_cnt.as<int>());
    fh::launch_select_faces(d->p_det.as<fh::FaceRec>(), d->p_cnt.as<int>(), n, F, F, reinterpret_cast<fh::FaceRec*>(faces), frame_of, dt, sd);
    return count_handoff(d, dt, sd);
}
int detect_select_count(fh_det* d, const uint8_t* frames, int n, int rows, int cols, int step, long stride, float score_thr, float nms_thr,
                        int F, fh_face* faces, int* frame_of, int* d_total, hipStream_t sd) {
    return detect_select_count_with(d, n, F, faces, frame_of, d_total, sd, [&](fh::FaceRec* out, int max_pf, int* counts) {
        d->det.detect_dev(frames, n, rows, cols, step, stride, score_thr, nms_thr, out, max_pf, counts, sd);
    });
}
// fh_pipeline_run_ragged_dev's body (arguments checked by the caller): the detector builds the frame table once, the align reads it
int pipeline_ragged(fh_det* d, fh_rec* r, const fh_frame* frames, int n, float score_thr, float nms_thr, int F, fh_face* faces,
                    int* frame_of, float* emb, hipStream_t s) {
    const int total = detect_select_count_with(d, n, F, faces, frame_of, nullptr, s, [&](fh::FaceRec* out, int max_pf, int* counts) {
        d->det.detect_ragged_dev(FI(frames), n, score_thr, nms_thr, out, max_pf, counts, s);
    });
    r->rec.embed_faces_table_dev(d->det.frame_table().table(), n, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, total, emb, nullptr, s);
    return total;
}
}  // namespace

int fh_pipeline_run_dev(fh_det* d, fh_rec* r, const uint8_t* frames, int n, int rows, int cols, int step, long long stride,
                        float score_thr, float nms_thr, int F, fh_face* faces, int* frame_of, float* emb, void* stream) {
    if (!d || !r || !frames || !faces || !frame_of || !emb) return arg_error("fh_pipeline_run_dev: null argument");
    if (n <= 0 || n > 4096 || rows <= 0 || cols <= 0 || F <= 0) return arg_error("fh_pipeline_run_dev: bad size");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        hipStream_t s = S(stream);
        const int total = detect_select_count(d, frames, n, rows, cols, step, (long)stride, score_thr, nms_thr, F, faces, frame_of, nullptr, s);
        r->rec.embed_faces_dev(frames, rows, cols, step, (long)stride, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, total, emb, nullptr, s);
        return total;
    });
}

int fh_pipeline_run_ragged_dev(fh_det* d, fh_rec* r, const fh_frame* frames, int n, float score_thr, float nms_thr, int F, fh_face* faces,
                               int* frame_of, float* emb, void* stream) {
    if (!d || !r || !faces || !frame_of || !emb) return arg_error("fh_pipeline_run_ragged_dev: null argument");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_pipeline_run_ragged_dev", bad);
    if (F <= 0) return arg_error("fh_pipeline_run_ragged_dev: bad size");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] { return pipeline_ragged(d, r, frames, n, score_thr, nms_thr, F, faces, frame_of, emb, S(stream)); });
}

// fh_pipeline_run_ragged_dev over tiled detection: the faces are in FRAME coordinates, so the align reads the detector's table of the
// frames (the ragged table of that call holds the views)
int fh_pipeline_run_tiled_dev(fh_det* d, fh_rec* r, const fh_frame* frames, int n, const fh_tiling* t, float score_thr, float nms_thr, int F,
                              fh_face* faces, int* frame_of, float* emb, void* stream) {
    if (!d || !r || !faces || !frame_of || !emb) return arg_error("fh_pipeline_run_tiled_dev: null argument");
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_pipeline_run_tiled_dev", bad);
    if (const char* bad = bad_tiling(t)) return frames_error("fh_pipeline_run_tiled_dev", bad);
    if (F <= 0) return arg_error("fh_pipeline_run_tiled_dev: bad size");
    if (tiled_view_total(nullptr, nullptr, frames, n, t) < 0) return arg_error("fh_pipeline_run_tiled_dev: more than FH_TILE_MAX_VIEWS views");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        hipStream_t s = S(stream);
        const int total = detect_select_count_with(d, n, F, faces, frame_of, nullptr, s, [&](fh::FaceRec* out, int max_pf, int* counts) {
            d->det.detect_tiled_dev(FI(frames), n, TL(t), score_thr, nms_thr, out, max_pf, counts, s);
        });
        r->rec.embed_faces_table_dev(d->det.tiled_frame_table().table(), n, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, total, emb,
                                     nullptr, s);
        return total;
    });
}

// The per-file enrolment loop (src/main.cpp:42,88-104) as one blocking call on host images of any sizes.
int fh_pipeline_run_images(fh_det* d, fh_rec* r, const fh_frame* imgs, int n, float score_thr, float nms_thr, int F, fh_face* faces,
                           int* frame_of, float* emb, int cap) {
    if (!d || !r) return arg_error("fh_pipeline_run_images: null handle");
    if (const char* bad = bad_frames(imgs, n)) return frames_error("fh_pipeline_run_images", bad);
    if (F <= 0 || cap < 0) return arg_error("fh_pipeline_run_images: bad size");
    size_t bytes = 0;
    int live = 0;
    for (int i = 0; i < n; ++i)
        if (imgs[i].bgr && imgs[i].rows > 0 && imgs[i].cols > 0) { bytes += (size_t)imgs[i].rows * imgs[i].cols * 3; ++live; }
    if (live == 0) return 0;                                                  // only empty images: no faces (src/face_detector.cpp:148-156)
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        hipStream_t s = d->cs.get();
        FH_HIP(hipStreamSynchronize(s));                                      // (a failed earlier call may have left a copy from the arena queued)
        d->h_arena.ensure(bytes);
        d->arena.ensure(bytes);
        const int dim = r->rec.dim();
        d->i_faces.ensure((size_t)n * F * sizeof(fh_face));
        d->i_fo.ensure((size_t)n * F * sizeof(int));
        d->i_emb.ensure((size_t)n * F * dim * sizeof(float));
        std::vector<fh_frame> dev_frames((size_t)n);
        uint8_t* const h = static_cast<uint8_t*>(d->h_arena.p);
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            const fh_frame& f = imgs[i];
            fh_frame& o = dev_frames[(size_t)i];
            o = fh_frame{nullptr, 0, 0, 0};
            if (!(f.bgr && f.rows > 0 && f.cols > 0)) continue;
            const size_t row = (size_t)f.cols * 3;
            for (int y = 0; y < f.rows; ++y) memcpy(h + off + (size_t)y * row, f.bgr + (size_t)y * f.step, row);
            o.bgr = d->arena.as<uint8_t>() + off; o.rows = f.rows; o.cols = f.cols; o.step = (int32_t)row;
            off += (size_t)f.rows * row;
        }
        FH_HIP(hipMemcpyAsync(d->arena.p, h, bytes, hipMemcpyHostToDevice, s));
        const int total = pipeline_ragged(d, r, dev_frames.data(), n, score_thr, nms_thr, F, d->i_faces.as<fh_face>(), d->i_fo.as<int>(),
                                          d->i_emb.as<float>(), s);
        FH_HIP(hipStreamSynchronize(s));
        const int m = total < cap ? total : cap;
        if (m > 0) {
            if (faces) FH_HIP(hipMemcpy(faces, d->i_faces.p, (size_t)m * sizeof(fh_face), hipMemcpyDeviceToHost));
            if (frame_of) FH_HIP(hipMemcpy(frame_of, d->i_fo.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
            if (emb) FH_HIP(hipMemcpy(emb, d->i_emb.p, (size_t)m * dim * sizeof(float), hipMemcpyDeviceToHost));
        }
        return total;
    });
}

// ---------------------------------------------------------------------------------- JPEG: host entropy decode, device reconstruction
struct fh_jpegdec {
    fh::JpegDev dev;
    PinnedBuf h_arena;                   // fh_jpeg_decode_batch: [coefficients of every JPEG | pixels of every host-decoded file]
    fh::DevBuf d_arena, d_pix;           // its device copy / the reconstructed pictures, packed row by row
    hipEvent_t ev_copy = nullptr;        // behind the copy out of h_arena: the next call rewrites the arena only after it
    bool copy_pending = false;
    ~fh_jpegdec() { if (ev_copy) { if (copy_pending) (void)hipEventSynchronize(ev_copy); (void)hipEventDestroy(ev_copy); } }
};
namespace {
// fn(i) for every i in [0, n) on `threads` host threads (the caller's included), one index per task.  fn must not throw.
extern "C++" template <class F>
void for_each_file(int n, int threads, F&& fn) {
    if (threads <= 1) { for (int i = 0; i < n; ++i) fn(i); return; }
    std::atomic<int> next{0};
    auto work = [&] { for (int i; (i = next.fetch_add(1)) < n;) fn(i); };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    } catch (...) {                                                           // no more threads to be had: the ones that started finish the job
    }
    work();
    for (std::thread& t : pool) t.join();
}
// null, or why fh_jpeg_reconstruct_batch_dev refuses the call (fh_jpeg_desc_check's complaint is already in g_err then: "")
const char* bad_jpeg_batch(const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base, const fh_frame* out) {
    if (!descs || !d_coef || !coef_base || !out) return "null argument";
    if (n <= 0 || n > 4096) return "need 1 <= n <= 4096 images";
    if (reinterpret_cast<uintptr_t>(d_coef) & 1) return "d_coef must be 2-byte aligned";
    for (int i = 0; i < n; ++i) {
        if (!out[i].bgr) continue;
        if (fh_jpeg_desc_check(&descs[i]) != 0) return "";
        if (coef_base[i] < 0) return "a negative coef_base";
        if (out[i].rows != descs[i].rows || out[i].cols != descs[i].cols) return "an output frame's rows / cols differ from its descriptor's";
        if ((long long)out[i].step < (long long)out[i].cols * 3) return "an output frame's step is smaller than cols * 3";
    }
    return nullptr;
}
// fh_jpeg_decode_batch's body (arguments checked): returns the number of decoded images; status may be null
int jpeg_decode_batch(fh_jpegdec* dec, const fh_blob* files, int n, int threads, fh_frame* frames_out, int* status, hipStream_t s) {
    threads = threads <= 0 ? std::min(16, n) : std::min(threads, 16);
    struct File { int kind = -1; fh_jpeg_desc desc; size_t coef_off = 0, px_off = 0; unsigned char* px = nullptr; int rows = 0, cols = 0; };
    std::vector<File> f((size_t)n);                                           // kind: 0 JPEG, 1 decoded on the host, -1 not decodable
    bool any_other = false;
    for (int i = 0; i < n; ++i) {
        const fh_blob& b = files[i];
        if (!b.bytes || b.n == 0) continue;
        if (b.n >= 3 && b.bytes[0] == 0xFF && b.bytes[1] == 0xD8) { if (fh_jpeg_header(b.bytes, b.n, &f[(size_t)i].desc) == 0) f[(size_t)i].kind = 0; }
        else { f[(size_t)i].kind = 1; any_other = true; }
    }
    if (any_other)                                                            // their sizes are known only once they are decoded
        for_each_file(n, threads, [&](int i) {
            File& x = f[(size_t)i];
            if (x.kind == 1 && fh_image_decode(files[i].bytes, files[i].n, &x.px, &x.rows, &x.cols) != 0) x.kind = -1;
        });
    size_t coef_elems = 0, host_px = 0, dev_px = 0;
    for (File& x : f) {
        if (x.kind == 0) { x.coef_off = coef_elems; coef_elems += ((size_t)x.desc.coef_count + 63) & ~(size_t)63; dev_px += (size_t)x.desc.rows * x.desc.cols * 3; }
        if (x.kind == 1) { x.px_off = host_px; host_px += (size_t)x.rows * x.cols * 3; }
    }
    const size_t coef_bytes = coef_elems * sizeof(int16_t), arena_bytes = coef_bytes + host_px;
    if (dec->copy_pending) { FH_HIP(hipEventSynchronize(dec->ev_copy)); dec->copy_pending = false; }
    if (arena_bytes) { dec->h_arena.ensure(arena_bytes); dec->d_arena.ensure(arena_bytes); }
    if (dev_px) dec->d_pix.ensure(dev_px);
    uint8_t* const h = static_cast<uint8_t*>(dec->h_arena.p);
    for_each_file(n, threads, [&](int i) {
        File& x = f[(size_t)i];
        if (x.kind == 0) {
            const size_t cap = (size_t)x.desc.coef_count;
            if (fh_jpeg_entropy(files[i].bytes, files[i].n, &x.desc, reinterpret_cast<int16_t*>(h) + x.coef_off, cap) != 0) x.kind = -1;
        } else if (x.kind == 1) {
            memcpy(h + coef_bytes + x.px_off, x.px, (size_t)x.rows * x.cols * 3);
            fh_image_free(x.px);
            x.px = nullptr;
        }
    });
    std::vector<fh_jpeg_desc> descs;
    std::vector<long long> base;
    std::vector<fh_frame> out;
    size_t px_off = 0;
    int decoded = 0;
    for (int i = 0; i < n; ++i) {
        const File& x = f[(size_t)i];
        fh_frame& o = frames_out[i];
        o = fh_frame{nullptr, 0, 0, 0};
        if (status) status[i] = x.kind;
        if (x.kind == 0) {
            o = fh_frame{dec->d_pix.as<uint8_t>() + px_off, x.desc.rows, x.desc.cols, x.desc.cols * 3};
            px_off += (size_t)x.desc.rows * x.desc.cols * 3;
            descs.push_back(x.desc); base.push_back((long long)x.coef_off); out.push_back(o);
        } else if (x.kind == 1) {
            o = fh_frame{dec->d_arena.as<uint8_t>() + coef_bytes + x.px_off, x.rows, x.cols, x.cols * 3};
        }
        decoded += x.kind >= 0;
    }
    if (decoded == 0) return 0;
    if (!dec->ev_copy) FH_HIP(hipEventCreateWithFlags(&dec->ev_copy, hipEventDisableTiming));
    FH_HIP(hipMemcpyAsync(dec->d_arena.p, h, arena_bytes, hipMemcpyHostToDevice, s));
    FH_HIP(hipEventRecord(dec->ev_copy, s));
    dec->copy_pending = true;
    if (!descs.empty()) {
        if (const char* bad = bad_jpeg_batch(descs.data(), (int)descs.size(), dec->d_arena.as<int16_t>(), base.data(), out.data()))
            throw std::runtime_error(std::string("fh_jpeg_decode_batch: ") + (*bad ? bad : g_err.c_str()));
        dec->dev.reconstruct(descs.data(), (int)descs.size(), dec->d_arena.as<int16_t>(), base.data(), FI(out.data()), s);
    }
    return decoded;
}
}  // namespace

fh_jpegdec* fh_jpegdec_create(void) {
    fh_jpegdec* h = nullptr;
    const int rc = guarded([&] { h = new fh_jpegdec(); return 0; });
    return rc == 0 ? h : nullptr;
}
void fh_jpegdec_destroy(fh_jpegdec* dec) { delete dec; }

int fh_jpeg_reconstruct_batch_dev(fh_jpegdec* dec, const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base,
                                  const fh_frame* out_frames, void* stream) {
    if (!dec) return arg_error("fh_jpeg_reconstruct_batch_dev: null handle");
    if (const char* bad = bad_jpeg_batch(descs, n, d_coef, coef_base, out_frames)) {
        if (*bad) g_err = std::string("fh_jpeg_reconstruct_batch_dev: ") + bad;
        return FH_ERR_ARG;
    }
    return guarded([&] { dec->dev.reconstruct(descs, n, d_coef, coef_base, FI(out_frames), S(stream)); return n; });
}

int fh_jpeg_decode_batch(fh_jpegdec* dec, const fh_blob* files, int n, int threads, fh_frame* frames_out, int* status, void* stream) {
    if (!dec || !files || !frames_out) return arg_error("fh_jpeg_decode_batch: null argument");
    if (n <= 0 || n > 4096) return arg_error("fh_jpeg_decode_batch: need 1 <= n <= 4096 files");
    return guarded([&] { return jpeg_decode_batch(dec, files, n, threads, frames_out, status, S(stream)); });
}

// fh_pipeline_run_images from file bytes: the decode above, then the ragged pipeline on the same stream.
int fh_pipeline_run_files(fh_det* d, fh_rec* r, fh_jpegdec* dec, const fh_blob* files, int n, int threads, float score_thr, float nms_thr, int F,
                          fh_face* faces, int* frame_of, float* emb, int cap, int* status) {
    if (!d || !r || !dec) return arg_error("fh_pipeline_run_files: null handle");
    if (!files) return arg_error("fh_pipeline_run_files: null files");
    if (n <= 0 || n > 4096) return arg_error("fh_pipeline_run_files: need 1 <= n <= 4096 files");
    if (F <= 0 || cap < 0) return arg_error("fh_pipeline_run_files: bad size");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        hipStream_t s = d->cs.get();
        FH_HIP(hipStreamSynchronize(s));
        std::vector<fh_frame> frames((size_t)n);
        if (jpeg_decode_batch(dec, files, n, threads, frames.data(), status, s) == 0) return 0;   // only empty images: no faces
        const int dim = r->rec.dim();
        d->i_faces.ensure((size_t)n * F * sizeof(fh_face));
        d->i_fo.ensure((size_t)n * F * sizeof(int));
        d->i_emb.ensure((size_t)n * F * dim * sizeof(float));
        const int total = pipeline_ragged(d, r, frames.data(), n, score_thr, nms_thr, F, d->i_faces.as<fh_face>(), d->i_fo.as<int>(),
                                          d->i_emb.as<float>(), s);
        FH_HIP(hipStreamSynchronize(s));
        const int m = total < cap ? total : cap;
        if (m > 0) {
            if (faces) FH_HIP(hipMemcpy(faces, d->i_faces.p, (size_t)m * sizeof(fh_face), hipMemcpyDeviceToHost));
            if (frame_of) FH_HIP(hipMemcpy(frame_of, d->i_fo.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
            if (emb) FH_HIP(hipMemcpy(emb, d->i_emb.p, (size_t)m * dim * sizeof(float), hipMemcpyDeviceToHost));
        }
        return total;
    });
}

// ---------------------------------------------------------------------------------- JPEG out: device forward path, host Huffman coding
struct fh_jpegenc {
    fh::JpegEnc dev;
    fh::DevBuf d_coef;                   // fh_jpeg_encode_batch: the coefficients of every frame ...
    PinnedBuf h_coef;                    // ... and where the one device-to-host copy lands
    std::vector<unsigned char> bytes[16];   // the byte arena: per host thread, the files it wrote, back to back
    fh::JpegHuff huff;                   // fh_jpeg_code_batch_dev: the device coder and its device byte arena
    PinnedBuf h_files;                   // fh_jpeg_encode_batch_gpu: where the one copy of that arena lands
};
namespace {
// null, or why fh_jpeg_forward_batch_dev refuses the call (fh_jpeg_enc_check's complaint is already in g_err then: "")
const char* bad_enc_batch(const fh_jpeg_desc* descs, int n, const fh_frame* frames, const int16_t* d_coef, const long long* coef_base) {
    if (!descs || !d_coef || !coef_base || !frames) return "null argument";
    if (n <= 0 || n > 4096) return "need 1 <= n <= 4096 images";
    if (reinterpret_cast<uintptr_t>(d_coef) & 1) return "d_coef must be 2-byte aligned";
    for (int i = 0; i < n; ++i) {
        if (!frames[i].bgr) continue;
        if (fh_jpeg_enc_check(&descs[i]) != 0) return "";
        if (coef_base[i] < 0) return "a negative coef_base";
        if (frames[i].rows != descs[i].rows || frames[i].cols != descs[i].cols) return "a frame's rows / cols differ from its descriptor's";
        if ((long long)frames[i].step < (long long)frames[i].cols * 3) return "a frame's step is smaller than cols * 3";
    }
    return nullptr;
}
// null, or why fh_jpeg_code_batch_dev refuses the call (as bad_enc_batch; a live slot is one with coef_base[i] >= 0)
const char* bad_code_batch(const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base, const fh_blob* files) {
    if (!descs || !d_coef || !coef_base || !files) return "null argument";
    if (n <= 0 || n > 4096) return "need 1 <= n <= 4096 images";
    if (reinterpret_cast<uintptr_t>(d_coef) & 1) return "d_coef must be 2-byte aligned";
    size_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (coef_base[i] < 0) continue;
        if (fh_jpeg_enc_check(&descs[i]) != 0) return "";
        blocks += (fh_jpeg_write_bound(&descs[i]) - 1024) / 416;              // the bound is 1024 + 416 bytes a block
    }
    if (blocks >= ((size_t)1 << 31)) return "the batch has 2^31 blocks or more: the coder's block indices are 31-bit";
    return nullptr;
}
// null, or why fh_jpeg_encode_batch / _gpu refuse the call
const char* bad_encode_frames(const fh_jpegenc* enc, const fh_frame* frames, int n, int subsampling, const fh_blob* files_out) {
    if (!enc || !frames || !files_out) return "null argument";
    if (n <= 0 || n > 4096) return "need 1 <= n <= 4096 frames";
    if (subsampling < 0 || subsampling > 2) return "subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)";
    for (int i = 0; i < n; ++i) {
        const fh_frame& f = frames[i];
        if (!(f.bgr && f.rows > 0 && f.cols > 0)) continue;
        if (f.rows > 65535 || f.cols > 65535) return "a frame is larger than 65535 in one direction";
        if ((long long)f.step < (long long)f.cols * 3) return "a frame's step is smaller than cols * 3";
    }
    return nullptr;
}
// the descriptors of fh_jpeg_encode_batch / _gpu: one per live frame, the images' coefficients back to back; order = the live frames
void encode_descs(const fh_frame* frames, int n, int quality, int subsampling, std::vector<fh_jpeg_desc>& descs, std::vector<long long>& base,
                  std::vector<fh_frame>& live, size_t& coef_elems, std::vector<int>& order) {
    coef_elems = 0;
    for (int i = 0; i < n; ++i) {
        live[(size_t)i] = frames[i];
        if (!(frames[i].bgr && frames[i].rows > 0 && frames[i].cols > 0)) { live[(size_t)i] = fh_frame{nullptr, 0, 0, 0}; continue; }
        if (fh_jpeg_enc_desc(frames[i].cols, frames[i].rows, 0, subsampling, quality, &descs[(size_t)i]) != 0) throw std::runtime_error(g_err);
        base[(size_t)i] = (long long)coef_elems;
        coef_elems += (size_t)descs[(size_t)i].coef_count;                    // a multiple of 64: every image starts 128-byte aligned
        order.push_back(i);
    }
}
// fh_jpeg_encode_batch_gpu's body (arguments checked): returns the number of files written
int jpeg_encode_batch_gpu(fh_jpegenc* enc, const fh_frame* frames, int n, int quality, int subsampling, fh_blob* files_out, hipStream_t s) {
    std::vector<fh_jpeg_desc> descs((size_t)n);
    std::vector<long long> base((size_t)n, -1);                               // -1: the coder's mark of a skipped slot
    std::vector<fh_frame> live((size_t)n);
    size_t coef_elems = 0;
    for (int i = 0; i < n; ++i) files_out[i] = fh_blob{nullptr, 0};
    std::vector<int> order;
    encode_descs(frames, n, quality, subsampling, descs, base, live, coef_elems, order);
    if (order.empty()) return 0;
    enc->d_coef.ensure(coef_elems * sizeof(int16_t));
    enc->dev.forward(descs.data(), n, FI(live.data()), enc->d_coef.as<int16_t>(), base.data(), s);
    if (const char* bad = bad_code_batch(descs.data(), n, enc->d_coef.as<int16_t>(), base.data(), files_out))
        throw std::runtime_error(std::string("fh_jpeg_encode_batch_gpu: ") + (*bad ? bad : g_err.c_str()));
    std::vector<fh_blob> dev_files((size_t)n);
    std::vector<int> status((size_t)n);
    const int m = enc->huff.code(descs.data(), n, enc->d_coef.as<int16_t>(), base.data(), dev_files.data(), status.data(), s);
    for (int i = 0; i < n; ++i)
        if (status[(size_t)i] < 0) throw std::runtime_error("fh_jpeg_encode_batch_gpu: coefficients without a baseline code");   // (no forward path makes them)
    const size_t bytes = enc->huff.arena_used();
    enc->h_files.ensure(bytes);
    FH_HIP(hipMemcpyAsync(enc->h_files.p, enc->huff.arena().p, bytes, hipMemcpyDeviceToHost, s));
    FH_HIP(hipStreamSynchronize(s));
    const unsigned char* const d0 = enc->huff.arena().as<unsigned char>();
    for (int i = 0; i < n; ++i)
        if (dev_files[(size_t)i].bytes) files_out[i] = fh_blob{static_cast<unsigned char*>(enc->h_files.p) + (dev_files[(size_t)i].bytes - d0), dev_files[(size_t)i].n};
    return m;
}
// fh_jpeg_encode_batch's body (arguments checked): returns the number of files written
int jpeg_encode_batch(fh_jpegenc* enc, const fh_frame* frames, int n, int quality, int subsampling, int threads, fh_blob* files_out, hipStream_t s) {
    threads = threads <= 0 ? std::min(16, n) : std::min(threads, 16);
    std::vector<fh_jpeg_desc> descs((size_t)n);
    std::vector<long long> base((size_t)n, 0);
    std::vector<fh_frame> live((size_t)n);
    size_t coef_elems = 0;
    for (int i = 0; i < n; ++i) files_out[i] = fh_blob{nullptr, 0};
    std::vector<int> order;                                                   // the live frames
    encode_descs(frames, n, quality, subsampling, descs, base, live, coef_elems, order);
    if (order.empty()) return 0;
    enc->d_coef.ensure(coef_elems * sizeof(int16_t));
    enc->h_coef.ensure(coef_elems * sizeof(int16_t));
    enc->dev.forward(descs.data(), n, FI(live.data()), enc->d_coef.as<int16_t>(), base.data(), s);
    FH_HIP(hipMemcpyAsync(enc->h_coef.p, enc->d_coef.p, coef_elems * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    FH_HIP(hipStreamSynchronize(s));
    // one file per task; a thread appends its files to its own buffer (which may move as it grows: offsets now, pointers after the join)
    struct Where { int thread = -1; size_t off = 0, size = 0; };
    std::vector<Where> where((size_t)n);
    const int16_t* const coef = static_cast<const int16_t*>(enc->h_coef.p);
    const int m = (int)order.size();
    std::atomic<int> next{0};
    std::atomic<bool> failed{false};
    auto work = [&](int t) {
        std::vector<unsigned char>& buf = enc->bytes[t];
        size_t used = 0;
        for (int k; (k = next.fetch_add(1)) < m;) {
            const int i = order[(size_t)k];
            const size_t bound = fh_jpeg_write_bound(&descs[(size_t)i]);
            size_t written = 0;
            try {
                if (buf.size() < used + bound) buf.resize(std::max(used + bound, buf.size() * 2));
            } catch (...) { failed = true; continue; }
            if (fh_jpeg_write(&descs[(size_t)i], coef + base[(size_t)i], buf.data() + used, bound, &written) != 0) { failed = true; continue; }
            where[(size_t)i] = Where{t, used, written};
            used += written;
        }
    };
    {
        std::vector<std::thread> pool;
        try {
            for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
        } catch (...) {                                                       // no more threads to be had: the ones that started finish the job
        }
        work(0);
        for (std::thread& t : pool) t.join();
    }
    if (failed) throw std::runtime_error("fh_jpeg_encode_batch: a file could not be written (out of memory, or coefficients without a baseline code)");
    for (int i : order) files_out[i] = fh_blob{enc->bytes[where[(size_t)i].thread].data() + where[(size_t)i].off, where[(size_t)i].size};
    return m;
}
}  // namespace

fh_jpegenc* fh_jpegenc_create(void) {
    fh_jpegenc* h = nullptr;
    const int rc = guarded([&] { h = new fh_jpegenc(); return 0; });
    return rc == 0 ? h : nullptr;
}
void fh_jpegenc_destroy(fh_jpegenc* enc) { delete enc; }

int fh_jpeg_forward_batch_dev(fh_jpegenc* enc, const fh_jpeg_desc* descs, int n, const fh_frame* frames, int16_t* d_coef, const long long* coef_base,
                              void* stream) {
    if (!enc) return arg_error("fh_jpeg_forward_batch_dev: null handle");
    if (const char* bad = bad_enc_batch(descs, n, frames, d_coef, coef_base)) {
        if (*bad) g_err = std::string("fh_jpeg_forward_batch_dev: ") + bad;
        return FH_ERR_ARG;
    }
    return guarded([&] { enc->dev.forward(descs, n, FI(frames), d_coef, coef_base, S(stream)); return n; });
}

int fh_jpeg_encode_batch(fh_jpegenc* enc, const fh_frame* frames, int n, int quality, int subsampling, int threads, fh_blob* files_out,
                         void* stream) {
    if (const char* bad = bad_encode_frames(enc, frames, n, subsampling, files_out)) { g_err = std::string("fh_jpeg_encode_batch: ") + bad; return FH_ERR_ARG; }
    return guarded([&] { return jpeg_encode_batch(enc, frames, n, quality, subsampling, threads, files_out, S(stream)); });
}

int fh_jpeg_code_batch_dev(fh_jpegenc* enc, const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base,
                           fh_blob* files_dev_out, int* status, void* stream) {
    if (!enc) return arg_error("fh_jpeg_code_batch_dev: null handle");
    if (const char* bad = bad_code_batch(descs, n, d_coef, coef_base, files_dev_out)) {
        if (*bad) g_err = std::string("fh_jpeg_code_batch_dev: ") + bad;
        return FH_ERR_ARG;
    }
    return guarded([&] { return enc->huff.code(descs, n, d_coef, coef_base, files_dev_out, status, S(stream)); });
}

int fh_jpeg_encode_batch_gpu(fh_jpegenc* enc, const fh_frame* frames, int n, int quality, int subsampling, fh_blob* files_out, void* stream) {
    if (const char* bad = bad_encode_frames(enc, frames, n, subsampling, files_out)) { g_err = std::string("fh_jpeg_encode_batch_gpu: ") + bad; return FH_ERR_ARG; }
    return guarded([&] { return jpeg_encode_batch_gpu(enc, frames, n, quality, subsampling, files_out, S(stream)); });
}

int fh_jpeg_stuff_chunk(void) { return FH_JPEG_STUFF_CHUNK; }

int fh_debug_jpeg_arena(fh_jpegenc* enc, int fill, void** dev, size_t* bytes) {
    if (!enc || !dev || !bytes) return arg_error("fh_debug_jpeg_arena: null argument");
    *dev = enc->huff.arena().p; *bytes = enc->huff.arena().bytes;
    if (fill < 0 || !*bytes) return 0;
    return guarded([&] { FH_HIP(hipDeviceSynchronize()); FH_HIP(hipMemset(*dev, fill & 255, *bytes)); FH_HIP(hipDeviceSynchronize()); return 0; });
}

long long fh_debug_jpeg_scan_bits(fh_jpegenc* enc, uint32_t* bits, size_t cap) {
    if (!enc || (!bits && cap)) return arg_error("fh_debug_jpeg_scan_bits: null argument");
    const long long B = enc->huff.blocks();
    if ((unsigned long long)B > cap) return arg_error("fh_debug_jpeg_scan_bits: the output holds fewer entries than the last call had blocks");
    const int rc = guarded([&] { if (B) FH_HIP(hipMemcpy(bits, enc->huff.bits().p, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost)); return 0; });
    return rc < 0 ? rc : B;
}

// Two-stream form for streaming callers: detect (+ decode + NMS + face selection) on stream_det, align + embed on stream_rec
// behind an event.  The host waits for the detector's face count only, so with batch k+1 submitted straight after batch k the
// HBM-bound detector of k+1 runs beside the MFMA-bound recogniser of k.
int fh_pipeline_submit_dev(fh_det* d, fh_rec* r, const uint8_t* frames, int n, int rows, int cols, int step, long long stride,
                           float score_thr, float nms_thr, int F, fh_face* faces, int* frame_of, float* emb, int* d_total,
                           void* stream_det, void* stream_rec) {
    if (!d || !r || !frames || !faces || !frame_of || !emb || !d_total) return arg_error("fh_pipeline_submit_dev: null argument");
    if (n <= 0 || n > 4096 || rows <= 0 || cols <= 0 || F <= 0) return arg_error("fh_pipeline_submit_dev: bad size");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        hipStream_t sd = S(stream_det), sr = S(stream_rec);
        const int total = detect_select_count(d, frames, n, rows, cols, step, (long)stride, score_thr, nms_thr, F, faces, frame_of, d_total, sd);
        if (sd != sr) FH_HIP(hipStreamWaitEvent(sr, d->ev_sel, 0));
        r->rec.embed_faces_dev(frames, rows, cols, step, (long)stride, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, total, emb, nullptr, sr);
        return total;
    });
}

// ---------------------------------------------------------------------------------- face tracker
struct fh_tracker {
    fh_tracker(int streams, int max_tracks, float iou_thr, int max_missed, int refresh) : t(streams, max_tracks, iou_thr, max_missed, refresh) {}
    fh::Tracker t;
};
namespace {
// the batch of a tracker call: 1 <= n <= 4096, per_frame >= 1, every stream index inside the tracker.  Null on success.
const char* bad_track_batch(const fh_tracker* t, int n, int per_frame, const int* stream_of) {
    if (n < 1 || n > fh::kTrackMaxFrames) return "need 1 <= n <= 4096 frames";
    if (per_frame < 1) return "need per_frame >= 1";
    if (stream_of)
        for (int f = 0; f < n; ++f)
            if (stream_of[f] < 0 || stream_of[f] >= t->t.streams()) return "a stream_of entry is outside [0, streams)";
    return nullptr;
}
}  // namespace

fh_tracker* fh_tracker_create(int streams, int max_tracks, float iou_thr, int max_missed, int refresh) {
    if (streams < 1 || streams > fh::kTrackMaxStreams || max_tracks < 1 || max_tracks > FH_TRACK_MAX || max_missed < 0 || refresh < 0) {
        g_err = "fh_tracker_create: need 1 <= streams <= 4096, 1 <= max_tracks <= FH_TRACK_MAX, max_missed >= 0, refresh >= 0";
        return nullptr;
    }
    fh_tracker* h = nullptr;
    const int rc = guarded([&] { h = new fh_tracker(streams, max_tracks, iou_thr, max_missed, refresh); return 0; });
    return rc == 0 ? h : nullptr;
}
void fh_tracker_destroy(fh_tracker* t) { delete t; }
int fh_tracker_reset(fh_tracker* t, int stream) {
    if (!t) return arg_error("fh_tracker_reset: null handle");
    if (stream < -1 || stream >= t->t.streams()) return arg_error("fh_tracker_reset: no such stream");
    return guarded([&] { t->t.reset(stream); return 0; });
}
int fh_tracker_get_state(fh_tracker* t, int stream, fh_track_state* out, int* frame_no, int* next_id) {
    if (!t) return arg_error("fh_tracker_get_state: null handle");
    if (stream < 0 || stream >= t->t.streams()) return arg_error("fh_tracker_get_state: no such stream");
    return guarded([&] { return t->t.get_state(stream, reinterpret_cast<fh::TrackState*>(out), frame_no, next_id); });
}
int fh_track_plan(const int* stream_of, int n, int streams, int* order, int* starts) {
    if (!order || !starts) return arg_error("fh_track_plan: null argument");
    if (fh::track_plan(stream_of, n, streams, order, starts) != 0)
        return arg_error("fh_track_plan: need 1 <= n <= 4096, 1 <= streams <= 4096 and every stream index in [0, streams)");
    return 0;
}
int fh_track_update_q_dev(fh_tracker* t, const fh_face* det, const int* counts, int n, int per_frame, const int* stream_of, int* track,
                          int* embed, int* slot, const int* quality, void* stream) {
    const char* const fn = quality ? "fh_track_update_q_dev" : slot ? "fh_track_update_slots_dev" : "fh_track_update_dev";
    if (!t || !det || !counts || !track || !embed) return frames_error(fn, "null argument");
    if (const char* bad = bad_track_batch(t, n, per_frame, stream_of)) return frames_error(fn, bad);
    return guarded([&] {
        t->t.update_dev(reinterpret_cast<const fh::FaceRec*>(det), counts, n, per_frame, stream_of, track, embed, slot, quality, S(stream));
        return n;
    });
}
int fh_track_update_slots_dev(fh_tracker* t, const fh_face* det, const int* counts, int n, int per_frame, const int* stream_of, int* track,
                              int* embed, int* slot, void* stream) {
    return fh_track_update_q_dev(t, det, counts, n, per_frame, stream_of, track, embed, slot, nullptr, stream);
}
int fh_track_update_dev(fh_tracker* t, const fh_face* det, const int* counts, int n, int per_frame, const int* stream_of, int* track,
                        int* embed, void* stream) {
    return fh_track_update_slots_dev(t, det, counts, n, per_frame, stream_of, track, embed, nullptr, stream);
}
int fh_track_select_dev(const fh_face* det, const int* embed, int n, int per_frame, fh_face* faces, int* frame_of, const int* track,
                        int* track_of, int* total, void* stream) {
    if (!det || !embed || !faces || !frame_of || !track || !track_of || !total) return arg_error("fh_track_select_dev: null argument");
    if (n < 1 || n > fh::kTrackMaxFrames || per_frame < 1) return arg_error("fh_track_select_dev: need 1 <= n <= 4096 frames and per_frame >= 1");
    return guarded([&] {
        fh::launch_track_select(reinterpret_cast<const fh::FaceRec*>(det), embed, track, n, per_frame, reinterpret_cast<fh::FaceRec*>(faces),
                                frame_of, track_of, total, S(stream));
        FH_HIP(hipGetLastError());
        return n;
    });
}
// fh_pipeline_run_dev with the tracker between the NMS and the selection: detect -> update -> flagged select -> the one 4-byte
// hand-off -> align + embed on exactly the flagged faces, all on `stream`.  (slot: null, or the update's third output.)  With the
// best-shot policy on, the quality kernel runs between the detector and the update, into the tracker's buffer, and the update reads it.
namespace {
int pipeline_tracked(fh_det* d, fh_rec* r, fh_tracker* t, const uint8_t* frames, int n, int rows, int cols, int step, long long stride,
                     const int* stream_of, float score_thr, float nms_thr, int F, fh_face* all, int* counts, int* track, int* flags, int* slot,
                     fh_face* faces, int* frame_of, int* track_of, float* emb, hipStream_t s) {
    d->p_total.ensure(sizeof(int));
    if (!d->ev_sel) FH_HIP(hipEventCreateWithFlags(&d->ev_sel, hipEventDisableTiming));
    if (!d->h_total) FH_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->h_total), sizeof(int), hipHostMallocDefault));
    fh::FaceRec* rec_all = reinterpret_cast<fh::FaceRec*>(all);
    d->det.detect_dev(frames, n, rows, cols, step, (long)stride, score_thr, nms_thr, rec_all, F, counts, s);
    int* const quality = t->t.bestshot() ? t->t.quality_scratch((size_t)n * F) : nullptr;
    if (quality) fh::launch_face_quality(frames, (long)stride, rows, cols, step, nullptr, n, rec_all, counts, F, quality, s);
    t->t.update_dev(rec_all, counts, n, F, stream_of, track, flags, slot, quality, s);
    fh::launch_track_select(rec_all, flags, track, n, F, reinterpret_cast<fh::FaceRec*>(faces), frame_of, track_of, d->p_total.as<int>(), s);
    const int total = count_handoff(d, d->p_total.as<int>(), s);
    r->rec.embed_faces_dev(frames, rows, cols, step, (long)stride, reinterpret_cast<const fh::FaceRec*>(faces), frame_of, total, emb, nullptr, s);
    return total;
}
// what fh_track_identify_dev and fh_pipeline_run_identified_dev ask of the tracker and the gallery.  Null on success.
const char* bad_identity(const fh_tracker* t, const fh_gallery* g) {
    if (t->t.identity_dim() == 0) return "identity is not enabled (fh_tracker_enable_identity)";
    if (g->g.dim() != t->t.identity_dim()) return "the gallery's dim is not the identity dim";
    return nullptr;
}
// what the two identify calls check alike, in their order (ptrs: the call's own device pointers are all given).  Null on success.
const char* bad_identify_call(fh_tracker* t, fh_gallery* g, bool ptrs, const int* quality, const float* emb, int total, int n,
                              int per_frame, const int* stream_of, const char* weighted_needs_quality) {
    if (!t || !g || !ptrs) return "null argument";
    if (const char* bad = bad_track_batch(t, n, per_frame, stream_of)) return bad;
    if (const char* bad = bad_identity(t, g)) return bad;
    if (total < 0 || (long long)total > (long long)n * per_frame) return "need 0 <= total <= n * per_frame";
    if (total > 0 && !emb) return "null embeddings with total > 0";
    if (!quality && t->t.identity_pool() == FH_TRACK_POOL_WEIGHTED) return weighted_needs_quality;
    return nullptr;
}
}  // namespace
int fh_pipeline_run_tracked_dev(fh_det* d, fh_rec* r, fh_tracker* t, const uint8_t* frames, int n, int rows, int cols, int step,
                                long long stride, const int* stream_of, float score_thr, float nms_thr, int F, fh_face* all, int* counts,
                                int* track, fh_face* faces, int* frame_of, int* track_of, float* emb, void* stream) {
    if (!d || !r || !t || !frames || !all || !counts || !track || !faces || !frame_of || !track_of || !emb)
        return arg_error("fh_pipeline_run_tracked_dev: null argument");
    if (const char* bad = bad_track_batch(t, n, F, stream_of)) return frames_error("fh_pipeline_run_tracked_dev", bad);
    if (rows <= 0 || cols <= 0 || step < cols * 3) return arg_error("fh_pipeline_run_tracked_dev: bad size");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        return pipeline_tracked(d, r, t, frames, n, rows, cols, step, stride, stream_of, score_thr, nms_thr, F, all, counts, track,
                                t->t.embed_scratch((size_t)n * F), nullptr, faces, frame_of, track_of, emb, S(stream));
    });
}

// ---------------------------------------------------------------------------------- face quality and the best-shot policy
namespace {
const char* bad_quality_batch(const fh_face* det, const int* counts, int n, int per_frame, const int* quality) {
    if (!det || !counts || !quality) return "null argument";
    if (n < 1 || n > fh::kTrackMaxFrames) return "need 1 <= n <= 4096 frames";
    if (per_frame < 1 || (long long)n * per_frame > 0x7fffffffLL) return "need per_frame >= 1 and n * per_frame < 2^31";
    return nullptr;
}
}  // namespace
int fh_face_quality_dev(const uint8_t* frames, int n, int rows, int cols, int step, long long stride, const fh_face* det, const int* counts,
                        int per_frame, int* quality, void* stream) {
    if (const char* bad = bad_quality_batch(det, counts, n, per_frame, quality)) return frames_error("fh_face_quality_dev", bad);
    if (!frames) return arg_error("fh_face_quality_dev: null argument");
    if (rows <= 0 || cols <= 0 || step < cols * 3) return arg_error("fh_face_quality_dev: bad size");
    return guarded([&] {
        fh::launch_face_quality(frames, (long)stride, rows, cols, step, nullptr, n, reinterpret_cast<const fh::FaceRec*>(det), counts, per_frame,
                                quality, S(stream));
        FH_HIP(hipGetLastError());
        return n;
    });
}
int fh_face_quality_ragged_dev(const fh_frame* frames, int n, const fh_face* det, const int* counts, int per_frame, int* quality, void* stream) {
    if (const char* bad = bad_frames(frames, n)) return frames_error("fh_face_quality_ragged_dev", bad);
    if (const char* bad = bad_quality_batch(det, counts, n, per_frame, quality)) return frames_error("fh_face_quality_ragged_dev", bad);
    return guarded([&] {
        hipStream_t s = S(stream);
        // the frame table of this entry point: one per calling thread, and a call on a DIFFERENT stream than the previous one first
        // waits for that one's kernel (as fh_postprocess_rows_dev's scratch; never destroyed, for the same reason)
        struct Scratch { fh::FrameTable tab; hipEvent_t done = nullptr; hipStream_t last = nullptr; bool used = false; };
        thread_local Scratch* scp = new Scratch();
        Scratch& sc = *scp;
        if (!sc.done) FH_HIP(hipEventCreateWithFlags(&sc.done, hipEventDisableTiming));
        if (sc.used && sc.last != s) FH_HIP(hipStreamWaitEvent(s, sc.done, 0));
        const fh::FrameDesc* table = sc.tab.upload(FI(frames), n, 0, 0, s);
        fh::launch_face_quality(nullptr, 0, 0, 0, 0, table, n, reinterpret_cast<const fh::FaceRec*>(det), counts, per_frame, quality, s);
        FH_HIP(hipGetLastError());
        FH_HIP(hipEventRecord(sc.done, s));
        sc.last = s; sc.used = true;
        return n;
    });
}
int fh_tracker_set_bestshot(fh_tracker* t, int on, int num, int den, int min_gap) {
    if (!t) return arg_error("fh_tracker_set_bestshot: null handle");
    if (den < 1 || num < den || num > 32768 || min_gap < 1) return arg_error("fh_tracker_set_bestshot: need 1 <= den <= num <= 32768 and min_gap >= 1");
    return guarded([&] { t->t.set_bestshot(on != 0, num, den, min_gap); return 0; });
}
int fh_tracker_get_quality(fh_tracker* t, int stream, int* out) {
    if (!t || !out) return arg_error("fh_tracker_get_quality: null argument");
    if (stream < 0 || stream >= t->t.streams()) return arg_error("fh_tracker_get_quality: no such stream");
    if (!t->t.has_best_quality()) return arg_error("fh_tracker_get_quality: the best-shot policy was never set (fh_tracker_set_bestshot)");
    return guarded([&] { return t->t.get_quality(stream, out); });
}
const int* fh_tracker_quality_dev(fh_tracker* t) { return t ? t->t.quality() : nullptr; }

// ---------------------------------------------------------------------------------- track identity
int fh_tracker_enable_identity(fh_tracker* t, int dim, int pool) {
    if (!t) return arg_error("fh_tracker_enable_identity: null handle");
    if (dim < 64 || dim > 4096 || dim % 64) return arg_error("fh_tracker_enable_identity: need dim % 64 == 0 and 64 <= dim <= 4096");
    // the weighted pool belongs to the quality feature: a tracker takes it only once fh_tracker_set_bestshot has been called on it
    const bool weighted_ok = pool == FH_TRACK_POOL_WEIGHTED && t->t.has_best_quality();
    if (pool != FH_TRACK_POOL_LAST && pool != FH_TRACK_POOL_SUM && !weighted_ok)
        return arg_error("fh_tracker_enable_identity: unknown pool mode (FH_TRACK_POOL_WEIGHTED needs fh_tracker_set_bestshot first)");
    return guarded([&] { t->t.enable_identity(dim, pool); return 0; });
}
int fh_track_identify_q_dev(fh_tracker* t, fh_gallery* g, float threshold, const int* track, const int* slot, const int* embed,
                            const int* quality, const float* emb, int total, int n, int per_frame, const int* stream_of, int* label,
                            float* score, void* stream) {
    const char* const fn = quality ? "fh_track_identify_q_dev" : "fh_track_identify_dev";
    const char* const bad = bad_identify_call(t, g, track && slot && embed && label && score, quality, emb, total, n, per_frame, stream_of,
                                              "the weighted pool needs the qualities (fh_track_identify_q_dev)");
    if (bad) return frames_error(fn, bad);
    if (t->t.relink()) {
        g_err = std::string(fn) + ": re-linking is on for this tracker: call fh_track_identify_link_dev";
        return FH_ERR_STATE;
    }
    return guarded([&] {
        t->t.identify_dev(g->g, threshold, track, slot, embed, quality, emb, total, n, per_frame, stream_of, label, score, S(stream));
        return n;
    });
}
int fh_track_identify_dev(fh_tracker* t, fh_gallery* g, float threshold, const int* track, const int* slot, const int* embed, const float* emb,
                          int total, int n, int per_frame, const int* stream_of, int* label, float* score, void* stream) {
    return fh_track_identify_q_dev(t, g, threshold, track, slot, embed, nullptr, emb, total, n, per_frame, stream_of, label, score, stream);
}
const float* fh_tracker_queries_dev(fh_tracker* t) { return t ? t->t.queries() : nullptr; }
int fh_tracker_get_identity(fh_tracker* t, int stream, fh_track_ident* out, float* sums_out) {
    if (!t) return arg_error("fh_tracker_get_identity: null handle");
    if (stream < 0 || stream >= t->t.streams()) return arg_error("fh_tracker_get_identity: no such stream");
    if (t->t.identity_dim() == 0) return arg_error("fh_tracker_get_identity: identity is not enabled (fh_tracker_enable_identity)");
    return guarded([&] { return t->t.get_identity(stream, reinterpret_cast<fh::TrackIdent*>(out), sums_out); });
}
// fh_pipeline_run_tracked_dev with the update reporting slots, then the identify step on what the recogniser produced
int fh_pipeline_run_identified_dev(fh_det* d, fh_rec* r, fh_tracker* t, fh_gallery* g, float threshold, const uint8_t* frames, int n, int rows,
                                   int cols, int step, long long stride, const int* stream_of, float score_thr, float nms_thr, int F,
                                   fh_face* all, int* counts, int* track, fh_face* faces, int* frame_of, int* track_of, float* emb, int* label,
                                   float* score, void* stream) {
    if (!d || !r || !t || !g || !frames || !all || !counts || !track || !faces || !frame_of || !track_of || !emb || !label || !score)
        return arg_error("fh_pipeline_run_identified_dev: null argument");
    if (const char* bad = bad_track_batch(t, n, F, stream_of)) return frames_error("fh_pipeline_run_identified_dev", bad);
    if (rows <= 0 || cols <= 0 || step < cols * 3) return arg_error("fh_pipeline_run_identified_dev: bad size");
    if (const char* bad = bad_identity(t, g)) return frames_error("fh_pipeline_run_identified_dev", bad);
    if (r->rec.dim() != t->t.identity_dim()) return arg_error("fh_pipeline_run_identified_dev: the recogniser's feature dim is not the identity dim");
    if (t->t.identity_pool() == FH_TRACK_POOL_WEIGHTED && !t->t.bestshot())
        return arg_error("fh_pipeline_run_identified_dev: the weighted pool needs the qualities: set the best-shot policy (fh_tracker_set_bestshot)");
    Owns owns(&d->det.net(), &r->rec.net());
    return guarded([&] {
        hipStream_t s = S(stream);
        int* const flags = t->t.embed_scratch((size_t)n * F);
        int* const slot = t->t.slot_scratch((size_t)n * F);
        const int total = pipeline_tracked(d, r, t, frames, n, rows, cols, step, stride, stream_of, score_thr, nms_thr, F, all, counts, track,
                                           flags, slot, faces, frame_of, track_of, emb, s);
        // re-linking on: the link form of the identify step, into the tracker's roots buffer (fh_tracker_roots_dev)
        t->t.identify_dev(g->g, threshold, track, slot, flags, t->t.bestshot() ? t->t.quality() : nullptr, emb, total, n, F, stream_of, label,
                          score, s, t->t.relink() ? t->t.roots_scratch((size_t)n * F) : nullptr);
        return total;
    });
}

// ---------------------------------------------------------------------------------- track re-linking
int fh_tracker_enable_relink(fh_tracker* t, int memory, float link_thr, int max_age) {
    if (!t) return arg_error("fh_tracker_enable_relink: null handle");
    if (t->t.identity_dim() == 0) {
        g_err = "fh_tracker_enable_relink: identity is not enabled (fh_tracker_enable_identity)";
        return FH_ERR_STATE;
    }
    if (memory < 0 || memory > fh::kTrackLinkMemory || !std::isfinite(link_thr) || max_age <= t->t.max_missed())
        return arg_error("fh_tracker_enable_relink: need 0 <= memory <= 256, a finite link_thr and max_age > max_missed");
    return guarded([&] { t->t.enable_relink(memory, link_thr, max_age); return 0; });
}
int fh_tracker_set_stream_masks(fh_tracker* t, const uint32_t* masks_host) {
    if (!t) return arg_error("fh_tracker_set_stream_masks: null handle");
    return guarded([&] { t->t.set_stream_masks(masks_host); return 0; });
}
int fh_track_identify_link_dev(fh_tracker* t, fh_gallery* g, float threshold, const int* track, const int* slot, const int* embed,
                               const int* quality, const float* emb, int total, int n, int per_frame, const int* stream_of, int* label,
                               float* score, int* root, void* stream) {
    const char* const bad = bad_identify_call(t, g, track && slot && embed && label && score && root, quality, emb, total, n, per_frame,
                                              stream_of, "the weighted pool needs the qualities");
    if (bad) return frames_error("fh_track_identify_link_dev", bad);
    return guarded([&] {
        t->t.identify_dev(g->g, threshold, track, slot, embed, quality, emb, total, n, per_frame, stream_of, label, score, S(stream), root);
        return n;
    });
}
int fh_tracker_get_links(fh_tracker* t, int stream, fh_track_link* out, float* sums_out) {
    if (!t || (!out && sums_out)) return arg_error("fh_tracker_get_links: null argument");
    if (stream < 0 || stream >= t->t.streams()) return arg_error("fh_tracker_get_links: no such stream");
    if (!t->t.relink()) {
        g_err = "fh_tracker_get_links: re-linking is not enabled (fh_tracker_enable_relink)";
        return FH_ERR_STATE;
    }
    if (!out) return t->t.link_rows();                           // the size query: nothing is written
    return guarded([&] { t->t.get_links(stream, reinterpret_cast<fh::TrackLink*>(out), sums_out); return t->t.link_rows(); });
}
const int* fh_tracker_roots_dev(fh_tracker* t) { return t ? t->t.roots() : nullptr; }

// ---------------------------------------------------------------------------------- streaming front end (host frames)
// The caller of the path (reference testWebcam, src/main.cpp:214-258: grab a frame, detect, embed every face, compare) over
// BATCHES of host frames: a ring of device slots, uploads on a copy stream while the previous batch computes, results
// fetched one batch later.  All device memory, streams and events belong to the object.
struct fh_stream {
    static constexpr int kSlots = 2;
    fh_det* det; fh_rec* rec;
    int n, rows, cols, F, dim;
    size_t frame_bytes;
    hipStream_t copy_s = nullptr, comp_s = nullptr;
    struct Slot {
        fh::DevBuf frames, faces, frame_of, emb;
        hipEvent_t uploaded = nullptr, done = nullptr;
        int total = -1;                       // faces of the batch in flight (-1 = slot free)
        int frames_in = 0;
    } slot[kSlots];
    long submitted = 0, collected = 0;
    fh_stream(fh_det* d, fh_rec* r, int n_, int rows_, int cols_, int F_) : det(d), rec(r), n(n_), rows(rows_), cols(cols_), F(F_) {
        dim = r->rec.dim();
        frame_bytes = (size_t)rows * cols * 3;
        FH_HIP(hipStreamCreateWithFlags(&copy_s, hipStreamNonBlocking));
        FH_HIP(hipStreamCreateWithFlags(&comp_s, hipStreamNonBlocking));
        for (auto& sl : slot) {
            sl.frames.ensure((size_t)n * frame_bytes);
            sl.faces.ensure((size_t)n * F * sizeof(fh_face));
            sl.frame_of.ensure((size_t)n * F * sizeof(int));
            sl.emb.ensure((size_t)n * F * dim * sizeof(float));
            FH_HIP(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
            FH_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        }
    }
    ~fh_stream() {
        (void)hipDeviceSynchronize();
        for (auto& sl : slot) { if (sl.uploaded) (void)hipEventDestroy(sl.uploaded); if (sl.done) (void)hipEventDestroy(sl.done); }
        if (copy_s) (void)hipStreamDestroy(copy_s);
        if (comp_s) (void)hipStreamDestroy(comp_s);
    }
};

fh_stream* fh_stream_create(fh_det* d, fh_rec* r, int frames_per_batch, int rows, int cols, int faces_per_frame) {
    if (!d || !r || frames_per_batch <= 0 || frames_per_batch > 4096 || rows <= 0 || cols <= 0 || faces_per_frame <= 0) {
        g_err = "fh_stream_create: bad argument";
        return nullptr;
    }
    fh_stream* h = nullptr;
    const int rc = guarded([&] { h = new fh_stream(d, r, frames_per_batch, rows, cols, faces_per_frame); return 0; });
    return rc == 0 ? h : nullptr;
}
void fh_stream_destroy(fh_stream* s) { delete s; }

int fh_stream_submit(fh_stream* st, const uint8_t* host_frames, int n_frames, float score_thr, float nms_thr) {
    if (!st || !host_frames) return arg_error("fh_stream_submit: null argument");
    if (n_frames <= 0 || n_frames > st->n) return arg_error("fh_stream_submit: batch larger than the stream was created for");
    if (st->submitted - st->collected >= fh_stream::kSlots) { g_err = "fh_stream_submit: ring full, collect a batch first"; return FH_ERR_STATE; }
    Owns owns(&st->det->det.net(), &st->rec->rec.net());
    return guarded([&] {
        fh_stream::Slot& sl = st->slot[st->submitted % fh_stream::kSlots];
        // upload on the copy stream (overlaps the batch computing on comp_s), compute behind the upload's event
        FH_HIP(hipMemcpyAsync(sl.frames.p, host_frames, (size_t)n_frames * st->frame_bytes, hipMemcpyHostToDevice, st->copy_s));
        FH_HIP(hipEventRecord(sl.uploaded, st->copy_s));
        FH_HIP(hipStreamWaitEvent(st->comp_s, sl.uploaded, 0));
        const int step = st->cols * 3;
        const int total = detect_select_count(st->det, sl.frames.as<uint8_t>(), n_frames, st->rows, st->cols, step, (long)st->frame_bytes, score_thr, nms_thr,
                                              st->F, sl.faces.as<fh_face>(), sl.frame_of.as<int>(), nullptr, st->comp_s);
        st->rec->rec.embed_faces_dev(sl.frames.as<uint8_t>(), st->rows, st->cols, step, (long)st->frame_bytes, sl.faces.as<fh::FaceRec>(),
                                     sl.frame_of.as<int>(), total, sl.emb.as<float>(), nullptr, st->comp_s);
        FH_HIP(hipEventRecord(sl.done, st->comp_s));
        sl.total = total; sl.frames_in = n_frames;
        ++st->submitted;
        return total;
    });
}

int fh_stream_collect(fh_stream* st, fh_face* faces, int* frame_of, float* emb, int cap) {
    if (!st) return arg_error("fh_stream_collect: null handle");
    if (st->collected >= st->submitted) { g_err = "fh_stream_collect: nothing in flight"; return FH_ERR_STATE; }
    Owns owns(&st->det->det.net(), &st->rec->rec.net());
    return guarded([&] {
        fh_stream::Slot& sl = st->slot[st->collected % fh_stream::kSlots];
        FH_HIP(hipEventSynchronize(sl.done));
        const int m = sl.total < cap ? sl.total : cap;
        if (m > 0) {
            if (faces) FH_HIP(hipMemcpy(faces, sl.faces.p, (size_t)m * sizeof(fh_face), hipMemcpyDeviceToHost));
            if (frame_of) FH_HIP(hipMemcpy(frame_of, sl.frame_of.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
            if (emb) FH_HIP(hipMemcpy(emb, sl.emb.p, (size_t)m * st->dim * sizeof(float), hipMemcpyDeviceToHost));
        }
        const int total = sl.total;
        sl.total = -1;
        ++st->collected;
        return total;
    });
}

// ---------------------------------------------------------------------------------- gallery
fh_gallery* fh_gallery_create(int dim) {
    if (dim <= 0) { g_err = "fh_gallery_create: bad dim"; return nullptr; }
    return new fh_gallery(dim);
}
void fh_gallery_destroy(fh_gallery* g) { delete g; }
int fh_gallery_upload(fh_gallery* g, const float* rows, long long n, int on_device, long long index_base) {
    if (!g || !rows || n <= 0) return arg_error("fh_gallery_upload: bad argument");
    return guarded([&] { g->g.upload(rows, nullptr, (long)n, on_device != 0, (long)index_base); return 0; });
}
long long fh_gallery_enroll(fh_gallery* g, const float* rows, long long n, int on_device) {
    if (!g || !rows || n <= 0) return arg_error("fh_gallery_enroll: bad argument");
    long long first = -1;
    const int rc = guarded([&] { first = g->g.enroll(rows, nullptr, (long)n, on_device != 0); return 0; });
    return rc < 0 ? rc : first;
}
long long fh_gallery_size(fh_gallery* g) { return g ? (long long)g->g.size() : (long long)arg_error("fh_gallery_size: null handle"); }
int fh_gallery_label_dev(fh_gallery* g, const float* q, int nq, float threshold, int* labels, float* scores, void* stream) {
    if (!g || !q || !labels || !scores) return arg_error("fh_gallery_label_dev: null argument");
    return guarded([&] { g->g.label_dev(q, nullptr, nq, threshold, false, labels, scores, S(stream)); return nq; });
}
int fh_gallery_topk_dev(fh_gallery* g, const float* q, int nq, int k, float* scores, int* indices, void* stream) {
    if (!g || !q || !scores || !indices) return arg_error("fh_gallery_topk_dev: null argument");
    return guarded([&] { g->g.topk_dev(q, nullptr, nq, k, false, scores, nullptr, indices, S(stream)); return nq; });
}

int fh_gallery_set_scan(fh_gallery* g, int mode) {
    if (!g) return arg_error("fh_gallery_set_scan: null handle");
    if (mode != FH_GAL_SCAN_FP32 && mode != FH_GAL_SCAN_F16_RERANK) return arg_error("fh_gallery_set_scan: unknown mode");
    return guarded([&] { g->g.set_scan(mode); return 0; });
}
int fh_gallery_get_scan(const fh_gallery* g) { return g ? g->g.scan() : arg_error("fh_gallery_get_scan: null handle"); }
int fh_gallery_scan_stats(fh_gallery* g, long long* certified, long long* fallback) {
    if (!g) return arg_error("fh_gallery_scan_stats: null handle");
    return guarded([&] { g->g.scan_stats(certified, fallback); return 0; });
}

int fh_topk_merge_dev(const float* ps, const int* pi, int nparts, int nq, int k, float* scores, int* indices, void* stream) {
    if (!ps || !pi || !scores || !indices) return arg_error("fh_topk_merge_dev: null argument");
    if (nparts <= 0 || nq <= 0 || k <= 0 || k > 16 || (long)nparts * k > 65536) return arg_error("fh_topk_merge_dev: bad size");
    return guarded([&] {
        fh::launch_topk_merge(ps, pi, nparts, nq, k, scores, indices, S(stream));
        FH_HIP(hipGetLastError());
        return nq;
    });
}

// ---- labelled gallery (gallery_ids.hip).  Ids are checked before anything changes: a host list here, a device list after one copy.
namespace {
bool any_negative(const int* ids, long long n) {
    for (long long i = 0; i < n; ++i)
        if (ids[i] < 0) return true;
    return false;
}
// 0 = fine, FH_ERR_ARG = a negative id, other < 0 = the copy failed
int check_ids(const char* who, const int* ids, long long n, int on_device) {
    if (!on_device) return any_negative(ids, n) ? arg_error(who) : 0;
    std::vector<int> h((size_t)n);
    const int rc = guarded([&] { FH_HIP(hipMemcpy(h.data(), ids, (size_t)n * sizeof(int), hipMemcpyDeviceToHost)); return 0; });
    if (rc < 0) return rc;
    return any_negative(h.data(), n) ? arg_error(who) : 0;
}
}  // namespace
long long fh_gallery_enroll_ids(fh_gallery* g, const float* rows, const int* ids, long long n, int on_device) {
    if (!g || !rows || !ids || n <= 0) return arg_error("fh_gallery_enroll_ids: bad argument");
    if (const int rc = check_ids("fh_gallery_enroll_ids: negative id", ids, n, on_device)) return rc;
    long long first = -1;
    const int rc = guarded([&] { first = g->g.enroll(rows, ids, (long)n, on_device != 0); return 0; });
    return rc < 0 ? rc : first;
}
int fh_gallery_upload_ids(fh_gallery* g, const float* rows, const int* ids, long long n, int on_device, long long index_base) {
    if (!g || !rows || !ids || n <= 0) return arg_error("fh_gallery_upload_ids: bad argument");
    if (const int rc = check_ids("fh_gallery_upload_ids: negative id", ids, n, on_device)) return rc;
    return guarded([&] { g->g.upload(rows, ids, (long)n, on_device != 0, (long)index_base); return 0; });
}
int fh_gallery_topk_ids_dev(fh_gallery* g, const float* q, int nq, int k, float* scores, int* ids, int* rows, void* stream) {
    if (!g || !q || !scores || !ids) return arg_error("fh_gallery_topk_ids_dev: null argument");
    if (nq <= 0 || nq > 256 || k <= 0 || k > 16) return arg_error("fh_gallery_topk_ids_dev: need 0 < nq <= 256 and 0 < k <= 16");
    return guarded([&] { g->g.topk_dev(q, nullptr, nq, k, true, scores, ids, rows, S(stream)); return nq; });
}
int fh_gallery_label_ids_dev(fh_gallery* g, const float* q, int nq, float threshold, int* ids, float* scores, void* stream) {
    if (!g || !q || !ids || !scores) return arg_error("fh_gallery_label_ids_dev: null argument");
    if (nq <= 0 || nq > 256) return arg_error("fh_gallery_label_ids_dev: need 0 < nq <= 256");
    return guarded([&] { g->g.label_dev(q, nullptr, nq, threshold, true, ids, scores, S(stream)); return nq; });
}
long long fh_gallery_remove_ids(fh_gallery* g, const int* ids_host, long long n_ids) {
    if (!g || !ids_host || n_ids <= 0) return arg_error("fh_gallery_remove_ids: bad argument");
    if (any_negative(ids_host, n_ids)) return arg_error("fh_gallery_remove_ids: negative id");
    long long removed = 0;
    const int rc = guarded([&] { removed = g->g.remove_ids(ids_host, (long)n_ids); return 0; });
    return rc < 0 ? rc : removed;
}
long long fh_gallery_get_ids(fh_gallery* g, long long first, long long n, int* ids_host_out) {
    if (!g || first < 0 || n < 0 || (n > 0 && !ids_host_out)) return arg_error("fh_gallery_get_ids: bad argument");
    if (first + n > (long long)g->g.size()) return arg_error("fh_gallery_get_ids: range outside the gallery");
    const int rc = guarded([&] { g->g.get_ids((long)first, (long)n, ids_host_out); return 0; });
    return rc < 0 ? rc : n;
}

// ---- watchlists (gallery_tags.hip): a tag per row, a mask per query, the predicate inside the scan's admission test
long long fh_gallery_set_tags(fh_gallery* g, long long first, long long n, const uint32_t* tags, int on_device) {
    if (!g || first < 0 || n < 0 || (n > 0 && !tags)) return arg_error("fh_gallery_set_tags: bad argument");
    if (first + n > (long long)g->g.size()) return arg_error("fh_gallery_set_tags: range outside the gallery");
    const int rc = guarded([&] { g->g.set_tags((long)first, (long)n, tags, on_device != 0); return 0; });
    return rc < 0 ? rc : n;
}
long long fh_gallery_get_tags(fh_gallery* g, long long first, long long n, uint32_t* tags_host_out) {
    if (!g || first < 0 || n < 0 || (n > 0 && !tags_host_out)) return arg_error("fh_gallery_get_tags: bad argument");
    if (first + n > (long long)g->g.size()) return arg_error("fh_gallery_get_tags: range outside the gallery");
    const int rc = guarded([&] { g->g.get_tags((long)first, (long)n, tags_host_out); return 0; });
    return rc < 0 ? rc : n;
}
int fh_gallery_topk_tagged_dev(fh_gallery* g, const float* q, const uint32_t* masks, int nq, int k, float* scores, int* indices, void* stream) {
    if (!g || !q || !masks || !scores || !indices) return arg_error("fh_gallery_topk_tagged_dev: null argument");
    return guarded([&] { g->g.topk_dev(q, masks, nq, k, false, scores, nullptr, indices, S(stream)); return nq; });
}
int fh_gallery_topk_ids_tagged_dev(fh_gallery* g, const float* q, const uint32_t* masks, int nq, int k, float* scores, int* ids, int* rows,
                                   void* stream) {
    if (!g || !q || !masks || !scores || !ids) return arg_error("fh_gallery_topk_ids_tagged_dev: null argument");
    if (nq <= 0 || nq > 256 || k <= 0 || k > 16) return arg_error("fh_gallery_topk_ids_tagged_dev: need 0 < nq <= 256 and 0 < k <= 16");
    return guarded([&] { g->g.topk_dev(q, masks, nq, k, true, scores, ids, rows, S(stream)); return nq; });
}
int fh_gallery_label_tagged_dev(fh_gallery* g, const float* q, const uint32_t* masks, int nq, float threshold, int* labels, float* scores,
                                void* stream) {
    if (!g || !q || !masks || !labels || !scores) return arg_error("fh_gallery_label_tagged_dev: null argument");
    return guarded([&] { g->g.label_dev(q, masks, nq, threshold, false, labels, scores, S(stream)); return nq; });
}
int fh_gallery_label_ids_tagged_dev(fh_gallery* g, const float* q, const uint32_t* masks, int nq, float threshold, int* ids, float* scores,
                                    void* stream) {
    if (!g || !q || !masks || !ids || !scores) return arg_error("fh_gallery_label_ids_tagged_dev: null argument");
    if (nq <= 0 || nq > 256) return arg_error("fh_gallery_label_ids_tagged_dev: need 0 < nq <= 256");
    return guarded([&] { g->g.label_dev(q, masks, nq, threshold, true, ids, scores, S(stream)); return nq; });
}
int fh_gallery_tag_stats(fh_gallery* g, long long* tiles_scanned, long long* tiles_skipped) {
    if (!g) return arg_error("fh_gallery_tag_stats: null handle");
    return guarded([&] { g->g.tag_stats(tiles_scanned, tiles_skipped); return 0; });
}
int fh_debug_tag_skip(int on) { fh::gallery_debug_tag_skip(on); return 0; }

int fh_topk_merge_ids_dev(const float* ps, const int* pd, const int* pr, int nparts, int nq, int k, float* scores, int* ids, int* rows,
                          void* stream) {
    if (!ps || !pd || !pr || !scores || !ids || !rows) return arg_error("fh_topk_merge_ids_dev: null argument");
    if (nparts <= 0 || nq <= 0 || k <= 0 || k > 16 || (long)nparts * k > 65536) return arg_error("fh_topk_merge_ids_dev: bad size");
    return guarded([&] {
        fh::launch_topk_merge_ids(ps, pd, pr, nparts, nq, k, scores, ids, rows, S(stream));
        FH_HIP(hipGetLastError());
        return nq;
    });
}

// ---- template pooling (gallery_fuse.hip) and what goes with it: the grouping on the host, the rows read back, the mislabel audit
long long fh_gallery_group_ids(const int* ids, long long n, int* order, long long* starts, int* uniq) {
    if (n < 0 || (n > 0 && !ids)) return arg_error("fh_gallery_group_ids: bad argument");
    long long m = -1;
    const int rc = guarded([&] { m = fh::group_ids(ids, n, order, starts, uniq); return 0; });      // (the sort may run out of memory)
    if (rc < 0) return rc;
    return m < 0 ? arg_error("fh_gallery_group_ids: negative id (or more than 2^31 - 1 rows)") : m;
}
long long fh_gallery_fuse_ids(fh_gallery* src, fh_gallery* dst, int mode) {
    if (!src || !dst || src == dst) return arg_error("fh_gallery_fuse_ids: need two different galleries");
    if (src->g.dim() != dst->g.dim()) return arg_error("fh_gallery_fuse_ids: the galleries' dims differ");
    if (mode != FH_FUSE_UNIT && mode != FH_FUSE_SUM) return arg_error("fh_gallery_fuse_ids: unknown mode");
    if (src->g.size() > 0 && !src->g.labelled()) {
        g_err = "gallery: fh_gallery_fuse_ids needs a labelled gallery (rows enrolled with ids)";
        return FH_ERR_STATE;
    }
    long long m = 0;
    const int rc = guarded([&] { m = dst->g.fuse_from(src->g, mode == FH_FUSE_UNIT, FH_FUSE_CHUNK); return 0; });
    return rc < 0 ? rc : m;
}
long long fh_gallery_get_rows(fh_gallery* g, long long first, long long n, float* rows_host_out) {
    if (!g || first < 0 || n < 0 || (n > 0 && !rows_host_out)) return arg_error("fh_gallery_get_rows: bad argument");
    if (first + n > (long long)g->g.size()) return arg_error("fh_gallery_get_rows: range outside the gallery");
    const int rc = guarded([&] { g->g.get_rows((long)first, (long)n, rows_host_out); return 0; });
    return rc < 0 ? rc : n;
}
int fh_gallery_self_scores_dev(fh_gallery* src, fh_gallery* tmpl, float* d_scores, void* stream) {
    if (!src || !tmpl || !d_scores) return arg_error("fh_gallery_self_scores_dev: null argument");
    if (src->g.dim() != tmpl->g.dim()) return arg_error("fh_gallery_self_scores_dev: the galleries' dims differ");
    return guarded([&] { src->g.self_scores_dev(tmpl->g, d_scores, S(stream)); return (int)FH_OK; });
}

// ---- unsupervised grouping: the rule on the host (cluster_plan.h), the same rule over the gallery's own rows (gallery_cluster.hip)
namespace {
const char* bad_cluster(int min_pts, int noise) {
    if (min_pts < 1) return "need min_pts >= 1";
    if (noise != FH_CLUSTER_NOISE_NONE && noise != FH_CLUSTER_NOISE_SELF) return "unknown noise mode";
    return nullptr;
}
}  // namespace
int fh_cluster_scores(const float* scores, int n, float threshold, int min_pts, int noise, int* labels, int* info) {
    if (n < 0 || (n > 0 && (!scores || !labels))) return arg_error("fh_cluster_scores: bad argument");
    if (const char* why = bad_cluster(min_pts, noise)) return frames_error("fh_cluster_scores", why);
    int m = -1;
    const int rc = guarded([&] { m = fh::cluster_scores(scores, n, threshold, min_pts, noise, labels, info); return 0; });   // (its scratch may run out of memory)
    if (rc < 0) return rc;
    return m < 0 ? arg_error("fh_cluster_scores: bad argument") : m;
}
int fh_gallery_cluster_dev(fh_gallery* g, float threshold, int min_pts, int noise, int* d_labels, int* d_info, void* stream) {
    if (!g || !d_labels) return arg_error("fh_gallery_cluster_dev: null argument");
    if (const char* why = bad_cluster(min_pts, noise)) return frames_error("fh_gallery_cluster_dev", why);
    return guarded([&] { g->g.cluster_dev(threshold, min_pts, noise == FH_CLUSTER_NOISE_SELF, d_labels, d_info, S(stream)); return (int)FH_OK; });
}
long long fh_gallery_set_ids(fh_gallery* g, const int* ids, int on_device) {
    if (!g) return arg_error("fh_gallery_set_ids: null handle");
    const long long n = (long long)g->g.size();
    if (n > 0 && !ids) return arg_error("fh_gallery_set_ids: null ids");
    if (n > 0)
        if (const int rc = check_ids("fh_gallery_set_ids: negative id", ids, n, on_device)) return rc;
    const int rc = guarded([&] { g->g.set_ids(ids, on_device != 0); return 0; });
    return rc < 0 ? rc : n;
}
int fh_debug_cluster_tiles(int tiles_per_wg) { fh::cluster_debug_tiles(tiles_per_wg); return 0; }

// ---- threshold calibration: the bin rule and the ROC read-out on the host (roc_plan.h), the pair histogram over the gallery's own rows
// (gallery_cluster.hip)
static_assert(FH_HIST_BINS == fh::kHistBins && sizeof(fh_roc_point) == sizeof(fh::RocPoint) && sizeof(unsigned long long) == sizeof(uint64_t) &&
              offsetof(fh_roc_point, bin) == offsetof(fh::RocPoint, bin) && offsetof(fh_roc_point, impostor) == offsetof(fh::RocPoint, impostor),
              "fh_roc_point mirrors roc_plan.h");
int fh_hist_bin(float score) { return fh::hist_bin(score); }
int fh_roc_from_hist(const unsigned long long* hist, double max_far, fh_roc_point out[2]) {
    if (!hist || !out) return arg_error("fh_roc_from_hist: null argument");
    if (!(max_far >= 0.0 && max_far <= 1.0)) return arg_error("fh_roc_from_hist: need 0 <= max_far <= 1");
    fh::RocPoint pt[2];
    if (fh::roc_from_hist(reinterpret_cast<const uint64_t*>(hist), max_far, pt) < 0) {
        g_err = "fh_roc_from_hist: a plane of the histogram is empty (no genuine or no impostor pairs)";
        return FH_ERR_STATE;
    }
    for (int k = 0; k < 2; ++k)
        out[k] = fh_roc_point{pt[k].threshold, pt[k].bin, pt[k].true_accepts, pt[k].false_accepts, pt[k].genuine, pt[k].impostor};
    return FH_OK;
}
int fh_gallery_pair_hist_dev(fh_gallery* g, unsigned long long* d_hist, unsigned long long* d_nan, void* stream) {
    if (!g || !d_hist) return arg_error("fh_gallery_pair_hist_dev: null argument");
    if (g->g.size() > 0 && !g->g.labelled()) {
        g_err = "gallery: fh_gallery_pair_hist_dev needs a labelled gallery (rows enrolled with ids, or fh_gallery_set_ids)";
        return FH_ERR_STATE;
    }
    return guarded([&] { g->g.pair_hist_dev(d_hist, d_nan, S(stream)); return (int)FH_OK; });
}
int fh_debug_hist_copies(int copies) { fh::cluster_debug_hist_copies(copies); return 0; }

// ---- the pair audit: the rule on the host (pairs_plan.h), the same rule on the pair pass's accumulators (gallery_cluster.hip,
// gallery_pairs.hip)
static_assert(FH_PAIRS_GENUINE == fh::kPairsGenuine && FH_PAIRS_IMPOSTOR == fh::kPairsImpostor && FH_PAIRS_ANY == fh::kPairsAny &&
              FH_PAIRS_ABOVE == fh::kPairsAbove && FH_PAIRS_NOT_ABOVE == fh::kPairsNotAbove && FH_PAIRS_MAX_CAP == fh::kPairsMaxCap &&
              FH_PAIRS_ROOM == fh::kPairsRoom, "facehip.h mirrors pairs_plan.h and kernels.h");
namespace {
const char* bad_pairs(int cls, int side, float threshold, int cap) {
    if (threshold != threshold) return "the threshold is a NaN";
    if (cls != FH_PAIRS_GENUINE && cls != FH_PAIRS_IMPOSTOR && cls != FH_PAIRS_ANY) return "unknown class";
    if (side != FH_PAIRS_ABOVE && side != FH_PAIRS_NOT_ABOVE) return "unknown side";
    if (cap < 1 || cap > FH_PAIRS_MAX_CAP) return "need 1 <= cap <= FH_PAIRS_MAX_CAP";
    return nullptr;
}
}  // namespace
int fh_pairs_from_scores(const float* scores, int n, const int* ids, int cls, int side, float threshold, int cap, long long room,
                         unsigned long long* info, float* out_scores, int* out_rows, int* out_ids) {
    if (const char* why = bad_pairs(cls, side, threshold, cap)) return frames_error("fh_pairs_from_scores", why);
    int listed = -1;
    const int rc = guarded([&] {                                   // (its scratch may run out of memory)
        listed = fh::pairs_from_scores(scores, n, ids, cls, side, threshold, cap, room, info, out_scores, out_rows, out_ids);
        return 0;
    });
    if (rc < 0) return rc;
    return listed < 0 ? arg_error("fh_pairs_from_scores: bad argument (n < 0, null scores or info, a class without ids, room < cap)") : listed;
}
int fh_gallery_pairs_dev(fh_gallery* g, int cls, int side, float threshold, int cap, unsigned long long* d_info, float* d_scores, int* d_rows,
                         int* d_ids, void* stream) {
    if (!g || !d_info) return arg_error("fh_gallery_pairs_dev: null argument");
    if (const char* why = bad_pairs(cls, side, threshold, cap)) return frames_error("fh_gallery_pairs_dev", why);
    if (g->g.dim() % 64) return arg_error("fh_gallery_pairs_dev: the gallery's dim must be a multiple of 64");
    if ((cls != FH_PAIRS_ANY || d_ids) && g->g.size() > 0 && !g->g.labelled()) {
        g_err = "gallery: fh_gallery_pairs_dev with a class other than FH_PAIRS_ANY or with d_ids needs a labelled gallery (rows enrolled with "
                "ids, or fh_gallery_set_ids)";
        return FH_ERR_STATE;
    }
    return guarded([&] { g->g.pairs_dev(cls, side, threshold, cap, d_info, d_scores, d_rows, d_ids, S(stream)); return (int)FH_OK; });
}
int fh_debug_pairs_room(int room) { fh::pairs_debug_room(room); return 0; }

// ---- threshold search: the rule on the host (range_plan.h), the same rule on the scan's accumulators (gallery_range.hip)
static_assert(FH_RANGE_MAX_CAP == fh::kRangeMaxCap && FH_TAG_ALL == fh::kRangeTagAll, "facehip.h mirrors range_plan.h");
int fh_range_from_scores(const float* scores, long long n, long long index_base, const uint32_t* tags, uint32_t mask, float threshold, int cap,
                         long long* count, float* out_scores, int* out_indices) {
    int listed = -1;
    const int rc = guarded([&] {                                   // (its scratch may run out of memory)
        listed = fh::range_from_scores(scores, n, index_base, tags, mask, threshold, cap, count, out_scores, out_indices);
        return 0;
    });
    if (rc < 0) return rc;
    return listed < 0 ? arg_error("fh_range_from_scores: bad argument (null scores or count, NaN threshold, cap outside 1..1024, index beyond 31 bits)")
                      : listed;
}
int fh_gallery_range_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks, int nq, float threshold, int cap, long long* d_counts,
                         float* d_scores, int* d_indices, int* d_ids, void* stream) {
    if (!g) return arg_error("fh_gallery_range_dev: null handle");
    if (nq < 0 || nq > 256) return arg_error("fh_gallery_range_dev: need 0 <= nq <= 256");
    if (cap < 1 || cap > FH_RANGE_MAX_CAP) return arg_error("fh_gallery_range_dev: need 1 <= cap <= FH_RANGE_MAX_CAP");
    if (threshold != threshold) return arg_error("fh_gallery_range_dev: the threshold is a NaN");
    if (g->g.dim() % 64) return arg_error("fh_gallery_range_dev: the gallery's dim must be a multiple of 64");
    if (nq == 0) return 0;
    if (!d_queries || !d_counts) return arg_error("fh_gallery_range_dev: null argument");
    if (d_ids && g->g.size() > 0 && !g->g.labelled()) {
        g_err = "gallery: fh_gallery_range_dev with d_ids needs a labelled gallery (rows enrolled with ids, or fh_gallery_set_ids)";
        return FH_ERR_STATE;
    }
    return guarded([&] { g->g.range_dev(d_queries, d_masks, nq, threshold, cap, d_counts, d_scores, d_indices, d_ids, S(stream)); return nq; });
}

// ---- deep top-k: the rule and the block rule on the host (deep_plan.h), the same on the scan's accumulators (gallery_deep.hip)
static_assert(FH_TOPK_DEEP_MAX == fh::kDeepMaxK && FH_TOPK_DEEP_MAX == fh::GAL_DEEP_MAX, "facehip.h and kernels.h mirror deep_plan.h");
int fh_topk_from_scores(const float* scores, long long n, long long index_base, const uint32_t* tags, uint32_t mask, int k, float* out_scores,
                        int* out_indices) {
    int listed = -1;
    const int rc = guarded([&] {                                   // (its scratch may run out of memory)
        listed = fh::topk_from_scores(scores, n, index_base, tags, mask, k, out_scores, out_indices);
        return 0;
    });
    if (rc < 0) return rc;
    return listed < 0 ? arg_error("fh_topk_from_scores: bad argument (null scores, k outside 1..1024, index beyond 31 bits)") : listed;
}
int fh_debug_deep_blocks(const float* scores, long long n, const uint32_t* tags, uint32_t mask, int k, long long* out_blocks) {
    if (!out_blocks) return arg_error("fh_debug_deep_blocks: null argument");
    int chosen = -1;
    const int rc = guarded([&] {
        std::vector<long long> blocks;
        chosen = fh::deep_chosen_blocks(scores, n, tags, mask, k, &blocks);
        std::copy(blocks.begin(), blocks.end(), out_blocks);
        return 0;
    });
    if (rc < 0) return rc;
    return chosen < 0 ? arg_error("fh_debug_deep_blocks: bad argument (null scores, k outside 1..1024)") : chosen;
}
int fh_gallery_topk_deep_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks, int nq, int k, float* d_scores, int* d_indices,
                             int* d_ids, void* stream) {
    if (!g) return arg_error("fh_gallery_topk_deep_dev: null handle");
    if (nq < 0 || nq > 256) return arg_error("fh_gallery_topk_deep_dev: need 0 <= nq <= 256");
    if (k < 1 || k > FH_TOPK_DEEP_MAX) return arg_error("fh_gallery_topk_deep_dev: need 1 <= k <= FH_TOPK_DEEP_MAX");
    if (g->g.dim() % 64) return arg_error("fh_gallery_topk_deep_dev: the gallery's dim must be a multiple of 64");
    if (!d_scores && !d_indices && !d_ids) return arg_error("fh_gallery_topk_deep_dev: all three list pointers are null");
    if (nq == 0) return 0;
    if (!d_queries) return arg_error("fh_gallery_topk_deep_dev: null argument");
    if (d_ids && g->g.size() > 0 && !g->g.labelled()) {
        g_err = "gallery: fh_gallery_topk_deep_dev with d_ids needs a labelled gallery (rows enrolled with ids, or fh_gallery_set_ids)";
        return FH_ERR_STATE;
    }
    return guarded([&] { g->g.topk_deep_dev(d_queries, d_masks, nq, k, d_scores, d_indices, d_ids, S(stream)); return nq; });
}

int fh_debug_topk_merge_strided_dev(const float* ps, const int* pi, int nparts, int nq, int k, long long part_stride, float* scores, int* indices,
                                    void* stream) {
    if (!ps || !pi || !scores || !indices) return arg_error("fh_debug_topk_merge_strided_dev: null argument");
    if (nparts <= 0 || nq <= 0 || k <= 0 || k > 16 || (long)nparts * k > 65536 || part_stride < (long long)nq * k)
        return arg_error("fh_debug_topk_merge_strided_dev: bad size");
    return guarded([&] {
        fh::launch_topk_merge_strided(ps, pi, nparts, nq, k, (long)part_stride, scores, indices, S(stream));
        FH_HIP(hipGetLastError());
        return nq;
    });
}

// ---------------------------------------------------------------------------------- timing / tuning
int fh_timing_enable(int on) { fh::KernelTimer::get().enabled = on != 0; return FH_OK; }
int fh_timing_num_tags(void) { return fh::KernelTimer::kTags; }
int fh_timing_collect(double* ms, double* flops, double* bytes, long long* launches, int n) {
    if (!ms || !flops || !bytes || !launches || n < fh::KernelTimer::kTags) return arg_error("fh_timing_collect: need fh_timing_num_tags()-entry arrays");
    return guarded([&] { fh::KernelTimer::get().collect(ms, flops, bytes, launches); return fh::KernelTimer::kTags; });
}
int fh_timing_collect_ops(double* ms, double* flops, int* tag, int cap) {
    if (!ms || !flops || !tag || cap <= 0) return arg_error("fh_timing_collect_ops: bad argument");
    return guarded([&] { return fh::KernelTimer::get().collect_ops(ms, flops, tag, cap); });
}
int fh_det_set_conv_cfg(fh_det* d, int cfg, int stream_k) {
    if (!d) return arg_error("null handle");
    d->det.net().force_cfg = cfg; d->det.net().sk_enable = stream_k != 0;
    return FH_OK;
}
int fh_det_set_winograd(fh_det* d, int on) { if (!d) return arg_error("null handle"); d->det.net().winograd = on != 0; return FH_OK; }
int fh_rec_set_winograd(fh_rec* r, int on) { if (!r) return arg_error("null handle"); r->rec.net().winograd = on != 0; return FH_OK; }
// the fp32 mode's Winograd GEMMs: 1 = three-piece bf16 (six bf16 MFMAs, fp32 results; the default unless FACEHIP_WINO_X3=0), 0 = the native
// f32 MFMA kernels.  Returns the number of layers that have the form (0 with on = 0), or an error code.  Synchronous on first use (the split weights).
int fh_rec_set_wino_x3(fh_rec* r, int on) {
    if (!r) return arg_error("null handle");
    Owns owns(&r->rec.net());
    return guarded([&] { return r->rec.net().set_wino_x3(on != 0, nullptr); });
}
int fh_rec_get_wino_x3(fh_rec* r) { return r && r->rec.net().wino_x3() ? 1 : 0; }
int fh_rec_get_conv_x3(fh_rec* r) { return r ? r->rec.net().conv_x3_layers() : 0; }
int fh_rec_get_pw_x3(fh_rec* r) { return r ? r->rec.net().pw_x3_layers() : 0; }
int fh_rec_get_wino2_x3(fh_rec* r) { return r ? r->rec.net().wino2_x3_layers() : 0; }
// the detector's 1x1 stride-1 convolutions: 1 = three-piece bf16 (conv_pw_x3_kernel where conv_pw_x3_bn / conv_pw_x3_pays admit the launch; the
// default unless FACEHIP_DET_X3=0), 0 = the native f32 kernels everywhere.  Returns the number of layers that have the form (0 with on = 0), or
// an error code.  Synchronous on first use (the split weights).
int fh_det_set_x3(fh_det* d, int on) {
    if (!d) return arg_error("null handle");
    Owns owns(&d->det.net());
    return guarded([&] { return d->det.net().set_pw_x3(on != 0, nullptr); });
}
int fh_det_get_x3(fh_det* d) { return d ? d->det.net().pw_x3_layers() : 0; }
int fh_rec_set_wino_fusion(fh_rec* r, int on) { if (!r) return arg_error("null handle"); r->rec.net().fuse_wino = on != 0; return FH_OK; }
// Opt-in precision mode of the recogniser, gated: the mode is only entered if, on a fixed pseudo-random batch of aligned crops, every
// embedding it produces stays within 1 - cos < 1e-3 of the fp32 path's (north-star tolerance).  Otherwise the handle stays fp32.
int fh_rec_set_precision(fh_rec* r, int mode, float* worst_out) {
    if (!r || (mode != FH_PREC_FP32 && mode != FH_PREC_BF16X2)) return arg_error("fh_rec_set_precision: bad argument");
    if (worst_out) *worst_out = 0.f;
    Owns owns(&r->rec.net());
    if (mode == FH_PREC_FP32) return guarded([&] { r->rec.net().set_bf16x2(false, nullptr); return (int)FH_OK; });
    return guarded([&] {
        fh::Net& net = r->rec.net();
        const int n = 64, dim = r->rec.dim();
        const size_t crop = (size_t)net.in_h() * net.in_w() * 3;
        std::vector<uint8_t> h((size_t)n * crop);
        uint32_t st = 0x9E3779B9u;
        for (int i = 0; i < n; ++i) {                                   // smooth ramp + noise, a different mix per crop
            const int amp = 16 + 3 * i;
            for (size_t e = 0; e < crop; ++e) {
                st = st * 1664525u + 1013904223u;
                const int px = (int)(e / 3) % net.in_w(), py = (int)(e / 3) / net.in_w();
                const int v = 128 + ((px * (i + 1) + py * (n - i)) % 97 - 48) + (int)((st >> 24) % (2 * amp + 1)) - amp;
                h[(size_t)i * crop + e] = (uint8_t)std::min(255, std::max(0, v));
            }
        }
        fh::DevBuf dc, de;
        dc.ensure(h.size()); de.ensure((size_t)2 * n * dim * sizeof(float));
        FH_HIP(hipMemcpy(dc.p, h.data(), h.size(), hipMemcpyHostToDevice));
        const bool was = net.bf16x2();
        net.set_bf16x2(false, nullptr);
        r->rec.embed_aligned_dev(dc.as<uint8_t>(), n, de.as<float>(), nullptr);
        const int layers = net.set_bf16x2(true, nullptr);
        if (layers == 0) { net.set_bf16x2(was, nullptr); throw std::runtime_error("fh_rec_set_precision: this model has no layer with a split-bf16 form"); }
        // from here to the gate the handle is in the mode it has NOT yet been admitted to: anything that throws (the second embed, the
        // synchronise, the read-back) must leave it fp32, as the header promises — the mode is committed only after `worst < gate`
        struct Rollback { fh::Net& n; bool armed = true; ~Rollback() { if (armed) { try { n.set_bf16x2(false, nullptr); } catch (...) {} } } } rollback{net};
        r->rec.embed_aligned_dev(dc.as<uint8_t>(), n, de.as<float>() + (size_t)n * dim, nullptr);
        std::vector<float> e((size_t)2 * n * dim);
        FH_HIP(hipDeviceSynchronize());
        FH_HIP(hipMemcpy(e.data(), de.p, e.size() * sizeof(float), hipMemcpyDeviceToHost));
        double worst = 0;
        for (int i = 0; i < n; ++i) {
            double dot = 0, na = 0, nb = 0;
            for (int c = 0; c < dim; ++c) {
                const double a = e[(size_t)i * dim + c], b = e[(size_t)(n + i) * dim + c];
                dot += a * b; na += a * a; nb += b * b;
            }
            const double err = (na > 0 && nb > 0) ? 1.0 - dot / std::sqrt(na * nb) : 1.0;
            worst = std::max(worst, std::isfinite(err) ? err : 1.0);
        }
        if (worst_out) *worst_out = (float)worst;
        double gate = 1e-3;                                             // FACEHIP_PRECISION_GATE may only TIGHTEN it (tests of the refusal path)
        if (const char* g = getenv("FACEHIP_PRECISION_GATE")) gate = std::min(gate, atof(g));
        if (!(worst < gate))                                            // (the guard above puts the handle back to fp32)
            throw std::runtime_error("fh_rec_set_precision: split-bf16 embeddings differ from fp32 by 1 - cos = " + std::to_string(worst) +
                                 " (gate " + std::to_string(gate) + "): staying fp32");
        rollback.armed = false;
        return layers;
    });
}
int fh_rec_get_precision(fh_rec* r) { return r && r->rec.net().bf16x2() ? FH_PREC_BF16X2 : FH_PREC_FP32; }
int fh_rec_set_shortcut_fold(fh_rec* r, int on) { if (!r) return arg_error("null handle"); r->rec.net().fold_shortcut = on != 0; return FH_OK; }
int fh_det_set_halo_conv(fh_det* d, int on) { if (!d) return arg_error("null handle"); d->det.net().halo_conv = on != 0; return FH_OK; }
int fh_det_set_cus(fh_det* d, int cus) { if (!d || cus < 0) return arg_error("bad argument"); d->det.net().cus = cus; return FH_OK; }
int fh_rec_set_cus(fh_rec* r, int cus) { if (!r || cus < 0) return arg_error("bad argument"); r->rec.net().cus = cus; return FH_OK; }
int fh_det_set_fused_stem(fh_det* d, int on) { if (!d) return arg_error("null handle"); d->det.net().fuse_stem = on != 0; return FH_OK; }
int fh_det_set_fused_front(fh_det* d, int on) { if (!d) return arg_error("null handle"); d->det.net().fuse_front = on != 0; return FH_OK; }
int fh_rec_set_fused_stem(fh_rec* r, int on) { if (!r) return arg_error("null handle"); r->rec.net().fuse_stem = on != 0; return FH_OK; }
int fh_rec_set_conv_cfg(fh_rec* r, int cfg, int stream_k) {
    if (!r) return arg_error("null handle");
    r->rec.net().force_cfg = cfg; r->rec.net().sk_enable = stream_k != 0;
    return FH_OK;
}

// ---------------------------------------------------------------------------------- single kernels
int fh_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    if (!dst || !src) return arg_error("fh_memcpy_d2h: null argument");
    return guarded([&] { FH_HIP(hipDeviceSynchronize()); FH_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return 0; });
}
int fh_resize_u8c3_dev(const uint8_t* src, int sh, int sw, int sstep, uint8_t* dst, int dh, int dw, int dstep, void* stream) {
    if (!src || !dst || sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0) return arg_error("fh_resize_u8c3_dev: bad argument");
    return guarded([&] {
        fh::launch_resize_u8c3(src, (long)sh * sstep, sh, sw, sstep, dst, (long)dh * dstep, dh, dw, dstep, 1, S(stream));
        FH_HIP(hipGetLastError());
        return 0;
    });
}
// Winograd form of one 3x3 stride-1 pad-1 convolution (+bias), for the parity tests: w_ohwi = host weights [cout][3*3][cin];
// precision = FH_PREC_BF16X2: the split-bf16 operand format (U packed here as Net::set_bf16x2 does, V by the input transform)
int fh_conv_winograd_ex_dev(const float* d_in, const float* w_ohwi, const float* d_bias, float* d_out, int batch, int h, int w, int cin,
                            int cout, int precision, void* stream) {
    if (!d_in || !w_ohwi || !d_out || cin % 32 || cout % 4 || (precision != FH_PREC_FP32 && precision != FH_PREC_BF16X2 && precision != FH_PREC_F32X3))
        return arg_error("fh_conv_winograd_dev: bad argument");
    const bool bf2 = precision == FH_PREC_BF16X2, x3 = precision == FH_PREC_F32X3;
    Owns owns(nullptr);                                                  // (no Net: the process-wide watchdog record)
    return guarded([&] {
        if ((bf2 || x3) && !fh::wino_gemm_ok_bf16x2(cin, cout)) throw std::runtime_error("winograd: this layer has no split-bf16 GEMM");
        const int rows = fh::conv_wt_rows(cout);
        std::vector<float> u36((size_t)36 * rows * cin, 0.f), uf((size_t)cout * cin);
        std::vector<double> uall((size_t)cout * cin * 36);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) {
                double g[9];
                for (int t = 0; t < 9; ++t) g[t] = w_ohwi[((size_t)co * 9 + t) * cin + ci];
                fh::wino_filter_transform(g, &uall[((size_t)co * cin + ci) * 36]);
            }
        for (int f = 0; f < 36; ++f) {
            for (size_t e = 0; e < uf.size(); ++e) uf[e] = (float)uall[e * 36 + f];
            fh::conv_pack_weights(uf.data(), cout, cin, 1, u36.data() + (size_t)f * rows * cin);
        }
        const size_t tiles = (size_t)batch * ((h + 3) / 4) * ((w + 3) / 4);
        fh::DevBuf dU, dV, dM;
        dU.ensure(u36.size() * sizeof(float));
        // (+ 100 x 128 rows: the mixed F(4x4) / F(2x2) tiling pads each of its up to 100 planes to whole 128-row GEMM tiles)
        dV.ensure((36 * (size_t)fh::wino_rows((long)tiles) + 100 * 128) * cin * sizeof(float));
        dM.ensure((36 * (size_t)fh::wino_rows((long)tiles) + 100 * 128) * cout * sizeof(float));
        FH_HIP(hipMemcpy(dU.p, u36.data(), u36.size() * sizeof(float), hipMemcpyHostToDevice));
        fh::DevBuf dUp;
        if (bf2) {
            dUp.ensure(u36.size() * sizeof(float));
            fh::launch_pack_bf16x2(dU.as<float>(), dUp.as<float>(), (long)u36.size(), S(stream));
        } else if (x3) {
            dUp.ensure(36 * fh::wino_x3_floats(rows, cin) * sizeof(float));
            fh::launch_pack_x3(dU.as<float>(), dUp.as<float>(), rows, cin, S(stream));
        }
        static fh::DevBuf slabs;
        static unsigned slabs_gen = 0;
        if (!slabs.p) { slabs.ensure(fh::conv_slab_floats() * sizeof(float)); fh::conv_workspace_init(slabs.as<float>()); slabs_gen = fh::conv_error_generation(); }
        if (slabs_gen != fh::conv_error_generation()) { fh::conv_workspace_reset_async(slabs.as<float>(), S(stream)); slabs_gen = fh::conv_error_generation(); }
        fh::ConvArgs a{};
        a.in = d_in; a.bias = d_bias; a.out1 = d_out; a.slabs = slabs.as<float>(); a.sk_enable = 1;
        a.B = batch; a.H = h; a.W = w; a.Ho = h; a.Wo = w; a.Cin = cin; a.Cout = cout; a.ks = 3; a.stride = 1; a.pad = 1;
        a.act = (int)fh::Act::NONE; a.res_mode = (int)fh::ResMode::NONE;
        fh::launch_conv_winograd(a, (bf2 || x3 ? dUp : dU).as<float>(), dV.as<float>(), dM.as<float>(), 2, nullptr, nullptr, S(stream), precision);
        FH_HIP(hipStreamSynchronize(S(stream)));                 // the workspaces die with this scope
        return 0;
    });
}
int fh_conv_winograd_dev(const float* d_in, const float* w_ohwi, const float* d_bias, float* d_out, int batch, int h, int w, int cin,
                         int cout, void* stream) {
    return fh_conv_winograd_ex_dev(d_in, w_ohwi, d_bias, d_out, batch, h, w, cin, cout, FH_PREC_FP32, stream);
}
// fp32 words -> split-bf16 words (winograd.hip wino_pack_bf16x2), for the format test.  Synchronous.
int fh_debug_pack_bf16x2_dev(const float* d_in, float* d_out, long long n) {
    if (!d_in || !d_out || n < 0 || n % 4) return arg_error("fh_debug_pack_bf16x2_dev: bad argument (n % 4 == 0)");
    return guarded([&] {
        fh::launch_pack_bf16x2(d_in, d_out, (long)n, nullptr);
        FH_HIP(hipGetLastError());
        FH_HIP(hipStreamSynchronize(nullptr));
        return 0;
    });
}
// The GEMM stage of the Winograd form alone.  Rows of V / M for a layer of `batch` h x w maps: the uniform tiling's 36 planes of
// wino_rows(tiles) rows, or (mixed) the mixed tiling's planes; < 0 where the arguments are bad or the mixed layout does not apply.
static long long wino_gemm_rows(int batch, int h, int w, int k, int n, int mixed, fh::WinoPlanes* pl) {
    if (batch <= 0 || h <= 0 || w <= 0 || k <= 0 || n <= 0 || k % 32 || n % 32) return -1;
    if (!mixed) return 36LL * fh::wino_rows((long)batch * ((h + 3) / 4) * ((w + 3) / 4));
    fh::WinoPlanes p{};
    if (!fh::wino_mix_layout(batch, h, w, k, n, &p)) return -2;
    if (pl) *pl = p;
    return 128LL * p.total_tiles;
}
long long fh_debug_wino_gemm_rows(int batch, int h, int w, int k, int n, int mixed) {
    const long long r = wino_gemm_rows(batch, h, w, k, n, mixed, nullptr);
    if (r == -2) return arg_error("fh_debug_wino_gemm_rows: the mixed tiling does not apply to this layer");
    if (r < 0) return arg_error("fh_debug_wino_gemm_rows: bad argument (k % 32 == 0, n % 32 == 0)");
    return r;
}
int fh_debug_wino_gemm_dev(const float* d_V, const float* d_U, float* d_M, int batch, int h, int w, int k, int n, int precision, int mixed,
                           void* stream) {
    if (!d_V || !d_U || !d_M || (precision != FH_PREC_FP32 && precision != FH_PREC_BF16X2 && precision != FH_PREC_F32X3))
        return arg_error("fh_debug_wino_gemm_dev: bad argument");
    fh::WinoPlanes pl{};
    const long long rows = wino_gemm_rows(batch, h, w, k, n, mixed, &pl);
    if (rows == -2) return arg_error("fh_debug_wino_gemm_dev: the mixed tiling does not apply to this layer");
    if (rows < 0) return arg_error("fh_debug_wino_gemm_dev: bad argument (k % 32 == 0, n % 32 == 0)");
    const bool bf2 = precision == FH_PREC_BF16X2, x3 = precision == FH_PREC_F32X3;
    Owns owns(nullptr);                                                  // (no Net: the process-wide watchdog record)
    return guarded([&] {
        if ((bf2 || x3) && !fh::wino_gemm_ok_bf16x2(k, n)) throw std::runtime_error("winograd: this layer has no split-bf16 GEMM");
        const size_t nv = (size_t)rows * k, nu = (size_t)36 * fh::conv_wt_rows(n) * k;
        fh::DevBuf dVp, dUp;
        if (bf2) {                                                       // the caller's operands stay f32: packed copies
            dVp.ensure(nv * sizeof(float)); dUp.ensure(nu * sizeof(float));
            fh::launch_pack_bf16x2(d_V, dVp.as<float>(), (long)nv, S(stream));
            fh::launch_pack_bf16x2(d_U, dUp.as<float>(), (long)nu, S(stream));
        } else if (x3) {                                                 // V stays the caller's f32; U split here as Net::set_wino_x3 does
            dUp.ensure(36 * fh::wino_x3_floats(fh::conv_wt_rows(n), k) * sizeof(float));
            fh::launch_pack_x3(d_U, dUp.as<float>(), fh::conv_wt_rows(n), k, S(stream));
        }
        fh::ConvArgs a{};
        a.B = batch; a.H = h; a.W = w; a.Ho = h; a.Wo = w; a.Cin = k; a.Cout = n; a.ks = 3; a.stride = 1; a.pad = 1;
        a.act = (int)fh::Act::NONE; a.res_mode = (int)fh::ResMode::NONE;
        fh::launch_wino_gemm(a, bf2 || x3 ? dUp.as<float>() : d_U, bf2 ? dVp.as<float>() : d_V, d_M, 2, precision, S(stream), mixed ? &pl : nullptr);
        FH_HIP(hipGetLastError());
        FH_HIP(hipStreamSynchronize(S(stream)));                 // the packed copies die with this scope
        return 0;
    });
}
// Fused Winograd F(2x2,3x3) form (conv_wino2.hip) of one 3x3 stride-1 pad-1 convolution, for the parity tests: w_ohwi = host weights
// [cout][3*3][cin]; d_bias [cout] or, with bias_cls, [9][cout]; act = fh::Act; d_slope / d_res optional
int fh_conv_wino2_ex_dev(const float* d_in, const float* w_ohwi, const float* d_bias, const float* d_slope, const float* d_res, float* d_out,
                         float* d_out2, const float* d_s2, const float* d_t2, int n_outs, float* const* d_outs, const int* oc0, const int* oact,
                         int batch, int h, int w, int cin, int cout, int act, int bias_cls, void* stream) {
    if (!d_in || !w_ohwi || batch <= 0 || h <= 0 || w <= 0 || cin != 64 || cout <= 0) return arg_error("fh_conv_wino2_dev: bad argument (cin = 64, positive sizes)");
    if (n_outs < 0 || n_outs > 3 || (n_outs > 0 && (!d_outs || !oc0 || !oact))) return arg_error("fh_conv_wino2_dev: bad merged-output description");
    if (n_outs == 0 && ((!d_out && !d_out2) || cout % 64)) return arg_error("fh_conv_wino2_dev: plain layers need an output and cout % 64 == 0");
    if (d_out2 && (!d_s2 || !d_t2)) return arg_error("fh_conv_wino2_dev: a second output needs its scale and shift");
    Owns owns(nullptr);                                                  // (no Net: the process-wide watchdog record)
    return guarded([&] {
        fh::ConvArgs a{};
        a.in = d_in; a.bias = d_bias; a.slope = d_slope; a.res = d_res; a.out1 = d_out; a.out2 = d_out2; a.s2 = d_s2; a.t2 = d_t2;
        a.B = batch; a.H = h; a.W = w; a.Ho = h; a.Wo = w; a.Cin = cin; a.Cout = cout; a.ks = 3; a.stride = 1; a.pad = 1;
        a.act = act; a.bias_cls = bias_cls; a.res_mode = d_res ? (int)fh::ResMode::SAME : (int)fh::ResMode::NONE;
        a.n_outs = n_outs;
        for (int g = 0; g < n_outs; ++g) { a.outs[g] = d_outs[g]; a.oact[g] = oact[g]; a.oc0[g] = oc0[g]; }
        if (n_outs > 0) a.oc0[n_outs] = oc0[n_outs];
        if (!fh::wino2_ok(a)) throw std::runtime_error("fh_conv_wino2_dev: layer shape not supported by the fused F(2x2) kernel");
        std::vector<float> u(fh::wino2_weight_floats(cin, cout));
        fh::wino2_pack_weights(w_ohwi, cout, cin, u.data());
        fh::DevBuf dU;
        dU.ensure(u.size() * sizeof(float));
        FH_HIP(hipMemcpy(dU.p, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice));
        a.wt = dU.as<float>();
        fh::launch_wino2(a, S(stream));
        FH_HIP(hipGetLastError());
        FH_HIP(hipStreamSynchronize(S(stream)));                 // the weight image dies with this scope
        return 0;
    });
}
int fh_conv_wino2_dev(const float* d_in, const float* w_ohwi, const float* d_bias, const float* d_slope, const float* d_res, float* d_out,
                      int batch, int h, int w, int cin, int cout, int act, int bias_cls, void* stream) {
    return fh_conv_wino2_ex_dev(d_in, w_ohwi, d_bias, d_slope, d_res, d_out, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, batch, h, w,
                                cin, cout, act, bias_cls, stream);
}
// The plain form of the same layer with a precision argument: FH_PREC_FP32 = wino2_kernel, FH_PREC_F32X3 = wino2_x3_kernel on an image
// packed here as the engine packs it (forced: wino2_x3_pays is the engine's question, the form's existence this call's)
int fh_conv_wino2_prec_dev(const float* d_in, const float* w_ohwi, const float* d_bias, const float* d_slope, const float* d_res, float* d_out,
                           float* d_out2, const float* d_s2, const float* d_t2, int batch, int h, int w, int cin, int cout, int act, int bias_cls,
                           int precision, int cus, void* stream) {
    if (!d_in || !w_ohwi || batch <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || cus < 0 || (!d_out && !d_out2) ||
        (precision != FH_PREC_FP32 && precision != FH_PREC_F32X3))
        return arg_error("fh_conv_wino2_prec_dev: bad argument");
    if (d_out2 && (!d_s2 || !d_t2)) return arg_error("fh_conv_wino2_prec_dev: a second output needs its scale and shift");
    if (precision == FH_PREC_F32X3 && !fh::wino2_x3_shape_ok(cin, cout))
        return arg_error("fh_conv_wino2_prec_dev: this layer has no three-piece bf16 form (it needs cin == 64 and cout % 64 == 0)");
    if (cin != 64 || cout % 64) return arg_error("fh_conv_wino2_prec_dev: plain layers need cin == 64 and cout % 64 == 0");
    Owns owns(nullptr);
    return guarded([&] {
        fh::ConvArgs a{};
        a.in = d_in; a.bias = d_bias; a.slope = d_slope; a.res = d_res; a.out1 = d_out; a.out2 = d_out2; a.s2 = d_s2; a.t2 = d_t2;
        a.B = batch; a.H = h; a.W = w; a.Ho = h; a.Wo = w; a.Cin = cin; a.Cout = cout; a.ks = 3; a.stride = 1; a.pad = 1;
        a.act = act; a.bias_cls = bias_cls; a.res_mode = d_res ? (int)fh::ResMode::SAME : (int)fh::ResMode::NONE;
        a.cus = cus;
        const bool x3 = precision == FH_PREC_F32X3;
        if (!(x3 ? fh::wino2_x3_ok(a) : fh::wino2_ok(a))) throw std::runtime_error("fh_conv_wino2_prec_dev: layer shape not supported by the fused F(2x2) kernel");
        std::vector<float> u(x3 ? fh::wino2_x3_weight_floats(cin, cout) : fh::wino2_weight_floats(cin, cout));
        if (x3) fh::wino2_pack_weights_x3(w_ohwi, cout, cin, reinterpret_cast<unsigned short*>(u.data()));
        else fh::wino2_pack_weights(w_ohwi, cout, cin, u.data());
        fh::DevBuf dU;
        dU.ensure(u.size() * sizeof(float));
        FH_HIP(hipMemcpy(dU.p, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice));
        a.wt = dU.as<float>();
        if (x3) fh::launch_wino2_x3(a, S(stream)); else fh::launch_wino2(a, S(stream));
        FH_HIP(hipGetLastError());
        FH_HIP(hipStreamSynchronize(S(stream)));                 // the weight image dies with this scope
        return 0;
    });
}
// wino2_pack_weights_x3 on the host, for the layout tests: dst = 16 * cin * cout * 3 bf16 words
int fh_debug_wino2_pack_x3(const float* w_ohwi, int cout, int cin, unsigned short* dst) {
    if (!w_ohwi || !dst || !fh::wino2_x3_shape_ok(cin, cout))
        return arg_error("fh_debug_wino2_pack_x3: this layer has no three-piece bf16 form (it needs cin == 64 and cout % 64 == 0)");
    return guarded([&] { fh::wino2_pack_weights_x3(w_ohwi, cout, cin, dst); return 0; });
}
// stem_pack_wfrag on the host, for the layout tests: out = cout / 16 * 3 * 64 * 4 dwords
int fh_debug_stem_pack(const float* wf, int cout, unsigned* out) {
    if (!wf || !out || cout <= 0 || cout % 16) return arg_error("fh_debug_stem_pack: bad argument (cout % 16 == 0)");
    return guarded([&] { fh::stem_pack_wfrag(wf, cout, out); return 0; });
}
double fh_debug_wino2_clock_mhz(void) { return fh::wino2_debug_clock_mhz(); }
int fh_conv_wt_rows(int cout) { return fh::conv_wt_rows(cout); }
int fh_conv_pack_weights(const float* w_ohwi, int cout, int cin, int ksize, float* dst_packed) {
    if (!w_ohwi || !dst_packed || cout <= 0 || cin <= 0) return arg_error("fh_conv_pack_weights: bad argument");
    memset(dst_packed, 0, (size_t)fh::conv_wt_rows(cout) * fh::conv_kpad(ksize * ksize * cin) * sizeof(float));
    fh::conv_pack_weights(w_ohwi, cout, cin, ksize, dst_packed);
    return 0;
}
int fh_conv_kpad(int ktot) { return fh::conv_kpad(ktot); }
const float* fh_det_workspace_dev(fh_det* d) { return d ? d->det.net().workspace() : nullptr; }
int fh_set_graph_replay(int on) { g_graph_replay = on != 0; return FH_OK; }
int fh_det_graph_stats(fh_det* d, long long* replays) {
    if (!d) return arg_error("null handle");
    if (replays) *replays = d->gcall.replays;
    return (int)d->gcall.nodes;
}
int fh_rec_graph_stats(fh_rec* r, long long* replays) {
    if (!r) return arg_error("null handle");
    if (replays) *replays = r->gcall.replays + r->gcall_simple.replays;
    return (int)(r->gcall.nodes ? r->gcall.nodes : r->gcall_simple.nodes);
}
int fh_debug_wino_slots(int slots) { fh::wino_debug_slots(slots); return 0; }
int fh_debug_streamk(int drop_publish, int timeout_ms) { fh::conv_debug_streamk(drop_publish, timeout_ms); return 0; }
// conv_plan.h asked without a GPU, with the default switches (ConvKnobs{}); see include/facehip.h for the five questions
int fh_debug_conv_plan(int what, const int* in, int n_in, long long* out, int n_out) {
    static const int BMs[4] = {128, 256, 128, 64}, BNs[4] = {128, 64, 32, 64};
    const fh::ConvKnobs knobs;
    auto need = [&](int ni, int no) { return n_in == ni && n_out == no && out && (in || !ni); };
    auto geom = [&] {       // in: B, H, W, Cin, Cout, ks, stride, pad, n_outs, up2x
        const int Ho = (in[1] + 2 * in[7] - in[5]) / in[6] + 1, Wo = (in[2] + 2 * in[7] - in[5]) / in[6] + 1;
        return fh::ConvGeom{(long)in[0] * Ho * Wo, in[1], in[2], in[3], Ho, Wo, in[4], in[5], in[6], in[7], fh::conv_kpad(in[5] * in[5] * in[3]), in[8],
                            false, false, in[9] != 0, false};
    };
    auto shape_ok = [&] { return in[0] > 0 && in[1] > 0 && in[2] > 0 && in[3] > 0 && in[4] > 0 && in[5] > 0 && in[6] > 0 && in[7] >= 0 && in[10] > 0 &&
                                 in[1] + 2 * in[7] >= in[5] && in[2] + 2 * in[7] >= in[5]; };      // (a non-empty output grid)
    if (what == 0 && need(8, 9) && in[0] >= 0 && in[1] > 0 && in[2] > 0 && in[3] > 0 && in[4] > 0) {
        const fh::ConvSkPlan p = fh::conv_streamk_plan(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7] != 0, knobs);
        const int v[9] = {p.full, p.rem, p.helpers, p.owners, p.fixup, p.units, p.q, p.owner_chunks, p.maxp};
        for (int i = 0; i < 9; ++i) out[i] = v[i];
    } else if (what == 1 && need(11, 1) && shape_ok()) {
        out[0] = fh::conv_pw_bn(geom(), in[10], knobs);
    } else if (what == 2 && need(12, 3) && shape_ok() && in[11] >= -1 && in[11] < 4) {
        const fh::ConvGeom g = geom();
        const int cfg = in[11] < 0 ? fh::conv_pick_cfg(g.M, g.Cout) : in[11], BM = BMs[cfg], BN = BNs[cfg];
        const int tiles_n = (g.Cout + BN - 1) / BN, tiles = (int)((g.M + BM - 1) / BM) * tiles_n;
        fh::ConvTallPlan t{0, 0, 0};
        if (cfg == 1 || cfg == 2) t = fh::conv_tall_plan(g, BM, BN, 32, tiles, tiles_n, in[10], knobs);
        out[0] = t.tiles; out[1] = t.tiles ? t.rows_a : 0; out[2] = t.tiles ? (long long)t.lds : 0;
    } else if (what == 3 && need(4, 2) && in[0] >= 0 && in[1] > in[0] && in[2] > 0 && in[3] > 0) {
        out[0] = out[1] = fh::conv_sk_nparts(in[0], in[2], in[3]);
        for (int r = in[0] + 1; r < in[1]; ++r) {
            const int n = fh::conv_sk_nparts(r, in[2], in[3]);
            if (n < out[0]) out[0] = n;
            if (n > out[1]) out[1] = n;
        }
    } else if (what == 4 && need(0, 2)) {
        out[0] = (long long)fh::SK_SLAB_FLOATS; out[1] = (long long)fh::SK_COUNTERS;
    } else if (what == 5 && need(4, 2) && in[0] >= 0 && in[1] > 0 && in[2] > 0 && in[3] > 0) {
        out[0] = fh::conv_x3_pays(in[0], in[1], in[2], in[3], knobs) ? 1 : 0; out[1] = fh::conv_x3_bn(in[2]);
    } else if (what == 6 && need(11, 3) && shape_ok()) {
        const fh::ConvGeom g = geom();
        const int bn = fh::conv_pw_x3_bn(g, in[10], knobs);
        out[0] = bn; out[1] = bn ? (g.M / 128) * ((g.Cout + bn - 1) / bn) : 0;
        out[2] = bn && fh::conv_pw_x3_pays(out[1], g.Kpad, g.Cout, in[10], knobs) ? 1 : 0;
    } else if (what == 7 && need(4, 1) && in[0] >= 0 && in[1] > 0 && in[2] > 0 && in[3] > 0) {
        out[0] = fh::conv_pw_x3_pays(in[0], in[1], in[2], in[3], knobs) ? 1 : 0;
    } else if (what == 8 && need(2, 1) && in[0] >= 0 && in[1] > 0) {
        out[0] = fh::wino2_x3_pays(in[0], in[1], knobs) ? 1 : 0;
    } else {
        return arg_error("fh_debug_conv_plan: unknown question, wrong array lengths or a non-positive size");
    }
    return n_out;
}
int fh_conv_forward_dev(const float* in, const float* wt, const float* bias, float* out, int batch, int h, int w, int cin, int cout,
                        int ks, int stride, int kpad, int cfg, void* stream) {
    return fh_conv_forward_ex_dev(in, wt, bias, out, batch, h, w, cin, cout, ks, stride, kpad, cfg, FH_PREC_FP32, nullptr, 0, 0, 0, 0, 0, stream);
}
int fh_conv_forward_ex_dev(const float* in, const float* wt, const float* bias, float* out, int batch, int h, int w, int cin, int cout,
                           int ks, int stride, int kpad, int cfg, int precision, const float* sc_in, int sc_h, int sc_w, int sc_c, int sc_stride,
                           int cus, void* stream) {
    return fh_conv_forward_ep_dev(in, wt, bias, out, batch, h, w, cin, cout, ks, stride, kpad, cfg, precision, sc_in, sc_h, sc_w, sc_c, sc_stride, cus,
                                  0, nullptr, stream);
}
int fh_conv_forward_ep_dev(const float* in, const float* wt, const float* bias, float* out, int batch, int h, int w, int cin, int cout,
                           int ks, int stride, int kpad, int cfg, int precision, const float* sc_in, int sc_h, int sc_w, int sc_c, int sc_stride,
                           int cus, int act, const float* res, void* stream) {
    static const char* const no_pw_x3 = "fh_conv_forward_ex_dev: this 1x1 layer has no three-piece bf16 form (it needs stride 1, cin % 4 == 0, "
                                        "cout % 4 == 0, kpad % 32 == 0, whole 128-row tiles and a tile per CU)";
    const bool x3 = precision == FH_PREC_F32X3, pw3 = x3 && ks == 1;
    if (pw3 && in && wt && out && batch > 0 && cin > 0 && cout > 0 && (cin % 4 || cout % 4 || stride != 1 || sc_in || kpad % 32 || kpad < cin))
        return arg_error(no_pw_x3);
    if (!in || !wt || !out || batch <= 0 || (ks != 1 && ks != 3) || cin % 4 || cout <= 0 || stride <= 0 || cus < 0 || (act != 0 && act != 1) ||
        (precision != FH_PREC_FP32 && precision != FH_PREC_F32X3) || (sc_in && (sc_h <= 0 || sc_w <= 0 || sc_c <= 0 || sc_stride <= 0)))
        return arg_error("fh_conv_forward_dev: bad argument");
    if (x3 && !pw3 && !fh::conv_x3_ok(cin, cout))
        return arg_error("fh_conv_forward_ex_dev: this layer has no three-piece bf16 form (it needs cin % 32 == 0 and cout % 64 == 0)");
    Owns owns(nullptr);                                                  // (no Net: the process-wide watchdog record)
    return guarded([&] {
        fh::ConvArgs a{};
        const int pad = ks / 2;
        a.in = in; a.wt = wt; a.bias = bias; a.out1 = out;
        a.B = batch; a.H = h; a.W = w; a.Cin = cin; a.Cout = cout; a.ks = ks; a.stride = stride; a.pad = pad;
        a.Ho = (h + 2 * pad - ks) / stride + 1; a.Wo = (w + 2 * pad - ks) / stride + 1;
        a.Kpad = kpad;
        a.cus = cus;
        a.act = act;
        if (res) { a.res = res; a.res_mode = (int)fh::ResMode::SAME; }
        if (sc_in) {
            if ((a.Ho - 1) * sc_stride >= sc_h || (a.Wo - 1) * sc_stride >= sc_w) throw std::runtime_error("conv: the shortcut's input does not cover the output grid");
            a.sc_in = sc_in; a.sc_H = sc_h; a.sc_W = sc_w; a.sc_C = sc_c; a.sc_stride = sc_stride;
        }
        static fh::DevBuf slabs;                 // test entry point only: one shared workspace
        static unsigned slabs_gen = 0;
        if (!slabs.p) { slabs.ensure(fh::conv_slab_floats() * sizeof(float)); fh::conv_workspace_init(slabs.as<float>()); slabs_gen = fh::conv_error_generation(); }
        if (slabs_gen != fh::conv_error_generation()) { fh::conv_workspace_reset_async(slabs.as<float>(), S(stream)); slabs_gen = fh::conv_error_generation(); }
        a.slabs = slabs.as<float>(); a.sk_enable = 1;
        if (x3) {                                // the weights split here as Net::set_wino_x3 splits them
            static fh::DevBuf w3;
            const int rows = fh::conv_wt_rows(cout);
            FH_HIP(hipStreamSynchronize(S(stream)));                      // (an earlier call's launch may still read w3)
            w3.ensure(fh::wino_x3_floats(rows, kpad) * sizeof(float));
            fh::launch_pack_x3(wt, w3.as<float>(), rows, kpad, S(stream), 1);
            if (pw3) {                           // (forced: conv_pw_x3_pays is the engine's question, the form's existence this call's)
                if (!fh::launch_conv_pw_x3(a, w3.as<float>(), true, S(stream))) throw std::invalid_argument(no_pw_x3);
            } else {
                a.wt = w3.as<float>();
                fh::launch_conv_x3(a, 0, S(stream));
            }
            FH_HIP(hipGetLastError());
            FH_HIP(hipStreamSynchronize(S(stream)));
            return 0;
        }
        fh::launch_conv(a, cfg, S(stream));
        FH_HIP(hipGetLastError());
        return 0;
    });
}

}  // extern "C"

namespace fh {
Gallery& gallery_of(fh_gallery* g) { return g->g; }      // (comm.cpp: the sharded top-k works on the same object)
}
