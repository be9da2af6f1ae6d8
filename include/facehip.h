/* facehip.h — C ABI of libfacehip.so: the MI355X (gfx950) implementation of the
 * detect -> align -> embed -> compare path of cucibala/FaceRecognizeOnnx.
 *
 * This is the drop-in boundary: every entry point names the reference interface it replaces
 * (paths relative to the reference root).  Plain pointers and sizes only; no C++ or torch types.
 * Host-pointer entry points reproduce the reference's batch-1 class API; the *_dev entry
 * points take device pointers (HBM-resident inputs/outputs) and a hipStream_t passed as
 * void*, and are asynchronous on that stream unless stated otherwise.
 *
 * Error convention: functions returning int give >= 0 on success and a negative fh_status on
 * failure; fh_last_error() holds the message of the calling thread's last failure.  Nothing
 * throws across this boundary.  Handles own all device memory; one handle = one device
 * (the device current when it was created) and calls on one handle must not overlap.
 */
#ifndef FACEHIP_H_
#define FACEHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FH_API __attribute__((visibility("default")))

enum fh_status { FH_OK = 0, FH_ERR_ARG = -1, FH_ERR_MODEL = -2, FH_ERR_DEVICE = -3, FH_ERR_STATE = -4 };

/* POD mirror of `struct FaceBox` (src/face_detector.h:8-12): cv::Rect box, float score,
 * cv::Point2f landmarks[5] (left eye, right eye, nose, left mouth, right mouth).  60 bytes. */
typedef struct fh_face {
    int32_t x, y, w, h;
    float score;
    float lm[10];
} fh_face;

typedef struct fh_det fh_det;         /* FaceDetector   (src/face_detector.h:14-43)   */
typedef struct fh_rec fh_rec;         /* FaceRecognizer (src/face_recognizer.h:9-38)  */
typedef struct fh_gallery fh_gallery; /* 1:N extension of compareFaces                */

FH_API const char* fh_version(void);
FH_API const char* fh_last_error(void);
/* Selects the HIP device for subsequently created handles; returns the device count or < 0. */
FH_API int fh_init(int device);

/* ---- host-only introspection (no GPU needed): parse + plan an .onnx, write a text summary. */
FH_API int fh_plan_describe(const char* onnx_path, int default_h, int default_w, char* buf, int cap);
/* The reader's own view of an .onnx file (what loadModel hands to the planner, src/face_detector.cpp:20-90 path), one canonical
 * text line per graph input / output / initializer (name, dtype, dims, element count, fp64 sum, first and last value) / node
 * (op, inputs, outputs, attributes sorted by name).  Exists so that the wire-format reader can be checked against an independent
 * protobuf decoder (tests/test_onnx_pin.py).  Returns the text length (truncated to cap - 1) or < 0. */
FH_API int fh_onnx_dump(const char* onnx_path, char* buf, int cap);

/* ---- FaceDetector ------------------------------------------------------------------------
 * fh_det_create   <- FaceDetector::FaceDetector + loadModel   (src/face_detector.cpp:5-12,20-90)
 *                    NULL on failure (the reference returns false).
 * fh_det_detect   <- FaceDetector::detect                    (src/face_detector.cpp:139-222)
 *                    host BGR u8 image (cv::Mat data/rows/cols/step); returns the number of
 *                    faces written to out (score-descending, <= max_out); 0 for the
 *                    reference's empty-result cases (null/empty image, bad size, unexpected
 *                    output layout).                                                        */
FH_API fh_det* fh_det_create(const char* onnx_path);
FH_API void fh_det_destroy(fh_det* d);
FH_API int fh_det_input_size(const fh_det* d, int* width, int* height);
FH_API int fh_det_num_anchors(const fh_det* d);
FH_API double fh_det_macs_per_frame(const fh_det* d);
FH_API double fh_det_act_bytes_per_frame(const fh_det* d);
FH_API int fh_det_detect(fh_det* d, const uint8_t* bgr, int rows, int cols, int step, float score_thr, float nms_thr,
                         fh_face* out, int max_out);
/* n frames of identical size resident in HBM.  d_out: [n][max_per_frame] fh_face, d_counts: [n]
 * (total survivors per frame; entries beyond max_per_frame are not stored). */
FH_API int fh_det_detect_batch_dev(fh_det* d, const uint8_t* d_frames, int n, int rows, int cols, int step,
                                   long long frame_stride, float score_thr, float nms_thr, fh_face* d_out,
                                   int max_per_frame, int* d_counts, void* stream);
/* Stage hooks for parity tests: run preprocess + network only / read a raw network output
 * (device pointer to [n][rows][cols] fp32, valid until the next call on the handle). */
FH_API int fh_det_run_network_dev(fh_det* d, const uint8_t* d_frames, int n, int rows, int cols, int step,
                                  long long frame_stride, void* stream);
/* Locality tests: the network on a caller-supplied PREPROCESSED input, d_input_nhwc4 = device [n][H][W][4] fp32 with lane 3 = 0
 * (copied into the handle's input tensor; what fh_det_run_network_dev computes with the fused stem off, minus the preprocess). */
FH_API int fh_det_run_input_dev(fh_det* d, const float* d_input_nhwc4, int n, void* stream);
FH_API int fh_det_num_outputs(const fh_det* d);
FH_API const float* fh_det_output_dev(fh_det* d, int index, int* rows, int* cols);
FH_API const float* fh_det_input_dev(fh_det* d);          /* preprocessed input, NHWC with 4 lanes */
FH_API int fh_det_postprocess_dev(fh_det* d, int n, float score_thr, float nms_thr, fh_face* d_out, int max_per_frame,
                                  int* d_counts, void* stream);
/* FaceDetector::postprocess + nms (src/face_detector.cpp:224-338,356-384) on caller-supplied pre-decoded rows:
 * d_rows = [n][rows_per_frame][feat >= 15] fp32 (x1,y1,x2,y2,score,10 kps) in HBM; `scale` is the letterbox scale the
 * reference divides by.  Same kernels as the detector's own post-processing, without a graph in front: for callers that
 * decode elsewhere, and the hook through which the parity tests push crafted rows (ties, zero-area boxes, > 2048
 * survivors) through both branches of the NMS kernel.  Uses one process-wide scratch: calls must not overlap. */
FH_API int fh_postprocess_rows_dev(const float* d_rows, int n, int rows_per_frame, int feat, float scale, float score_thr,
                                   float nms_thr, fh_face* d_out, int max_per_frame, int* d_counts, void* stream);

/* ---- FaceRecognizer ----------------------------------------------------------------------
 * fh_rec_create          <- FaceRecognizer ctor + loadModel (src/face_recognizer.cpp:5-13,21-91)
 * fh_rec_extract         <- extractFeature(image, face)     (src/face_recognizer.cpp:236-304)
 * fh_rec_extract_simple  <- extractFeatureSimple(image)     (src/face_recognizer.cpp:152-234)
 *                           return the feature length written to out (L2-normalised), 0 for the
 *                           reference's empty-vector cases, < 0 on error.
 * fh_compare             <- compareFaces(f1, f2)            (src/face_recognizer.cpp:320-334)  */
FH_API fh_rec* fh_rec_create(const char* onnx_path);
FH_API void fh_rec_destroy(fh_rec* r);
FH_API int fh_rec_input_size(const fh_rec* r, int* width, int* height);
FH_API int fh_rec_feature_dim(const fh_rec* r);
FH_API double fh_rec_macs_per_face(const fh_rec* r);
FH_API double fh_rec_act_bytes_per_face(const fh_rec* r);
FH_API int fh_rec_set_chunk(fh_rec* r, int faces_per_pass);
FH_API int fh_rec_extract(fh_rec* r, const uint8_t* bgr, int rows, int cols, int step, const fh_face* face, float* out,
                          int out_cap);
FH_API int fh_rec_extract_simple(fh_rec* r, const uint8_t* bgr, int rows, int cols, int step, float* out, int out_cap);
FH_API float fh_compare(const float* f1, int n1, const float* f2, int n2);
/* n pre-aligned crops [n][H][W][3] BGR u8 in HBM -> d_out [n][dim] L2-normalised; d_raw (may be
 * NULL) receives the un-normalised network output. */
FH_API int fh_rec_embed_aligned_dev(fh_rec* r, const uint8_t* d_crops, int n, float* d_out, float* d_raw, void* stream);
/* Locality tests: as above from a caller-supplied preprocessed input, device [n][H][W][4] fp32 with lane 3 = 0. */
FH_API int fh_rec_run_input_dev(fh_rec* r, const float* d_input_nhwc4, int n, float* d_emb, float* d_raw, void* stream);
/* Waits for `stream` and reports an error a launch of THIS handle raised after its asynchronous call had already returned (today: a
 * convolution hand-off that timed out, FH_ERR_DEVICE + fh_last_error()).  Such an error is otherwise returned by the next call
 * on the same handle; calls on other handles never see it.  FH_OK when the queued work completed. */
FH_API int fh_det_sync(fh_det* d, void* stream);
FH_API int fh_rec_sync(fh_rec* r, void* stream);
/* alignFace for n faces (d_frame_of[i] = frame index of face i, NULL = identity): writes crops
 * [n][H][W][3] and d_ok[n] (1 warped, 2 crop-resize fallback, 0 empty). */
FH_API int fh_rec_align_dev(fh_rec* r, const uint8_t* d_frames, int rows, int cols, int step, long long frame_stride,
                            const fh_face* d_faces, const int* d_frame_of, int n, uint8_t* d_crops, int* d_ok,
                            void* stream);
/* preprocessed network input of the last pass (NHWC, 4 lanes; only materialised with fh_rec_set_fused_stem(r, 0)) */
FH_API const float* fh_rec_input_dev(fh_rec* r);
FH_API int fh_rec_embed_faces_dev(fh_rec* r, const uint8_t* d_frames, int rows, int cols, int step,
                                  long long frame_stride, const fh_face* d_faces, const int* d_frame_of, int n,
                                  float* d_out, int* d_ok, void* stream);

/* ---- detect -> align -> embed on a batch of HBM-resident frames (the headline metric path).
 * Takes the first min(count, faces_per_frame) faces of each frame (score order) — the reference embeds "for every face"
 * (src/main.cpp:221-238).  d_faces / d_frame_of / d_emb must hold n*faces_per_frame entries; the compacted face list is
 * written front-to-back.  ONE host hand-off: after detect + NMS + selection the face count comes back through pinned memory
 * (the call waits for the detector only), and align + embed are then launched on exactly that many faces — dead slots cost
 * nothing.  Returns the number of faces (>= 0) or < 0; the embeddings are complete when `stream` has drained. */
FH_API int fh_pipeline_run_dev(fh_det* d, fh_rec* r, const uint8_t* d_frames, int n, int rows, int cols, int step,
                               long long frame_stride, float score_thr, float nms_thr, int faces_per_frame,
                               fh_face* d_faces, int* d_frame_of, float* d_emb, void* stream);

/* ---- mixed-size frame batches: detect, align and embed a COLLECTION of images that each have their own size in one call (gallery
 * enrolment from photographs; the reference's per-file flow, src/main.cpp:42,71-72,88-104, over a batch).  The uniform entry points
 * above stay the path for same-size streams.
 * fh_frame  one image: cv::Mat data / rows / cols / step (src/face_detector.cpp:139).  The ARRAY of descriptors is host memory (read
 *           before the call returns); bgr points to DEVICE memory, anywhere and with any alignment (fh_pipeline_run_images: host).
 *           bgr == NULL, rows <= 0 or cols <= 0 is the reference's empty image (src/face_detector.cpp:148-156): that frame yields zero
 *           faces and the call succeeds.  step < cols * 3 on a non-empty frame fails the call with FH_ERR_ARG before anything is
 *           launched.  1 <= n <= 4096.
 * fh_letterbox_plan  host only, no GPU: FaceDetector::preprocess' float arithmetic (src/face_detector.cpp:101-113) — scale =
 *           min((float)in_w / cols, (float)in_h / rows), new_w = (int)((float)cols * scale), new_h likewise.  Returns 1 for a live frame;
 *           0, with *scale = 0 and a 0 x 0 plan, for an empty image or new_w <= 0 || new_h <= 0 ("Invalid resize dimensions",
 *           :109-113).  The uniform and the ragged detector both plan through this one function.  Output pointers may be NULL. */
typedef struct fh_frame { const uint8_t* bgr; int32_t rows, cols, step; } fh_frame;   /* 24 bytes; bgr = DEVICE pointer */
FH_API int fh_letterbox_plan(int rows, int cols, int in_w, int in_h, int* new_w, int* new_h, float* scale);
/* Stage hooks, for the parity tests and for callers that want the canvas.  fh_det_letterbox_ragged_dev: cv::resize + the paste onto the
 * zero canvas (src/face_detector.cpp:117-121) for all n frames in one launch: d_canvas = [n][inH][inW][3] BGR u8 (4-byte aligned), frame
 * i resized to its plan top-left, zeros elsewhere, all zeros for a dead frame.  fh_det_run_network_ragged_dev: that canvas (the
 * handle's own) through the network (:170); read the heads with fh_det_output_dev, fh_det_postprocess_dev then un-scales per frame. */
FH_API int fh_det_letterbox_ragged_dev(fh_det* d, const fh_frame* frames, int n, uint8_t* d_canvas, void* stream);
FH_API int fh_det_run_network_ragged_dev(fh_det* d, const fh_frame* frames, int n, void* stream);
/* FaceDetector::detect (src/face_detector.cpp:139-222) on n frames of ANY sizes: d_out / d_counts / max_per_frame, ordering and
 * truncation exactly as fh_det_detect_batch_dev; every frame's records are divided by its own scale (:255-275); a dead frame's count
 * is 0.  Asynchronous on `stream`; the next call on the handle may follow at once with another descriptor array. */
FH_API int fh_det_detect_ragged_dev(fh_det* d, const fh_frame* frames, int n, float score_thr, float nms_thr, fh_face* d_out,
                                    int max_per_frame, int* d_counts, void* stream);
/* alignFace (src/face_recognizer.cpp:93-133) / alignFace + extractFeature's network pass (:236-304) for n faces on n_frames frames of
 * different sizes: d_frame_of[i] = index into `frames` of face i's image (NULL = identity, as fh_rec_align_dev; n <= n_frames then);
 * crops, d_ok (1 warped, 2 crop-resize fallback, 0 empty — also for a face on an empty frame or with a frame index outside
 * [0, n_frames)) and embeddings as fh_rec_align_dev / fh_rec_embed_faces_dev. */
FH_API int fh_rec_align_ragged_dev(fh_rec* r, const fh_frame* frames, int n_frames, const fh_face* d_faces, const int* d_frame_of,
                                   int n, uint8_t* d_crops, int* d_ok, void* stream);
FH_API int fh_rec_embed_faces_ragged_dev(fh_rec* r, const fh_frame* frames, int n_frames, const fh_face* d_faces, const int* d_frame_of,
                                         int n, float* d_out, int* d_ok, void* stream);
/* fh_pipeline_run_dev on frames of any sizes ("for every face", src/main.cpp:221-238): same selection (first min(count,
 * faces_per_frame) faces per frame), compaction, d_frame_of, host hand-off and return value; dead frames contribute nothing; slots
 * beyond the returned count are not written.  The frame table is built once and shared by the detector and the align. */
FH_API int fh_pipeline_run_ragged_dev(fh_det* d, fh_rec* r, const fh_frame* frames, int n, float score_thr, float nms_thr,
                                      int faces_per_frame, fh_face* d_faces, int* d_frame_of, float* d_emb, void* stream);
/* The enrolment loop over files (src/main.cpp:42,88-104: imread, detect, extractFeature per image) as ONE call on HOST images of any
 * sizes; blocking.  imgs[i].bgr is a HOST pointer here (fh_imread's output fits).  The live images are packed row by row, without
 * padding, into one pinned arena, sent with one copy and run through fh_pipeline_run_ragged_dev; the first min(total, cap) faces /
 * frame indices / embeddings ([cap][dim]) come back (any of the three pointers may be NULL).  Returns the total number of faces.  The
 * arena and the device buffers belong to the fh_det handle and grow on demand. */
FH_API int fh_pipeline_run_images(fh_det* d, fh_rec* r, const fh_frame* imgs, int n, float score_thr, float nms_thr,
                                  int faces_per_frame, fh_face* faces, int* frame_of, float* emb, int cap);

/* ---- tiled detection of large frames.  The detector letterboxes a frame of any size onto its one input canvas, so a face in a
 * 1920 x 1080 or 4K frame reaches the network 3x / 6x smaller.  These calls run the detector on the whole frame AND on overlapping
 * full-resolution tiles of it, and merge everything with ONE NMS per frame.  The existing entry points are unchanged.
 *
 * fh_tile_plan  host only, no GPU; the detector plans through the same function.  Per axis (x shown, y alike), integers only:
 *     cols <= tile_w: one tile at 0, cols wide; otherwise sx = tile_w - overlap, nx = ceil((cols - tile_w) / sx) + 1,
 *     x_j = min(j * sx, cols - tile_w), tile_w wide (the last tile is shifted inward, never cut short).
 *   View 0 is the whole frame (0, 0, cols, rows), edges = 0; if nx * ny > 1 the nx * ny tiles follow, row-major.  fh_view::edges: bit
 *   0 left, 1 top, 2 right, 3 bottom = that edge is INTERIOR (x > 0, y > 0, x + w < cols, y + h < rows).  Returns the view count; 0
 *   for an empty image (rows <= 0 || cols <= 0); FH_ERR_ARG for tile_w or tile_h < 16, overlap < 0, overlap >= min(tile_w, tile_h),
 *   or — with views != NULL — more views than cap.  views == NULL only counts.  border < 0 switches the border rule off.
 *
 * The contract of a tiled detection, for frame f with views v = 0..V-1 of the plan:
 *   1. per view  the view (pixels at bgr + y * step + 3 * x, the frame's step) is the reference's image for FaceDetector::preprocess /
 *      postprocess: letterbox plan fh_letterbox_plan(view.h, view.w, in_w, in_h), candidates by the reference's row loop (strict
 *      score > thr, / scale, (int) truncation, width from the float difference; src/face_detector.cpp:249-278).  A view whose plan is
 *      dead contributes nothing (a frame whose whole view is dead may still have live tiles).
 *   2. border rule, tiles only (never view 0), with b = border >= 0 and the integer box in VIEW coordinates — dropped if:  left edge
 *      interior and x <= b;  right interior and x + w >= view.w - b;  top interior and y <= b;  bottom interior and y + h >= view.h - b.
 *   3. shift, tiles only (view 0 is at the origin and is left as it is): x += view.x, y += view.y as integers; each landmark
 *      coordinate becomes lm + (float)view.x / (float)view.y — one fp32 add after the division.
 *   4. merge  the surviving candidates of ALL views of the frame go through FaceDetector::nms once (integer IoU, strict >, greedy;
 *      :340-384) in the total order (score descending, view index ascending, anchor / row index ascending).  No per-view NMS.
 *   5. output as fh_det_detect_batch_dev: d_out[f][max_per_frame] in that order, d_counts[f] = all survivors, stored or not.
 *   A frame that fits one tile has only view 0: its records are bitwise those of fh_det_detect_ragged_dev.
 * Limits: 1 <= n <= 4096 frames, and at most FH_TILE_MAX_VIEWS views per call IN TOTAL — more returns FH_ERR_ARG before anything is
 * launched; split the batch.  Memory: the views of a call are one ragged batch, so the handle reserves what a ragged batch of that many
 * frames needs (canvas, activations, one [cap] candidate block per view; cap = the power of two >= the anchor count), plus key / flag
 * segments of the power of two >= views * cap per frame.  Asynchronous on `stream`; the next call may follow at once with other tables.
 * What this proves: the composition is exact.  Whether tiling finds faces the plain call misses depends on trained weights. */
#define FH_TILE_MAX_VIEWS 256
typedef struct fh_tiling { int32_t tile_w, tile_h, overlap, border; } fh_tiling;
typedef struct fh_view { int32_t x, y, w, h, edges; } fh_view;
FH_API int fh_tile_plan(int rows, int cols, const fh_tiling* t, fh_view* views, int cap);
FH_API int fh_det_detect_tiled_dev(fh_det* d, const fh_frame* frames, int n, const fh_tiling* t, float score_thr, float nms_thr,
                                   fh_face* d_out, int max_per_frame, int* d_counts, void* stream);
/* Stage hook: plan + letterbox + network on every view; returns the total view count (0: only empty frames).  The heads are read
 * with fh_det_output_dev: one row block per view, in plan order (the views of frame 0, then of frame 1, ...). */
FH_API int fh_det_run_network_tiled_dev(fh_det* d, const fh_frame* frames, int n, const fh_tiling* t, void* stream);
/* fh_postprocess_rows_dev's tiled twin, steps 1 (from the row loop on) to 5 on caller-supplied pre-decoded rows: d_rows =
 * [total views][rows_per_view][feat >= 15] for every view of every frame in plan order; frame_rows / frame_cols = HOST arrays of the
 * n frame sizes (<= 0: an empty frame, no views); in_w x in_h = the network input the view scales are planned for.  The same device
 * code as the detector's, without a graph in front; rows_per_view <= 2^21.  One scratch per calling thread: calls must not overlap. */
FH_API int fh_postprocess_rows_tiled_dev(const float* d_rows, const int* frame_rows, const int* frame_cols, int n_frames,
                                         const fh_tiling* t, int in_w, int in_h, int rows_per_view, int feat, float score_thr,
                                         float nms_thr, fh_face* d_out, int max_per_frame, int* d_counts, void* stream);
/* fh_pipeline_run_ragged_dev over tiled detection: same selection, compaction, d_frame_of, hand-off and return value; the align reads
 * the FRAMES (the faces are in frame coordinates), not the views. */
FH_API int fh_pipeline_run_tiled_dev(fh_det* d, fh_rec* r, const fh_frame* frames, int n, const fh_tiling* t, float score_thr,
                                     float nms_thr, int faces_per_frame, fh_face* d_faces, int* d_frame_of, float* d_emb, void* stream);
/* FaceDetector::detect on ONE host image, tiled (fh_det_detect's arguments and return value); blocking, eager (not graph-captured). */
FH_API int fh_det_detect_tiled(fh_det* d, const uint8_t* bgr, int rows, int cols, int step, const fh_tiling* t, float score_thr,
                               float nms_thr, fh_face* out, int max_out);

/* Two-stream form for streaming callers (the testWebcam loop shape, src/main.cpp:214-258, over batches): detect + decode +
 * NMS + face selection on stream_det, align + embed on stream_rec behind an event.  The host waits for the detector's face
 * count only; a recogniser queued earlier on stream_rec keeps running, so submitting batch k+1 straight after batch k
 * overlaps the HBM-bound detector with the MFMA-bound recogniser.  d_total (device int) also receives the count.  Every
 * buffer passed in (frames included) must stay untouched until stream_rec has drained; give each in-flight batch its own
 * d_faces / d_frame_of / d_emb / d_total.  Returns the number of faces or < 0. */
FH_API int fh_pipeline_submit_dev(fh_det* d, fh_rec* r, const uint8_t* d_frames, int n, int rows, int cols, int step,
                                  long long frame_stride, float score_thr, float nms_thr, int faces_per_frame,
                                  fh_face* d_faces, int* d_frame_of, float* d_emb, int* d_total, void* stream_det,
                                  void* stream_rec);

/* ---- streaming front end for HOST frames: the caller of the path (testWebcam, src/main.cpp:214-258: grab, detect, embed
 * every face) over batches.  The object owns a 2-slot ring of device buffers, a copy stream and a compute stream:
 * fh_stream_submit uploads the batch (tightly packed [n_frames][rows][cols][3] BGR u8; pinned memory makes the copy truly
 * asynchronous) while the previous batch is still computing, queues detect -> align -> embed behind it and returns the
 * batch's face count; fh_stream_collect waits for the OLDEST batch in flight and copies out its first min(count, cap)
 * faces / frame indices / embeddings (any of the three pointers may be NULL).  At most 2 batches in flight. */
typedef struct fh_stream fh_stream;
FH_API fh_stream* fh_stream_create(fh_det* d, fh_rec* r, int frames_per_batch, int rows, int cols, int faces_per_frame);
FH_API void fh_stream_destroy(fh_stream* s);
FH_API int fh_stream_submit(fh_stream* s, const uint8_t* host_frames, int n_frames, float score_thr, float nms_thr);
FH_API int fh_stream_collect(fh_stream* s, fh_face* faces, int* frame_of, float* emb, int cap);

/* ---- face tracker for VIDEO: stable per-camera track ids on the device, and a recogniser that runs once per track instead of once per
 * face per frame.  The entry points above reproduce the webcam loop literally (src/main.cpp:214-258: detect, then embed EVERY face of
 * EVERY frame) and are unchanged.  The tracker sits between the detector's NMS and the face selection; fh_pipeline_run_tracked_dev then
 * aligns and embeds only the faces that OPEN a track, whose track is due for a REFRESH, or that found NO FREE SLOT.  Everything is
 * integers plus FaceDetector::iou (src/face_detector.cpp:340-354: integer intersection and areas, one fp32 division — the function the
 * NMS uses), so the result is defined to the bit.
 *
 * Limits (anything else: FH_ERR_ARG — NULL from fh_tracker_create — before anything is launched, no state changes): 1 <= streams <= 4096,
 * 1 <= max_tracks <= FH_TRACK_MAX, max_missed >= 0, refresh >= 0, 1 <= n <= 4096, per_frame >= 1, every stream_of[f] in [0, streams).
 * Frame order: within one call the frames of a stream are consecutive in time in batch order, and successive calls continue the
 *   stream.  stream_of (HOST memory, read before the call returns; NULL = every frame on stream 0) may interleave cameras freely: a
 *   [t][camera] live batch and one camera's clip are the same case.  The next call may follow at once with another array.
 * fh_track_plan (host only, no GPU) is the stable counting sort the device walks: order[n] = the frame indices grouped by stream,
 *   ascending within a stream; stream s owns order[starts[s] .. starts[s + 1]).  Returns 0 or FH_ERR_ARG.
 * State, per stream, on the device: frame_no (frames ever seen, from 0), next_id (from 0) and max_tracks slots of fh_track_state; a
 *   slot with id = -1 is free.  All counters are int32: a stream of more than 2^31 - 1 frames is outside the contract.
 *
 * The update.  Frame f belongs to stream s and t = that stream's frame_no; its considered detections are j = 0 .. c - 1 in the
 * detector's (score) order, c = min(max(d_counts[f], 0), per_frame).
 *   1. expire  every live slot that has been absent for more than max_missed frames, t - last_seen - 1 > max_missed, is freed: a track
 *              may miss max_missed consecutive frames and still be matched in the next one; after max_missed + 1 it is gone.
 *   2. match   for each j ascending: the candidates are the live slots neither matched nor opened earlier in this frame; a candidate
 *              qualifies when iou(track box, detection box) > iou_thr (strict, so the NaN of 0 / 0 fails); the largest iou wins, ties
 *              go to the smallest track id.  The winner's box becomes the detection's, last_seen = t, hits += 1, d_track[f][j] = id;
 *              d_embed[f][j] = 1 and last_embed = t when refresh > 0 && t - last_embed >= refresh, else d_embed[f][j] = 0.
 *   3. open    an unmatched detection takes the LOWEST free slot: id = next_id++, the detection's box, last_seen = last_embed = t,
 *              hits = 1, d_track[f][j] = id, d_embed[f][j] = 1.  With no free slot the face is untracked: d_track[f][j] = -1,
 *              d_embed[f][j] = 1 (the reference's behaviour: embed it) and no state changes.
 *   4. close   entries j >= c of both outputs are written as (-1, 0); frame_no += 1, also for a frame without detections.
 *   refresh == 0: a track is embedded once, when it opens.  Greedy in score order, as the NMS in front of it.
 * fh_tracker_reset / fh_tracker_get_state are synchronous (they wait for the device).  get_state writes the live slots, ascending, to
 *   the front of host_out[max_tracks] (the rest: id = -1) and returns their number; frame_no / next_id may be NULL.
 * fh_track_select_dev  the flagged twin of the pipeline's face selection: the records with d_embed != 0, densely in (frame, slot)
 *   order, into d_faces with d_frame_of and d_track_of (= d_track of that entry); d_total[0] = their number; room for n * per_frame.
 * fh_pipeline_run_tracked_dev  on `stream`: fh_det_detect_batch_dev with max_per_frame = faces_per_frame into d_all / d_counts (bit
 *   for bit that call's output), the update, the select, the ONE 4-byte hand-off of fh_pipeline_run_dev, then align + embed of exactly
 *   the selected faces.  d_track = [n][F]; d_faces / d_frame_of / d_track_of / d_emb hold up to n * F entries.  Returns the number of
 *   faces embedded.  One tracker serves one pipeline at a time (it owns the flag buffer).  The ragged, tiled, two-stream and fh_stream
 *   forms have no tracked twin yet. */
#define FH_TRACK_MAX 64                      /* track slots per stream (one wave's lanes) */
typedef struct fh_tracker fh_tracker;
typedef struct fh_track_state { int32_t id, x, y, w, h, last_seen, last_embed, hits; } fh_track_state;  /* 32 bytes */
FH_API fh_tracker* fh_tracker_create(int streams, int max_tracks, float iou_thr, int max_missed, int refresh);
FH_API void fh_tracker_destroy(fh_tracker* t);
FH_API int fh_tracker_reset(fh_tracker* t, int stream /* -1: all */);
FH_API int fh_tracker_get_state(fh_tracker* t, int stream, fh_track_state* host_out /*[max_tracks]*/, int* frame_no, int* next_id);
FH_API int fh_track_plan(const int* stream_of, int n, int streams, int* order, int* starts /*[streams+1]*/);
FH_API int fh_track_update_dev(fh_tracker* t, const fh_face* d_det, const int* d_counts, int n, int per_frame,
                               const int* stream_of /*HOST [n] or NULL*/, int* d_track /*[n][per_frame]*/, int* d_embed /*[n][per_frame]*/,
                               void* stream);
FH_API int fh_track_select_dev(const fh_face* d_det, const int* d_embed, int n, int per_frame, fh_face* d_faces, int* d_frame_of,
                               const int* d_track, int* d_track_of, int* d_total, void* stream);
FH_API int fh_pipeline_run_tracked_dev(fh_det* d, fh_rec* r, fh_tracker* t, const uint8_t* d_frames, int n, int rows, int cols, int step,
                                       long long frame_stride, const int* stream_of, float score_thr, float nms_thr, int faces_per_frame,
                                       fh_face* d_all /*[n][F]*/, int* d_counts /*[n]*/, int* d_track /*[n][F]*/, fh_face* d_faces,
                                       int* d_frame_of, int* d_track_of, float* d_emb, void* stream);

/* ---- track identity: a label and a similarity for EVERY face of EVERY frame, what the webcam loop (src/main.cpp:221-238: embed each
 * face, compare, "Match" / "Unknown") produces, from one recogniser run per track.  Each track keeps a running template (the sum of its
 * embeddings, in time order); each newly embedded face is labelled against a gallery THROUGH its track's pooled template, and the answer
 * is carried on the device to every later face of the track until the next refresh replaces it.  Everything but the float normalisation
 * is defined to the bit.
 *
 * fh_track_update_slots_dev  fh_track_update_dev with a third output (fh_track_update_dev is this call with d_slot = NULL; one kernel):
 *   d_slot[f][j] = the slot (lane) that holds the detection's track for a matched or opened detection, -1 for an untracked one and for
 *   j >= c.  All other outputs and the state are bit for bit fh_track_update_dev's.
 * fh_tracker_enable_identity  synchronous; needs dim % 64 == 0, 64 <= dim <= 4096 and a known pool mode (else FH_ERR_ARG, nothing
 *   changes); allocates, per (stream, slot): owner (a track id, -1: none), n_emb, label, score and sum[dim] in fp32.  A second call clears
 *   and re-sizes.  fh_tracker_reset(stream) clears the identity state of that stream too (track ids restart at 0 there).
 * fh_track_identify_dev  called once after each update, in the updates' order and with their stream_of.  d_emb = [total][dim], 16-byte
 *   aligned; row e belongs to the e-th flagged entry (d_embed != 0) in (frame, slot) order — the order fh_track_select_dev writes — and
 *   total is that call's d_total.  A flagged entry of rank >= total is never read, answers (-1, -1.0f) and leaves the state alone.  Three
 *   stages, asynchronous on `stream`:
 *   A. pool   the flagged faces of a stream in time order (fh_track_plan; j ascending within a frame); face e with tid = d_track, slot =
 *             d_slot.  slot < 0 (untracked): the query q_e is emb_e verbatim, no state changes.  owner[slot] != tid: the slot is
 *             (re)opened — owner = tid, n_emb = 1, sum = emb_e, q_e = emb_e verbatim (the same bits, not re-normalised).  Otherwise
 *             n_emb += 1 and, FH_TRACK_POOL_SUM: sum = sum + emb_e (one fp32 add per component, strictly in time order), q_e =
 *             FaceRecognizer::normalize of sum (src/face_recognizer.cpp:306-318: sum / sqrt(sum of squares) when that is > 0, else sum as
 *             it is); FH_TRACK_POOL_LAST: sum = emb_e, q_e = emb_e verbatim.  fh_tracker_queries_dev returns the [total][dim] queries
 *             (a stage hook; valid until the next identify call on the handle).
 *   B. label  the queries, in chunks of at most 256, through fh_gallery_label_ids_dev (a labelled gallery: labels are identity ids) or
 *             fh_gallery_label_dev (labels are row indices): strict > threshold; an empty gallery answers (-1, -1.0f).
 *   C. carry  frames in time order; a flagged entry takes its query's answer, which — if slot >= 0 — also becomes the slot's (label,
 *             score) with owner = tid; an unflagged entry with slot >= 0 gets the slot's current (label, score) (so a track whose
 *             identify call was skipped or cut short by `total` shows what the slot last held); every other entry gets (-1, -1.0f).
 *   FH_ERR_ARG before anything is launched, no state changes: a NULL tracker, gallery or buffer (d_emb may be NULL only when total == 0),
 *   identity not enabled, the gallery's dim != the identity dim, total < 0 or > n * per_frame, and fh_track_update_dev's batch checks.
 * fh_tracker_get_identity  synchronous; the live slots, ascending, in the positions of fh_tracker_get_state (the rest: id = -1), their
 *   sums into sums_out[max_tracks][dim] (may be NULL); returns their number.  A live slot whose identity owner is not its track id —
 *   identify was skipped for it — reports n_emb = 0, label = -1, score = -1.0f (and a zero sum).
 * fh_pipeline_run_identified_dev  fh_pipeline_run_tracked_dev (the same hand-off, the same return value, every output bit for bit) with
 *   the update reporting slots into a buffer of the tracker's, then fh_track_identify_dev on d_emb; the recogniser's feature dim must
 *   be the identity dim (FH_ERR_ARG).  The ragged, tiled, two-stream and fh_stream forms have no identified twin either. */
enum fh_track_pool { FH_TRACK_POOL_LAST = 0, FH_TRACK_POOL_SUM = 1, FH_TRACK_POOL_WEIGHTED = 2 };
typedef struct fh_track_ident { int32_t id, n_emb, label; float score; } fh_track_ident;   /* 16 bytes */
FH_API int fh_track_update_slots_dev(fh_tracker* t, const fh_face* d_det, const int* d_counts, int n, int per_frame, const int* stream_of,
                                     int* d_track, int* d_embed, int* d_slot /*[n][per_frame] or NULL*/, void* stream);
FH_API int fh_tracker_enable_identity(fh_tracker* t, int dim, int pool);
FH_API int fh_track_identify_dev(fh_tracker* t, fh_gallery* g, float threshold, const int* d_track, const int* d_slot, const int* d_embed,
                                 const float* d_emb, int total, int n, int per_frame, const int* stream_of /*HOST [n] or NULL*/,
                                 int* d_label /*[n][per_frame]*/, float* d_score /*[n][per_frame]*/, void* stream);
FH_API const float* fh_tracker_queries_dev(fh_tracker* t);
FH_API int fh_tracker_get_identity(fh_tracker* t, int stream, fh_track_ident* host_out /*[max_tracks]*/,
                                   float* sums_out /*[max_tracks][dim] or NULL*/);
FH_API int fh_pipeline_run_identified_dev(fh_det* d, fh_rec* r, fh_tracker* t, fh_gallery* g, float threshold, const uint8_t* d_frames, int n,
                                          int rows, int cols, int step, long long frame_stride, const int* stream_of, float score_thr,
                                          float nms_thr, int faces_per_frame, fh_face* d_all, int* d_counts, int* d_track, fh_face* d_faces,
                                          int* d_frame_of, int* d_track_of, float* d_emb, int* d_label /*[n][F]*/, float* d_score /*[n][F]*/,
                                          void* stream);

/* ---- face quality and best-shot re-embedding: WHICH frame of a track the recogniser sees.  The tracker above embeds a track when it
 * opens — the frame on which the face enters the picture — and then on a timer.  This section adds a per-face quality score, a tracker
 * policy that embeds a track again when its face has become clearly better than the best one embedded so far, and a quality-weighted
 * template pool.  All of it is opt-in: with the policy off and the old pool modes every entry point above is bit for bit what it was.
 * The score is DEFINED TO THE BIT (integers, plus one fp32 term in a fixed order), so the policy is reproducible; its constants are a
 * proposal whose effect on recognition accuracy nobody has measured.
 *
 * The score.  Frame f, entry j < c, c = min(max(d_counts[f], 0), per_frame), record (x, y, w, h, score, lm[10]):
 *     q = (S * Z * P) >> 8, an int32 >= 0 (at most 1020 * 112 * 256 >> 8);    entries j >= c get 0.
 *   S  sharpness, integers only.  Clip the box to where 4-neighbours exist, in int64 (records can hold anything): x0 = max(x, 1), y0 =
 *      max(y, 1), x1 = min(x + w, cols - 1), y1 = min(y + h, rows - 1).  x1 - x0 < 8 or y1 - y0 < 8: S = 0.  Otherwise the stride is d =
 *      max(1, min(x1 - x0, y1 - y0) / 64) and the samples are px = x0 + i * d < x1, py = y0 + k * d < y1 (i, k = 0, 1, ...).  Luma Y =
 *      (29 * B + 150 * G + 77 * R + 128) >> 8.  At each sample L = |4 * Y(px, py) - Y(px - 1, py) - Y(px + 1, py) - Y(px, py - 1) -
 *      Y(px, py + 1)|: the neighbour distance is 1 whatever the stride — the sharpness of the capture, not of the face's scale.  S =
 *      (sum of L) / (number of samples), an integer division of an int64 sum; 0 <= S <= 1020.  Every read is inside the frame.
 *   Z  size.  Z = min(max(min(w, h), 0), 112): 112 is the recogniser's input side, a larger face adds nothing.
 *   P  pose, fp32 in this order, one division, not contracted (as FaceDetector::iou).  Landmarks in the record's order: left eye le =
 *      lm[0..1], right eye re = lm[2..3], nose = lm[4..5].  dx = |re.x - le.x|; e = dx > 1.0f ? dx : 1.0f; m = (le.x + re.x) * 0.5f;
 *      v = 256.0f * (1.0f - 2.0f * |nose.x - m| / e); P = v > 0 ? min((int)(v < 256.0f ? v : 256.0f), 256) : 0.  A NaN landmark fails
 *      the comparison: P = 0.
 * fh_face_quality_dev  the scores of n uniform frames (frame f at d_frames + f * frame_stride, rows x cols, row pitch step) into
 *   d_quality[n][per_frame], asynchronously on `stream`.  FH_ERR_ARG before anything is launched: a NULL pointer, n outside 1 .. 4096,
 *   per_frame < 1, n * per_frame >= 2^31, rows or cols <= 0, step < cols * 3.
 * fh_face_quality_ragged_dev  the same kernel over frames of any sizes (fh_frame as fh_det_detect_ragged_dev: HOST descriptors of
 *   DEVICE pixels, read before the call returns); an empty frame scores 0 everywhere.  One frame table per calling thread: calls on
 *   different streams are ordered one after the other.
 *
 * The policy.  fh_tracker_set_bestshot(t, on, num, den, min_gap)  synchronous; needs 1 <= den <= num <= 32768 and min_gap >= 1 (else
 *   FH_ERR_ARG, nothing changes).  Allocates one int32 best_q per (stream, slot) and clears it — on every call, whatever `on` is;
 *   fh_tracker_reset(stream) clears that stream's.  on = 0 switches the policy off.
 * fh_track_update_q_dev  fh_track_update_slots_dev with one more input, d_quality[n][per_frame] (fh_track_update_slots_dev is this call
 *   with d_quality = NULL; one kernel).  With d_quality == NULL or the policy off, the outputs and the state are bit for bit
 *   fh_track_update_slots_dev's and best_q is not touched.  With the policy on and qualities given, q = d_quality[f][j], and steps 2
 *   and 3 of the update read:
 *   2. match   ... timer = refresh > 0 && t - last_embed >= refresh (the rule above); better = (int64)q * den > (int64)best_q * num
 *              && t - last_embed >= min_gap; d_embed[f][j] = timer || better.  When it is set: last_embed = t and best_q =
 *              max(best_q, q).  Strict: a face exactly num / den times as good as the best one is not embedded again.
 *   3. open    ... as above (d_embed[f][j] = 1), and best_q[slot] = q.  An untracked face: as above.
 *   TrackState stays 32 bytes: best_q lives beside it.  fh_tracker_get_quality  synchronous; best_q of the live slots, ascending, in the
 *   positions of fh_tracker_get_state (the rest: 0); returns their number; FH_ERR_ARG before fh_tracker_set_bestshot was ever called.
 *
 * The pool.  FH_TRACK_POOL_WEIGHTED for fh_tracker_enable_identity — on a tracker on which fh_tracker_set_bestshot has been called (with
 *   on = 0 or 1: that call is what opts a tracker into the quality feature); on any other tracker the mode stays unknown, FH_ERR_ARG,
 *   nothing changes, as before — and fh_track_identify_q_dev = fh_track_identify_dev plus
 *   d_quality[n][per_frame] (the old call is the new one with NULL).  In stage A, flagged face e with quality q has the weight wq =
 *   (float)max(q, 1).  (Re)opened slot: sum = wq * emb_e, q_e = emb_e verbatim.  Otherwise: sum = sum + wq * emb_e — one fp32 multiply
 *   and one fp32 add per component, not fused, in time order — and q_e = normalize(sum).  WEIGHTED with d_quality == NULL: FH_ERR_ARG
 *   before anything is launched.  The other two modes ignore the array and stay bit for bit as they are.
 *
 * The pipelines.  With the policy on, fh_pipeline_run_tracked_dev and fh_pipeline_run_identified_dev run fh_face_quality_dev on `stream`
 *   between the detector and the update, into a buffer of the tracker's (fh_tracker_quality_dev: a stage hook, [n][F], valid until the
 *   next pipeline call on the handle), call fh_track_update_q_dev and — the identified one — fh_track_identify_q_dev.  With the policy
 *   off nothing new is launched; the identified pipeline then refuses FH_TRACK_POOL_WEIGHTED (FH_ERR_ARG). */
FH_API int fh_face_quality_dev(const uint8_t* d_frames, int n, int rows, int cols, int step, long long frame_stride, const fh_face* d_det,
                               const int* d_counts, int per_frame, int* d_quality /*[n][per_frame]*/, void* stream);
FH_API int fh_face_quality_ragged_dev(const fh_frame* frames, int n, const fh_face* d_det, const int* d_counts, int per_frame,
                                      int* d_quality /*[n][per_frame]*/, void* stream);
FH_API int fh_tracker_set_bestshot(fh_tracker* t, int on, int num, int den, int min_gap);
FH_API int fh_tracker_get_quality(fh_tracker* t, int stream, int* host_out /*[max_tracks]*/);
FH_API const int* fh_tracker_quality_dev(fh_tracker* t);
FH_API int fh_track_update_q_dev(fh_tracker* t, const fh_face* d_det, const int* d_counts, int n, int per_frame, const int* stream_of,
                                 int* d_track, int* d_embed, int* d_slot /*or NULL*/, const int* d_quality /*[n][per_frame] or NULL*/,
                                 void* stream);
FH_API int fh_track_identify_q_dev(fh_tracker* t, fh_gallery* g, float threshold, const int* d_track, const int* d_slot, const int* d_embed,
                                   const int* d_quality /*[n][per_frame] or NULL*/, const float* d_emb, int total, int n, int per_frame,
                                   const int* stream_of, int* d_label, float* d_score, void* stream);

/* ---- track re-linking: a lost track is RESUMED by appearance when its face comes back.  The tracker above associates by IoU alone: a
 * face hidden for more than max_missed frames loses its track, returns under a new id, and its pooled template, n_emb and name start
 * again.  With re-linking on, the first embedding of every newly opened track is compared with the templates of the stream's recently
 * lost tracks, and the new track continues the best one: template, count and chain root carry over, and d_root tells the caller which
 * track ids are one person.  Opt-in: with re-linking off every entry point above is bit for bit what it was.  Everything but the float
 * normalisation of the queries is defined to the bit.  The defaults of the Python layer (link_thr 0.6 = the reference's match
 * threshold, main.cpp:229-233; max_age 150 = five seconds at 30 fps) are a proposal whose effect on accuracy nobody has measured.
 * No spatial or motion gate, no linking across streams (the gallery label does that for enrolled people).
 *
 * fh_tracker_enable_relink(t, memory, link_thr, max_age)  synchronous.  Needs fh_tracker_enable_identity first (else FH_ERR_STATE,
 *   nothing changes), 0 <= memory <= FH_TRACK_LINK_MEMORY, a finite link_thr and max_age > max_missed (else FH_ERR_ARG, nothing
 *   changes).  Allocates, per stream, a table of max_tracks + memory fh_track_link records and one sum[dim] per record.  Rows 0 ..
 *   max_tracks - 1 are the slots' records (their owner, n_emb, label, score and sum ARE the identity state above); the other rows are
 *   the stream's memory of lost tracks.  owner = -1: the row is free; root = the id of the first track of the chain; last_seen = the
 *   frame time t of the last entry that carried the track; links = how many times the chain was resumed.  The call CLEARS the identity
 *   state and the table of every stream (a track that is live then is re-opened by its next embedding).  A second
 *   fh_tracker_enable_identity clears everything and switches re-linking off; fh_tracker_reset(stream) clears that stream's table.
 *   memory = 0 is legal: only records still sitting in slots are candidates.
 * fh_track_identify_link_dev  fh_track_identify_q_dev's arguments (d_quality may be NULL unless the pool is WEIGHTED) plus d_root
 *   [n][per_frame], which must not be NULL.  Re-linking off: fh_track_identify_q_dev, plus d_root = the entry's own track id where
 *   d_slot >= 0, -1 elsewhere.  Re-linking on: stage A below; fh_track_identify_dev / _q_dev then return FH_ERR_STATE (nothing
 *   launched), so that a caller never gets a silently different answer.
 *   t = the update contract's frame time of the entry's frame: identify is called once after each update, so t = the stream's frame_no
 *   after the update minus the number of that stream's frames from this one (included) to the end of the call.  A record is DEAD at t
 *   iff owner != -1 && t - last_seen - 1 > max_missed (the tracker's own expiry rule) and IN REACH iff also t - last_seen - 1 <= max_age.
 *   A. ONE serial walk per stream: its frames in time order, j ascending, all slots interleaved.  For each entry with slot >= 0 and track
 *      id tid, rec = the slot's record:
 *      1. open event: the entry is flagged, rank < total, rec.owner != tid.  Every record of the table — slot rows, this slot's own
 *         included, and memory rows — that is dead at t and in reach is a candidate, scored against emb_e (below).  The best candidate
 *         with score > link_thr (strict) wins: the higher score, then the smaller owner.
 *         no winner: the slot's old record is RETIRED (below) if it is dead at t and in reach, else dropped; the slot opens as above —
 *           owner = tid, n_emb = 1, sum = (wq *) emb_e, q_e = emb_e verbatim — with root = tid, links = 0.
 *         winner c: c is taken out of the table (copied, its row freed); the slot's old record is retired as above unless it was c;
 *           c is installed in the slot with owner = tid, links + 1; root, n_emb and sum are kept, and the face is the next embedding of
 *           a continued track: n_emb += 1 and, SUM / WEIGHTED: sum = sum + (wq *) emb_e, q_e = normalize(sum); LAST: sum = emb_e, q_e =
 *           emb_e verbatim.
 *      2. continued track (flagged, rank < total, rec.owner == tid): as above.
 *      3. then, for EVERY entry with slot >= 0, flagged or not, rank < total or not: if rec.owner == tid, rec.last_seen = t.
 *      4. d_root[f][j] = rec.root if rec.owner == tid, else -1; also -1 for untracked entries and j >= c.
 *      A flagged entry of rank >= total takes no part in 1 and 2, as above.
 *      label, score: stage C runs after stage A, so during the walk a slot's record carries the (label, score) its slot held when the
 *      CALL began — until an open event replaces the record: a record opened without a winner is UNNAMED, (-1, -1.0f); a resumed one
 *      keeps the WINNER's (label, score), as it keeps its root and sum.  Whatever the record carries goes to the memory with it when
 *      it retires (also later in the same call) and is reported there by fh_tracker_get_links.  A slot row itself is named by stage C
 *      of the same call, from the face's own query, as any flagged face; fh_tracker_get_links reports that for the slot rows.
 *      retiring: the record goes to the lowest memory row that is free or no longer in reach at t; if there is none it replaces the row
 *      with the smallest last_seen, ties to the smaller owner; with memory == 0 it is dropped.
 *      score of candidate c against emb_e, to the bit (fp32, not contracted): d = dot(emb_e, sum_c), ss = dot(sum_c, sum_c).  Lane l of
 *      64 owns the 16-byte columns l, l + 64, ... in ascending order; per column acc = acc + (((x0 * y0 + x1 * y1) + x2 * y2) + x3 * y3)
 *      (the form of the pool's sum of squares), acc from 0.0f; the lanes meet in the xor butterfly 32, 16, .., 1 (v = v + v[lane ^ o]).
 *      One wave scores one row at a time.  nrm = sqrtf(ss); c = nrm > 0 ? d / nrm : d; score = (c + 1.0f) * 0.5f.  A NaN never exceeds
 *      the threshold.
 *   B, C. unchanged; of the table stage C writes the slot rows' label and score and nothing else (a row's owner is stage A's: a slot
 *      whose record a link took away later in the call stays free, whatever face stage C saw there last).
 * fh_tracker_get_links  synchronous; the whole table of one stream by row into host_out[max_tracks + memory] and the sums into sums_out
 *   [max_tracks + memory][dim] (may be NULL; zero for a free row); returns the number of rows.  With host_out and sums_out both NULL it
 *   writes nothing and only returns the number of rows (what a caller sizes its buffers by).  FH_ERR_STATE with re-linking off.
 * fh_tracker_roots_dev  a stage hook: the [n][F] roots of the last fh_pipeline_run_identified_dev on a tracker with re-linking on,
 *   which then runs fh_track_identify_link_dev (with the tracker's quality buffer when the best-shot policy is on) into a buffer of the
 *   tracker's; every other output is produced as before.  With re-linking off nothing new is allocated or launched. */
#define FH_TRACK_LINK_MEMORY 256             /* memory rows per stream, at most */
typedef struct fh_track_link { int32_t owner, root, n_emb, label; float score; int32_t last_seen, links, pad; } fh_track_link;  /* 32 bytes */
FH_API int fh_tracker_enable_relink(fh_tracker* t, int memory, float link_thr, int max_age);
FH_API int fh_track_identify_link_dev(fh_tracker* t, fh_gallery* g, float threshold, const int* d_track, const int* d_slot, const int* d_embed,
                                      const int* d_quality /*[n][per_frame] or NULL*/, const float* d_emb, int total, int n, int per_frame,
                                      const int* stream_of, int* d_label, float* d_score, int* d_root /*[n][per_frame]*/, void* stream);
FH_API int fh_tracker_get_links(fh_tracker* t, int stream, fh_track_link* host_out /*[max_tracks + memory] or NULL*/,
                                float* sums_out /*[max_tracks + memory][dim] or NULL*/);
FH_API const int* fh_tracker_roots_dev(fh_tracker* t);

/* ---- gallery (1:N compareFaces): rows are L2-normalised features; scores are (dot+1)/2. */
FH_API fh_gallery* fh_gallery_create(int dim);
FH_API void fh_gallery_destroy(fh_gallery* g);
FH_API int fh_gallery_upload(fh_gallery* g, const float* rows, long long n, int rows_on_device, long long index_base);
FH_API int fh_gallery_topk_dev(fh_gallery* g, const float* d_queries, int nq, int k, float* d_scores, int* d_indices,
                               void* stream);
/* Scan mode of a gallery (default FP32).  F16_RERANK scans an fp16 copy of the rows for 32 candidates per query, re-scores
 * them from the fp32 rows exactly as the fp32 scan does and proves per query that no other row can reach the top-k; a query
 * whose proof fails is answered by the fp32 scan on the device.  fh_gallery_topk_dev, fh_gallery_label_dev and
 * fh_gallery_topk_sharded_dev return the FP32 answer bit for bit (scores and indices, -1 slots included) for finite rows and
 * queries, asynchronously on the caller's stream, capturable into a graph after one call of the same (nq, k); limits as
 * fh_gallery_topk_dev.  Extra device memory: G x dim x 2 bytes.  A gallery holding a non-finite value or one beyond the fp16
 * range (|x| > 65504), or a dim that is not a multiple of 128, is scanned in fp32 whatever the mode. */
enum fh_gallery_scan { FH_GAL_SCAN_FP32 = 0, FH_GAL_SCAN_F16_RERANK = 1 };
/* Synchronous.  F16_RERANK builds an fp16 copy of the rows already uploaded / enrolled (and keeps it in step with later
 * upload / enroll calls) beside the fp32 rows; FP32 frees it.  FH_ERR_ARG for an unknown mode or a NULL handle. */
FH_API int fh_gallery_set_scan(fh_gallery* g, int mode);
FH_API int fh_gallery_get_scan(const fh_gallery* g);
/* Waits for the handle's queued calls; number of queries answered by the certified fp16 path and by the fp32 fallback
 * since the last call of this function (which resets both). */
FH_API int fh_gallery_scan_stats(fh_gallery* g, long long* certified, long long* fallback);
/* Merge step of a row-SHARDED gallery (one shard per rank): d_part_scores / d_part_idx = [nparts][nq][k]
 * per-shard top-k lists (global row indices, -1 = empty slot) as one all-gather delivers them -> the overall top-k by
 * (score desc, index asc), the same total order and the same kernel fh_gallery_topk_dev finishes with, so a sharded
 * gallery returns exactly the single-gallery answer.  nparts * k <= 65536. */
FH_API int fh_topk_merge_dev(const float* d_part_scores, const int* d_part_idx, int nparts, int nq, int k, float* d_scores,
                             int* d_indices, void* stream);
/* ---- the exchange step of a row-sharded gallery behind the boundary (the reference's compareFaces loop,
 * src/face_recognizer.cpp:320-334 / src/main.cpp:221-238, over a gallery split across the GPUs of one node).  One process (or
 * thread) per rank; the collectives are RCCL (librccl, loaded on first use) on the CALLER's stream — no torch, no host copy.
 *   fh_comm_unique_id   rank 0 fills a 128-byte id; the caller hands it to the other ranks (any side channel: MPI, a file,
 *                       torch.distributed's store ...).
 *   fh_comm_create      binds this process to `device` (hipSetDevice) and joins the communicator; collective over all ranks.
 *                       Create it BEFORE the first fh_* object of the process where possible (RCCL sizes its buffers once).
 *   fh_gallery_topk_sharded_dev
 *                       every rank passes its nq_local query rows [nq_local][dim] (device) and its gallery shard `g` (uploaded
 *                       with its global index base): all-gather of the queries -> scan of the local shard for all
 *                       world * nq_local queries -> ONE all-gather of the per-rank (score, global index) lists -> merge
 *                       (the kernel fh_gallery_topk_dev finishes with).  d_scores / d_indices = [world * nq_local][k] on EVERY
 *                       rank, rank r's own queries in rows [r * nq_local, (r + 1) * nq_local): exactly the single-gallery
 *                       answer (score desc, index asc).  All ranks must call it with the same nq_local and k.  Asynchronous
 *                       on `stream`.  Returns world * nq_local, or < 0. */
#define FH_COMM_ID_BYTES 128
typedef struct fh_comm fh_comm;
FH_API int fh_comm_unique_id(unsigned char id[FH_COMM_ID_BYTES]);
FH_API fh_comm* fh_comm_create(int rank, int world, const unsigned char id[FH_COMM_ID_BYTES], int device);
FH_API void fh_comm_destroy(fh_comm* c);
FH_API int fh_comm_rank(const fh_comm* c);
FH_API int fh_comm_world(const fh_comm* c);
/* all-gather of equally sized float blocks on the caller's stream: d_recv = [world][count] (the frame-sharded callers use it for
 * per-rank embeddings; the sharded top-k uses it internally) */
FH_API int fh_comm_allgather_f32_dev(fh_comm* c, const float* d_send, float* d_recv, long long count, void* stream);
FH_API int fh_gallery_topk_sharded_dev(fh_gallery* g, fh_comm* c, const float* d_queries_local, int nq_local, int k,
                                       float* d_scores, int* d_indices, void* stream);
/* The webcam loop's reference handling (src/main.cpp:211-212,229-233,253-256) for an enrolled SET instead of one
 * refFeature: enroll appends rows (the 's' key; returns the index of the first new row), label gives every query its
 * best row when (dot+1)/2 > threshold ("Match", reference threshold 0.6, strict) and -1 otherwise ("Unknown");
 * d_scores[q] = the best mapped score (-1 for an empty gallery). */
FH_API long long fh_gallery_enroll(fh_gallery* g, const float* rows, long long n, int rows_on_device);
FH_API long long fh_gallery_size(fh_gallery* g);
FH_API int fh_gallery_label_dev(fh_gallery* g, const float* d_queries, int nq, float threshold, int* d_labels,
                                float* d_scores, void* stream);

/* ---- labelled gallery: every row carries an identity id (int32 >= 0, chosen by the caller: arbitrary, neither dense nor sorted),
 * real enrolments hold several templates per person, and the identity queries answer with k different PEOPLE where
 * fh_gallery_topk_dev answers with k rows.
 *   kind      a gallery is labelled or unlabelled: the first *_ids enrol or upload into an empty gallery makes it labelled.  A mix
 *             is an error, not a guess: fh_gallery_enroll / fh_gallery_upload on a non-empty labelled gallery, fh_gallery_enroll_ids
 *             on a non-empty unlabelled one, and the identity queries, fh_gallery_get_ids and fh_gallery_remove_ids on a non-empty
 *             unlabelled one return FH_ERR_STATE and change nothing.  fh_gallery_upload_ids replaces everything and makes the gallery
 *             labelled; an emptied gallery takes either kind.  A negative id returns FH_ERR_ARG and nothing changes.  rows and ids
 *             are both host or both device pointers.
 *   scores    exactly fh_gallery_topk_dev's fp32 score of the row; entry (s, r) is better than (s', r') iff s > s', or s == s' and
 *             r < r' (r = global row index); NaN scores are never listed.
 *   topk_ids  an identity is represented by its best row; the answer is the first k representatives: d_scores / d_ids / d_rows
 *             (may be NULL) = [nq][k] (score, identity id, representative's global row index), empty slots (-1.0f, -1, -1).
 *             Limits as fh_gallery_topk_dev (1 <= k <= 16, nq <= 256, dim % 64 == 0); asynchronous on `stream`, capturable into
 *             a graph after one call of the same (nq, k).  With k > 1 it ALWAYS runs the fp32 scan, whatever the scan mode (the 32
 *             row candidates of F16_RERANK cannot certify an identity list); fh_gallery_scan_stats counts those queries as
 *             fall-backs.  k == 1 and label_ids are the row top-1 of the scan mode plus its id.
 *   label_ids d_ids[q] = the best identity's id when the best score is strictly above the threshold, else -1; d_scores as
 *             fh_gallery_label_dev.
 *   remove    fh_gallery_remove_ids removes every row whose id is in the host list and returns the number of rows removed (unknown
 *             ids: 0; duplicates in the list are harmless).  Synchronous, like enroll.  The compaction is stable: surviving rows
 *             keep their order and move down, so the global indices of later rows shrink; index_base stays.  It goes through a
 *             second buffer: transiently the surviving rows (fp32, ids, the fp16 copy of F16_RERANK) are held twice, plus 4 bytes
 *             per surviving row.  After removing everything the gallery is empty: queries answer -1, enrolment starts afresh.
 *   get_ids   the ids of rows [first, first + n) by position (persistence, tests; fh_gallery_get_rows returns the rows); returns n.
 *   merge_ids the merge step of a row-SHARDED labelled gallery: part w = the identity top-k of shard w, [nparts][nq][k] in three
 *             planes as topk_ids writes them -> the identity top-k of the union (per-part lists suffice: an identity of the answer
 *             is listed, with its representative, by the part that holds it).  nparts * k <= 65536. */
FH_API long long fh_gallery_enroll_ids(fh_gallery* g, const float* rows, const int* ids, long long n, int on_device);
FH_API int fh_gallery_upload_ids(fh_gallery* g, const float* rows, const int* ids, long long n, int on_device, long long index_base);
FH_API int fh_gallery_topk_ids_dev(fh_gallery* g, const float* d_queries, int nq, int k, float* d_scores, int* d_ids, int* d_rows,
                                   void* stream);
FH_API int fh_gallery_label_ids_dev(fh_gallery* g, const float* d_queries, int nq, float threshold, int* d_ids_out, float* d_scores,
                                    void* stream);
FH_API long long fh_gallery_remove_ids(fh_gallery* g, const int* ids_host, long long n_ids);
FH_API long long fh_gallery_get_ids(fh_gallery* g, long long first, long long n, int* ids_host_out);
FH_API int fh_topk_merge_ids_dev(const float* d_part_scores, const int* d_part_ids, const int* d_part_rows, int nparts, int nq, int k,
                                 float* d_scores, int* d_ids, int* d_rows, void* stream);

/* ---- template pooling: one row per PERSON.  A labelled gallery keeps every template as a row for ever: the scan grows with templates,
 * not with people, and an identity list (k > 1) is closed to F16_RERANK.  fh_gallery_fuse_ids builds, on the device, the gallery that
 * holds one row per identity — the L2-normalised sum of that identity's rows — so that the identity top-k IS the row top-k
 * (fh_gallery_topk_dev / fh_gallery_topk_ids_dev) of a gallery T times smaller, in either scan mode; pooling changes scores by design.
 *   group_ids   host only, no GPU, and the one place the grouping is defined (fuse_ids groups through it): order[n] = the row positions
 *               sorted by (id ascending, position ascending), uniq[m] = the distinct ids, ascending, starts[m + 1] = each identity's
 *               offset into order; returns m.  Any of the three output pointers may be NULL.  A negative id (or n > 2^31 - 1) returns
 *               FH_ERR_ARG; n == 0 returns 0.
 *   fuse_ids    dst is replaced entirely, as by fh_gallery_upload_ids with index base 0: a labelled gallery of m rows in ascending id
 *               order, row j carrying uniq[j]; returns m.  Synchronous, like remove_ids, and like it waits first for the work queued on
 *               both handles (an empty src needs no wait: nothing is read, freed or rewritten, dst only forgets its rows).  fp32 throughout, and the ORDER of the additions is part of the contract, so a result reproduces bit for
 *               bit: an identity with one template keeps that row verbatim (the same bits, not re-normalised, in both modes); otherwise
 *               the identity's rows, in row order, are cut into chunks of FH_FUSE_CHUNK rows, each chunk is summed sequentially from its
 *               first row (p = row0; p = p + row1; ...), and the chunk partials are added sequentially in chunk order.  FH_FUSE_SUM
 *               stores that sum (for callers that keep running sums, and for exact tests); FH_FUSE_UNIT applies FaceRecognizer::normalize
 *               (src/face_recognizer.cpp:306-318): divided by sqrt(sum s^2) when that is > 0, else left as it is (a cancelled sum stays
 *               zero, a NaN stays NaN).  dst keeps its scan mode; with F16_RERANK its fp16 copy, bounds and bad-value flag are rebuilt as
 *               upload does.  The argument and state errors change nothing: NULL handle, src == dst, unequal dims or an unknown mode ->
 *               FH_ERR_ARG; a non-empty unlabelled src -> FH_ERR_STATE.  Past those checks a failure leaves dst undefined until its next
 *               upload or fuse (its buffers may have grown and its ids been rewritten): FH_ERR_DEVICE for a failed allocation, copy or
 *               launch, FH_ERR_STATE for a src whose device ids cannot be grouped (a negative id, which no entry point lets in, or more
 *               than 2^31 - 1 rows) or a host allocation that failed.  An empty src empties dst and returns 0.  Transient device memory: 4 bytes per src row,
 *               16 bytes per work item, one scratch row per chunk of an identity longer than one chunk.  The ids are grouped on the host
 *               (a sort) and that sort IS the call's time: measured at 1 M x 512 with 8 templates per identity, 52 ms for the call, the
 *               sum kernel 0.43 - 0.48 ms of it (profiles/gallery_fuse.md) — a maintenance call that sits beside remove_ids, not a
 *               per-frame one.  Fusion is PER GALLERY: a sharded deployment fuses first and shards the fused gallery; fusing each shard
 *               would leave a person whose templates straddle shards with one row per shard.
 *   get_rows    the fp32 rows [first, first + n) by position, of either kind of gallery (persistence next to get_ids; tests); argument
 *               and range checks as fh_gallery_get_ids; returns n.
 *   self_scores the mislabel audit: d_scores[r] (device, one float per row of src) = (dot(src row r, the row of tmpl whose id is src's
 *               id of row r) + 1) / 2 in fp32, -1.0f when tmpl has no such id; a template that is somebody else's face scores far
 *               below its identity's other rows.  tmpl must be the result of fh_gallery_fuse_ids, possibly after fh_gallery_remove_ids
 *               (which keeps ids distinct and ascending): the handle remembers that, upload and enroll forget it, and any other tmpl
 *               returns FH_ERR_STATE, as does a non-empty unlabelled src.  NULL or unequal dims -> FH_ERR_ARG.  Asynchronous on `stream`;
 *               returns FH_OK. */
#define FH_FUSE_CHUNK 512
enum fh_gallery_fuse { FH_FUSE_UNIT = 0, FH_FUSE_SUM = 1 };
FH_API long long fh_gallery_group_ids(const int* ids, long long n, int* order, long long* starts, int* uniq);
FH_API long long fh_gallery_fuse_ids(fh_gallery* src, fh_gallery* dst, int mode);
FH_API long long fh_gallery_get_rows(fh_gallery* g, long long first, long long n, float* rows_host_out);
FH_API int fh_gallery_self_scores_dev(fh_gallery* src, fh_gallery* tmpl, float* d_scores, void* stream);

/* ---- unsupervised grouping: rows in, one identity label per row out (exact DBSCAN).  Everything above needs ids that come from outside;
 * the embeddings of a photo collection, the pooled templates of the tracker's tracks and the "Unknown" faces of the identified pipeline
 * have none.  The output feeds the calls above: fh_gallery_set_ids -> fh_gallery_fuse_ids (one row per person), fh_gallery_self_scores_dev.
 *   cluster_scores  host only, no GPU, and the one place the rule is defined.  scores[n][n] row-major; labels[n]; info[4] or NULL.
 *               edge    (i, j), i != j, iff s(i, j) > threshold: strict, in fp32, so a NaN score and a NaN threshold give no edge.  Only
 *                       the entries with i < j are read: the matrix is taken as symmetric; the self pair is never an edge.
 *               core    deg(i) = the number of edges at i; row i is core iff deg(i) + 1 >= min_pts (the row counts itself).  min_pts == 1
 *                       makes every row core: plain single-linkage connected components.
 *               cluster a connected component of the graph restricted to core rows and core-core edges; its label is the smallest
 *                       position of a core row in it.
 *               border  a non-core row with at least one core neighbour takes the label of its best core neighbour: higher score, then
 *                       lower position (the scan's ranking).  Border rows never link clusters.
 *               noise   every other row: label -1 (FH_CLUSTER_NOISE_NONE) or its own position (FH_CLUSTER_NOISE_SELF; no collision: a
 *                       cluster's label is a core row's position).
 *               info    {clusters, core rows, border rows, noise rows}; the last three sum to n.
 *               Returns the number of clusters; n == 0 returns 0.  FH_ERR_ARG, nothing written: NULL scores or labels with n > 0, n < 0,
 *               min_pts < 1, an unknown noise mode.  All indexing in 64 bits; 16 bytes of host scratch per row.
 *   cluster_dev     exactly cluster_scores on s(i, j) = the fp32 mapped score fh_gallery_topk_dev reports for query = row i against
 *               row j — the v_mfma_f32_32x32x2_f32 chain in k order (k0 = 64 kc + 8 s + e, k1 = k0 + 4), then (acc + 1.0f) / 2.0f — so
 *               "row i and row j are linked" means precisely "the scan scores the pair above the threshold"; the chain is symmetric in
 *               its operands, so s(i, j) and s(j, i) have the same bits and every pair is evaluated once.  d_labels[size] are positions,
 *               0-based (the index base plays no part); ids are ignored (labelled and unlabelled galleries alike); the fp32 rows are
 *               read whatever the scan mode.  Asynchronous on `stream`; returns FH_OK.  An empty gallery writes zeros to d_info and
 *               nothing else.  dim % 64 == 0 as for every scan.  FH_ERR_ARG before anything is launched: the errors of cluster_scores,
 *               a NULL handle or d_labels.  Scratch lives in the handle and grows on demand — 4 bytes (degree) + 4 (union-find parent) +
 *               8 (best core neighbour) per row — and is cleared on `stream` at the start of every call.  Two G x G pair passes (degree,
 *               then link; min_pts == 1 skips the first) and a flatten; labels and counters are identical to the host rule's, not close.
 *   set_ids     replaces the ids of ALL rows by position (ids[size], host or device) and makes an unlabelled gallery labelled;
 *               synchronous like enroll; returns the row count.  An id < 0 returns FH_ERR_ARG and changes nothing.  Clears the handle's
 *               "fused" mark (fh_gallery_self_scores_dev); rows, the fp16 copy and the scan mode are untouched.  The intended flow with
 *               FH_CLUSTER_NOISE_SELF: fh_gallery_cluster_dev -> fh_gallery_set_ids(d_labels, 1) -> fh_gallery_fuse_ids. */
enum fh_cluster_noise { FH_CLUSTER_NOISE_NONE = 0, FH_CLUSTER_NOISE_SELF = 1 };
FH_API int fh_cluster_scores(const float* scores, int n, float threshold, int min_pts, int noise, int* labels, int* info);
FH_API int fh_gallery_cluster_dev(fh_gallery* g, float threshold, int min_pts, int noise, int* d_labels, int* d_info, void* stream);
FH_API long long fh_gallery_set_ids(fh_gallery* g, const int* ids, int on_device);

/* ---- threshold calibration: every decision above is the strict test `score > threshold`; these calls measure, on the caller's own
 * labelled gallery, what a threshold does: exact genuine / impostor score histograms over all pairs of rows, and the operating points
 * read off them.  (What the resulting thresholds mean for recognition accuracy depends on the trained weights: not measured here.)
 *   hist_bin    host only, and the one place the bin rule is defined (the device runs the same function).  FH_HIST_BINS = 2048 bins over
 *               the mapped score: with t = score * 2048.0f (a power of two: exact) it returns -1 for a NaN, 0 for t <= 1, 2047 for
 *               t > 2047 (+inf too), (int)ceilf(t) - 1 otherwise.  Bin b holds b/2048 < s <= (b+1)/2048; bin 0 also everything at or
 *               below 1/2048 (scores <= 0), bin 2047 everything above 2047/2048 (a score a hair above 1).  The half-open side makes the
 *               suffix sum A[b] = sum of h[b'] over b' >= b EXACTLY the number of pairs that `s > b/2048` accepts, for every b in
 *               1..2047 (b/2048 is an exact fp32 value); A[0] counts every non-NaN pair.
 *   roc_from_hist   host only, no GPU.  hist[2][FH_HIST_BINS]: plane 0 genuine, plane 1 impostor; N_g, N_i = the plane sums.
 *               out[0] = the operating point of max_far: the smallest b in 1..2047 with A_i[b] <= (uint64)floor(max_far * (double)N_i);
 *               out[1] = the equal-error point: the smallest b in 1..2047 with FAR_b <= FRR_b, decided in integers
 *               (A_i[b] * N_g <= (N_g - A_g[b]) * N_i in 128 bits).  A point is {threshold = b / 2048.0f, bin = b, true_accepts = A_g[b],
 *               false_accepts = A_i[b], genuine = N_g, impostor = N_i}; one for which no b exists has bin -1, threshold 1.0f and zero
 *               accept counts.  Returns FH_OK; nothing is written on FH_ERR_ARG (NULL pointer, max_far outside [0, 1] or NaN) and on
 *               FH_ERR_STATE (N_g == 0 or N_i == 0).
 *   pair_hist_dev   over all G (G - 1) / 2 unordered pairs of the gallery's fp32 rows, whatever the scan mode: the score of a pair is
 *               exactly the one fh_gallery_topk_dev reports for query = row i against row j (see fh_gallery_cluster_dev: the same pair
 *               pass with another epilogue), binned by hist_bin; a pair is genuine iff the two rows carry the same id.  d_hist
 *               [2][FH_HIST_BINS] and d_nan [2] (may be NULL) are device buffers and are OVERWRITTEN, not accumulated; a NaN-scored pair
 *               is in no bin and is counted per class in d_nan.  So
 *                   sum(hist[0]) + nan[0] = sum over identities of n_id (n_id - 1) / 2,
 *                   sum(hist[0]) + sum(hist[1]) + nan[0] + nan[1] = G (G - 1) / 2.
 *               The index base plays no part.  Asynchronous on `stream`; returns FH_OK.  Before anything is launched: FH_ERR_ARG for a
 *               NULL handle or d_hist, FH_ERR_STATE for a non-empty UNLABELLED gallery (such a caller uses fh_gallery_set_ids first).  An
 *               empty gallery writes zeros and launches nothing else.  dim % 64 == 0 as for every scan.  Scratch (one
 *               histogram, 32 KB) lives in the handle, grows on demand and is cleared on `stream` by every call.  Counts are
 *               identical to the host rule's on the scan's scores, not close.  Pairs are PER GALLERY: cross-shard pairs of a sharded
 *               deployment are out of scope, so such a deployment calibrates on an unsharded sample. */
#define FH_HIST_BINS 2048
typedef struct fh_roc_point {
    float threshold;
    int32_t bin;
    unsigned long long true_accepts, false_accepts, genuine, impostor;
} fh_roc_point;
FH_API int fh_hist_bin(float score);
FH_API int fh_roc_from_hist(const unsigned long long* hist, double max_far, fh_roc_point out[2]);
FH_API int fh_gallery_pair_hist_dev(fh_gallery* g, unsigned long long* d_hist, unsigned long long* d_nan, void* stream);

/* ---- the pair audit: WHICH pairs lie behind a threshold.  The histogram says how many impostor pairs a threshold accepts and how many
 * genuine pairs it rejects; these calls list them.  Impostor pairs above the threshold are people enrolled twice under two ids, or label
 * errors; genuine pairs at or below it are a wrong photo filed under a person, or a ruined template.  The flow: fh_gallery_pair_hist_dev
 * -> fh_roc_from_hist -> the pairs -> fh_gallery_remove_ids / fh_gallery_set_ids / fh_gallery_fuse_ids.
 *   pairs_from_scores   host only, no GPU, and the one place the rule is defined.  scores[n][n] row-major, taken as symmetric: only the
 *               entries with i < j are read.  ids[n] or NULL.
 *               class     a pair (i, j), i < j, is genuine iff ids[i] == ids[j]; cls = FH_PAIRS_GENUINE, FH_PAIRS_IMPOSTOR or
 *                         FH_PAIRS_ANY.  With ids == NULL only FH_PAIRS_ANY is legal.
 *               selected  the pair is in the class, its score is not a NaN, and it passes the side test in fp32: FH_PAIRS_ABOVE
 *                         `s > threshold` (strict: the test of labelling, clustering and range search), FH_PAIRS_NOT_ABOVE
 *                         `s <= threshold`.  A NaN-scored pair of the class is selected by neither side and counted in `nan`, so
 *                         count(ABOVE) + count(NOT_ABOVE) + nan = the class's pairs at any threshold; and at threshold = b / 2048.0f,
 *                         b in 1..2047, count(ABOVE) is the suffix sum A[b] of fh_gallery_pair_hist_dev's plane.
 *               order     most extreme first.  ABOVE: score descending, then i ascending, then j ascending; NOT_ABOVE: score ascending,
 *                         then i, then j.  Scores are compared as fp32 values (a mapped score is never -0).
 *               the cut   bounds the memory and is part of the contract.  Selected pairs are binned by fh_hist_bin; bins are walked
 *                         from the extreme end (2047 downward for ABOVE, 0 upward for NOT_ABOVE); cum(b) = the selected pairs in bins
 *                         at least as extreme as b; want = min(cap, count); b* = the first bin with cum(b*) >= want.  cum(b*) <= room:
 *                         returned = want, complete = 1.  Otherwise returned = cum of the bins strictly more extreme than b* (< cap),
 *                         complete = 0.  Either way the list is EXACTLY the first `returned` entries of the full ordered list: nothing
 *                         approximate is ever returned.  count == 0: returned = 0, complete = 1.
 *               outputs   info[4] = {count, nan, returned, complete}; count is never clipped.  out_scores [cap], out_rows [cap][2]
 *                         (positions i < j), out_ids [cap][2] (the two rows' ids; -1 with ids == NULL): any of them may be NULL.  Slots
 *                         behind `returned` carry (-1.0f, -1, -1).
 *               Returns `returned`.  FH_ERR_ARG, nothing written: n < 0, NULL scores with n > 0, NULL info, a NaN threshold, an unknown
 *               cls or side, a class other than FH_PAIRS_ANY without ids, cap outside 1..FH_PAIRS_MAX_CAP, room < cap.  All indexing in
 *               64 bits.
 *   pairs_dev   exactly pairs_from_scores with room = max(FH_PAIRS_ROOM, cap) on s(i, j) = the fp32 mapped score the scan reports for
 *               query = row i against row j (see fh_gallery_cluster_dev: the same pair pass with two more epilogues), over the fp32
 *               rows whatever the scan mode.  Positions are 0-based: the index base, tags, and the scan and tag statistics play no
 *               part.  d_info [4], d_scores [cap], d_rows [cap][2], d_ids [cap][2] are device buffers; any subset of the three lists
 *               may be NULL (all three: counts only, one pair pass).  Asynchronous on `stream`; returns FH_OK.  Two pair passes — count
 *               (per-bin counters of the selected pairs), then, after a one-workgroup cut, collect (the pairs in the bins the cut
 *               admits, appended through one atomic counter) — and a one-workgroup select that sorts the candidates.  The order in
 *               which candidates are appended depends on timing, the selection is under a total order: two calls with the same inputs
 *               produce identical bytes.  FH_ERR_ARG before anything is launched: a NULL handle or d_info, a NaN threshold, a bad cls,
 *               side or cap, dim % 64 != 0.  FH_ERR_STATE for a non-empty UNLABELLED gallery with a class other than FH_PAIRS_ANY or a
 *               non-NULL d_ids.  An empty gallery writes {0, 0, 0, 1} to d_info and empty lists, and launches nothing else.  Scratch
 *               lives in the handle, grows on demand and is cleared on `stream` by every call: 16 KB of counters, the cut, the counter
 *               and 16 bytes per candidate (1 MB).  When complete == 0 the caller tightens the threshold to the last returned score
 *               and calls again.
 *   out of scope  pairs across two galleries or across shards; tag filtering; cap above 1024; any automatic re-run when complete == 0. */
#define FH_PAIRS_MAX_CAP 1024
#define FH_PAIRS_ROOM 65536
enum fh_pairs_class { FH_PAIRS_GENUINE = 0, FH_PAIRS_IMPOSTOR = 1, FH_PAIRS_ANY = 2 };
enum fh_pairs_side { FH_PAIRS_ABOVE = 0, FH_PAIRS_NOT_ABOVE = 1 };
FH_API int fh_pairs_from_scores(const float* scores, int n, const int* ids /* or NULL */, int cls, int side, float threshold, int cap,
                                long long room, unsigned long long* info, float* out_scores /* [cap] or NULL */,
                                int* out_rows /* [cap][2] or NULL */, int* out_ids /* [cap][2] or NULL */);
FH_API int fh_gallery_pairs_dev(fh_gallery* g, int cls, int side, float threshold, int cap, unsigned long long* d_info,
                                float* d_scores /* [cap] or NULL */, int* d_rows /* [cap][2] or NULL */, int* d_ids /* [cap][2] or NULL */,
                                void* stream);

/* ---- watchlists: row tags and tag-filtered exact 1:N search.  One gallery serves several tenants, doors or lists: every row carries a
 * uint32 TAG (a bit set of up to 32 caller-defined groups), every query a uint32 MASK, and row r is ADMITTED for query q iff
 * (tag[r] & mask[q]) != 0.  The predicate sits inside the scan's admission test, so a tagged query is answered from its admitted rows
 * alone — asking for the top 16 and filtering afterwards is wrong as soon as more than 16 excluded rows outrank the first admitted one.
 *   tags      a gallery whose tags were never set behaves as if every row carried FH_TAG_ALL.  Rows added by fh_gallery_enroll* get
 *             FH_TAG_ALL; fh_gallery_upload* replaces everything and resets all tags to FH_TAG_ALL.  fh_gallery_remove_ids moves the
 *             tags with the rows, in the same stable compaction.  fh_gallery_fuse_ids gives dst row j the OR of the tags of identity
 *             j's rows (a src whose tags were never set leaves dst without tags).  fh_gallery_set_ids, clustering and the pair
 *             histogram ignore tags.  Memory: 4 bytes per row of capacity and 4 bytes per 128 rows, from the first set_tags or tagged
 *             query on.
 *   set_tags  the tags of rows [first, first + n) by position (tags[n], host or device); synchronous, like fh_gallery_set_ids, and like
 *             it waits for the handle's queued work; labelled and unlabelled galleries alike; argument and range checks as
 *             fh_gallery_get_ids (FH_ERR_ARG, nothing changes); returns n.
 *   get_tags  the twin of fh_gallery_get_ids: the tags of rows [first, first + n) into tags_host_out; returns n.
 *   queries   d_masks = device [nq] uint32, read on the device when the call runs (a replayed graph sees the buffer's current contents).
 *             The answer of query q is EXACTLY — scores, indices, ids, rows, bit for bit — the answer the untagged call of the same
 *             name gives on the gallery made of q's admitted rows only, with every listed row keeping its global index in the full
 *             gallery (index_base + position): score bits are the fp32 scan's (a row's score does not depend on its position or its
 *             neighbours), entry order is (score desc, global index asc), NaN is never listed, empty slots are (-1.0f, -1[, -1]); in the
 *             identity forms an identity is represented by its best ADMITTED row.  Mask 0 admits nothing: all slots empty, the label
 *             forms answer (-1, -1.0f) as for an empty gallery.  Limits as fh_gallery_topk_dev (1 <= k <= 16, nq <= 256, dim % 64 == 0);
 *             asynchronous on `stream`, capturable into a graph after one call of the same (nq, k).  Labelled / unlabelled state errors
 *             are those of the untagged twins; a NULL mask pointer returns FH_ERR_ARG.  Tagged queries ALWAYS run the fp32 scan,
 *             whatever the scan mode (the 32 unfiltered fp16 candidates of F16_RERANK certify nothing about a subset — the precedent of
 *             topk_ids with k > 1); fh_gallery_scan_stats counts them as fall-backs.
 *   skipping  the handle keeps the OR of the tags of every 128-row tile, by position; a workgroup of the scan (64 queries) passes over a
 *             tile that has no bit in common with the OR of its 64 masks without reading it, so a selective query against enrolments
 *             GROUPED by tag reads a fraction of the gallery, while scattered tags read all of it.  The answer does not depend on it.
 *   tag_stats waits for the handle's queued work; the (workgroup, row tile) visits that tagged scans multiplied / skipped since the last
 *             call of this function, which resets both; the seed passes of large galleries are included.
 *   sharding  there is no sharded tagged entry point; fh_topk_merge_dev and fh_topk_merge_ids_dev merge per-shard tagged lists unchanged
 *             (a tagged list is a top-k list of a sub-gallery, and the merge never looks at tags).
 *   tracker   fh_tracker_set_stream_masks: masks_host[streams], one watchlist per camera; NULL switches the masks off (the default);
 *             synchronous, the masks are copied to the device.  With masks set, stage B of fh_track_identify_dev (and of the _q, _link
 *             and fh_pipeline_run_identified_dev forms) labels every query — those of untracked faces too — through
 *             fh_gallery_label_ids_tagged_dev / fh_gallery_label_tagged_dev with the mask of the stream its frame belongs to.  Stages A
 *             and C, re-linking and pooling are untouched; with masks off the call issues no extra launch and every output is bit for
 *             bit what it was. */
#define FH_TAG_ALL 0xFFFFFFFFu
FH_API long long fh_gallery_set_tags(fh_gallery* g, long long first, long long n, const uint32_t* tags, int on_device);
FH_API long long fh_gallery_get_tags(fh_gallery* g, long long first, long long n, uint32_t* tags_host_out);
FH_API int fh_gallery_topk_tagged_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks, int nq, int k, float* d_scores,
                                      int* d_indices, void* stream);
FH_API int fh_gallery_topk_ids_tagged_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks, int nq, int k, float* d_scores,
                                          int* d_ids, int* d_rows, void* stream);
FH_API int fh_gallery_label_tagged_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks, int nq, float threshold,
                                       int* d_labels, float* d_scores, void* stream);
FH_API int fh_gallery_label_ids_tagged_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks, int nq, float threshold,
                                           int* d_ids_out, float* d_scores, void* stream);
FH_API int fh_gallery_tag_stats(fh_gallery* g, long long* tiles_scanned, long long* tiles_skipped);
FH_API int fh_tracker_set_stream_masks(fh_tracker* t, const uint32_t* masks_host /*[streams] or NULL*/);

/* ---- threshold search: EVERY row above a score, not the best k <= 16.  "Which rows score above thr for this face, all of them?" — a
 * person enrolled with 20 templates, a watchlist with several matching entries, every photo of one person in an archive, the rows a new
 * enrolment would duplicate.  fh_gallery_pair_hist_dev / fh_roc_from_hist hand the caller a threshold; this is the query behind it.
 *   hit       row r is a hit of query q iff it is ADMITTED (d_masks == NULL, or (tag[r] & mask[q]) != 0; a gallery whose tags were never
 *             set carries FH_TAG_ALL), its mapped score is STRICTLY above the threshold — (dot + 1) / 2 > threshold in fp32, the test
 *             of fh_gallery_label_dev and of the clustering — and its score is not a NaN (a NaN score is never a hit).
 *   scores    the fp32 scan's, bit for bit: the bits fh_gallery_topk_dev returns for that pair, whichever scan mode the gallery is in
 *             (the call always reads the fp32 rows and leaves fh_gallery_scan_stats and fh_gallery_tag_stats alone).
 *   counts    d_counts[q] = the exact number of hits, NOT clipped by cap; written even when all three list pointers are NULL — the
 *             count-only form, which gathers no row.
 *   lists     row q of d_scores / d_indices / d_ids [nq][cap] holds the best min(count, cap) hits ranked as everywhere (score
 *             descending, then global row index ascending); the slots behind them carry (-1.0f, -1, -1); nothing outside [nq][cap] is
 *             written.  Indices are global (index_base + position).  d_ids = each listed row's identity id and needs a labelled gallery
 *             (FH_ERR_STATE otherwise, unless the gallery is empty).  Any subset of the three may be NULL.  A count above cap still
 *             yields the BEST cap hits, not the first.
 *   limits    as fh_gallery_topk_dev: nq <= 256, dim % 64 == 0; 1 <= cap <= FH_RANGE_MAX_CAP.  FH_ERR_ARG before anything is launched
 *             for a NULL handle, queries or d_counts, a NaN threshold, a bad cap, nq outside 0..256 or such a dim; nq == 0 returns 0.
 *             An empty gallery gives counts of 0 and empty lists.  Returns nq.
 *   execution asynchronous on `stream`; two calls with the same inputs produce identical bytes (no atomics, nothing timing-dependent).
 *             Scratch lives in the handle and grows, synchronously, on the first call of a larger (nq, rows): the hit bitmap — one bit
 *             per (row, query of a whole 64-query tile), at most ceil(G / 32) * 256 * 4 bytes = 1.6 % of the fp32 rows at dim 512 — and
 *             its per-8192-row counts.  The scan costs what a top-k scan costs; the lists cost grows with the number of hits: a
 *             threshold that admits a large share of the gallery is slow, and still right.
 *   sharding  there is no sharded entry point: a shard's call already returns global indices, and the shards' hits concatenate.
 *   range_from_scores   host only, no GPU, and the one definition of the rule: the same answer for ONE query from its row of n
 *             precomputed mapped scores (global index = index_base + position).  tags == NULL: every row carries FH_TAG_ALL; the
 *             unmasked query is tags == NULL with mask == FH_TAG_ALL.  *count = the hits; out_scores / out_indices [cap] (either may
 *             be NULL) as above.  Returns the number of entries listed; FH_ERR_ARG — nothing written — for n < 0, NULL scores with
 *             n > 0, a NULL count, a NaN threshold, a bad cap or an index beyond 31 bits. */
#define FH_RANGE_MAX_CAP 1024
FH_API int fh_gallery_range_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks /* [nq] or NULL */, int nq, float threshold,
                                int cap, long long* d_counts /* [nq] */, float* d_scores /* [nq][cap] or NULL */,
                                int* d_indices /* [nq][cap] or NULL */, int* d_ids /* [nq][cap] or NULL */, void* stream);
FH_API int fh_range_from_scores(const float* scores, long long n, long long index_base, const uint32_t* tags /* or NULL */, uint32_t mask,
                                float threshold, int cap, long long* count, float* out_scores, int* out_indices);

/* ---- deep top-k: the best k rows of every query for 16 < k <= 1024 too, with NO threshold asked of the caller — the best 50 for a human
 * reviewer, the best 200 to re-rank with another model, the best 1000 for an audit.  (fh_gallery_topk_dev stops at 16, the depth of the
 * scan's register lists; fh_gallery_range_dev goes deeper but needs a threshold the caller does not know in advance.)
 *   eligible  row r is eligible for query q iff it is ADMITTED (d_masks == NULL, or (tag[r] & mask[q]) != 0; a gallery whose tags were
 *             never set carries FH_TAG_ALL), its mapped score is not a NaN, and its mapped score is > -inf.
 *   lists     row q of d_scores / d_indices / d_ids [nq][k] holds the best min(k, eligible) rows ranked as everywhere (score descending,
 *             then global row index ascending); the slots behind them carry (-1.0f, -1, -1); nothing outside [nq][k] is written.  This
 *             is by definition the list part of fh_gallery_range_dev(threshold = -inf, cap = k).  Indices are global (index_base +
 *             position).  d_ids = each listed row's identity id and needs a labelled gallery (FH_ERR_STATE otherwise, unless the gallery
 *             is empty).  Any subset of the three may be NULL, not all of them.
 *   scores    the fp32 scan's, bit for bit, whichever scan mode the gallery is in (the call always reads the fp32 rows and leaves
 *             fh_gallery_scan_stats and fh_gallery_tag_stats alone).  For finite rows and queries and k <= 16 the lists are bit for bit
 *             those of fh_gallery_topk_dev (with masks: of fh_gallery_topk_tagged_dev).
 *   limits    nq <= 256, dim % 64 == 0, 1 <= k <= FH_TOPK_DEEP_MAX.  FH_ERR_ARG before anything is launched for a NULL handle or
 *             queries, all three list pointers NULL, a bad k, nq outside 0..256 or such a dim; nq == 0 returns 0.  An empty gallery gives
 *             empty lists.  Returns nq.
 *   cost      one scan of the gallery — the block-maximum scan: the best eligible score of every (32-row block, query) — then per query
 *             the best k blocks by that maximum and the re-score of their rows: at most 32 k rows per query, WHATEVER the data (the
 *             exact top-k lies in those blocks: DESIGN.md 3.4c has the proof).  That tail grows with k — 32 k * dim * 4 bytes of row
 *             reads per query, 64 MB at k = 1024 and dim 512, and 32 k MFMAs per 64 of dim — and dominates the call at k = 1024
 *             (measured at 1 M x 512, nq = 64: 0.76 ms at k = 16, 0.93 ms at k = 128, 2.3 ms at k = 1024; profiles/gallery_deep.md).
 *   execution asynchronous on `stream`; two calls with the same inputs produce identical bytes (no atomics, nothing timing-dependent).
 *             Scratch lives in the handle and grows, synchronously, on the first call of a larger (nq, rows, k): two floats per (32-row
 *             block, query of a whole 64-query tile) — twice the range call's hit bitmap — and 132 bytes per list entry (nq * k).
 *   sharding  there is no sharded entry point: a shard's call already returns global indices; fh_topk_merge_dev merges lists of
 *             k <= 16 only, so deeper per-shard lists are merged by the caller (concatenate, sort by (score desc, index asc), cut).
 *   out of scope   deep lists of IDENTITIES (one entry per id), tile skip for masks, k above 1024.
 *   topk_from_scores   host only, no GPU, and the one definition of the rule: the same answer for ONE query from its row of n
 *             precomputed mapped scores (global index = index_base + position).  tags == NULL: every row carries FH_TAG_ALL.
 *             out_scores / out_indices [k] (either may be NULL) as above.  Returns the number of entries listed; FH_ERR_ARG — nothing
 *             written — for n < 0, NULL scores with n > 0, a bad k or an index beyond 31 bits. */
#define FH_TOPK_DEEP_MAX 1024
FH_API int fh_gallery_topk_deep_dev(fh_gallery* g, const float* d_queries, const uint32_t* d_masks /* [nq] or NULL */, int nq, int k,
                                    float* d_scores /* [nq][k] or NULL */, int* d_indices /* [nq][k] or NULL */,
                                    int* d_ids /* [nq][k] or NULL */, void* stream);
FH_API int fh_topk_from_scores(const float* scores, long long n, long long index_base, const uint32_t* tags /* or NULL */,
                               uint32_t mask, int k, float* out_scores, int* out_indices);
/* test hook: the chosen blocks of deep_plan.h's block rule for one query's scores, best first, into out_blocks [k]; returns their number */
FH_API int fh_debug_deep_blocks(const float* scores, long long n, const uint32_t* tags /* or NULL */, uint32_t mask, int k,
                                long long* out_blocks);

/* ---- measurement hooks (bench.py): per-launch HIP-event timing of the network kernels.
 * Tags 0..3 = conv_igemm tile configs (128x128, 256x64, 128x32, 64x64), 4 = depthwise / depthwise+pointwise,
 * 5 = other graph ops, 6 = conv stream-K fix-up, 7 = Winograd GEMM (its FLOPs = executed; bytes slot = the layer's
 * direct-form FLOPs), 8 = Winograd transforms, 9 = spatial-tile (LDS halo) 3x3 convolutions, 10 = conv_tall_kernel (whole tile rounds of the 3x3 stride-1 layers), 11 = conv_pw_kernel (1x1 stride-1 convolutions as plain GEMMs), 12 = wino2_kernel (fused Winograd F(2x2,3x3): FLOPs = executed, bytes slot = the
 * layer's direct-form FLOPs).  fh_timing_num_tags() = 13 today; fh_timing_collect synchronises, fills n >= fh_timing_num_tags() entry arrays (elapsed ms,
 * algorithmic FLOP, algorithmic activation bytes, launches) and resets the counters.
 * fh_*_set_conv_cfg forces one tile config for every dense conv of a handle (-1 = automatic)
 * and switches the stream-K remainder wave on/off (tuning / A-B measurements). */
FH_API int fh_timing_enable(int on);
FH_API int fh_timing_num_tags(void);
FH_API int fh_timing_collect(double* ms, double* flops, double* bytes, long long* launches, int n);
FH_API int fh_timing_collect_ops(double* ms, double* flops, int* tag, int cap);   /* per launch, in order */
FH_API int fh_det_set_conv_cfg(fh_det* d, int cfg, int stream_k);
FH_API int fh_rec_set_conv_cfg(fh_rec* r, int cfg, int stream_k);
/* 3x3 stride-1 convolutions with >= 128 input channels run as Winograd F(4x4,3x3) (a quarter of the matrix-core work,
 * fp32 rounding error ~25x the direct form's: see DESIGN.md) unless switched off here; 0 = direct form everywhere. */
FH_API int fh_det_set_winograd(fh_det* d, int on);
FH_API int fh_rec_set_winograd(fh_rec* r, int on);
/* on (default): between two consecutive Winograd layers on a map of <= 16x16 pixels the output transform of the first and the input
 * transform of the second run as one kernel (the activation stays in LDS); off: separate transform kernels. */
FH_API int fh_rec_set_wino_fusion(fh_rec* r, int on);
/* on (default): the strided 1x1 shortcut convolution of an IResNet block runs as a tenth tap inside the K loop of the 3x3 convolution
 * it is added to (weights concatenated along K, one launch, no residual round trip); off: two convolutions + residual add. */
FH_API int fh_rec_set_shortcut_fold(fh_rec* r, int on);
/* Opt-in precision mode of the recogniser (the default and the headline stay fp32 = the reference's own arithmetic,
 * src/face_recognizer.cpp:58 float tensors through onnxruntime).  FH_PREC_BF16X2: the Winograd GEMMs (the 3x3 convolutions with >= 128
 * channels, ~80% of IResNet-50's FLOPs) take each operand as a (hi, mid) pair of bf16 — 16 mantissa bits — and run three bf16 MFMAs
 * with f32 accumulation in place of one f32 MFMA; transforms, epilogues, all other layers and the embedding stay fp32.
 * The call is GATED: it embeds a fixed pseudo-random batch of 64 crops in both modes and enters the mode only if every pair of
 * embeddings agrees to 1 - cos < 1e-3; otherwise it returns FH_ERR_STATE, the handle stays fp32 and fh_last_error() quotes the measured
 * value.  *worst (may be NULL) receives the measured max(1 - cos).  Returns the number of layers switched (>= 1), or < 0. */
/* FH_PREC_F32X3 is no mode of fh_rec_set_precision: it names, for the single-kernel entry points below, the three-piece bf16 form of
 * the Winograd GEMM that the fp32 mode runs by default (fh_rec_set_wino_x3); there FH_PREC_FP32 means the native f32 MFMA kernels. */
enum fh_precision { FH_PREC_FP32 = 0, FH_PREC_BF16X2 = 1, FH_PREC_F32X3 = 2 };
FH_API int fh_rec_set_precision(fh_rec* r, int mode, float* worst);
FH_API int fh_rec_get_precision(fh_rec* r);
/* The fp32 mode's Winograd GEMMs.  on (default; FACEHIP_WINO_X3=0 in the environment makes off the default): every fp32 operand is split
 * EXACTLY into three bf16 pieces (8 + 8 + 8 significand bits) and six of the nine piece products run on bf16 MFMAs with f32 accumulation —
 * fp32 results (the dropped terms are below 2^-22 of each product, under the f32 accumulation's own rounding), not bit-identical to the
 * f32 MFMA's.  The split weights are a second device image of 1.5 x the Winograd weights' bytes.  off: the native f32 MFMA kernels.
 * Returns the number of layers that have the form (0 for off), or < 0.  Synchronous the first time it is switched on. */
FH_API int fh_rec_set_wino_x3(fh_rec* r, int on);
FH_API int fh_rec_get_wino_x3(fh_rec* r);
/* The same switch governs the direct convolutions that carry a folded shortcut (IResNet's stride-2 3x3 layers): where the launch gains
 * (fh_debug_conv_plan question 5) their K loop runs on the same three pieces and six products.  Number of layers of this handle that have
 * that form while the switch is on (0 while it is off). */
FH_API int fh_rec_get_conv_x3(fh_rec* r);
/* ... and the 1x1 stride-1 convolutions (all of MobileFaceNet's; IResNet has none): where the launch gains (fh_debug_conv_plan question 6)
 * they run on conv_pw_x3_kernel, the plain GEMM on the same three pieces.  Number of layers of this handle that have that form while the
 * switch is on (0 while it is off). */
FH_API int fh_rec_get_pw_x3(fh_rec* r);
/* ... and the fused F(2x2) Winograd layers with 64 input channels (IResNet's stage 1 and stage-2 entry): where the launch gains
 * (fh_debug_conv_plan question 8) they run on wino2_x3_kernel, the same fused kernel with its products on the three pieces
 * (FACEHIP_WINO2_X3 = 0 / 2 in the environment: none / every launch that has the form).  Number of layers of this handle that have that
 * form while the switch is on (0 while it is off). */
FH_API int fh_rec_get_wino2_x3(fh_rec* r);
/* The detector's own switch for the same form of its 1x1 stride-1 convolutions (SCRFD's 288 / 152 / 72-deep ones and the FPN laterals).
 * on is the default (FACEHIP_DET_X3=0 in the environment makes off the default); off: the native f32 kernels, the bits of a build without
 * the form.  Which launches take it depends on layer geometry, batch and CU count only (FACEHIP_PW_X3 = 0 / 2 in the environment: none /
 * all that have the form).  fh_det_set_x3 returns the number of layers that have the form (0 for off), or < 0; synchronous the first
 * time it is switched on.  fh_det_get_x3: that number while the switch is on, 0 while it is off. */
FH_API int fh_det_set_x3(fh_det* d, int on);
FH_API int fh_det_get_x3(fh_det* d);
/* A handle whose stream is restricted to a subset of the CUs (hipExtStreamCreateWithCUMask, e.g. detector and
 * recogniser side by side on disjoint CU sets) should say how many it gets: it sizes the convolution kernels'
 * remainder round.  0 = the whole device (default). */
FH_API int fh_det_set_cus(fh_det* d, int cus);
FH_API int fh_rec_set_cus(fh_rec* r, int cus);
/* on (default): the u8 preprocess is fused into the first convolution and the preprocessed input tensor is
 * never materialised; off: separate preprocess kernel (needed for fh_det_input_dev). */
FH_API int fh_det_set_fused_stem(fh_det* d, int on);
FH_API int fh_rec_set_fused_stem(fh_rec* r, int on);
/* on (default): when the graph opens with conv 3x3 (16 channels) -> depthwise 3x3 -> pointwise 1x1 (SCRFD's first block), the stem
 * is computed inside the depthwise -> pointwise kernel and its output map never reaches memory; off: separate kernels. */
FH_API int fh_det_set_fused_front(fh_det* d, int on);
/* on (default): dense 3x3 stride-1 convolutions with 16 input and <= 64 output channels on large maps (SCRFD's FPN and head
 * convolutions) run on 8x16 spatial tiles with an LDS halo (conv_halo.hip); off: the generic implicit-GEMM kernel. */
FH_API int fh_det_set_halo_conv(fh_det* d, int on);

/* ---- image files -> BGR u8, replaces cv::imread(path) (reference src/main.cpp:42,71-72,140-141; OpenCV's default
 * IMREAD_COLOR: 8-bit BGR, alpha dropped, grey replicated, JPEG EXIF orientation applied).  Host code.  JPEG
 * (baseline + progressive; libjpeg's islow IDCT / fancy up-sampling / YCbCr tables restated), PNG, BMP, PPM/PGM.
 * *bgr is malloc'ed [rows*cols*3], release it with fh_image_free.  0 on success, < 0 + fh_last_error(). */
FH_API int fh_imread(const char* path, unsigned char** bgr, int* rows, int* cols);
FH_API int fh_image_decode(const unsigned char* bytes, size_t n, unsigned char** bgr, int* rows, int* cols);
FH_API void fh_image_free(unsigned char* bgr);

/* ---- JPEG in two halves: entropy decoding on the host, pixel reconstruction on the device.  Huffman decoding is serial per file and
 * independent across files (host threads); everything behind it — de-quantisation, the islow IDCT, chroma up-sampling, YCbCr -> RGB, the
 * EXIF orientation — is integer arithmetic that is independent per pixel (kernels, csrc/jpeg_dev.hip).  The cut is the decoder's own
 * intermediate: every component's coefficients as a dense int16 plane.  fh_imread / fh_image_decode keep their behaviour and their bits:
 * for a JPEG, fh_image_decode IS fh_jpeg_entropy followed by fh_jpeg_reconstruct.
 *
 * fh_jpeg_desc  what reconstruction needs besides the coefficients; a POD, 528 bytes.  width / height as coded (before the
 *           orientation), rows / cols of the picture handed out (after it: swapped for orientations 5..8); ncomp 1 or 3; hmax / vmax the
 *           largest sampling factors; color 0 grey, 1 YCbCr, 2 RGB (an Adobe marker with transform 0, or component ids 'R','G','B');
 *           orientation 1..8 (EXIF tag 0x0112; 1 when absent); coef_count = int16 elements of all components.  Per component: sampling
 *           factors h / v, the block grid wblocks x hblocks (padded to whole MCUs: ceil(width / (8 hmax)) * h, likewise down), the real
 *           sample size dw = ceil(width * h / hmax) / dh, coef_off = where its [hblocks][wblocks][64] coefficients (natural order, not
 *           zigzag) start, in int16 elements, and quant[64], natural order, the table latched at the component's first scan.
 * fh_jpeg_header  reads markers up to the frame header only: sizes, sampling factors, block grids, coef_count, and the orientation / Adobe
 *           marker when they stand in front of the frame header (where writers put them) — enough to size buffers.  quant stays zero.
 * fh_jpeg_entropy  the whole parse: zero-fills coef[0 .. coef_count) in the CALLER's memory, decodes every scan into it and completes
 *           *desc.  cap = the int16 elements coef holds; coef_count > cap is an error, and nothing at or behind coef + coef_count is ever
 *           written, whatever later markers of a damaged file say.  A damaged header is an error; entropy data that ends early decodes as
 *           zeros (libjpeg's behaviour, as fh_image_decode).
 * fh_jpeg_reconstruct  host: coefficients -> BGR u8 [rows][cols] at pitch `step` (>= cols * 3; bytes of a row behind cols * 3 are not
 *           written).  The bit-exact oracle of the device path.
 * fh_jpeg_desc_check  the one validator both reconstructions run first: FH_ERR_ARG for ncomp / sampling factors out of range, hmax % h or
 *           vmax % v != 0, block grids or dw / dh that do not follow from width / height, coef_off ranges that overlap or pass coef_count,
 *           an orientation outside 1..8, rows / cols that do not follow from it, a color outside 0..2 or one that disagrees with ncomp.  A
 *           descriptor can be made by hand: a bad one never reaches a kernel.
 * All five: 0 on success, < 0 + fh_last_error().  Host code, no GPU. */
typedef struct fh_jpeg_comp {
    int32_t h, v, wblocks, hblocks, dw, dh;
    int64_t coef_off;
    uint16_t quant[64];
} fh_jpeg_comp;                                                                          /* 160 bytes */
typedef struct fh_jpeg_desc {
    int32_t width, height, rows, cols, ncomp, hmax, vmax, color, orientation, reserved;
    int64_t coef_count;
    fh_jpeg_comp comp[3];
} fh_jpeg_desc;                                                                          /* 528 bytes */
FH_API int fh_jpeg_header(const unsigned char* bytes, size_t n, fh_jpeg_desc* desc);
FH_API int fh_jpeg_entropy(const unsigned char* bytes, size_t n, fh_jpeg_desc* desc, int16_t* coef, size_t cap);
FH_API int fh_jpeg_reconstruct(const fh_jpeg_desc* desc, const int16_t* coef, unsigned char* bgr, int step);
FH_API int fh_jpeg_desc_check(const fh_jpeg_desc* desc);
/* fh_jpegdec  owner of the device side: the device copy of the descriptor table, the workspace of IDCT output planes, and (for
 *           fh_jpeg_decode_batch) the pinned coefficient arena, its device copy and the device pixel arena.  All grow on demand.
 * fh_jpeg_reconstruct_batch_dev  fh_jpeg_reconstruct for n images (1 <= n <= 4096) in TWO launches, whatever n is: descs = HOST array
 *           (read before the call returns), d_coef = DEVICE int16, coef_base[i] = image i's offset in it (int16 elements; image i reads
 *           [coef_base[i], coef_base[i] + descs[i].coef_count)), out_frames[i].bgr = DEVICE memory for rows x cols pixels at pitch step >=
 *           cols * 3, whose rows / cols must equal the descriptor's.  A slot with bgr == NULL is skipped.  Only the bytes
 *           [row * step, row * step + cols * 3) of a frame are written, and they equal fh_jpeg_reconstruct's for every descriptor
 *           fh_jpeg_desc_check accepts and every int16 / uint16 value.  Every descriptor is checked before anything is launched: one bad
 *           one fails the call with FH_ERR_ARG and nothing is written.  Asynchronous on `stream`; returns n. */
typedef struct fh_jpegdec fh_jpegdec;
FH_API fh_jpegdec* fh_jpegdec_create(void);
FH_API void fh_jpegdec_destroy(fh_jpegdec* dec);
FH_API int fh_jpeg_reconstruct_batch_dev(fh_jpegdec* dec, const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base,
                                         const fh_frame* out_frames, void* stream);
/* fh_jpeg_decode_batch  n files (1 <= n <= 4096) -> n device images.  fh_jpeg_header sizes one pinned coefficient arena and one device
 *           pixel arena; fh_jpeg_entropy runs on up to `threads` host threads (clipped to [1, 16]; 0 = min(16, n)), one file per task,
 *           straight into the pinned arena; ONE host-to-device copy; one fh_jpeg_reconstruct_batch_dev.  frames_out[i] describes image i
 *           in the device arena (step = cols * 3), valid until the next call on `dec`.  status[i]: 0 = JPEG, reconstructed on the device;
 *           1 = another format fh_image_decode accepts, decoded on the host (by the same threads), pixels sent in the same copy; < 0 = not
 *           decodable: frames_out[i] is the empty frame (cv::imread's empty Mat) and the call still succeeds.  status may be NULL.
 *           Asynchronous on `stream` behind the host work; returns the number of decoded images.
 * fh_pipeline_run_files  the above followed by fh_pipeline_run_ragged_dev on the detector's own stream, blocking: outputs, cap and return
 *           value as fh_pipeline_run_images, and every result equals, bit for bit, fh_image_decode per file + fh_pipeline_run_images. */
typedef struct fh_blob { const unsigned char* bytes; size_t n; } fh_blob;
FH_API int fh_jpeg_decode_batch(fh_jpegdec* dec, const fh_blob* files, int n, int threads, fh_frame* frames_out, int* status, void* stream);
FH_API int fh_pipeline_run_files(fh_det* d, fh_rec* r, fh_jpegdec* dec, const fh_blob* files, int n, int threads, float score_thr,
                                 float nms_thr, int faces_per_frame, fh_face* faces, int* frame_of, float* emb, int cap, int* status);

/* ---- JPEG out: the decode split in mirror image.  Colour conversion, chroma down-sampling, the forward DCT and quantisation are integer
 * arithmetic that is independent per block (kernels, csrc/jpeg_enc.hip); Huffman coding is serial per file and independent across files
 * (host threads; or, opt-in, parallel over blocks on the device: fh_jpeg_code_batch_dev below).  The cut is the same dense int16 coefficient plane per component, described by the same fh_jpeg_desc.  The arithmetic
 * is libjpeg's (jccolor.c, jcsample.c without smoothing, jfdctint.c "islow", jcdctmgr.c, jccoefct.c's dummy blocks): the coefficients
 * are, bit for bit, the ones libjpeg(-turbo) stores for the same pixels, sampling and quality (tests/test_jpeg_enc_cpu.py, against files
 * written by Pillow).  The files are baseline sequential JFIF with the four Annex K Huffman tables (libjpeg without `optimize`), one
 * interleaved scan; no restart markers, no EXIF, no progressive mode.
 *
 * fh_jpeg_quant_tables  libjpeg's jpeg_quality_scaling on the Annex K base tables: quality clipped to 1..100, scale = 5000 / q below 50,
 *           200 - 2 q otherwise, entry = (base * scale + 50) / 100 clamped to 1..255.  Natural order.
 * fh_jpeg_enc_desc  the descriptor of a width x height picture (1..65535 each): gray != 0 one component (subsampling is ignored), else
 *           Y Cb Cr with subsampling 0 = 4:4:4, 1 = 4:2:2 (luma 2 x 1), 2 = 4:2:0 (luma 2 x 2); block grids padded to whole MCUs, dw / dh,
 *           coef_off (multiples of 64), coef_count and quant (fh_jpeg_quant_tables of `quality`) filled; orientation 1, color 0 or 1,
 *           rows / cols = height / width.
 * fh_jpeg_enc_check  fh_jpeg_desc_check plus what the forward paths and the writer rely on: orientation 1, color 0 or 1, width and
 *           height <= 65535, sampling factors of one of the layouts above (chroma 1 x 1; grey 1 x 1), every quantiser in 1..255.  Both
 *           forward paths and the writer run it first: a bad descriptor never reaches a kernel and nothing is written.
 * fh_jpeg_forward  host: BGR u8 [rows][cols] at pitch `step` (>= cols * 3) -> all coef_count coefficients, natural order, dummy blocks
 *           of the padded grid included.  A grey descriptor takes Y from the B, G, R of every pixel (what cv::imwrite does with a
 *           3-channel image; a caller with grey data passes B = G = R, which gives Y = that value).  cap < coef_count is an error raised
 *           before the first write.  The bit-exact oracle of the device path.
 * fh_jpeg_write  coefficients -> the file's bytes.  A DC difference outside +-2047 or an AC value outside +-1023 (which no forward path
 *           produces) returns FH_ERR_ARG, *written = 0.  Otherwise *written = the size of the file whatever cap is; cap smaller than that
 *           returns FH_ERR_ARG and nothing at or behind out + cap is written, so that a caller can size and retry.
 * fh_jpeg_write_bound  an upper bound of *written for the descriptor (0 for one fh_jpeg_enc_check refuses).
 * fh_jpeg_write_header  the bytes fh_jpeg_write emits in front of the first entropy-coded byte (SOI .. the SOS header), from the same code;
 *           cap / *written as fh_jpeg_write (*written = the size whatever cap is; nothing at or behind out + cap is written).
 * fh_jpeg_scan_bits  bits[b] = the bits fh_jpeg_write's block coder emits for block b of the scan, in SCAN order: MCU by MCU, inside an
 *           MCU component by component, v rows of h blocks each.  cap = the entries `bits` holds (>= the blocks of all components).
 *           FH_ERR_ARG for a coefficient fh_jpeg_write refuses.  The host rule of the device coder's size pass.
 * fh_imwrite_jpeg  fh_jpeg_enc_desc + fh_jpeg_forward + fh_jpeg_write + a file write: cv::imwrite(path.jpg, bgr) with
 *           IMWRITE_JPEG_QUALITY = quality and the chroma sampling chosen by `subsampling`.
 * All: 0 on success, < 0 + fh_last_error().  Host code, no GPU. */
FH_API int fh_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma);
FH_API int fh_jpeg_enc_desc(int width, int height, int gray, int subsampling, int quality, fh_jpeg_desc* desc);
FH_API int fh_jpeg_enc_check(const fh_jpeg_desc* desc);
FH_API int fh_jpeg_forward(const fh_jpeg_desc* desc, const unsigned char* bgr, int step, int16_t* coef, size_t cap);
FH_API int fh_jpeg_write(const fh_jpeg_desc* desc, const int16_t* coef, unsigned char* out, size_t cap, size_t* written);
FH_API size_t fh_jpeg_write_bound(const fh_jpeg_desc* desc);
FH_API int fh_jpeg_write_header(const fh_jpeg_desc* desc, unsigned char* out, size_t cap, size_t* written);
FH_API int fh_jpeg_scan_bits(const fh_jpeg_desc* desc, const int16_t* coef, uint32_t* bits, size_t cap);
FH_API int fh_imwrite_jpeg(const char* path, const unsigned char* bgr, int rows, int cols, int step, int quality, int subsampling);
/* fh_jpegenc  owner of the device side: the device copy of the descriptor table, the workspace of sample planes and (for
 *           fh_jpeg_encode_batch) the device and pinned coefficient arenas and the output byte arena, and the device Huffman coder's
 *           tables, streams and device byte arena (fh_jpeg_code_batch_dev).  All grow on demand.
 * fh_jpeg_forward_batch_dev  fh_jpeg_forward for n images (1 <= n <= 4096) of any sizes and layouts in TWO launches, whatever n is: descs =
 *           HOST array (read before the call returns), frames[i].bgr = DEVICE pixels at any address and any pitch step >= cols * 3, whose
 *           rows / cols must equal the descriptor's; d_coef = DEVICE int16 (2-byte aligned), image i writes [coef_base[i], coef_base[i] +
 *           descs[i].coef_count).  A slot with bgr == NULL is skipped and its coefficient range is not written.  Only bytes
 *           [row * step, row * step + cols * 3) of real rows are read.  The coefficients equal fh_jpeg_forward's for every descriptor
 *           fh_jpeg_enc_check accepts and every pixel value.  Every descriptor is checked before anything is launched: one bad one fails the
 *           call with FH_ERR_ARG and nothing is written.  Asynchronous on `stream`; returns n.
 * fh_jpeg_encode_batch  n DEVICE frames (1 <= n <= 4096) -> n files: a descriptor per frame (fh_jpeg_enc_desc, colour), the forward
 *           path on the device, ONE device-to-host copy of the coefficient arena into pinned memory, fh_jpeg_write on up to `threads` host
 *           threads (clipped to [1, 16]; 0 = min(16, n)), one file per task.  files_out[i] points into the handle's byte arena, valid until
 *           the next call on `enc`; an empty frame (bgr == NULL or a non-positive size) gives {NULL, 0} and the call still succeeds.  Every
 *           file equals fh_jpeg_write(fh_jpeg_forward(...)) on the host, byte for byte, whatever `threads` is.  Blocking; returns the number
 *           of files written.
 *
 * Huffman coding on the device (kernels, csrc/jpeg_huff.hip): baseline coding is parallel over blocks — a block's code depends on its
 * own 64 coefficients and the DC of the previous block of its component in scan order, its place in the stream is a prefix sum of code
 * lengths, and byte stuffing a second prefix sum over bytes.  No kernel waits for another workgroup; nothing depends on timing.
 * fh_jpeg_code_batch_dev  fh_jpeg_write for n images (1 <= n <= 4096) whose coefficients lie in DEVICE memory: descs / d_coef / coef_base
 *           as fh_jpeg_forward_batch_dev, except that the SKIPPED slots are those with coef_base[i] < 0 (their descriptors are not looked
 *           at).  Every live descriptor passes fh_jpeg_enc_check before anything is launched: one bad one fails the call with FH_ERR_ARG
 *           and nothing is written; so does a batch of 2^31 blocks or more.  The files lie back to back, in slot order, in a device byte
 *           arena owned by the handle: files_dev_out[i] = {DEVICE pointer, size}, valid until the next call on `enc`.  status[i] (may be
 *           NULL): 0 = coded, the file equals fh_jpeg_write's byte for byte; 1 = skipped slot; FH_ERR_ARG = the image holds a DC
 *           difference outside +-2047 or an AC value outside +-1023 — its file is {NULL, 0}, as a skipped slot's, and the other images
 *           are still written.  d_coef is only read.  The call synchronises `stream` TWICE (after the size pass, for the images' bit
 *           totals, and after the 0xFF count, for the files' sizes); the last kernels are asynchronous on `stream`.  Returns the number
 *           of files coded.
 * fh_jpeg_encode_batch_gpu  fh_jpeg_encode_batch without host coding: the same descriptors and forward path, then
 *           fh_jpeg_code_batch_dev, then ONE device-to-host copy of the file bytes alone into pinned memory (a third synchronisation).
 *           files_out[i] points into that host arena, valid until the next call on `enc`; an empty frame gives {NULL, 0}.  The bytes
 *           equal fh_jpeg_encode_batch's.  Blocking; returns the number of files written.
 * FH_JPEG_STUFF_CHUNK (fh_jpeg_stuff_chunk())  the bytes of an image's unstuffed stream one workgroup of the stuffing passes handles. */
#define FH_JPEG_STUFF_CHUNK 1024
typedef struct fh_jpegenc fh_jpegenc;
FH_API fh_jpegenc* fh_jpegenc_create(void);
FH_API void fh_jpegenc_destroy(fh_jpegenc* enc);
FH_API int fh_jpeg_forward_batch_dev(fh_jpegenc* enc, const fh_jpeg_desc* descs, int n, const fh_frame* frames, int16_t* d_coef,
                                     const long long* coef_base, void* stream);
FH_API int fh_jpeg_encode_batch(fh_jpegenc* enc, const fh_frame* frames, int n, int quality, int subsampling, int threads, fh_blob* files_out,
                                void* stream);
FH_API int fh_jpeg_code_batch_dev(fh_jpegenc* enc, const fh_jpeg_desc* descs, int n, const int16_t* d_coef, const long long* coef_base,
                                  fh_blob* files_dev_out, int* status, void* stream);
FH_API int fh_jpeg_encode_batch_gpu(fh_jpegenc* enc, const fh_frame* frames, int n, int quality, int subsampling, fh_blob* files_out,
                                    void* stream);
FH_API int fh_jpeg_stuff_chunk(void);
/* test hooks: the device byte arena of the last fh_jpeg_code_batch_dev (its base and capacity; fill in 0..255 sets every byte of it to
 * that value first, fill < 0 leaves it alone), and the size pass's bits per block of that call — the live images' blocks in scan order,
 * image after image — copied to the host (returns the count; cap = entries of `bits`). */
FH_API int fh_debug_jpeg_arena(fh_jpegenc* enc, int fill, void** dev, size_t* bytes);
FH_API long long fh_debug_jpeg_scan_bits(fh_jpegenc* enc, uint32_t* bits, size_t cap);

/* ---- single kernels exposed for parity tests and micro-benchmarks (device pointers). */
FH_API int fh_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes);   /* synchronous */
FH_API int fh_resize_u8c3_dev(const uint8_t* d_src, int sh, int sw, int sstep, uint8_t* d_dst, int dh, int dw, int dstep,
                              void* stream);
FH_API int fh_conv_forward_dev(const float* d_in, const float* d_wt_packed, const float* d_bias, float* d_out, int batch,
                               int h, int w, int cin, int cout, int ksize, int stride, int kpad, int cfg, void* stream);
/* The same with a precision argument, an optional folded shortcut and the CU count the launcher plans with.  precision = FH_PREC_FP32: the
 * f32 MFMA kernels; FH_PREC_F32X3: conv_igemm_kernel's three-piece bf16 K loop (fp32 products from six bf16 MFMAs; cfg is ignored, the
 * tile is 128 x 128 or 128 x 64) on a copy of the weights split here as the engine splits them — refused for layers without the form
 * ("... no three-piece bf16 form": cin % 32 != 0, cout % 64 != 0; this entry point has no grouped layers).  d_sc_in (may be NULL): the input
 * [batch][sc_h][sc_w][sc_c] of a 1x1 convolution of stride sc_stride on the same output grid, run as a tenth tap of the K loop: d_wt_packed
 * is then [fh_conv_wt_rows(cout)][9 cin + sc_c] with the shortcut's weights behind the 3x3 ones, kpad = 9 cin + sc_c, ksize = 3,
 * cin % 32 == 0, sc_c % 32 == 0.  cus > 0: the launcher plans the stream-K remainder as for a device of that many CUs (ConvArgs::cus), so
 * that small layers reach every role; 0 = the device's own count.  Synchronous for FH_PREC_F32X3.
 * ksize = 1, stride = 1 with FH_PREC_F32X3: conv_pw_x3_kernel (the 1x1 GEMM on three bf16 pieces; kpad % 32 == 0, kpad >= cin), refused
 * with the same message where the layer has no such form: cin % 4 != 0, cout % 4 != 0, batch * h * w % 128 != 0 or fewer tiles than CUs
 * (question 6 of fh_debug_conv_plan; pass a small `cus` for small layers).  Every other ksize = 1 layer is refused under FH_PREC_F32X3. */
FH_API int fh_conv_forward_ex_dev(const float* d_in, const float* d_wt_packed, const float* d_bias, float* d_out, int batch,
                                  int h, int w, int cin, int cout, int ksize, int stride, int kpad, int cfg, int precision,
                                  const float* d_sc_in, int sc_h, int sc_w, int sc_c, int sc_stride, int cus, void* stream);
/* The same with the epilogue's activation and residual: act = 0 none / 1 ReLU, d_res (may be NULL) = a tensor of the output's shape added
 * after the activation.  fh_conv_forward_ex_dev is this call with act = 0 and no residual. */
FH_API int fh_conv_forward_ep_dev(const float* d_in, const float* d_wt_packed, const float* d_bias, float* d_out, int batch,
                                  int h, int w, int cin, int cout, int ksize, int stride, int kpad, int cfg, int precision,
                                  const float* d_sc_in, int sc_h, int sc_w, int sc_c, int sc_stride, int cus, int act, const float* d_res,
                                  void* stream);
/* 3x3 stride-1 pad-1 convolution (+bias) in the Winograd F(4x4,3x3) form the deep layers use; w_ohwi = HOST weights
 * [cout][3*3][cin]; cin % 32 == 0, cout % 4 == 0.  Synchronous. */
FH_API int fh_conv_winograd_dev(const float* d_in, const float* w_ohwi_host, const float* d_bias, float* d_out, int batch, int h, int w,
                                int cin, int cout, void* stream);
/* The same with a precision argument (enum fh_precision).  FH_PREC_BF16X2: the split-bf16 operand format of fh_rec_set_precision on this
 * one layer — the weight image is packed as the engine packs it, the input transform writes packed V, the GEMM is the three-product bf16
 * form.  Layers without that form (cin % 32 != 0 or cout % 64 != 0) are refused ("... no split-bf16 GEMM").  FH_PREC_F32X3: the three-piece bf16
 * GEMM of fh_rec_set_wino_x3 on this one layer (V stays fp32, the weight image is split as the engine splits it; same layers);
 * FH_PREC_FP32: the native f32 MFMA kernels. */
FH_API int fh_conv_winograd_ex_dev(const float* d_in, const float* w_ohwi_host, const float* d_bias, float* d_out, int batch, int h, int w,
                                   int cin, int cout, int precision, void* stream);
/* The same convolution in the fused Winograd F(2x2,3x3) form the 64-channel stages use (conv_wino2.hip): cin == 64, cout % 64 == 0;
 * d_bias = [cout] or, with bias_cls != 0, [9][cout] (one vector per border class of the output pixel: a pre-conv BatchNorm folded in);
 * act = 0 none / 1 ReLU / 2 PReLU (d_slope [cout]) ...; d_res = optional residual of the output's shape.  Synchronous. */
FH_API int fh_conv_wino2_dev(const float* d_in, const float* w_ohwi_host, const float* d_bias, const float* d_slope, const float* d_res,
                             float* d_out, int batch, int h, int w, int cin, int cout, int act, int bias_cls, void* stream);
/* The full argument set of that kernel: d_out2 = d_out * d_s2 + d_t2 (a following block's BatchNorm; any of d_out / d_out2 may be NULL
 * when the other is given), and the MERGED form SCRFD's heads use — n_outs (1..3) sibling convolutions evaluated as one with cout <= 32
 * channels in all: output g takes channels [oc0[g], oc0[g + 1]) into d_outs[g] ([pixels][oc0[g + 1] - oc0[g]]) through activation
 * oact[g] (0 none / 1 ReLU / 3 sigmoid); no residual, second output or bias classes in that form.  Synchronous. */
FH_API int fh_conv_wino2_ex_dev(const float* d_in, const float* w_ohwi_host, const float* d_bias, const float* d_slope, const float* d_res,
                                float* d_out, float* d_out2, const float* d_s2, const float* d_t2, int n_outs, float* const* d_outs,
                                const int* oc0, const int* oact, int batch, int h, int w, int cin, int cout, int act, int bias_cls,
                                void* stream);
/* Diagnostic builds of conv_wino2.hip (-DFACEHIP_W2_PROF, scripts/wino2_prof.sh, FACEHIP_W2_ABLATE set): median shader clock in MHz the
 * waves of the last wino2 launch measured (s_memtime against the 100 MHz s_memrealtime).  0 in production builds. */
FH_API double fh_debug_wino2_clock_mhz(void);
/* Batch-1 host-pointer calls (fh_det_detect, fh_rec_extract, fh_rec_extract_simple — the reference's own mode, src/main.cpp:88-104) are
 * captured into a HIP graph per call shape (image size / pitch, thresholds) and replayed: first call with a shape eager, second
 * captured, later ones one hipGraphLaunch each.  Results are bitwise those of the eager path.  fh_set_graph_replay(0) (or
 * FACEHIP_GRAPH=0) turns it off process-wide; fh_*_graph_stats return the node count of the handle's captured graph (0 = none yet)
 * and the number of replayed calls. */
FH_API int fh_set_graph_replay(int on);
FH_API const float* fh_det_workspace_dev(fh_det* d);          /* tuning hook: the detector's stream-K workspace (diagnostic kernel builds write phase stamps there) */
FH_API int fh_det_graph_stats(fh_det* d, long long* replays);
FH_API int fh_rec_graph_stats(fh_rec* r, long long* replays);
/* Stream-K watchdog test hook (conv_mfma.hip): drop_publish != 0 makes the helper workgroups of a remainder round "lose" their
 * publication, timeout_ms bounds the owners' wait (0 = the 2 s default).  An owner whose wait times out abandons its tile and the
 * next call on the same handle (or fh_det_sync / fh_rec_sync) returns FH_ERR_DEVICE ("stream-K hand-off timed out ...") instead of
 * the process hanging with the GPU; other handles are unaffected. */
FH_API int fh_debug_streamk(int drop_publish, int timeout_ms);
/* The launch arithmetic of the direct convolutions (csrc/conv_plan.h) — host only, no GPU, the default tuning switches.  `in` holds n_in
 * ints, `out` receives n_out values; returns n_out, or FH_ERR_ARG for an unknown question, wrong lengths or a non-positive size.
 *   what 0  stream-K remainder: in = T tiles, S resident workgroup slots, K chunks per tile, accumulators per tile, CUs, Kpad, tile0,
 *           slabs allowed (8) -> out = full, rem, helpers, owners, fixup, units, q, owner_chunks, maxp (9; ConvSkPlan)
 *   what 1  conv_pw_kernel: in = B, H, W, Cin, Cout, ksize, stride, pad, merged outputs, residual through 2x up-sampling, CUs (11)
 *           -> out = its tile width 96 / 64 / 32, or 0 = the layer stays with conv_igemm_kernel (1)
 *   what 2  conv_tall_kernel: in = the same 11, tile config 0..3 or -1 = automatic (12) -> out = tiles it takes, LDS image rows, LDS bytes (3)
 *   what 3  slabs per remainder tile: in = r0, r1, chunks per tile left to the helpers, q (4) -> out = min, max over r0 <= r < r1 (2)
 *   what 4  the workspace: in = nothing -> out = slab floats, counter words (2)
 *   what 5  the three-piece bf16 K loop of a direct convolution: in = 128-row tiles x column tiles of the x3 tile width, Kpad, Cout, CUs (4)
 *           -> out = 1 if the launch runs it (conv_x3_pays), x3 tile width 128 / 64 or 0 = Cout has no such form (2)
 *   what 6  conv_pw_x3_kernel: in = the 11 of question 1 -> out = its tile width 96 / 64 / 32 or 0 = no such form at this batch
 *           (conv_pw_x3_bn; never a form where question 1 answers 0), its tiles, 1 if the launch runs it with the handle's switch on (3)
 *   what 7  conv_pw_x3_pays alone: in = tiles, Kpad, Cout, CUs (4) -> out = 1 if such a launch runs the x3 form (1)
 *   what 8  wino2_x3_pays: in = workgroups, CUs (2) -> out = 1 if such a launch of the fused F(2x2) layer runs wino2_x3_kernel (1) */
FH_API int fh_debug_conv_plan(int what, const int* in, int n_in, long long* out, int n_out);
/* The plain form of fh_conv_wino2_ex_dev (no merged outputs) with a precision argument and the CU count: FH_PREC_FP32 = wino2_kernel,
 * FH_PREC_F32X3 = wino2_x3_kernel (fp32 products from six bf16 MFMAs) on an image split here as the engine splits it — refused for layers
 * without the form ("... no three-piece bf16 form": cin != 64 or cout % 64 != 0).  Synchronous. */
FH_API int fh_conv_wino2_prec_dev(const float* d_in, const float* w_ohwi_host, const float* d_bias, const float* d_slope, const float* d_res,
                                  float* d_out, float* d_out2, const float* d_s2, const float* d_t2, int batch, int h, int w, int cin,
                                  int cout, int act, int bias_cls, int precision, int cus, void* stream);
/* The host pack of that image, for the layout tests: dst = 16 * cin * cout * 3 bf16 words in the order
 * [cout / 64][16 f][2 s][2 waves][3 planes h, m, l][2][64 lanes][8]. */
FH_API int fh_debug_wino2_pack_x3(const float* w_ohwi_host, int cout, int cin, unsigned short* dst);
/* The host pack of the matrix-core stems' weights (stem_mfma_kernel, front_kernel), for the layout tests: wf = the folded filter
 * [27][cout] (tap-major: (ky * 9 + kx * 3 + byte) x channel), cout % 16 == 0 -> out = cout / 16 * 3 * 64 * 4 dwords in the order
 * [cout / 16][3 pieces hi, mid, lo][64 lanes][4], two bf16 per dword.  Needs no device. */
FH_API int fh_debug_stem_pack(const float* wf, int cout, unsigned* out);
/* fh_det_run_network_dev without the letterbox plan, for the stem tests: the n device frames (rows <= input height, cols <= input width)
 * are pasted at the net input's origin as they are — scale 1 whatever their shape — and the rest of the net input is canvas.  Returns n. */
FH_API int fh_debug_det_run_pasted_dev(fh_det* det, const uint8_t* d_frames, int n, int rows, int cols, int step, long long stride, void* stream);
/* Test hook of the multi-tile Winograd GEMM (winograd.hip wino_gemm_pers_kernel): launches with more tiles than resident workgroup
 * slots walk several tiles per workgroup; slots > 0 makes the launcher pretend the device has that many (rounded up to 8), so that small
 * test layers take the multi-tile path with many tiles per workgroup; 0 restores the device's own count. */
FH_API int fh_debug_wino_slots(int slots);
/* Test hook of the clustering pair passes (gallery_cluster.hip): a workgroup walks a run of A tiles (128 rows each) against its B tile, and
 * the launcher gives runs of more than one tile only to large galleries; tiles_per_wg > 0 fixes the run length, so that a small gallery
 * walks runs of several tiles; 0 restores the automatic choice. */
FH_API int fh_debug_cluster_tiles(int tiles_per_wg);
/* Measurement hook of fh_gallery_pair_hist_dev: the number of privatised histogram copies its workgroups flush into (1..4096; 0 restores
 * the default, 1).  The result does not depend on it (scripts/gallery_hist_ab.py --copies). */
FH_API int fh_debug_hist_copies(int copies);
/* Test hook of fh_gallery_pairs_dev: the candidate room of the cut (FH_PAIRS_ROOM by default).  room > 0 replaces it, 0 restores the
 * default; the value in force for a call is max(room, cap).  A small room makes a small gallery take the "boundary bin does not fit"
 * branch of the cut. */
FH_API int fh_debug_pairs_room(int room);
/* Test / measurement hook of the tagged scans (gallery_tags.hip): 0 = every tile is multiplied, none is skipped; non-zero (the default)
 * = tiles without an admitted row for any of a workgroup's queries are skipped.  The answer is the same bits either way. */
FH_API int fh_debug_tag_skip(int on);
/* Test hook of the split-bf16 operand format (winograd.hip wino_pack_bf16x2): n f32 words -> n packed words, hi = bf16(x) in the low half,
 * mid = bf16(x - hi) in the high half, both round-to-nearest-even.  n % 4 == 0.  Synchronous. */
FH_API int fh_debug_pack_bf16x2_dev(const float* d_in, float* d_out, long long n);
/* Test hook: the GEMM stage of the Winograd form alone, M[plane] = V[plane] * U[frequency of the plane]^T, on caller-supplied f32
 * operands.  d_V [rows][k] and d_M [rows][n] in the plane layout the transforms use (rows = fh_debug_wino_gemm_rows: 36 planes of the
 * tile count rounded up to 256 or, mixed != 0, the planes of the mixed F(4x4) / F(2x2) tiling — refused where that tiling does not
 * apply); d_U [36][fh_conv_wt_rows(n)][k] row-major.  k % 32 == 0, n % 32 == 0.  precision = FH_PREC_BF16X2 packs copies of V and U
 * and runs the three-product bf16 kernel (n % 64 == 0); FH_PREC_F32X3 splits a copy of U into three bf16 planes and runs the six-product
 * kernel on the caller's f32 V (n % 64 == 0); FH_PREC_FP32 runs the native f32 MFMA kernels.  Synchronous. */
FH_API long long fh_debug_wino_gemm_rows(int batch, int h, int w, int k, int n, int mixed);
FH_API int fh_debug_wino_gemm_dev(const float* d_V, const float* d_U, float* d_M, int batch, int h, int w, int k, int n, int precision,
                                  int mixed, void* stream);
/* Test hook of the top-k merge (face_kernels.hip topk_merge_kernel) with the list layout of the sharded exchange: part w's [nq][k]
 * scores start at ps + w * part_stride and its indices at pi + w * part_stride (comm.cpp gathers [scores | indices] per rank, so
 * part_stride = 2 * nq * k there).  Needs 1 <= k <= 16, nparts * k <= 65536 and part_stride >= nq * k; returns nq. */
FH_API int fh_debug_topk_merge_strided_dev(const float* d_ps, const int* d_pi, int nparts, int nq, int k, long long part_stride,
                                           float* d_scores, int* d_indices, void* stream);
FH_API int fh_conv_wt_rows(int cout);
/* host: weights [cout][ksize*ksize][cin] (O,H,W,I) -> the kernel's packed image [fh_conv_wt_rows][fh_conv_kpad] */
FH_API int fh_conv_pack_weights(const float* w_ohwi, int cout, int cin, int ksize, float* dst_packed);
FH_API int fh_conv_kpad(int ktot);

#ifdef __cplusplus
}
#endif
#endif /* FACEHIP_H_ */
