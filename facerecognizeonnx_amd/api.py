"""Host-side mirror of the reference's class API over the C ABI (libfacehip.so).

`FaceDetector` / `FaceRecognizer` keep the reference's method names, argument order, defaults and
error behaviour (reference src/face_detector.h:14-43, src/face_recognizer.h:9-38):
``loadModel`` returns False on failure, ``detect`` / ``extractFeature`` return empty results
instead of raising, ``compareFaces`` returns 0.0 on size mismatch.  Images are numpy
``uint8[rows, cols, 3]`` BGR arrays (the cv::Mat the reference takes).

The ``*_dev`` methods are the batch additions: they take device pointers (e.g.
``torch.Tensor.data_ptr()``) so frames stay resident in HBM between detect and embed.
There is no CPU path here: without libfacehip.so and a GPU these classes fail loudly.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import FACE_DTYPE, TRACK_DTYPE, check


@dataclass
class FaceBox:
    """struct FaceBox (src/face_detector.h:8-12): box = (x, y, width, height)."""
    box: tuple = (0, 0, 0, 0)
    score: float = 0.0
    landmarks: np.ndarray = field(default_factory=lambda: np.zeros((5, 2), np.float32))

    def to_record(self) -> np.ndarray:
        r = np.zeros(1, FACE_DTYPE)
        r[0]["x"], r[0]["y"], r[0]["w"], r[0]["h"] = self.box
        r[0]["score"] = self.score
        r[0]["lm"] = np.asarray(self.landmarks, np.float32).reshape(10)
        return r

    @staticmethod
    def from_record(r) -> "FaceBox":
        return FaceBox((int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])), float(r["score"]),
                       np.array(r["lm"], np.float32).reshape(5, 2))


def _img(image) -> Optional[np.ndarray]:
    if image is None:
        return None
    a = np.asarray(image)
    if a.size == 0:
        return None
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise TypeError("image must be uint8[rows, cols, 3] (BGR)")
    if a.strides[2] != 1 or a.strides[1] != 3:
        a = np.ascontiguousarray(a)
    return a


def frame_array(frames):
    """A ctypes array of fh_frame from an iterable of (ptr, rows, cols[, step]) — ptr an int device (or host) address, step defaulting
    to cols * 3; None or a zero ptr / size is an empty frame.  A ready-made ``(FhFrame * n)`` array passes through."""
    if isinstance(frames, C.Array) and getattr(frames, "_type_", None) is _lib.FhFrame:
        return frames
    frames = list(frames)
    arr = (_lib.FhFrame * max(len(frames), 1))()
    for i, f in enumerate(frames):
        if f is None:
            continue
        ptr, rows, cols = f[0], int(f[1]), int(f[2])
        step = int(f[3]) if len(f) > 3 and f[3] else cols * 3
        arr[i].bgr, arr[i].rows, arr[i].cols, arr[i].step = (int(ptr) or None), rows, cols, step
    arr._n = len(frames)
    return arr


def _frame_count(arr) -> int:
    return getattr(arr, "_n", len(arr))


def letterbox_plan(rows: int, cols: int, in_w: int, in_h: int):
    """FaceDetector::preprocess' letterbox arithmetic (face_detector.cpp:101-113) as the detector does it (fh_letterbox_plan, host
    code): returns (live, new_w, new_h, scale); a dead frame (empty image or "Invalid resize dimensions") is (False, 0, 0, 0.0)."""
    nw, nh, sc = C.c_int(), C.c_int(), C.c_float()
    live = _lib.lib().fh_letterbox_plan(int(rows), int(cols), int(in_w), int(in_h), C.byref(nw), C.byref(nh), C.byref(sc))
    return bool(live), nw.value, nh.value, float(sc.value)


def Tiling(tile, overlap: int = 0, border: int = 2):
    """An fh_tiling for the tiled calls: tile = the side of a square tile or (tile_w, tile_h); border < 0 switches the border rule
    off.  (FaceDetector.tiling fills `tile` with the detector's input size.)"""
    tw, th = (tile, tile) if np.isscalar(tile) else tile
    return _lib.FhTiling(int(tw), int(th), int(overlap), int(border))


def _tiling(t):
    return t if isinstance(t, _lib.FhTiling) else Tiling(*t)


def tile_plan(rows: int, cols: int, tile, overlap: int = 0, border: int = 2):
    """The views of a tiled detection of a rows x cols frame (fh_tile_plan, host code): a list of (x, y, w, h, edges), view 0 the
    whole frame, then the tiles row-major; edges bit 0 left, 1 top, 2 right, 3 bottom = that edge is interior."""
    t = Tiling(tile, overlap, border)
    n = check(_lib.lib().fh_tile_plan(int(rows), int(cols), C.byref(t), None, 0), "fh_tile_plan")
    views = (_lib.FhView * max(n, 1))()
    n = check(_lib.lib().fh_tile_plan(int(rows), int(cols), C.byref(t), views, n), "fh_tile_plan")
    return [(v.x, v.y, v.w, v.h, v.edges) for v in views[:n]]


class FaceDetector:
    def __init__(self):
        self._h = None

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(_lib, "_LIB", None) is not None:
            _lib._LIB.fh_det_destroy(self._h)
        self._h = None

    # -- reference API ---------------------------------------------------------------------
    def loadModel(self, modelPath: str) -> bool:                      # face_detector.cpp:20-90
        self.close()
        self._h = _lib.lib().fh_det_create(str(modelPath).encode())
        return bool(self._h)

    def detect_records(self, image, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4,
                       max_faces: Optional[int] = None) -> np.ndarray:
        if not self._h:
            return np.zeros(0, FACE_DTYPE)                            # "Model not loaded!" :142-145
        a = _img(image)
        if a is None:
            return np.zeros(0, FACE_DTYPE)                            # :148-156
        if max_faces is None:                                         # the reference's std::vector is unbounded: every candidate row can survive
            max_faces = max(1, self.num_anchors())
        out = np.zeros(max_faces, FACE_DTYPE)
        n = check(_lib.lib().fh_det_detect(self._h, a.ctypes.data, a.shape[0], a.shape[1], a.strides[0],
                                            scoreThreshold, nmsThreshold, out.ctypes.data, max_faces), "fh_det_detect")
        return out[:n].copy()

    def detect(self, image, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4) -> List[FaceBox]:
        return [FaceBox.from_record(r) for r in self.detect_records(image, scoreThreshold, nmsThreshold)]

    # -- batch / device additions -----------------------------------------------------------
    @property
    def handle(self):
        return self._h

    def input_size(self):
        w, h = C.c_int(), C.c_int()
        check(_lib.lib().fh_det_input_size(self._h, C.byref(w), C.byref(h)), "fh_det_input_size")
        return w.value, h.value

    def num_anchors(self) -> int:
        return _lib.lib().fh_det_num_anchors(self._h)

    def macs_per_frame(self) -> float:
        return _lib.lib().fh_det_macs_per_frame(self._h)

    def detect_batch_dev(self, frames_ptr: int, n: int, rows: int, cols: int, out_ptr: int, max_per_frame: int,
                         counts_ptr: int, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4,
                         step: int = 0, frame_stride: int = 0, stream: int = 0) -> int:
        step = step or cols * 3
        frame_stride = frame_stride or rows * step
        return check(_lib.lib().fh_det_detect_batch_dev(self._h, frames_ptr, n, rows, cols, step, frame_stride,
                                                        scoreThreshold, nmsThreshold, out_ptr, max_per_frame,
                                                        counts_ptr, stream), "fh_det_detect_batch_dev")

    def detect_ragged_dev(self, frames, out_ptr: int, max_per_frame: int, counts_ptr: int, scoreThreshold: float = 0.5,
                          nmsThreshold: float = 0.4, stream: int = 0) -> int:
        """detect on frames of ANY sizes in one call (fh_det_detect_ragged_dev): frames = iterable of (device ptr, rows, cols[, step])
        or an fh_frame array (frame_array); out / counts as detect_batch_dev.  Empty frames count 0."""
        arr = frame_array(frames)
        return check(_lib.lib().fh_det_detect_ragged_dev(self._h, arr, _frame_count(arr), scoreThreshold, nmsThreshold, out_ptr,
                                                         max_per_frame, counts_ptr, stream), "fh_det_detect_ragged_dev")

    def tiling(self, tile=None, overlap: int = 0, border: int = 2):
        """A Tiling whose tile defaults to this detector's input size (views of that size reach the network at scale 1)."""
        return Tiling(self.input_size() if tile is None else tile, overlap, border)

    def detect_tiled_dev(self, frames, tiling, out_ptr: int, max_per_frame: int, counts_ptr: int, scoreThreshold: float = 0.5,
                         nmsThreshold: float = 0.4, stream: int = 0) -> int:
        """detect_ragged_dev on the whole frame AND overlapping tiles of it, merged by one NMS per frame (fh_det_detect_tiled_dev);
        tiling = Tiling(...) / self.tiling(...) or a (tile, overlap, border) tuple."""
        arr, t = frame_array(frames), _tiling(tiling)
        return check(_lib.lib().fh_det_detect_tiled_dev(self._h, arr, _frame_count(arr), C.byref(t), scoreThreshold, nmsThreshold,
                                                        out_ptr, max_per_frame, counts_ptr, stream), "fh_det_detect_tiled_dev")

    def detect_tiled_records(self, image, tiling=None, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4,
                             max_faces: Optional[int] = None) -> np.ndarray:
        """detect_records with tiled detection on one host image (fh_det_detect_tiled); tiling defaults to self.tiling()."""
        if not self._h:
            return np.zeros(0, FACE_DTYPE)
        a = _img(image)
        if a is None:
            return np.zeros(0, FACE_DTYPE)
        t = self.tiling() if tiling is None else _tiling(tiling)
        if max_faces is None:                                         # every candidate of every view can survive
            views = check(_lib.lib().fh_tile_plan(a.shape[0], a.shape[1], C.byref(t), None, 0), "fh_tile_plan")
            max_faces = max(1, self.num_anchors() * views)
        out = np.zeros(max_faces, FACE_DTYPE)
        n = check(_lib.lib().fh_det_detect_tiled(self._h, a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], C.byref(t),
                                                  scoreThreshold, nmsThreshold, out.ctypes.data, max_faces), "fh_det_detect_tiled")
        return out[:n].copy()

    def sync(self, stream: int = 0) -> None:
        """Waits for `stream`; raises if a launch of this handle failed after its asynchronous call returned (fh_det_sync)."""
        check(_lib.lib().fh_det_sync(self._h, stream), "fh_det_sync")


class FaceRecognizer:
    def __init__(self):
        self._h = None

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(_lib, "_LIB", None) is not None:
            _lib._LIB.fh_rec_destroy(self._h)
        self._h = None

    # -- reference API ---------------------------------------------------------------------
    def loadModel(self, modelPath: str) -> bool:                      # face_recognizer.cpp:21-91
        self.close()
        self._h = _lib.lib().fh_rec_create(str(modelPath).encode())
        return bool(self._h)

    def extractFeature(self, image, face) -> np.ndarray:             # face_recognizer.cpp:236-304
        if not self._h:
            return np.zeros(0, np.float32)
        a = _img(image)
        if a is None:
            return np.zeros(0, np.float32)
        rec = face.to_record() if isinstance(face, FaceBox) else np.asarray(face, FACE_DTYPE).reshape(1)
        dim = self.feature_dim()
        out = np.zeros(dim, np.float32)
        n = check(_lib.lib().fh_rec_extract(self._h, a.ctypes.data, a.shape[0], a.shape[1], a.strides[0],
                                             rec.ctypes.data, out.ctypes.data, dim), "fh_rec_extract")
        return out[:n]

    def extractFeatureSimple(self, image) -> np.ndarray:             # face_recognizer.cpp:152-234
        if not self._h:
            return np.zeros(0, np.float32)
        a = _img(image)
        if a is None:
            return np.zeros(0, np.float32)
        dim = self.feature_dim()
        out = np.zeros(dim, np.float32)
        n = check(_lib.lib().fh_rec_extract_simple(self._h, a.ctypes.data, a.shape[0], a.shape[1], a.strides[0],
                                                    out.ctypes.data, dim), "fh_rec_extract_simple")
        return out[:n]

    @staticmethod
    def compareFaces(feature1, feature2) -> float:                   # face_recognizer.cpp:320-334
        f1 = np.ascontiguousarray(feature1, np.float32).reshape(-1)
        f2 = np.ascontiguousarray(feature2, np.float32).reshape(-1)
        return float(_lib.lib().fh_compare(f1.ctypes.data, f1.size, f2.ctypes.data, f2.size))

    # -- batch / device additions -----------------------------------------------------------
    @property
    def handle(self):
        return self._h

    def feature_dim(self) -> int:
        return _lib.lib().fh_rec_feature_dim(self._h)

    def macs_per_face(self) -> float:
        return _lib.lib().fh_rec_macs_per_face(self._h)

    def set_chunk(self, n: int):
        check(_lib.lib().fh_rec_set_chunk(self._h, n), "fh_rec_set_chunk")

    def set_precision(self, mode: str = "fp32") -> float:
        """"fp32" (default, the reference's arithmetic) or "bf16x2" (split-bf16 Winograd GEMMs, opt-in).  The library gates the
        switch on its own check (max 1 - cos < 1e-3 against fp32 on a fixed batch) and raises if it fails, staying fp32.
        Returns the measured max(1 - cos)."""
        import ctypes as C
        modes = {"fp32": 0, "bf16x2": 1}
        if mode not in modes:
            raise ValueError(f"precision {mode!r}: expected one of {sorted(modes)}")
        worst = C.c_float(0.0)
        check(_lib.lib().fh_rec_set_precision(self._h, modes[mode], C.byref(worst)), "fh_rec_set_precision")
        return float(worst.value)

    def set_wino_x3(self, on: bool = True) -> int:
        """The fp32 mode's Winograd GEMMs: six bf16 MFMAs on exactly split operands (fp32 results; the default) or, off, the native
        f32 MFMA kernels.  Returns the number of layers that have the form (0 for off)."""
        return check(_lib.lib().fh_rec_set_wino_x3(self._h, 1 if on else 0), "fh_rec_set_wino_x3")

    def precision(self) -> str:
        return "bf16x2" if _lib.lib().fh_rec_get_precision(self._h) == 1 else "fp32"

    def embed_aligned_dev(self, crops_ptr: int, n: int, out_ptr: int, raw_ptr: int = 0, stream: int = 0) -> int:
        return check(_lib.lib().fh_rec_embed_aligned_dev(self._h, crops_ptr, n, out_ptr, raw_ptr, stream),
                     "fh_rec_embed_aligned_dev")

    def sync(self, stream: int = 0) -> None:
        """Waits for `stream`; raises if a launch of this handle failed after its asynchronous call returned (fh_rec_sync)."""
        check(_lib.lib().fh_rec_sync(self._h, stream), "fh_rec_sync")


def pipeline_run_dev(det: FaceDetector, rec: FaceRecognizer, frames_ptr: int, n: int, rows: int, cols: int,
                     faces_per_frame: int, faces_ptr: int, frame_of_ptr: int, emb_ptr: int,
                     scoreThreshold: float = 0.5, nmsThreshold: float = 0.4, stream: int = 0) -> int:
    """detect -> align -> embed on n HBM-resident frames; returns the number of faces embedded."""
    step = cols * 3
    return check(_lib.lib().fh_pipeline_run_dev(det.handle, rec.handle, frames_ptr, n, rows, cols, step, rows * step,
                                                scoreThreshold, nmsThreshold, faces_per_frame, faces_ptr,
                                                frame_of_ptr, emb_ptr, stream), "fh_pipeline_run_dev")


def pipeline_run_ragged_dev(det: FaceDetector, rec: FaceRecognizer, frames, faces_per_frame: int, faces_ptr: int, frame_of_ptr: int,
                            emb_ptr: int, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4, stream: int = 0) -> int:
    """pipeline_run_dev on HBM-resident frames of any sizes (fh_pipeline_run_ragged_dev); frames as FaceDetector.detect_ragged_dev.
    The output buffers hold len(frames) * faces_per_frame entries; returns the number of faces embedded."""
    arr = frame_array(frames)
    return check(_lib.lib().fh_pipeline_run_ragged_dev(det.handle, rec.handle, arr, _frame_count(arr), scoreThreshold, nmsThreshold,
                                                       faces_per_frame, faces_ptr, frame_of_ptr, emb_ptr, stream),
                 "fh_pipeline_run_ragged_dev")


def pipeline_run_tiled_dev(det: FaceDetector, rec: FaceRecognizer, frames, tiling, faces_per_frame: int, faces_ptr: int,
                           frame_of_ptr: int, emb_ptr: int, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4,
                           stream: int = 0) -> int:
    """pipeline_run_ragged_dev with tiled detection (fh_pipeline_run_tiled_dev); tiling as FaceDetector.detect_tiled_dev."""
    arr, t = frame_array(frames), _tiling(tiling)
    return check(_lib.lib().fh_pipeline_run_tiled_dev(det.handle, rec.handle, arr, _frame_count(arr), C.byref(t), scoreThreshold,
                                                      nmsThreshold, faces_per_frame, faces_ptr, frame_of_ptr, emb_ptr, stream),
                 "fh_pipeline_run_tiled_dev")


def _stream_of(stream_of, n: int):
    """HOST int32[n] stream indices of a tracker call (None = every frame on stream 0): (array kept alive by the caller, pointer)."""
    if stream_of is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(stream_of, np.int32).reshape(-1))
    if a.size != n:
        raise ValueError(f"stream_of holds {a.size} entries for {n} frames")
    return a, a.ctypes.data


def track_plan(stream_of, streams: int):
    """(order, starts) of fh_track_plan — host only: the frame indices grouped by stream, ascending within a stream, and each stream's
    offset into them (streams + 1 entries).  The order in which Tracker.update_dev walks a batch."""
    a = np.ascontiguousarray(np.asarray(stream_of, np.int32).reshape(-1))
    order, starts = np.empty(max(a.size, 1), np.int32), np.empty(max(int(streams), 0) + 1, np.int32)
    check(_lib.lib().fh_track_plan(a.ctypes.data if a.size else None, a.size, int(streams), order.ctypes.data, starts.ctypes.data),
          "fh_track_plan")
    return order[:a.size].copy(), starts


def face_quality_dev(frames, det_ptr: int, counts_ptr: int, per_frame: int, quality_ptr: int, n: Optional[int] = None,
                     rows: Optional[int] = None, cols: Optional[int] = None, step: Optional[int] = None, stream: int = 0) -> int:
    """The quality score of every detected face (include/facehip.h, "face quality") into quality_ptr = int32 [n][per_frame]; entries
    behind a frame's count get 0.  frames = a device pointer of n uniform frames of rows x cols (row pitch step, default cols * 3; the
    frames follow each other at rows * step) — or, with n = None, frames of any sizes as FaceDetector.detect_ragged_dev takes them
    (fh_face_quality_ragged_dev)."""
    if n is None:
        arr = frame_array(frames)
        return check(_lib.lib().fh_face_quality_ragged_dev(arr, _frame_count(arr), det_ptr, counts_ptr, per_frame, quality_ptr, stream),
                     "fh_face_quality_ragged_dev")
    step = cols * 3 if step is None else step
    return check(_lib.lib().fh_face_quality_dev(frames, n, rows, cols, step, rows * step, det_ptr, counts_ptr, per_frame, quality_ptr,
                                                stream), "fh_face_quality_dev")


class Tracker:
    """fh_tracker: device-resident face tracks per camera stream (include/facehip.h, "face tracker").  `refresh` = 0 embeds a track
    once, when it opens; k > 0 again every k frames.  A track survives `max_missed` consecutive frames without a detection."""

    def __init__(self, streams: int = 1, max_tracks: int = _lib.TRACK_MAX, iou_thr: float = 0.3, max_missed: int = 0, refresh: int = 0):
        self._h = _lib.lib().fh_tracker_create(int(streams), int(max_tracks), float(iou_thr), int(max_missed), int(refresh))
        if not self._h:
            raise _lib.FaceHipError(f"fh_tracker_create failed: {_lib.last_error()}")
        self.streams, self.max_tracks = int(streams), int(max_tracks)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().fh_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    def update_dev(self, det_ptr: int, counts_ptr: int, n: int, per_frame: int, track_ptr: int, embed_ptr: int, stream_of=None,
                   stream: int = 0, slot_ptr=None, quality_ptr=None) -> int:
        """Steps 1-4 of the contract on n frames of [per_frame] records; writes track ids and embed flags [n][per_frame] — and, with
        slot_ptr, the slot of each detection's track (fh_track_update_slots_dev), which identify_dev needs.  quality_ptr = the faces'
        qualities [n][per_frame] (face_quality_dev): what the best-shot policy decides by (fh_track_update_q_dev)."""
        keep, sp = _stream_of(stream_of, n)
        if quality_ptr is not None:
            return check(_lib.lib().fh_track_update_q_dev(self._h, det_ptr, counts_ptr, n, per_frame, sp, track_ptr, embed_ptr, slot_ptr,
                                                          quality_ptr, stream), "fh_track_update_q_dev")
        if slot_ptr is None:
            return check(_lib.lib().fh_track_update_dev(self._h, det_ptr, counts_ptr, n, per_frame, sp, track_ptr, embed_ptr, stream),
                         "fh_track_update_dev")
        return check(_lib.lib().fh_track_update_slots_dev(self._h, det_ptr, counts_ptr, n, per_frame, sp, track_ptr, embed_ptr, slot_ptr,
                                                          stream), "fh_track_update_slots_dev")

    def set_bestshot(self, num: int = 5, den: int = 4, min_gap: int = 1) -> None:
        """Switch the best-shot policy on: a track is embedded again when its face's quality q has become better than the best one
        embedded so far by more than num / den (q * den > best_q * num) and min_gap frames or more have passed since its last
        embedding.  Clears the per-slot best qualities."""
        check(_lib.lib().fh_tracker_set_bestshot(self._h, 1, int(num), int(den), int(min_gap)), "fh_tracker_set_bestshot")

    def clear_bestshot(self) -> None:
        """Switch the best-shot policy off (and clear the per-slot best qualities)."""
        check(_lib.lib().fh_tracker_set_bestshot(self._h, 0, 1, 1, 1), "fh_tracker_set_bestshot")

    def best_quality(self, stream: int = 0) -> np.ndarray:
        """The best embedded quality of the live slots of one stream, ascending (the positions of state()), int32."""
        out = np.zeros(self.max_tracks, np.int32)
        live = check(_lib.lib().fh_tracker_get_quality(self._h, int(stream), out.ctypes.data), "fh_tracker_get_quality")
        return out[:live].copy()

    def quality_ptr(self) -> int:
        """Device pointer of the [n][F] qualities of the last pipeline call with the best-shot policy on (a stage hook for tests)."""
        return _lib.lib().fh_tracker_quality_dev(self._h) or 0

    def enable_identity(self, dim: int, pool: int = _lib.TRACK_POOL_SUM) -> None:
        """Allocate (or clear and re-size) the per-track identity state: a running template of `dim` floats per track slot, pooled as
        the sum of the track's embeddings (TRACK_POOL_SUM), that sum weighted by the faces' qualities (TRACK_POOL_WEIGHTED; only after
        set_bestshot() or clear_bestshot() has opted the tracker into the quality feature) or just the latest one (TRACK_POOL_LAST)."""
        check(_lib.lib().fh_tracker_enable_identity(self._h, int(dim), int(pool)), "fh_tracker_enable_identity")
        self.identity_dim = int(dim)

    def identify_dev(self, gallery, threshold: float, track_ptr: int, slot_ptr: int, embed_ptr: int, emb_ptr, total: int, n: int,
                     per_frame: int, label_ptr: int, score_ptr: int, stream_of=None, stream: int = 0, quality_ptr=None,
                     root_ptr=None) -> int:
        """After update_dev(..., slot_ptr=...) and the embedding of the `total` flagged faces (emb_ptr = [total][dim], in select_dev's
        order): pool each into its track's template, label the templates against `gallery`, and write a label and a score for EVERY
        entry [n][per_frame] — the faces that were not embedded carry their track's.  quality_ptr = the faces' qualities
        [n][per_frame], which TRACK_POOL_WEIGHTED needs (fh_track_identify_q_dev).  root_ptr = int32 [n][per_frame] selects
        fh_track_identify_link_dev: the chain root of every tracked entry (its own track id unless enable_relink() is on), the call a
        tracker with re-linking on needs."""
        keep, sp = _stream_of(stream_of, n)
        if root_ptr is not None:
            return check(_lib.lib().fh_track_identify_link_dev(self._h, gallery._h if gallery is not None else None, float(threshold),
                                                               track_ptr, slot_ptr, embed_ptr, quality_ptr, emb_ptr, int(total), n,
                                                               per_frame, sp, label_ptr, score_ptr, root_ptr, stream),
                         "fh_track_identify_link_dev")
        if quality_ptr is not None:
            return check(_lib.lib().fh_track_identify_q_dev(self._h, gallery._h if gallery is not None else None, float(threshold),
                                                            track_ptr, slot_ptr, embed_ptr, quality_ptr, emb_ptr, int(total), n, per_frame,
                                                            sp, label_ptr, score_ptr, stream), "fh_track_identify_q_dev")
        return check(_lib.lib().fh_track_identify_dev(self._h, gallery._h if gallery is not None else None, float(threshold), track_ptr,
                                                      slot_ptr, embed_ptr, emb_ptr, int(total), n, per_frame, sp, label_ptr, score_ptr,
                                                      stream), "fh_track_identify_dev")

    def set_stream_masks(self, masks=None) -> None:
        """A watchlist per camera (fh_tracker_set_stream_masks): masks = uint32[streams]; identify_dev then labels every face of
        stream s against the gallery rows whose tag shares a bit with masks[s] (Gallery.set_tags).  None switches the masks off."""
        if masks is None:
            check(_lib.lib().fh_tracker_set_stream_masks(self._h, None), "fh_tracker_set_stream_masks")
            return
        masks = np.ascontiguousarray(np.asarray(masks).reshape(-1).astype(np.uint32))
        if masks.size != self.streams:
            raise ValueError("set_stream_masks: need one mask per stream")
        check(_lib.lib().fh_tracker_set_stream_masks(self._h, masks.ctypes.data), "fh_tracker_set_stream_masks")

    def queries_ptr(self) -> int:
        """Device pointer of the [total][dim] queries of the last identify_dev (a stage hook for tests)."""
        return _lib.lib().fh_tracker_queries_dev(self._h) or 0

    def identity(self, stream: int = 0, sums: bool = False):
        """The live slots' identities, ascending (the positions of state()), as TRACK_IDENT_DTYPE records; with sums=True: (records,
        float32 [live][dim] running templates)."""
        out = np.zeros(self.max_tracks, _lib.TRACK_IDENT_DTYPE)
        acc = np.zeros((self.max_tracks, getattr(self, "identity_dim", 0)), np.float32) if sums else None
        live = check(_lib.lib().fh_tracker_get_identity(self._h, int(stream), out.ctypes.data, acc.ctypes.data if sums else None),
                     "fh_tracker_get_identity")
        return (out[:live].copy(), acc[:live].copy()) if sums else out[:live].copy()

    def enable_relink(self, memory: int = 64, link_thr: float = 0.6, max_age: int = 150) -> None:
        """Switch track re-linking on (after enable_identity): a newly opened track whose first embedding scores above link_thr against
        the template of a track lost at most max_age frames ago continues it — template, count and chain root.  `memory` = how many
        lost tracks per stream are remembered beyond those still sitting in slots.  The defaults (the reference's match threshold;
        five seconds at 30 fps) are a proposal: their effect on accuracy has not been measured.  Clears the identity state."""
        check(_lib.lib().fh_tracker_enable_relink(self._h, int(memory), float(link_thr), int(max_age)), "fh_tracker_enable_relink")
        self.link_memory = int(memory)

    def roots_ptr(self) -> int:
        """Device pointer of the [n][F] chain roots of the last identified pipeline call with re-linking on (a stage hook)."""
        return _lib.lib().fh_tracker_roots_dev(self._h) or 0

    def links(self, stream: int = 0, sums: bool = False):
        """The whole re-linking table of one stream by row (slot rows, then the memory) as TRACK_LINK_DTYPE records, free rows with
        owner = -1; with sums=True: (records, float32 [rows][dim] templates)."""
        rows = check(_lib.lib().fh_tracker_get_links(self._h, int(stream), None, None), "fh_tracker_get_links")   # the library's count
        out = np.zeros(rows, _lib.TRACK_LINK_DTYPE)
        acc = np.zeros((rows, getattr(self, "identity_dim", 0)), np.float32) if sums else None
        check(_lib.lib().fh_tracker_get_links(self._h, int(stream), out.ctypes.data, acc.ctypes.data if sums else None),
              "fh_tracker_get_links")
        return (out, acc) if sums else out

    @staticmethod
    def select_dev(det_ptr: int, embed_ptr: int, n: int, per_frame: int, faces_ptr: int, frame_of_ptr: int, track_ptr: int,
                   track_of_ptr: int, total_ptr: int, stream: int = 0) -> int:
        """The flagged records, densely in (frame, slot) order, with frame index and track id; total_ptr[0] = their number."""
        return check(_lib.lib().fh_track_select_dev(det_ptr, embed_ptr, n, per_frame, faces_ptr, frame_of_ptr, track_ptr, track_of_ptr,
                                                    total_ptr, stream), "fh_track_select_dev")

    def reset(self, stream: int = -1) -> None:
        check(_lib.lib().fh_tracker_reset(self._h, int(stream)), "fh_tracker_reset")

    def state(self, stream: int = 0, counters: bool = False):
        """The live slots of one stream, ascending, as TRACK_DTYPE records; with counters=True: (records, frame_no, next_id)."""
        out = np.zeros(self.max_tracks, TRACK_DTYPE)
        fno, nid = C.c_int(), C.c_int()
        live = check(_lib.lib().fh_tracker_get_state(self._h, int(stream), out.ctypes.data, C.byref(fno), C.byref(nid)),
                     "fh_tracker_get_state")
        return (out[:live].copy(), fno.value, nid.value) if counters else out[:live].copy()


def pipeline_run_tracked_dev(det: FaceDetector, rec: FaceRecognizer, tracker: Tracker, frames_ptr: int, n: int, rows: int, cols: int,
                             faces_per_frame: int, all_ptr: int, counts_ptr: int, track_ptr: int, faces_ptr: int, frame_of_ptr: int,
                             track_of_ptr: int, emb_ptr: int, stream_of=None, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4,
                             stream: int = 0) -> int:
    """pipeline_run_dev for video (fh_pipeline_run_tracked_dev): detect every frame, track, and align + embed only the faces that open a
    track, are due for a refresh or found no free slot.  all_ptr / counts_ptr / track_ptr = every frame's records [n][F], counts [n]
    and track ids [n][F]; the embedded list (faces, frame index, track id, embedding) holds up to n * F entries.  Returns its length."""
    step = cols * 3
    keep, sp = _stream_of(stream_of, n)
    return check(_lib.lib().fh_pipeline_run_tracked_dev(det.handle, rec.handle, tracker.handle if tracker is not None else None,
                                                        frames_ptr, n, rows, cols, step, rows * step, sp, scoreThreshold, nmsThreshold,
                                                        faces_per_frame, all_ptr, counts_ptr, track_ptr, faces_ptr, frame_of_ptr,
                                                        track_of_ptr, emb_ptr, stream), "fh_pipeline_run_tracked_dev")


def pipeline_run_identified_dev(det: FaceDetector, rec: FaceRecognizer, tracker: Tracker, gallery, threshold: float, frames_ptr: int, n: int,
                                rows: int, cols: int, faces_per_frame: int, all_ptr: int, counts_ptr: int, track_ptr: int, faces_ptr: int,
                                frame_of_ptr: int, track_of_ptr: int, emb_ptr: int, label_ptr: int, score_ptr: int, stream_of=None,
                                scoreThreshold: float = 0.5, nmsThreshold: float = 0.4, stream: int = 0) -> int:
    """pipeline_run_tracked_dev plus a name for every face (fh_pipeline_run_identified_dev): the embedded faces are pooled into their
    tracks' templates and labelled against `gallery`; label_ptr / score_ptr = [n][F], where the faces that were not embedded carry their
    track's answer.  The tracker needs enable_identity(rec.feature dim).  Returns the number of faces embedded."""
    step = cols * 3
    keep, sp = _stream_of(stream_of, n)
    return check(_lib.lib().fh_pipeline_run_identified_dev(det.handle, rec.handle, tracker.handle if tracker is not None else None,
                                                           gallery._h if gallery is not None else None, float(threshold), frames_ptr, n,
                                                           rows, cols, step, rows * step, sp, scoreThreshold, nmsThreshold, faces_per_frame,
                                                           all_ptr, counts_ptr, track_ptr, faces_ptr, frame_of_ptr, track_of_ptr, emb_ptr,
                                                           label_ptr, score_ptr, stream), "fh_pipeline_run_identified_dev")


def pipeline_images(det: FaceDetector, rec: FaceRecognizer, images, faces_per_frame: int = 1, scoreThreshold: float = 0.5,
                    nmsThreshold: float = 0.4, cap: Optional[int] = None):
    """The enrolment loop over decoded photographs (main.cpp:42,88-104: imread, detect, extractFeature per file) as ONE call:
    images = list of uint8[rows, cols, 3] BGR arrays of any sizes (None / empty = no image).  Returns (faces: FACE_DTYPE[m],
    frame_of: int32[m], emb: float32[m][dim]) with m = the total number of faces (the first min(count, faces_per_frame) of every
    image, in image order), or the first `cap` of them when cap is given."""
    imgs = [_img(im) for im in images]
    n = len(imgs)
    dim = rec.feature_dim()
    if n == 0:
        return np.zeros(0, FACE_DTYPE), np.zeros(0, np.int32), np.zeros((0, dim), np.float32)
    arr = frame_array([None if a is None else (a.ctypes.data, a.shape[0], a.shape[1], a.strides[0]) for a in imgs])
    room = n * faces_per_frame if cap is None else max(int(cap), 0)
    faces = np.zeros(max(room, 1), FACE_DTYPE); frame_of = np.zeros(max(room, 1), np.int32); emb = np.zeros((max(room, 1), dim), np.float32)
    total = check(_lib.lib().fh_pipeline_run_images(det.handle, rec.handle, arr, n, scoreThreshold, nmsThreshold, faces_per_frame,
                                                    faces.ctypes.data, frame_of.ctypes.data, emb.ctypes.data, room),
                  "fh_pipeline_run_images")
    m = min(total, room)
    return faces[:m].copy(), frame_of[:m].copy(), emb[:m].copy()


def _blobs(files):
    """(fh_blob array, the buffers it points into) from a list of paths or bytes-like objects; an unreadable path is an empty blob."""
    keep = []
    arr = (_lib.FhBlob * max(len(files), 1))()
    for i, f in enumerate(files):
        if isinstance(f, (bytes, bytearray, memoryview)):
            data = bytes(f)
        else:
            try:
                with open(f, "rb") as fp:
                    data = fp.read()
            except OSError:
                data = b""
        buf = C.create_string_buffer(data, len(data)) if data else None
        keep.append(buf)
        arr[i].bytes, arr[i].n = (C.addressof(buf) if buf is not None else None), len(data)
    return arr, keep


class JpegDecoder:
    """fh_jpegdec: JPEG files -> BGR pictures with the entropy decoding on host threads and everything behind it (IDCT, up-sampling,
    colour conversion, EXIF orientation) on the GPU; the pixels are fh_image_decode's, bit for bit."""

    def __init__(self):
        self.handle = _lib.lib().fh_jpegdec_create()
        if not self.handle:
            raise _lib.FaceHipError(f"fh_jpegdec_create failed: {_lib.last_error()}")

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            _lib.lib().fh_jpegdec_destroy(h)

    def decode_dev(self, files, threads: int = 0, stream: int = 0):
        """fh_jpeg_decode_batch: files = list of paths or bytes.  Returns (fh_frame array of DEVICE images, valid until the next call on
        this decoder; status int32[n]: 0 JPEG on the device, 1 another format decoded on the host, < 0 not decodable = empty frame)."""
        files = list(files)
        n = len(files)
        blobs, keep = _blobs(files)
        frames = (_lib.FhFrame * max(n, 1))()
        frames._n = n
        status = np.full(max(n, 1), -1, np.int32)
        if n:
            check(_lib.lib().fh_jpeg_decode_batch(self.handle, blobs, n, int(threads), frames, status.ctypes.data, stream), "fh_jpeg_decode_batch")
        del keep
        return frames, status[:n]

    def decode(self, files, threads: int = 0):
        """decode_dev, then the pictures copied back: (list of uint8[rows, cols, 3] BGR arrays, None for a file that cannot be decoded;
        status as decode_dev)."""
        frames, status = self.decode_dev(files, threads)
        out = []
        for i in range(len(status)):
            f = frames[i]
            if not f.bgr:
                out.append(None)
                continue
            a = np.empty((f.rows, f.cols, 3), np.uint8)
            check(_lib.lib().fh_memcpy_d2h(a.ctypes.data, f.bgr, a.nbytes), "fh_memcpy_d2h")   # (synchronous: behind the decode on stream 0)
            out.append(a)
        return out, status


class JpegEncoder:
    """fh_jpegenc: BGR pictures -> baseline JPEG files with colour conversion, chroma down-sampling, the forward DCT and quantisation on
    the GPU and the Huffman coding on host threads (coder = "host", the default) or on the GPU as well (coder = "device"); the
    coefficients are the ones libjpeg stores for the same pixels, bit for bit, and the bytes are fh_jpeg_write(fh_jpeg_forward(...))'s."""

    SUBSAMPLING = {"4:4:4": 0, "444": 0, 0: 0, "4:2:2": 1, "422": 1, 1: 1, "4:2:0": 2, "420": 2, 2: 2}

    def __init__(self):
        self.handle = _lib.lib().fh_jpegenc_create()
        if not self.handle:
            raise _lib.FaceHipError(f"fh_jpegenc_create failed: {_lib.last_error()}")

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            _lib.lib().fh_jpegenc_destroy(h)

    def encode_dev(self, frames, quality: int = 95, subsampling="4:2:0", threads: int = 0, stream: int = 0, coder: str = "host"):
        """fh_jpeg_encode_batch: frames = DEVICE pictures as frame_array takes them ((ptr, rows, cols[, step]) or None).  Blocking.
        coder = "host": Huffman coding on `threads` host threads; "device": on the GPU too (fh_jpeg_encode_batch_gpu; `threads` is not
        used), only the files' bytes come back.  The same bytes either way.  Returns a list of bytes, None for an empty frame."""
        if coder not in ("host", "device"):
            raise ValueError('coder must be "host" or "device"')
        arr = frame_array(frames)
        n = _frame_count(arr)
        if n == 0:
            return []
        blobs = (_lib.FhBlob * n)()
        if coder == "device":
            check(_lib.lib().fh_jpeg_encode_batch_gpu(self.handle, arr, n, int(quality), self.SUBSAMPLING[subsampling], blobs, stream),
                  "fh_jpeg_encode_batch_gpu")
        else:
            check(_lib.lib().fh_jpeg_encode_batch(self.handle, arr, n, int(quality), self.SUBSAMPLING[subsampling], int(threads), blobs, stream),
                  "fh_jpeg_encode_batch")
        return [C.string_at(b.bytes, b.n) if b.bytes else None for b in blobs]

    def encode(self, frames, quality: int = 95, subsampling="4:2:0", threads: int = 0, coder: str = "host"):
        """encode_dev on HOST pictures (uint8[rows, cols, 3] BGR arrays; None or an empty array = an empty frame), uploaded first."""
        import torch
        imgs = [_img(f) for f in frames]
        keep = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in imgs]
        torch.cuda.synchronize()
        out = self.encode_dev([None if t is None else (t.data_ptr(), t.shape[0], t.shape[1]) for t in keep], quality, subsampling, threads,
                              coder=coder)
        del keep
        return out


def imwrite(path: str, image, quality: int = 95, subsampling="4:2:0") -> bool:
    """cv::imwrite(path.jpg, image): the host encoder (fh_imwrite_jpeg).  False when the file cannot be written."""
    a = _img(image)
    if a is None:
        return False
    return _lib.lib().fh_imwrite_jpeg(str(path).encode(), a.ctypes.data, a.shape[0], a.shape[1], a.strides[0], int(quality),
                                      JpegEncoder.SUBSAMPLING[subsampling]) == 0


def face_chips(rec: FaceRecognizer, image, faces, quality: int = 95, subsampling="4:2:0", encoder: Optional[JpegEncoder] = None,
               coder: str = "host"):
    """The aligned crop of every face of one HOST picture as a JPEG file: fh_rec_align_dev -> fh_jpeg_encode_batch, pixels never
    leave the device (nor, with coder = "device", the coefficients: JpegEncoder.encode_dev).  faces = FACE_DTYPE records (FaceDetector.detect_records).  Returns (list of bytes — None for a
    face whose crop is empty —, the crops uint8[n, H, W, 3] as the device made them)."""
    import torch
    a = _img(image)
    faces = np.ascontiguousarray(faces, FACE_DTYPE)
    n = len(faces)
    h, w = C.c_int(0), C.c_int(0)
    check(_lib.lib().fh_rec_input_size(rec.handle, C.byref(h), C.byref(w)), "fh_rec_input_size")
    if a is None or n == 0:
        return [], np.zeros((0, h.value, w.value, 3), np.uint8)
    img = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_faces = torch.from_numpy(faces.view(np.uint8).reshape(-1).copy()).cuda()
    d_fo = torch.zeros(n, dtype=torch.int32, device="cuda")
    crops = torch.zeros((n, h.value, w.value, 3), dtype=torch.uint8, device="cuda")
    ok = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    check(_lib.lib().fh_rec_align_dev(rec.handle, img.data_ptr(), a.shape[0], a.shape[1], a.shape[1] * 3, 0, d_faces.data_ptr(), d_fo.data_ptr(),
                                      n, crops.data_ptr(), ok.data_ptr(), 0), "fh_rec_align_dev")
    rec.sync()
    live = ok.cpu().numpy() != 0
    enc = encoder if encoder is not None else JpegEncoder()
    one = h.value * w.value * 3
    files = enc.encode_dev([(crops.data_ptr() + i * one, h.value, w.value) if live[i] else None for i in range(n)], quality, subsampling,
                           coder=coder)
    return files, crops.cpu().numpy()


def pipeline_files(det: FaceDetector, rec: FaceRecognizer, files, faces_per_frame: int = 1, scoreThreshold: float = 0.5,
                   nmsThreshold: float = 0.4, cap: Optional[int] = None, threads: int = 0, decoder: Optional[JpegDecoder] = None):
    """pipeline_images from FILES (paths or bytes): JPEGs are entropy-decoded on `threads` host threads and reconstructed on the GPU
    (fh_pipeline_run_files), other formats decoded on the host.  Returns (faces, frame_of, emb, status) — the first three exactly as
    imread per file + pipeline_images gives them; status[i] 0 / 1 / < 0 as JpegDecoder.decode_dev."""
    files = list(files)
    n = len(files)
    dim = rec.feature_dim()
    if n == 0:
        return np.zeros(0, FACE_DTYPE), np.zeros(0, np.int32), np.zeros((0, dim), np.float32), np.zeros(0, np.int32)
    dec = decoder if decoder is not None else JpegDecoder()
    blobs, keep = _blobs(files)
    room = n * faces_per_frame if cap is None else max(int(cap), 0)
    faces = np.zeros(max(room, 1), FACE_DTYPE); frame_of = np.zeros(max(room, 1), np.int32); emb = np.zeros((max(room, 1), dim), np.float32)
    status = np.full(n, -1, np.int32)
    total = check(_lib.lib().fh_pipeline_run_files(det.handle, rec.handle, dec.handle, blobs, n, int(threads), scoreThreshold, nmsThreshold,
                                                   faces_per_frame, faces.ctypes.data, frame_of.ctypes.data, emb.ctypes.data, room,
                                                   status.ctypes.data), "fh_pipeline_run_files")
    del keep
    m = min(total, room)
    return faces[:m].copy(), frame_of[:m].copy(), emb[:m].copy(), status


def pipeline_submit_dev(det: FaceDetector, rec: FaceRecognizer, frames_ptr: int, n: int, rows: int, cols: int,
                        faces_per_frame: int, faces_ptr: int, frame_of_ptr: int, emb_ptr: int, total_ptr: int,
                        stream_det: int, stream_rec: int, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4) -> int:
    """Two-stream detect -> align -> embed: detector on stream_det, recogniser on stream_rec; the host waits for the
    detector's face count only.  Returns the number of faces."""
    step = cols * 3
    return check(_lib.lib().fh_pipeline_submit_dev(det.handle, rec.handle, frames_ptr, n, rows, cols, step, rows * step,
                                                   scoreThreshold, nmsThreshold, faces_per_frame, faces_ptr, frame_of_ptr,
                                                   emb_ptr, total_ptr, stream_det, stream_rec), "fh_pipeline_submit_dev")


class FrameStream:
    """Streaming front end for batches of HOST frames (fh_stream_*): the reference's webcam loop (src/main.cpp:214-258) over
    batches.  submit() uploads + queues a batch and returns its face count, collect() returns the oldest batch's results."""

    def __init__(self, det: FaceDetector, rec: FaceRecognizer, frames_per_batch: int, rows: int, cols: int, faces_per_frame: int = 1):
        self._h = _lib.lib().fh_stream_create(det.handle, rec.handle, frames_per_batch, rows, cols, faces_per_frame)
        if not self._h:
            raise _lib.FaceHipError("fh_stream_create failed: " + _lib.last_error())
        self._keep = (det, rec)
        self.cap = frames_per_batch * faces_per_frame
        self.dim = rec.feature_dim()

    def close(self):
        if getattr(self, "_h", None) and getattr(_lib, "_LIB", None) is not None:
            _lib._LIB.fh_stream_destroy(self._h)
        self._h = None

    __del__ = close

    def submit(self, frames, scoreThreshold: float = 0.5, nmsThreshold: float = 0.4) -> int:
        """frames: contiguous uint8 [n, rows, cols, 3] BGR (a numpy array, or an int pointer with n given as frames[1])."""
        if isinstance(frames, tuple):
            ptr, n = frames
        else:
            a = np.ascontiguousarray(frames, np.uint8)
            ptr, n = a.ctypes.data, a.shape[0]
        return check(_lib.lib().fh_stream_submit(self._h, ptr, n, scoreThreshold, nmsThreshold), "fh_stream_submit")

    def collect(self):
        faces = np.zeros(self.cap, FACE_DTYPE); frame_of = np.zeros(self.cap, np.int32); emb = np.zeros((self.cap, self.dim), np.float32)
        n = check(_lib.lib().fh_stream_collect(self._h, faces.ctypes.data, frame_of.ctypes.data, emb.ctypes.data, self.cap), "fh_stream_collect")
        return faces[:n], frame_of[:n], emb[:n]

    def collect_count(self) -> int:
        return check(_lib.lib().fh_stream_collect(self._h, None, None, None, 0), "fh_stream_collect")


class Gallery:
    """1:N generalisation of compareFaces: top-k mapped scores (dot+1)/2 over enrolled rows.

    scan="f16": fp16 scan + exact fp32 re-rank (fh_gallery_set_scan), the same answer as "fp32" bit for bit; G x dim x 2 bytes more."""

    _SCANS = {"fp32": 0, "f16": 1}

    def __init__(self, dim: int = 512, scan: str = "fp32"):
        self._h = _lib.lib().fh_gallery_create(dim)
        self.dim = dim
        if scan != "fp32":
            self.set_scan(scan)

    def set_scan(self, mode: str = "fp32"):
        """"fp32" (default) or "f16" (fp16 candidate scan, fp32 re-score, per-query certificate, fp32 fallback); synchronous."""
        if mode not in self._SCANS:
            raise ValueError(f"scan {mode!r}: expected one of {sorted(self._SCANS)}")
        check(_lib.lib().fh_gallery_set_scan(self._h, self._SCANS[mode]), "fh_gallery_set_scan")

    @property
    def scan(self) -> str:
        return "f16" if _lib.lib().fh_gallery_get_scan(self._h) == 1 else "fp32"

    def scan_stats(self):
        """(certified, fallback): queries answered by the certified fp16 path / by the fp32 fallback since the last call (resets)."""
        c, f = C.c_longlong(0), C.c_longlong(0)
        check(_lib.lib().fh_gallery_scan_stats(self._h, C.byref(c), C.byref(f)), "fh_gallery_scan_stats")
        return int(c.value), int(f.value)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None and getattr(_lib, "_LIB", None) is not None:
            _lib._LIB.fh_gallery_destroy(self._h)
        self._h = None

    def upload(self, rows_ptr: int, n: int, on_device: bool, index_base: int = 0, ids_ptr: Optional[int] = None):
        """Replace the row set.  ids_ptr (int32[n], host or device as the rows): one identity id >= 0 per row -> a LABELLED gallery
        (fh_gallery_upload_ids), for topk_ids_dev / label_ids_dev / remove_ids."""
        if ids_ptr is None:
            check(_lib.lib().fh_gallery_upload(self._h, rows_ptr, n, int(on_device), index_base), "fh_gallery_upload")
        else:
            check(_lib.lib().fh_gallery_upload_ids(self._h, rows_ptr, ids_ptr, n, int(on_device), index_base), "fh_gallery_upload_ids")

    def topk_dev(self, q_ptr: int, nq: int, k: int, scores_ptr: int, idx_ptr: int, stream: int = 0):
        check(_lib.lib().fh_gallery_topk_dev(self._h, q_ptr, nq, k, scores_ptr, idx_ptr, stream), "fh_gallery_topk_dev")

    def enroll(self, rows, ids=None) -> int:
        """Append L2-normalised feature rows (host array [n, dim]); the webcam loop's 's' key (main.cpp:253-256).
        ids (int32[n] >= 0, or one int for all rows): the identity each row is a template of (a labelled gallery).
        Returns the index of the first new row."""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, self.dim)
        if ids is None:
            return check(_lib.lib().fh_gallery_enroll(self._h, rows.ctypes.data, rows.shape[0], 0), "fh_gallery_enroll")
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(ids, np.int32).reshape(-1), (rows.shape[0],)))
        return check(_lib.lib().fh_gallery_enroll_ids(self._h, rows.ctypes.data, ids.ctypes.data, rows.shape[0], 0), "fh_gallery_enroll_ids")

    def topk_ids_dev(self, q_ptr: int, nq: int, k: int, scores_ptr: int, ids_ptr: int, rows_ptr: Optional[int] = None, stream: int = 0):
        """The best k IDENTITIES per query, each by its best row: [nq][k] scores / identity ids / (optional) global row indices,
        empty slots (-1.0, -1, -1).  Scores are the fp32 scan's, bit for bit."""
        check(_lib.lib().fh_gallery_topk_ids_dev(self._h, q_ptr, nq, k, scores_ptr, ids_ptr, rows_ptr, stream), "fh_gallery_topk_ids_dev")

    def label_ids_dev(self, q_ptr: int, nq: int, threshold: float, ids_ptr: int, scores_ptr: int, stream: int = 0):
        """ids[q] = the best identity's id if (dot+1)/2 > threshold else -1."""
        check(_lib.lib().fh_gallery_label_ids_dev(self._h, q_ptr, nq, threshold, ids_ptr, scores_ptr, stream), "fh_gallery_label_ids_dev")

    def remove_ids(self, ids) -> int:
        """Un-enrol: remove every row of the listed identities (stable compaction; later rows' global indices shrink).
        Returns the number of rows removed."""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        if ids.size == 0:
            return 0
        return check(_lib.lib().fh_gallery_remove_ids(self._h, ids.ctypes.data, ids.size), "fh_gallery_remove_ids")

    def ids(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Identity ids of rows [first, first + n) by position (default: to the end)."""
        if n is None:
            n = len(self) - first
        out = np.empty(max(n, 0), np.int32)
        check(_lib.lib().fh_gallery_get_ids(self._h, first, n, out.ctypes.data if n > 0 else None), "fh_gallery_get_ids")
        return out

    def rows(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """fp32 rows [first, first + n) by position (default: to the end), of either kind of gallery (fh_gallery_get_rows)."""
        if n is None:
            n = len(self) - first
        out = np.empty((max(n, 0), self.dim), np.float32)
        check(_lib.lib().fh_gallery_get_rows(self._h, first, n, out.ctypes.data if n > 0 else None), "fh_gallery_get_rows")
        return out

    _FUSE = {"unit": 0, "sum": 1}

    def fuse(self, dst: Optional["Gallery"] = None, mode: str = "unit") -> "Gallery":
        """Template pooling (fh_gallery_fuse_ids): `dst` (default: a new gallery of the same dim) is replaced by one row per identity
        of this labelled gallery, ascending ids — the identity's rows summed in a fixed order, L2-normalised ("unit") or as the sum is
        ("sum"); an identity of one template keeps its row verbatim.  Synchronous; returns dst."""
        if mode not in self._FUSE:
            raise ValueError(f"fuse mode {mode!r}: expected one of {sorted(self._FUSE)}")
        if dst is None:
            dst = Gallery(self.dim)
        check(_lib.lib().fh_gallery_fuse_ids(self._h, dst._h, self._FUSE[mode]), "fh_gallery_fuse_ids")
        return dst

    def self_scores_dev(self, tmpl: "Gallery", scores_ptr: int, stream: int = 0):
        """The mislabel audit: scores[r] = (dot(row r, tmpl's row of row r's identity) + 1) / 2, -1 where tmpl lacks the identity;
        tmpl = the result of fuse() (fh_gallery_self_scores_dev).  Asynchronous on `stream`."""
        check(_lib.lib().fh_gallery_self_scores_dev(self._h, tmpl._h, scores_ptr, stream), "fh_gallery_self_scores_dev")

    def cluster_dev(self, threshold: float, min_pts: int, noise, labels_ptr: int, info_ptr: Optional[int] = None, stream: int = 0):
        """Exact DBSCAN over the gallery's own rows (fh_gallery_cluster_dev): labels[len(self)] (device int32) = the position of the
        cluster's smallest core row, -1 ("none") or the row's own position ("self") for noise; info[4] (device int32, optional) =
        (clusters, core, border, noise).  Two rows are linked iff the fp32 scan scores the pair above `threshold`; a row is core iff it
        has at least min_pts - 1 such neighbours.  Asynchronous on `stream`."""
        check(_lib.lib().fh_gallery_cluster_dev(self._h, threshold, min_pts, _noise_mode(noise), labels_ptr, info_ptr, stream),
              "fh_gallery_cluster_dev")

    def cluster(self, threshold: float, min_pts: int = 1, noise="none"):
        """(labels int32[len(self)], info int32[4]) of cluster_dev — a synchronous convenience that allocates and copies back."""
        import torch
        n = len(self)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        info = torch.empty(4, dtype=torch.int32, device="cuda")
        self.cluster_dev(threshold, min_pts, noise, labels.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return labels[:n].cpu().numpy(), info.cpu().numpy()

    def pair_hist_dev(self, hist_ptr: int, nan_ptr: Optional[int] = None, stream: int = 0):
        """Exact genuine / impostor score histograms over all unordered pairs of the gallery's rows (fh_gallery_pair_hist_dev):
        hist[2][HIST_BINS] (device uint64; plane 0 = pairs with the same id, plane 1 = the rest) and nan[2] (device uint64, optional:
        the NaN-scored pairs per class) are overwritten.  A pair's score is the fp32 scan's, its bin is hist_bin's.  Needs a labelled
        gallery.  Asynchronous on `stream`."""
        check(_lib.lib().fh_gallery_pair_hist_dev(self._h, hist_ptr, nan_ptr, stream), "fh_gallery_pair_hist_dev")

    def pair_hist(self):
        """(hist uint64[2, HIST_BINS], nan uint64[2]) of pair_hist_dev — a synchronous convenience that allocates and copies back;
        roc_from_hist reads the operating thresholds off it."""
        import torch
        buf = torch.empty(2 * _lib.HIST_BINS + 2, dtype=torch.int64, device="cuda")
        self.pair_hist_dev(buf.data_ptr(), buf.data_ptr() + 2 * _lib.HIST_BINS * 8, torch.cuda.current_stream().cuda_stream)
        out = buf.cpu().numpy().view(np.uint64)
        return out[:2 * _lib.HIST_BINS].reshape(2, _lib.HIST_BINS).copy(), out[2 * _lib.HIST_BINS:].copy()

    def pairs_dev(self, cls, side, threshold: float, cap: int, info_ptr: int, scores_ptr: Optional[int] = None,
                  rows_ptr: Optional[int] = None, ids_ptr: Optional[int] = None, stream: int = 0):
        """The pair audit (fh_gallery_pairs_dev): WHICH pairs of rows of class `cls` ("genuine": same id, "impostor", "any") score
        strictly above `threshold` (side "above") or at or below it ("not_above"), most extreme first.  info[4] (device uint64) =
        (count, nan, returned, complete); scores [cap] (device float32), rows [cap][2] (device int32: 0-based positions i < j) and ids
        [cap][2] (device int32) — each optional — hold the first `returned` pairs of the ordered list and (-1.0, -1, -1) behind them.
        complete == 0: the bin the cap falls into did not fit the library's candidate room and the list stops before it — it is still
        an exact prefix.  A pair's score is the fp32 scan's.  "genuine" / "impostor" and ids need a labelled gallery.
        1 <= cap <= PAIRS_MAX_CAP.  Asynchronous on `stream`."""
        check(_lib.lib().fh_gallery_pairs_dev(self._h, _pairs_enum(_lib.PAIRS_CLASS, cls, "class"), _pairs_enum(_lib.PAIRS_SIDE, side, "side"),
                                              float(np.float32(threshold)), int(cap), info_ptr, scores_ptr, rows_ptr, ids_ptr, stream),
              "fh_gallery_pairs_dev")

    def pairs(self, cls, side, threshold: float, cap: int = 64, ids: Optional[bool] = None):
        """(info dict — count, nan, returned, complete —, scores float32[returned], rows int32[returned, 2], ids int32[returned, 2] or
        None) of pairs_dev — a synchronous convenience that allocates and copies back.  ids: whether the listed rows' ids are fetched
        (they need a labelled gallery); by default they are for the classes "genuine" and "impostor", which need one anyway."""
        import torch
        cap = int(cap)
        n = max(cap, 1)
        with_ids = _pairs_enum(_lib.PAIRS_CLASS, cls, "class") != _lib.PAIRS_CLASS["any"] if ids is None else bool(ids)
        info = torch.empty(4, dtype=torch.int64, device="cuda")
        scores = torch.empty(n, dtype=torch.float32, device="cuda")
        rows = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        ids = torch.empty((n, 2), dtype=torch.int32, device="cuda") if with_ids else None
        self.pairs_dev(cls, side, threshold, cap, info.data_ptr(), scores.data_ptr(), rows.data_ptr(), ids.data_ptr() if with_ids else None,
                       torch.cuda.current_stream().cuda_stream)
        d = _pairs_info(info.cpu().numpy().view(np.uint64))
        m = d["returned"]
        return d, scores[:m].cpu().numpy(), rows[:m].cpu().numpy(), ids[:m].cpu().numpy() if with_ids else None

    def set_ids(self, ids) -> int:
        """Replace the ids of all rows by position (int32[len(self)] >= 0, host array or a device tensor) and make the gallery labelled
        (fh_gallery_set_ids); with noise="self" labels: cluster -> set_ids -> fuse.  Synchronous; returns the row count."""
        if hasattr(ids, "data_ptr"):                                   # a torch tensor: device or host memory, as it is
            import torch
            if ids.dtype != torch.int32 or not ids.is_contiguous() or ids.numel() != len(self):
                raise ValueError("set_ids: need a contiguous int32 tensor with one id per row")
            return check(_lib.lib().fh_gallery_set_ids(self._h, ids.data_ptr(), int(ids.is_cuda)), "fh_gallery_set_ids")
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        if ids.size != len(self):
            raise ValueError("set_ids: need one id per row")
        return check(_lib.lib().fh_gallery_set_ids(self._h, ids.ctypes.data if ids.size else None, 0), "fh_gallery_set_ids")

    def set_tags(self, tags, first: int = 0) -> int:
        """Set the watchlist tags (uint32 bit sets; one int for all rows) of rows [first, first + len(tags)) by position
        (fh_gallery_set_tags): a host array or a contiguous device tensor of 4-byte integers.  Row r is admitted for a query with mask
        m iff tag[r] & m != 0; rows whose tags were never set carry TAG_ALL.  Synchronous; returns the number of rows set."""
        if hasattr(tags, "data_ptr"):
            if tags.element_size() != 4 or not tags.is_contiguous():
                raise ValueError("set_tags: need a contiguous tensor of 4-byte integers")
            return check(_lib.lib().fh_gallery_set_tags(self._h, first, tags.numel(), tags.data_ptr(), int(tags.is_cuda)), "fh_gallery_set_tags")
        tags = np.asarray(tags)
        if tags.ndim == 0:
            tags = np.full(len(self) - first, tags)
        tags = np.ascontiguousarray(tags.reshape(-1).astype(np.uint32))
        return check(_lib.lib().fh_gallery_set_tags(self._h, first, tags.size, tags.ctypes.data if tags.size else None, 0), "fh_gallery_set_tags")

    def get_tags(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Tags of rows [first, first + n) by position (default: to the end), uint32 (fh_gallery_get_tags)."""
        if n is None:
            n = len(self) - first
        out = np.empty(max(n, 0), np.uint32)
        check(_lib.lib().fh_gallery_get_tags(self._h, first, n, out.ctypes.data if n > 0 else None), "fh_gallery_get_tags")
        return out

    def topk_tagged_dev(self, q_ptr: int, masks_ptr: int, nq: int, k: int, scores_ptr: int, idx_ptr: int, stream: int = 0):
        """topk_dev over each query's ADMITTED rows only (masks = device uint32[nq]); indices stay global; exact, bit for bit."""
        check(_lib.lib().fh_gallery_topk_tagged_dev(self._h, q_ptr, masks_ptr, nq, k, scores_ptr, idx_ptr, stream), "fh_gallery_topk_tagged_dev")

    def topk_ids_tagged_dev(self, q_ptr: int, masks_ptr: int, nq: int, k: int, scores_ptr: int, ids_ptr: int, rows_ptr: Optional[int] = None,
                            stream: int = 0):
        """topk_ids_dev over each query's admitted rows only: an identity is represented by its best ADMITTED row."""
        check(_lib.lib().fh_gallery_topk_ids_tagged_dev(self._h, q_ptr, masks_ptr, nq, k, scores_ptr, ids_ptr, rows_ptr, stream),
              "fh_gallery_topk_ids_tagged_dev")

    def label_tagged_dev(self, q_ptr: int, masks_ptr: int, nq: int, threshold: float, labels_ptr: int, scores_ptr: int, stream: int = 0):
        """label_dev over each query's admitted rows only (mask 0: -1, -1.0)."""
        check(_lib.lib().fh_gallery_label_tagged_dev(self._h, q_ptr, masks_ptr, nq, threshold, labels_ptr, scores_ptr, stream),
              "fh_gallery_label_tagged_dev")

    def label_ids_tagged_dev(self, q_ptr: int, masks_ptr: int, nq: int, threshold: float, ids_ptr: int, scores_ptr: int, stream: int = 0):
        """label_ids_dev over each query's admitted rows only."""
        check(_lib.lib().fh_gallery_label_ids_tagged_dev(self._h, q_ptr, masks_ptr, nq, threshold, ids_ptr, scores_ptr, stream),
              "fh_gallery_label_ids_tagged_dev")

    def range_dev(self, q_ptr: int, nq: int, threshold: float, cap: int, counts_ptr: int, scores_ptr: Optional[int] = None,
                  idx_ptr: Optional[int] = None, ids_ptr: Optional[int] = None, masks_ptr: Optional[int] = None, stream: int = 0):
        """Threshold search (fh_gallery_range_dev): counts[nq] (device int64) = the exact number of rows — admitted rows with masks
        (device uint32[nq]) — whose mapped score is strictly above `threshold`; scores / idx / ids [nq][cap] (device, each optional) =
        the best min(count, cap) of them, (score desc, global row asc), empty slots (-1.0, -1, -1).  Scores are the fp32 scan's, bit
        for bit, in either scan mode.  ids needs a labelled gallery.  1 <= cap <= RANGE_MAX_CAP.  Asynchronous on `stream`."""
        check(_lib.lib().fh_gallery_range_dev(self._h, q_ptr, masks_ptr, nq, threshold, cap, counts_ptr, scores_ptr, idx_ptr, ids_ptr, stream),
              "fh_gallery_range_dev")

    def range(self, queries, threshold: float, cap: int = 64, masks=None, ids: bool = False):
        """(counts int64[nq], scores float32[nq, cap], indices int32[nq, cap][, ids int32[nq, cap]]) of range_dev for host queries
        [nq, dim] (masks: uint32[nq], optional) — a synchronous convenience that uploads, allocates and copies back."""
        import torch
        q = np.array(queries, np.float32, order="C").reshape(-1, self.dim)      # (a copy: torch takes no read-only array)
        nq = q.shape[0]
        qd = torch.from_numpy(q).cuda()
        md = None if masks is None else torch.from_numpy(np.ascontiguousarray(np.asarray(masks).astype(np.uint32)).view(np.int32).reshape(nq)).cuda()
        counts = torch.zeros(max(nq, 1), dtype=torch.int64, device="cuda")
        sc = torch.empty((max(nq, 1), cap), dtype=torch.float32, device="cuda")
        ix = torch.empty((max(nq, 1), cap), dtype=torch.int32, device="cuda")
        di = torch.empty((max(nq, 1), cap), dtype=torch.int32, device="cuda") if ids else None
        self.range_dev(qd.data_ptr(), nq, threshold, cap, counts.data_ptr(), sc.data_ptr(), ix.data_ptr(), None if di is None else di.data_ptr(),
                       None if md is None else md.data_ptr(), torch.cuda.current_stream().cuda_stream)
        out = (counts[:nq].cpu().numpy(), sc[:nq].cpu().numpy(), ix[:nq].cpu().numpy())
        return out + (di[:nq].cpu().numpy(),) if ids else out

    def topk_deep_dev(self, q_ptr: int, nq: int, k: int, scores_ptr: Optional[int] = None, idx_ptr: Optional[int] = None,
                      ids_ptr: Optional[int] = None, masks_ptr: Optional[int] = None, stream: int = 0):
        """Deep top-k (fh_gallery_topk_deep_dev): scores / idx / ids [nq][k] (device, each optional, not all three) = the best
        min(k, eligible) rows of every query — admitted rows with masks (device uint32[nq]); a NaN or -inf score is never listed —
        (score desc, global row asc), empty slots (-1.0, -1, -1).  1 <= k <= TOPK_DEEP_MAX, no threshold.  Scores are the fp32
        scan's, bit for bit, in either scan mode.  ids needs a labelled gallery.  Asynchronous on `stream`."""
        check(_lib.lib().fh_gallery_topk_deep_dev(self._h, q_ptr, masks_ptr, nq, k, scores_ptr, idx_ptr, ids_ptr, stream),
              "fh_gallery_topk_deep_dev")

    def topk_deep(self, queries, k: int, masks=None, ids: bool = False):
        """(scores float32[nq, k], indices int32[nq, k][, ids int32[nq, k]]) of topk_deep_dev for host queries [nq, dim] (masks:
        uint32[nq], optional) — a synchronous convenience that uploads, allocates and copies back."""
        import torch
        q = np.array(queries, np.float32, order="C").reshape(-1, self.dim)      # (a copy: torch takes no read-only array)
        nq = q.shape[0]
        qd = torch.from_numpy(q).cuda()
        md = None if masks is None else torch.from_numpy(np.ascontiguousarray(np.asarray(masks).astype(np.uint32)).view(np.int32).reshape(nq)).cuda()
        sc = torch.empty((max(nq, 1), k), dtype=torch.float32, device="cuda")
        ix = torch.empty((max(nq, 1), k), dtype=torch.int32, device="cuda")
        di = torch.empty((max(nq, 1), k), dtype=torch.int32, device="cuda") if ids else None
        self.topk_deep_dev(qd.data_ptr(), nq, k, sc.data_ptr(), ix.data_ptr(), None if di is None else di.data_ptr(),
                           None if md is None else md.data_ptr(), torch.cuda.current_stream().cuda_stream)
        out = (sc[:nq].cpu().numpy(), ix[:nq].cpu().numpy())
        return out + (di[:nq].cpu().numpy(),) if ids else out

    def tag_stats(self):
        """(tiles_scanned, tiles_skipped): the (workgroup, 128-row tile) visits the tagged scans multiplied / skipped since the last
        call (resets; waits for the handle's queued work)."""
        a, b = C.c_longlong(0), C.c_longlong(0)
        check(_lib.lib().fh_gallery_tag_stats(self._h, C.byref(a), C.byref(b)), "fh_gallery_tag_stats")
        return int(a.value), int(b.value)

    def __len__(self) -> int:
        return int(_lib.lib().fh_gallery_size(self._h))

    def label_dev(self, q_ptr: int, nq: int, threshold: float, labels_ptr: int, scores_ptr: int, stream: int = 0):
        """labels[q] = best row if (dot+1)/2 > threshold else -1 ("Match" / "Unknown", main.cpp:229-233)."""
        check(_lib.lib().fh_gallery_label_dev(self._h, q_ptr, nq, threshold, labels_ptr, scores_ptr, stream), "fh_gallery_label_dev")


class Comm:
    """RCCL communicator behind the C ABI (fh_comm_*): one per process / rank.  `Comm.unique_id()` on rank 0, hand the 128 bytes to
    the other ranks (torch.distributed's store, MPI, a file), then `Comm(rank, world, id, device)` on every rank."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        check(_lib.lib().fh_comm_unique_id(C.cast(buf, C.c_void_p)), "fh_comm_unique_id")
        return bytes(buf)

    def __init__(self, rank: int, world: int, uid: bytes, device: int = 0):
        if len(uid) != 128:
            raise ValueError("unique id must be 128 bytes")
        self._id = (C.c_ubyte * 128).from_buffer_copy(uid)
        self._h = _lib.lib().fh_comm_create(rank, world, C.cast(self._id, C.c_void_p), device)
        if not self._h:
            raise _lib.FaceHipError("fh_comm_create failed: " + _lib.last_error())
        self.rank, self.world = rank, world

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().fh_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    def allgather_f32_dev(self, send_ptr: int, recv_ptr: int, count: int, stream: int = 0) -> int:
        return check(_lib.lib().fh_comm_allgather_f32_dev(self._h, send_ptr, recv_ptr, count, stream), "fh_comm_allgather_f32_dev")

    def gallery_topk_sharded_dev(self, gallery: "Gallery", q_ptr: int, nq_local: int, k: int, scores_ptr: int, idx_ptr: int,
                                 stream: int = 0) -> int:
        """queries all-gather -> local shard scan -> one top-k all-gather -> merge, all on `stream` (fh_gallery_topk_sharded_dev);
        scores / indices = [world * nq_local][k] on every rank."""
        return check(_lib.lib().fh_gallery_topk_sharded_dev(gallery._h, self._h, q_ptr, nq_local, k, scores_ptr, idx_ptr, stream),
                     "fh_gallery_topk_sharded_dev")


def topk_merge_ids_dev(part_scores_ptr: int, part_ids_ptr: int, part_rows_ptr: int, nparts: int, nq: int, k: int, scores_ptr: int,
                       ids_ptr: int, rows_ptr: int, stream: int = 0) -> int:
    """Merge step of a row-sharded labelled gallery (fh_topk_merge_ids_dev): [nparts][nq][k] identity lists -> the identity top-k of
    their union."""
    return check(_lib.lib().fh_topk_merge_ids_dev(part_scores_ptr, part_ids_ptr, part_rows_ptr, nparts, nq, k, scores_ptr, ids_ptr,
                                                  rows_ptr, stream), "fh_topk_merge_ids_dev")


def group_ids(ids):
    """(order, starts, uniq) of fh_gallery_group_ids — host only: row positions by (id, position), each identity's offset into them
    (len(uniq) + 1 entries), the distinct ids ascending.  The grouping Gallery.fuse sums by."""
    ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
    n = ids.size
    order, starts, uniq = np.empty(n, np.int32), np.empty(n + 1, np.int64), np.empty(n, np.int32)
    m = check(_lib.lib().fh_gallery_group_ids(ids.ctypes.data if n else None, n, order.ctypes.data if n else None, starts.ctypes.data,
                                              uniq.ctypes.data if n else None), "fh_gallery_group_ids")
    return order, starts[:m + 1].copy(), uniq[:m].copy()


_NOISE = {"none": 0, "self": 1}                                # enum fh_cluster_noise


def _noise_mode(noise) -> int:
    """"none" / "self" -> the enum; an int passes through (the library checks it)."""
    if isinstance(noise, str):
        if noise not in _NOISE:
            raise ValueError(f"noise {noise!r}: expected one of {sorted(_NOISE)}")
        return _NOISE[noise]
    return int(noise)


def cluster_scores(scores, threshold: float, min_pts: int = 1, noise="none"):
    """(labels int32[n], info int32[4]) of fh_cluster_scores — host only, the one definition of the clustering rule: rows i < j are
    linked iff scores[i, j] > threshold (strict, fp32; only the upper triangle is read), core iff degree + 1 >= min_pts, a cluster =
    a component of the core rows labelled by its smallest position, a non-core row joins its best core neighbour (higher score, then
    lower position), the rest is noise (-1, or the row's own position with noise="self").  info = (clusters, core, border, noise)."""
    scores = np.ascontiguousarray(scores, np.float32)
    if scores.ndim != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("cluster_scores: need a square matrix")
    n = scores.shape[0]
    labels, info = np.empty(n, np.int32), np.zeros(4, np.int32)
    check(_lib.lib().fh_cluster_scores(scores.ctypes.data if n else None, n, threshold, min_pts, _noise_mode(noise),
                                       labels.ctypes.data if n else None, info.ctypes.data), "fh_cluster_scores")
    return labels, info


def hist_bin(score: float) -> int:
    """The bin of a mapped score (fh_hist_bin — host only, the one definition of the bin rule): -1 for a NaN, else b with
    b/2048 < score <= (b+1)/2048, clamped to 0 below and HIST_BINS - 1 above, so that the suffix sum of a histogram from bin b >= 1 is
    exactly the number of scores the strict test `score > b/2048` accepts."""
    return int(_lib.lib().fh_hist_bin(float(np.float32(score))))


def roc_from_hist(hist, max_far: float):
    """(operating point of max_far, equal-error point) of fh_roc_from_hist — host only.  hist = uint64[2, HIST_BINS] (genuine,
    impostor: Gallery.pair_hist).  A point is a dict of the struct's fields — threshold, bin, true_accepts, false_accepts, genuine,
    impostor — plus far = false_accepts / impostor and tar = true_accepts / genuine as Python floats.  The first is the smallest
    threshold b/2048 whose false accepts stay within floor(max_far * impostor); feed its threshold to label / cluster / the tracker.
    bin == -1 (threshold 1.0, no accepts): no such threshold exists."""
    hist = np.ascontiguousarray(hist, np.uint64)
    if hist.shape != (2, _lib.HIST_BINS):
        raise ValueError(f"roc_from_hist: need a [2, {_lib.HIST_BINS}] histogram")
    out = np.zeros(2, _lib.ROC_POINT_DTYPE)
    check(_lib.lib().fh_roc_from_hist(hist.ctypes.data, float(max_far), out.ctypes.data), "fh_roc_from_hist")
    pts = []
    for p in out:
        d = {"threshold": float(p["threshold"]), "bin": int(p["bin"])}
        d.update({k: int(p[k]) for k in ("true_accepts", "false_accepts", "genuine", "impostor")})
        d["far"] = d["false_accepts"] / d["impostor"]
        d["tar"] = d["true_accepts"] / d["genuine"]
        pts.append(d)
    return pts[0], pts[1]


def _pairs_enum(table, value, what):
    """a name of the table -> the enum; an int passes through (the library checks it)."""
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"pairs {what} {value!r}: expected one of {sorted(table)}")
        return table[value]
    return int(value)


def _pairs_info(info):
    return {k: int(v) for k, v in zip(("count", "nan", "returned", "complete"), info)}


def pairs_from_scores(scores, ids, cls, side, threshold: float, cap: int = 64, room: Optional[int] = None):
    """(info dict, scores float32[cap], rows int32[cap, 2], ids int32[cap, 2]) of fh_pairs_from_scores — host only, the one definition
    of the pair audit: of the pairs i < j of the square matrix `scores` (only its upper triangle is read) that are of class `cls`
    ("genuine": ids[i] == ids[j], "impostor", "any"; ids=None allows only "any") and whose score is strictly above `threshold` (side
    "above") or at or below it ("not_above"; a NaN score is on neither side and counted in info["nan"]), the most extreme
    info["returned"] — score descending (ascending for "not_above"), then i, then j — and (-1.0, -1, -1) behind them.
    info["count"] is exact.  returned = min(cap, count) and complete = 1 unless the score bin the cap falls into, together with the
    bins beyond it, holds more than `room` pairs (default PAIRS_ROOM, at least cap): then the list stops before that bin, complete = 0."""
    scores = np.ascontiguousarray(scores, np.float32)
    if scores.ndim != 2 or scores.shape[0] != scores.shape[1]:
        raise ValueError("pairs_from_scores: need a square matrix")
    n = scores.shape[0]
    if ids is not None:
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1).astype(np.int32))
        if ids.size != n:
            raise ValueError("pairs_from_scores: need one id per row")
    cap = int(cap)
    room = max(_lib.PAIRS_ROOM, cap) if room is None else int(room)
    m = max(cap, 0)
    info, out_s, out_r, out_d = np.zeros(4, np.uint64), np.empty(m, np.float32), np.empty((m, 2), np.int32), np.empty((m, 2), np.int32)
    check(_lib.lib().fh_pairs_from_scores(scores.ctypes.data if n else None, n, None if ids is None else ids.ctypes.data,
                                          _pairs_enum(_lib.PAIRS_CLASS, cls, "class"), _pairs_enum(_lib.PAIRS_SIDE, side, "side"),
                                          float(np.float32(threshold)), cap, room, info.ctypes.data, out_s.ctypes.data, out_r.ctypes.data,
                                          out_d.ctypes.data), "fh_pairs_from_scores")
    return _pairs_info(info), out_s, out_r, out_d


def range_from_scores(scores, threshold: float, cap: int = 64, index_base: int = 0, tags=None, mask: int = _lib.TAG_ALL):
    """(count, scores float32[cap], indices int32[cap]) of fh_range_from_scores — host only, the one definition of the threshold search
    rule, for ONE query's row of mapped scores: a row is a hit iff (tag & mask) != 0 (tags=None: every row carries TAG_ALL), its score
    is strictly above `threshold` in float32 and is not a NaN; count is exact, the lists hold the best min(count, cap) hits (score
    desc, index_base + position asc) and (-1.0, -1) behind them."""
    scores = np.ascontiguousarray(scores, np.float32).reshape(-1)
    n = scores.size
    if tags is not None:
        tags = np.ascontiguousarray(np.asarray(tags).reshape(-1).astype(np.uint32))
        if tags.size != n:
            raise ValueError("range_from_scores: need one tag per score")
    cap = int(cap)
    out_s, out_i = np.empty(max(cap, 0), np.float32), np.empty(max(cap, 0), np.int32)
    count = C.c_longlong(0)
    check(_lib.lib().fh_range_from_scores(scores.ctypes.data if n else None, n, int(index_base), None if tags is None or n == 0 else tags.ctypes.data,
                                          int(mask) & 0xFFFFFFFF, float(np.float32(threshold)), cap, C.byref(count), out_s.ctypes.data,
                                          out_i.ctypes.data), "fh_range_from_scores")
    return int(count.value), out_s, out_i


def topk_from_scores(scores, k: int, index_base: int = 0, tags=None, mask: int = _lib.TAG_ALL):
    """(listed, scores float32[k], indices int32[k]) of fh_topk_from_scores — host only, the one definition of the deep top-k, for ONE
    query's row of mapped scores: a row is eligible iff (tag & mask) != 0 (tags=None: every row carries TAG_ALL) and its score is
    neither a NaN nor -inf; the lists hold the best min(k, eligible) rows (score desc, index_base + position asc) and (-1.0, -1)
    behind them — the list part of range_from_scores(threshold=-inf, cap=k)."""
    scores = np.ascontiguousarray(scores, np.float32).reshape(-1)
    n = scores.size
    if tags is not None:
        tags = np.ascontiguousarray(np.asarray(tags).reshape(-1).astype(np.uint32))
        if tags.size != n:
            raise ValueError("topk_from_scores: need one tag per score")
    k = int(k)
    out_s, out_i = np.empty(max(k, 0), np.float32), np.empty(max(k, 0), np.int32)
    listed = check(_lib.lib().fh_topk_from_scores(scores.ctypes.data if n else None, n, int(index_base),
                                                  None if tags is None or n == 0 else tags.ctypes.data, int(mask) & 0xFFFFFFFF, k,
                                                  out_s.ctypes.data, out_i.ctypes.data), "fh_topk_from_scores")
    return int(listed), out_s, out_i


def plan_describe(path: str, default_h: int, default_w: int) -> str:
    buf = C.create_string_buffer(1 << 18)
    check(_lib.lib().fh_plan_describe(str(path).encode(), default_h, default_w, buf, len(buf)), "fh_plan_describe")
    return buf.value.decode()


def imread(path: str) -> Optional[np.ndarray]:
    """cv::imread(path) (reference src/main.cpp:42): BGR u8 [rows, cols, 3], or None when the file cannot be read or
    decoded (cv::imread returns an empty Mat).  JPEG / PNG / BMP / PPM, decoded by the library's own host code."""
    L = _lib.lib()
    p, r, c = C.c_void_p(), C.c_int(), C.c_int()
    if L.fh_imread(str(path).encode(), C.byref(p), C.byref(r), C.byref(c)) != 0:
        return None
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), (r.value, c.value, 3)).copy()
    finally:
        L.fh_image_free(p)
