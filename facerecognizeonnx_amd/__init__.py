"""facerecognizeonnx_amd — MI355X-native detect -> align -> embed -> compare.

Drop-in for the hot path of cucibala/FaceRecognizeOnnx (FaceDetector::detect,
FaceRecognizer::extractFeature / compareFaces) behind a C ABI (include/facehip.h) implemented
as hand-written gfx950 HIP kernels (csrc/).  See DESIGN.md.
"""
from .api import (Comm, FaceBox, FaceDetector, FaceRecognizer, FrameStream, Gallery, pipeline_run_dev, pipeline_submit_dev,  # noqa: F401
                  imread, plan_describe, topk_merge_ids_dev, group_ids, frame_array, letterbox_plan, pipeline_run_ragged_dev, pipeline_images,
                  Tiling, tile_plan, pipeline_run_tiled_dev, Tracker, track_plan, pipeline_run_tracked_dev, pipeline_run_identified_dev,
                  face_quality_dev, cluster_scores, hist_bin, roc_from_hist, range_from_scores, topk_from_scores, pairs_from_scores, JpegDecoder,
                  pipeline_files, JpegEncoder, imwrite, face_chips)
from ._lib import HIST_BINS, RANGE_MAX_CAP, TOPK_DEEP_MAX, PAIRS_MAX_CAP, PAIRS_ROOM, ROC_POINT_DTYPE, FACE_DTYPE, TRACK_DTYPE, TRACK_IDENT_DTYPE, TRACK_LINK_DTYPE, TRACK_POOL_LAST, TRACK_POOL_SUM, TRACK_POOL_WEIGHTED, FaceHipError, FhFrame, FhTiling, FhView, FhJpegDesc, FhJpegComp, FhBlob, build, lib  # noqa: F401

__all__ = ["Comm", "FaceBox", "FaceDetector", "FaceRecognizer", "Gallery", "FrameStream", "pipeline_run_dev", "pipeline_submit_dev", "plan_describe", "imread", "topk_merge_ids_dev", "group_ids", "frame_array", "letterbox_plan", "pipeline_run_ragged_dev", "pipeline_images", "FhFrame",
           "Tiling", "tile_plan", "pipeline_run_tiled_dev", "FhTiling", "FhView",
           "Tracker", "track_plan", "pipeline_run_tracked_dev", "TRACK_DTYPE",
           "pipeline_run_identified_dev", "TRACK_IDENT_DTYPE", "TRACK_POOL_LAST", "TRACK_POOL_SUM",
           "face_quality_dev", "TRACK_POOL_WEIGHTED", "cluster_scores", "TRACK_LINK_DTYPE",
           "hist_bin", "roc_from_hist", "HIST_BINS", "ROC_POINT_DTYPE", "range_from_scores", "RANGE_MAX_CAP", "topk_from_scores", "TOPK_DEEP_MAX",
           "pairs_from_scores", "PAIRS_MAX_CAP", "PAIRS_ROOM",
           "JpegDecoder", "pipeline_files", "JpegEncoder", "imwrite", "face_chips", "FhJpegDesc", "FhJpegComp", "FhBlob",
           "FACE_DTYPE", "FaceHipError", "build", "lib"]
