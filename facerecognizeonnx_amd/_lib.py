"""ctypes binding of libfacehip.so (the C ABI in include/facehip.h).

The library is the product; there is no CPU fallback.  If it is missing it is built with
`make` (hipcc cross-compiles gfx950 without a GPU); if that fails the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfacehip.so")
CSRC = os.path.join(_HERE, "csrc")

FACE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"),
                       ("score", "<f4"), ("lm", "<f4", (10,))])
assert FACE_DTYPE.itemsize == 60


class FhFace(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("score", C.c_float), ("lm", C.c_float * 10)]


class FhFrame(C.Structure):
    """fh_frame: one image of a mixed-size batch (device pixels; host pixels for fh_pipeline_run_images).  24 bytes."""
    _fields_ = [("bgr", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("step", C.c_int32)]


class FhTiling(C.Structure):
    """fh_tiling: tile size, overlap and border of a tiled detection.  16 bytes."""
    _fields_ = [("tile_w", C.c_int32), ("tile_h", C.c_int32), ("overlap", C.c_int32), ("border", C.c_int32)]


class FhView(C.Structure):
    """fh_view: one view of a tile plan (edges: bit 0 left, 1 top, 2 right, 3 bottom = interior).  20 bytes."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("edges", C.c_int32)]


class FhJpegComp(C.Structure):
    """fh_jpeg_comp: one component of an fh_jpeg_desc.  160 bytes."""
    _fields_ = [("h", C.c_int32), ("v", C.c_int32), ("wblocks", C.c_int32), ("hblocks", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32),
                ("coef_off", C.c_int64), ("quant", C.c_uint16 * 64)]


class FhJpegDesc(C.Structure):
    """fh_jpeg_desc: what JPEG reconstruction needs besides the coefficients (fh_jpeg_header / fh_jpeg_entropy fill it).  528 bytes."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("ncomp", C.c_int32),
                ("hmax", C.c_int32), ("vmax", C.c_int32), ("color", C.c_int32), ("orientation", C.c_int32), ("reserved", C.c_int32),
                ("coef_count", C.c_int64), ("comp", FhJpegComp * 3)]


class FhBlob(C.Structure):
    """fh_blob: the bytes of one file.  16 bytes."""
    _fields_ = [("bytes", C.c_void_p), ("n", C.c_size_t)]


TRACK_DTYPE = np.dtype([(k, "<i4") for k in ("id", "x", "y", "w", "h", "last_seen", "last_embed", "hits")])
assert TRACK_DTYPE.itemsize == 32
TRACK_MAX = 64                                                 # FH_TRACK_MAX
TRACK_IDENT_DTYPE = np.dtype([("id", "<i4"), ("n_emb", "<i4"), ("label", "<i4"), ("score", "<f4")])     # fh_track_ident
assert TRACK_IDENT_DTYPE.itemsize == 16
TRACK_POOL_LAST, TRACK_POOL_SUM, TRACK_POOL_WEIGHTED = 0, 1, 2    # enum fh_track_pool
TRACK_LINK_DTYPE = np.dtype([("owner", "<i4"), ("root", "<i4"), ("n_emb", "<i4"), ("label", "<i4"), ("score", "<f4"), ("last_seen", "<i4"),
                             ("links", "<i4"), ("pad", "<i4")])  # fh_track_link
assert TRACK_LINK_DTYPE.itemsize == 32
TRACK_LINK_MEMORY = 256                                        # FH_TRACK_LINK_MEMORY
HIST_BINS = 2048                                               # FH_HIST_BINS
TAG_ALL = 0xFFFFFFFF                                           # FH_TAG_ALL
RANGE_MAX_CAP = 1024                                           # FH_RANGE_MAX_CAP
TOPK_DEEP_MAX = 1024                                           # FH_TOPK_DEEP_MAX
PAIRS_MAX_CAP = 1024                                           # FH_PAIRS_MAX_CAP
PAIRS_ROOM = 65536                                             # FH_PAIRS_ROOM
PAIRS_CLASS = {"genuine": 0, "impostor": 1, "any": 2}          # enum fh_pairs_class
PAIRS_SIDE = {"above": 0, "not_above": 1}                      # enum fh_pairs_side
ROC_POINT_DTYPE = np.dtype([("threshold", "<f4"), ("bin", "<i4"), ("true_accepts", "<u8"), ("false_accepts", "<u8"), ("genuine", "<u8"),
                            ("impostor", "<u8")])              # fh_roc_point
assert ROC_POINT_DTYPE.itemsize == 40


class FhTrackState(C.Structure):
    """fh_track_state: one track slot of a stream (id = -1: free).  32 bytes."""
    _fields_ = [(k, C.c_int32) for k in ("id", "x", "y", "w", "h", "last_seen", "last_embed", "hits")]


def build(force: bool = False) -> str:
    """Compile libfacehip.so in-tree (so that it travels with the source snapshot)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(_HERE, "..", "include", "facehip.h")]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-j8", "-s"])
    return LIB_PATH


def csrc_fingerprint() -> str:
    """sha256 (first 16 hex digits) over the kernel / host sources the library is built from: the stamp that ties a committed counter
    profile (profiles/traffic.json) to the code it was measured on (bench.py reports `roofline.traffic` only when it still matches)."""
    import hashlib
    h = hashlib.sha256()
    host_only = {"image_io.cpp", "onnx_reader.cpp", "onnx_reader.h", "comm.cpp"}     # file parsers / RCCL glue: no kernel, no launch decision
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".cpp", ".h")) and f not in host_only:
            h.update(f.encode()); h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


_vp, _i, _f, _ll, _d = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_double
_ip = C.POINTER(C.c_int)

# name -> (restype, argtypes); one row per symbol declared in include/facehip.h
PROTOTYPES = {
    "fh_version": (C.c_char_p, []),
    "fh_last_error": (C.c_char_p, []),
    "fh_init": (_i, [_i]),
    "fh_plan_describe": (_i, [C.c_char_p, _i, _i, C.c_char_p, _i]),
    "fh_onnx_dump": (_i, [C.c_char_p, C.c_char_p, _i]),
    "fh_det_create": (_vp, [C.c_char_p]),
    "fh_det_destroy": (None, [_vp]),
    "fh_det_input_size": (_i, [_vp, _ip, _ip]),
    "fh_det_num_anchors": (_i, [_vp]),
    "fh_det_macs_per_frame": (_d, [_vp]),
    "fh_det_act_bytes_per_frame": (_d, [_vp]),
    "fh_det_detect": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _i]),
    "fh_det_detect_batch_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _f, _f, _vp, _i, _vp, _vp]),
    "fh_det_run_network_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _vp]),
    "fh_det_run_input_dev": (_i, [_vp, _vp, _i, _vp]),
    "fh_det_num_outputs": (_i, [_vp]),
    "fh_det_output_dev": (_vp, [_vp, _i, _ip, _ip]),
    "fh_det_input_dev": (_vp, [_vp]),
    "fh_det_postprocess_dev": (_i, [_vp, _i, _f, _f, _vp, _i, _vp, _vp]),
    "fh_postprocess_rows_dev": (_i, [_vp, _i, _i, _i, _f, _f, _f, _vp, _i, _vp, _vp]),
    "fh_rec_create": (_vp, [C.c_char_p]),
    "fh_rec_destroy": (None, [_vp]),
    "fh_rec_input_size": (_i, [_vp, _ip, _ip]),
    "fh_rec_feature_dim": (_i, [_vp]),
    "fh_rec_macs_per_face": (_d, [_vp]),
    "fh_rec_act_bytes_per_face": (_d, [_vp]),
    "fh_rec_set_chunk": (_i, [_vp, _i]),
    "fh_rec_extract": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i]),
    "fh_rec_extract_simple": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "fh_compare": (_f, [_vp, _i, _vp, _i]),
    "fh_rec_embed_aligned_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "fh_rec_run_input_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "fh_rec_align_dev": (_i, [_vp, _vp, _i, _i, _i, _ll, _vp, _vp, _i, _vp, _vp, _vp]),
    "fh_rec_input_dev": (_vp, [_vp]),
    "fh_rec_embed_faces_dev": (_i, [_vp, _vp, _i, _i, _i, _ll, _vp, _vp, _i, _vp, _vp, _vp]),
    "fh_pipeline_run_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _ll, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "fh_pipeline_submit_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _ll, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fh_letterbox_plan": (_i, [_i, _i, _i, _i, _ip, _ip, C.POINTER(C.c_float)]),
    "fh_det_letterbox_ragged_dev": (_i, [_vp, _vp, _i, _vp, _vp]),
    "fh_det_run_network_ragged_dev": (_i, [_vp, _vp, _i, _vp]),
    "fh_det_detect_ragged_dev": (_i, [_vp, _vp, _i, _f, _f, _vp, _i, _vp, _vp]),
    "fh_rec_align_ragged_dev": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "fh_rec_embed_faces_ragged_dev": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "fh_pipeline_run_ragged_dev": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "fh_pipeline_run_images": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp, _vp, _i]),
    "fh_tile_plan": (_i, [_i, _i, _vp, _vp, _i]),
    "fh_det_detect_tiled_dev": (_i, [_vp, _vp, _i, _vp, _f, _f, _vp, _i, _vp, _vp]),
    "fh_det_run_network_tiled_dev": (_i, [_vp, _vp, _i, _vp, _vp]),
    "fh_postprocess_rows_tiled_dev": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _f, _vp, _i, _vp, _vp]),
    "fh_pipeline_run_tiled_dev": (_i, [_vp, _vp, _vp, _i, _vp, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "fh_det_detect_tiled": (_i, [_vp, _vp, _i, _i, _i, _vp, _f, _f, _vp, _i]),
    "fh_stream_create": (_vp, [_vp, _vp, _i, _i, _i, _i]),
    "fh_stream_destroy": (None, [_vp]),
    "fh_stream_submit": (_i, [_vp, _vp, _i, _f, _f]),
    "fh_stream_collect": (_i, [_vp, _vp, _vp, _vp, _i]),
    "fh_tracker_create": (_vp, [_i, _i, _f, _i, _i]),
    "fh_tracker_destroy": (None, [_vp]),
    "fh_tracker_reset": (_i, [_vp, _i]),
    "fh_tracker_get_state": (_i, [_vp, _i, _vp, _ip, _ip]),
    "fh_track_plan": (_i, [_vp, _i, _i, _vp, _vp]),
    "fh_track_update_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_track_select_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fh_pipeline_run_tracked_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _ll, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fh_track_update_slots_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "fh_tracker_enable_identity": (_i, [_vp, _i, _i]),
    "fh_track_identify_dev": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_tracker_queries_dev": (_vp, [_vp]),
    "fh_tracker_get_identity": (_i, [_vp, _i, _vp, _vp]),
    "fh_pipeline_run_identified_dev": (_i, [_vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _ll, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp]),
    "fh_face_quality_dev": (_i, [_vp, _i, _i, _i, _i, _ll, _vp, _vp, _i, _vp, _vp]),
    "fh_face_quality_ragged_dev": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp]),
    "fh_tracker_set_bestshot": (_i, [_vp, _i, _i, _i, _i]),
    "fh_tracker_get_quality": (_i, [_vp, _i, _vp]),
    "fh_tracker_quality_dev": (_vp, [_vp]),
    "fh_track_update_q_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fh_track_identify_q_dev": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_tracker_enable_relink": (_i, [_vp, _i, _f, _i]),
    "fh_track_identify_link_dev": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "fh_tracker_get_links": (_i, [_vp, _i, _vp, _vp]),
    "fh_tracker_roots_dev": (_vp, [_vp]),
    "fh_gallery_create": (_vp, [_i]),
    "fh_gallery_destroy": (None, [_vp]),
    "fh_gallery_upload": (_i, [_vp, _vp, _ll, _i, _ll]),
    "fh_gallery_enroll": (_ll, [_vp, _vp, _ll, _i]),
    "fh_gallery_size": (_ll, [_vp]),
    "fh_gallery_label_dev": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp]),
    "fh_gallery_topk_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "fh_gallery_set_scan": (_i, [_vp, _i]),
    "fh_gallery_get_scan": (_i, [_vp]),
    "fh_gallery_scan_stats": (_i, [_vp, C.POINTER(_ll), C.POINTER(_ll)]),
    "fh_topk_merge_dev": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "fh_gallery_enroll_ids": (_ll, [_vp, _vp, _vp, _ll, _i]),
    "fh_gallery_upload_ids": (_i, [_vp, _vp, _vp, _ll, _i, _ll]),
    "fh_gallery_topk_ids_dev": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_gallery_label_ids_dev": (_i, [_vp, _vp, _i, _f, _vp, _vp, _vp]),
    "fh_gallery_remove_ids": (_ll, [_vp, _vp, _ll]),
    "fh_gallery_get_ids": (_ll, [_vp, _ll, _ll, _vp]),
    "fh_topk_merge_ids_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_gallery_group_ids": (_ll, [_vp, _ll, _vp, _vp, _vp]),
    "fh_gallery_fuse_ids": (_ll, [_vp, _vp, _i]),
    "fh_gallery_get_rows": (_ll, [_vp, _ll, _ll, _vp]),
    "fh_gallery_self_scores_dev": (_i, [_vp, _vp, _vp, _vp]),
    "fh_cluster_scores": (_i, [_vp, _i, _f, _i, _i, _vp, _vp]),
    "fh_gallery_cluster_dev": (_i, [_vp, _f, _i, _i, _vp, _vp, _vp]),
    "fh_hist_bin": (_i, [_f]),
    "fh_roc_from_hist": (_i, [_vp, _d, _vp]),
    "fh_gallery_pair_hist_dev": (_i, [_vp, _vp, _vp, _vp]),
    "fh_pairs_from_scores": (_i, [_vp, _i, _vp, _i, _i, _f, _i, _ll, _vp, _vp, _vp, _vp]),
    "fh_gallery_pairs_dev": (_i, [_vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "fh_gallery_set_ids": (_ll, [_vp, _vp, _i]),
    "fh_gallery_set_tags": (_ll, [_vp, _ll, _ll, _vp, _i]),
    "fh_gallery_get_tags": (_ll, [_vp, _ll, _ll, _vp]),
    "fh_gallery_topk_tagged_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "fh_gallery_topk_ids_tagged_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_gallery_label_tagged_dev": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "fh_gallery_label_ids_tagged_dev": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _vp]),
    "fh_gallery_tag_stats": (_i, [_vp, C.POINTER(_ll), C.POINTER(_ll)]),
    "fh_tracker_set_stream_masks": (_i, [_vp, _vp]),
    "fh_gallery_range_dev": (_i, [_vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "fh_range_from_scores": (_i, [_vp, _ll, _ll, _vp, C.c_uint32, _f, _i, C.POINTER(_ll), _vp, _vp]),
    "fh_gallery_topk_deep_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "fh_topk_from_scores": (_i, [_vp, _ll, _ll, _vp, C.c_uint32, _i, _vp, _vp]),
    "fh_debug_deep_blocks": (_i, [_vp, _ll, _vp, C.c_uint32, _i, _vp]),
    "fh_comm_unique_id": (_i, [_vp]),
    "fh_comm_create": (_vp, [_i, _i, _vp, _i]),
    "fh_comm_destroy": (None, [_vp]),
    "fh_comm_rank": (_i, [_vp]),
    "fh_comm_world": (_i, [_vp]),
    "fh_comm_allgather_f32_dev": (_i, [_vp, _vp, _vp, _ll, _vp]),
    "fh_gallery_topk_sharded_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "fh_timing_enable": (_i, [_i]),
    "fh_timing_num_tags": (_i, []),
    "fh_timing_collect": (_i, [_vp, _vp, _vp, _vp, _i]),
    "fh_timing_collect_ops": (_i, [_vp, _vp, _vp, _i]),
    "fh_det_set_conv_cfg": (_i, [_vp, _i, _i]),
    "fh_rec_set_conv_cfg": (_i, [_vp, _i, _i]),
    "fh_memcpy_d2h": (_i, [_vp, _vp, C.c_size_t]),
    "fh_det_sync": (_i, [_vp, _vp]),
    "fh_rec_sync": (_i, [_vp, _vp]),
    "fh_imread": (_i, [C.c_char_p, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)]),
    "fh_image_decode": (_i, [_vp, C.c_size_t, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)]),
    "fh_image_free": (None, [_vp]),
    "fh_jpeg_header": (_i, [_vp, C.c_size_t, _vp]),
    "fh_jpeg_entropy": (_i, [_vp, C.c_size_t, _vp, _vp, C.c_size_t]),
    "fh_jpeg_reconstruct": (_i, [_vp, _vp, _vp, _i]),
    "fh_jpeg_desc_check": (_i, [_vp]),
    "fh_jpegdec_create": (_vp, []),
    "fh_jpegdec_destroy": (None, [_vp]),
    "fh_jpeg_reconstruct_batch_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "fh_jpeg_decode_batch": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "fh_pipeline_run_files": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _f, _i, _vp, _vp, _vp, _i, _vp]),
    "fh_jpeg_quant_tables": (_i, [_i, _vp, _vp]),
    "fh_jpeg_enc_desc": (_i, [_i, _i, _i, _i, _i, _vp]),
    "fh_jpeg_enc_check": (_i, [_vp]),
    "fh_jpeg_forward": (_i, [_vp, _vp, _i, _vp, C.c_size_t]),
    "fh_jpeg_write": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "fh_jpeg_write_bound": (C.c_size_t, [_vp]),
    "fh_imwrite_jpeg": (_i, [C.c_char_p, _vp, _i, _i, _i, _i, _i]),
    "fh_jpegenc_create": (_vp, []),
    "fh_jpegenc_destroy": (None, [_vp]),
    "fh_jpeg_forward_batch_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "fh_jpeg_encode_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "fh_jpeg_write_header": (_i, [_vp, _vp, C.c_size_t, _vp]),
    "fh_jpeg_scan_bits": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "fh_jpeg_code_batch_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "fh_jpeg_encode_batch_gpu": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "fh_jpeg_stuff_chunk": (_i, []),
    "fh_debug_jpeg_arena": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "fh_debug_jpeg_scan_bits": (_ll, [_vp, _vp, C.c_size_t]),
    "fh_det_set_winograd": (_i, [_vp, _i]),
    "fh_rec_set_winograd": (_i, [_vp, _i]),
    "fh_rec_set_wino_fusion": (_i, [_vp, _i]),
    "fh_rec_set_wino_x3": (_i, [_vp, _i]),
    "fh_rec_get_wino_x3": (_i, [_vp]),
    "fh_rec_get_conv_x3": (_i, [_vp]),
    "fh_rec_get_pw_x3": (_i, [_vp]),
    "fh_rec_get_wino2_x3": (_i, [_vp]),
    "fh_det_set_x3": (_i, [_vp, _i]),
    "fh_det_get_x3": (_i, [_vp]),
    "fh_rec_set_shortcut_fold": (_i, [_vp, _i]),
    "fh_rec_set_precision": (_i, [_vp, _i, C.POINTER(C.c_float)]),
    "fh_rec_get_precision": (_i, [_vp]),
    "fh_det_set_cus": (_i, [_vp, _i]),
    "fh_rec_set_cus": (_i, [_vp, _i]),
    "fh_debug_streamk": (_i, [_i, _i]),
    "fh_debug_conv_plan": (_i, [_i, _vp, _i, _vp, _i]),
    "fh_debug_wino_slots": (_i, [_i]),
    "fh_debug_cluster_tiles": (_i, [_i]),
    "fh_debug_hist_copies": (_i, [_i]),
    "fh_debug_pairs_room": (_i, [_i]),
    "fh_debug_tag_skip": (_i, [_i]),
    "fh_debug_topk_merge_strided_dev": (_i, [_vp, _vp, _i, _i, _i, _ll, _vp, _vp, _vp]),
    "fh_set_graph_replay": (_i, [_i]),
    "fh_det_workspace_dev": (_vp, [_vp]),
    "fh_det_graph_stats": (_i, [_vp, _vp]),
    "fh_rec_graph_stats": (_i, [_vp, _vp]),
    "fh_det_set_fused_stem": (_i, [_vp, _i]),
    "fh_rec_set_fused_stem": (_i, [_vp, _i]),
    "fh_det_set_fused_front": (_i, [_vp, _i]),
    "fh_det_set_halo_conv": (_i, [_vp, _i]),
    "fh_resize_u8c3_dev": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "fh_conv_forward_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fh_conv_forward_ex_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "fh_conv_forward_ep_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "fh_conv_winograd_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fh_conv_winograd_ex_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fh_debug_pack_bf16x2_dev": (_i, [_vp, _vp, _ll]),
    "fh_debug_wino_gemm_rows": (_ll, [_i, _i, _i, _i, _i, _i]),
    "fh_debug_wino_gemm_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fh_debug_wino2_clock_mhz": (_d, []),
    "fh_conv_wino2_prec_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fh_debug_wino2_pack_x3": (_i, [_vp, _i, _i, _vp]),
    "fh_debug_stem_pack": (_i, [_vp, _i, _vp]),
    "fh_debug_det_run_pasted_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _ll, _vp]),
    "fh_conv_wino2_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fh_conv_wino2_ex_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fh_conv_wt_rows": (_i, [_i]),
    "fh_conv_pack_weights": (_i, [_vp, _i, _i, _i, _vp]),
    "fh_conv_kpad": (_i, [_i]),
}

_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        path = build()
        # FACEHIP_LIB: a diagnostic build of the same library (phase stamps: scripts/wino2_prof.sh) loaded INSTEAD of the in-tree one —
        # a side copy, so that a failed diagnostic run can never leave a non-production library installed
        path = os.environ.get("FACEHIP_LIB") or path
        # PyTorch (device memory / streams / torch.distributed plumbing) bundles its own HIP
        # runtime.  It has to be loaded FIRST so that libfacehip.so binds to the same runtime
        # instance; two runtimes in one process do not share a device context.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def last_error() -> str:
    return lib().fh_last_error().decode(errors="replace")


class FaceHipError(RuntimeError):
    pass


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise FaceHipError(f"{what} failed ({rc}): {last_error()}")
    return rc
