"""ctypes binding of libsvo_hip.so (the C-ABI declared in include/svo.h).

There is no CPU fallback: if the HIP library has not been built the import of this module fails
loudly, and every call fails with SvoError when no MI355X is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsvo_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "stereo_visual_odometry_amd: %s is missing. Build the HIP extension first "
        "(python -c 'import __graft_entry__ as g; g.build()' or make -C stereo_visual_odometry_amd/csrc). "
        "There is no CPU fallback." % LIB_PATH)

# Load order: the PyTorch ROCm wheel bundles its own libamdhip64 / libhsa-runtime64.  If the system ROCm runtime (a
# dependency of libsvo_hip.so) is initialised first, torch's copy later reports "No HIP GPUs are available"; the other order
# works (measured on the MI355X box).  torch is plumbing here (device tensors in bench.py), so when it is installed it is
# imported first.  Set SVO_NO_TORCH_PRELOAD=1 to skip.
if not os.environ.get("SVO_NO_TORCH_PRELOAD"):
    try:
        import torch  # noqa: F401
    except Exception:
        pass

lib = C.CDLL(LIB_PATH)

SVO_OK, SVO_ERR_ARG, SVO_ERR_HIP, SVO_ERR_CAPACITY, SVO_ERR_STATE, SVO_ERR_INTERNAL = 0, -1, -2, -3, -4, -5
# svo_get_last_frame_path bits (svo.h SVO_PATH_*)
PATH_LEAN, PATH_LK_CHAINED, PATH_INGEST_AHEAD, PATH_FRONT_FUSED, PATH_TRI_EPNP_FUSED, PATH_GRAPH = 1, 2, 4, 8, 16, 32
PATH_INPUT_CONVERTED, PATH_POSE_COV, PATH_DETECT_MASKED, PATH_CLAHE, PATH_TRACK_IDS = 64, 128, 256, 512, 1024
PATH_MOTION_PRIOR, PATH_PRIOR_PREDICTED, PATH_DESCRIPTORS = 2048, 4096, 8192
# observation rows (svo.h svo_track_obs flags), descriptor rows, descriptor-index results, relocalisation
OBS_INLIER, OBS_HAS_XYZ = 1, 2
DESC_BYTES = 32
MATCH_NONE, MATCH_NO_DIST = -1, 257
POINT_NONE, RELOC_MAX_QUERIES = -1, 4096
RELOC_BATCH_MAX_CAMERAS, RELOC_BATCH_MAX_QUERIES = 1024, 1 << 20
ALIGN_MAX_ROWS, ALIGN_MAX_HYPOTHESES = 4096, 1024
# index maintenance (svo.h SVO_RETIRE_*)
RETIRE_BY_TAG, RETIRE_BY_IDS, RETIRE_LATEST_PER_ID, RETIRE_SCOPE = 1, 2, 4, 8
# motion priors (svo.h SVO_PRIOR_*)
PRIOR_EXPLICIT, PRIOR_LAST_ROTATION = 0, 1
PRIOR_MODES = {"explicit": PRIOR_EXPLICIT, "last_rotation": PRIOR_LAST_ROTATION}
# pose covariance (svo.h SVO_COV_*)
COV_OFF, COV_RESIDUAL, COV_FIXED_SIGMA = 0, 1, 2
COV_MODES = {"off": COV_OFF, "residual": COV_RESIDUAL, "fixed": COV_FIXED_SIGMA}
# input formats (svo.h SVO_INPUT_*): what the bytes of the caller's frames are; the sensor_msgs encoding names map onto them
INPUT_MONO8, INPUT_BGR8, INPUT_RGB8, INPUT_BGRA8, INPUT_RGBA8, INPUT_UYVY, INPUT_YUY2 = range(7)
INPUT_ENCODINGS = {"mono8": INPUT_MONO8, "bgr8": INPUT_BGR8, "rgb8": INPUT_RGB8, "bgra8": INPUT_BGRA8, "rgba8": INPUT_RGBA8,
                   "yuv422": INPUT_UYVY, "yuv422_yuy2": INPUT_YUY2}
INPUT_BPP = (1, 3, 3, 4, 4, 2, 2)
# svo_get_pyramid / svo_get_derivatives: which pyramid pair
PYR_T1, PYR_LAST_LEFT = 0, 1


class SvoError(RuntimeError):
    pass


class SvoConfig(C.Structure):
    _fields_ = [
        ("bucket_start_row", C.c_int), ("buckets_along_height", C.c_int), ("buckets_along_width", C.c_int),
        ("features_per_bucket", C.c_int), ("features_threshold", C.c_int),
        ("pre_matching_feature_threshold", C.c_int), ("age_threshold", C.c_int), ("fast_threshold", C.c_int),
        ("ransac_reprojection_error", C.c_float), ("ransac_iterations", C.c_int),
        ("optical_flow_min_eig_threshold", C.c_double), ("circular_matching_success_threshold", C.c_double),
        ("max_translation_norm", C.c_double), ("max_rotation_norm", C.c_double),
        ("win_w", C.c_int), ("win_h", C.c_int), ("max_level", C.c_int), ("lk_max_count", C.c_int),
        ("lk_epsilon", C.c_double), ("ransac_confidence", C.c_float), ("max_features", C.c_int), ("channels", C.c_int),
        ("lk_float_sums", C.c_int),
    ]


class SvoFrameStats(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "n_after_detect", "second_pass", "n_into_lk", "n_after_circular", "n_after_bounds",
        "n_inliers", "ransac_iters", "fail_reason", "n_features_out", "lk_level_visits", "lk_newton_steps",
        "lk_dead_after_pass0", "lk_dead_after_pass1", "lk_dead_after_pass2")]

    def as_dict(self):
        return {f[0]: getattr(self, f[0]) for f in self._fields_}


class SvoCameraInfo(C.Structure):
    """svo_camera_info: what rectification needs of a ROS sensor_msgs/CameraInfo (raw width x height)."""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 8), ("n_d", C.c_int), ("R", C.c_double * 9), ("P", C.c_double * 12),
                ("width", C.c_int), ("height", C.c_int)]


class SvoTrackObs(C.Structure):
    """svo_track_obs: the 64-byte observation row; TRACK_OBS_DTYPE is the same row as a numpy structured dtype"""
    _fields_ = [("id", C.c_int64), ("l0", C.c_float * 2), ("r0", C.c_float * 2), ("l1", C.c_float * 2), ("r1", C.c_float * 2),
                ("xyz", C.c_float * 3), ("age", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32)]


TRACK_OBS_DTYPE = np.dtype([("id", "<i8"), ("l0", "<f4", 2), ("r0", "<f4", 2), ("l1", "<f4", 2), ("r1", "<f4", 2),
                            ("xyz", "<f4", 3), ("age", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert TRACK_OBS_DTYPE.itemsize == 64 and C.sizeof(SvoTrackObs) == 64
# svo_desc_match: the descriptor index's 32-byte result row
DESC_MATCH_DTYPE = np.dtype([("id", "<u8"), ("id2", "<u8"), ("row", "<i4"), ("row2", "<i4"), ("dist", "<u2"), ("dist2", "<u2"), ("reserved", "<u4")])
assert DESC_MATCH_DTYPE.itemsize == 32


class SvoDescIndexStats(C.Structure):
    _fields_ = [("last_kernels_ms", C.c_float), ("scratch_allocations", C.c_int32), ("scratch_bytes", C.c_uint64), ("scratch_bytes_outgrown", C.c_uint64)]


class SvoRelocParams(C.Structure):
    _fields_ = [("row_lo", C.c_int32), ("row_hi", C.c_int32), ("max_dist", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32),
                ("min_candidates", C.c_int32), ("ransac_iterations", C.c_int32), ("reproj_error", C.c_float), ("confidence", C.c_float)]


class SvoRelocResult(C.Structure):
    _fields_ = [("success", C.c_int32), ("n_candidates", C.c_int32), ("n_inliers", C.c_int32), ("iters_run", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("T", C.c_double * 16)]


class SvoRelocGuide(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("radius", C.c_float), ("reserved", C.c_int32)]


class SvoAlignParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("src_lo", "src_hi", "dst_lo", "dst_hi", "max_dist", "ratio_num", "ratio_den", "min_pairs",
                                         "hypotheses", "refit_rounds")] + [("inlier_dist", C.c_float), ("reserved", C.c_int32)]


class SvoAlignResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("success", "n_pairs", "n_inliers", "best_hypothesis", "best_count", "refit_rounds_run")] + \
               [("R", C.c_double * 9), ("t", C.c_double * 3), ("T", C.c_double * 16), ("rms", C.c_double)]


class SvoFuseParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("src_lo", "src_hi", "dst_lo", "dst_hi", "relabel_lo", "relabel_hi", "max_dist", "ratio_num",
                                         "ratio_den")] + [("radius", C.c_float), ("reserved", C.c_int32)]


class SvoFuseResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_pairs", "n_same", "n_fused", "n_rows_relabelled")]


class SvoPlaceParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("row_lo", "row_hi", "max_dist", "ratio_num", "ratio_den", "tag_lo", "tag_hi", "min_votes", "separation",
                                         "max_places")]


class SvoPlaceResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_landmarks", "n_tags_voted", "n_places")]


PLACE_DTYPE = np.dtype([("tag", "<i4"), ("votes", "<i4"), ("rows", "<i4"), ("row_first", "<i4"), ("row_end", "<i4"), ("reserved", "<i4", 3)])
assert PLACE_DTYPE.itemsize == 32
PLACE_MAX_TAGS, PLACE_MAX_PLACES, PLACE_MAX_IDS = 1 << 20, 64, 4096
PLACE_BATCH_MAX_CAMERAS, PLACE_BATCH_MAX_IDS, PLACE_BATCH_MAX_BINS = 1024, 1 << 20, 1 << 24


class SvoConsolidateParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("row_lo", "row_hi", "tag_lo", "tag_hi")] + [("radius", C.c_float), ("reserved", C.c_int32)]


class SvoConsolidateResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_members", "n_groups", "n_dropped", "n_far_views", "n_capped_groups", "n_kept")] + \
               [("reserved", C.c_int32 * 2)]


CONSOLIDATE_MAX_VIEWS = 64


class SvoDescInsertStats(C.Structure):
    _fields_ = [("last_kernels_ms", C.c_float), ("last_path", C.c_int32), ("rows_scanned", C.c_uint64), ("rows_added", C.c_uint64)]


INSERT_MAX_ENTRIES, INSERT_MAX_OBS_ROWS = 1024, 1 << 18
INSERT_PATH_NONE, INSERT_PATH_RING, INSERT_PATH_STAGED = 0, 1, 2


class SvoRetireRule(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("row_lo", C.c_int32), ("row_hi", C.c_int32), ("tag_lo", C.c_int32), ("tag_hi", C.c_int32),
                ("n_ids", C.c_int32), ("ids", C.c_void_p)]


class SvoDescRetireStats(C.Structure):
    _fields_ = SvoDescIndexStats._fields_


# Every function include/svo.h declares, in its order: name -> (restype, argtypes).  tests/test_abi.py parses the header and compares
# it with this table argument by argument.  Every pointer or array argument is P: an array's ptr(), C.byref(x), a ctypes array, None
# or a raw address (a tensor's data_ptr()).
I, I32, U32, I64, SZ, F, D, P = C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_size_t, C.c_float, C.c_double, C.c_void_p
PROTOTYPES = {
    "svo_last_error": (C.c_char_p, ()),
    "svo_device_count": (I, ()),
    "svo_config_default": (None, (P,)),
    "svo_create": (I, (P, I, I, I, I, P)),
    "svo_destroy": (None, (P,)),
    "svo_set_projection": (I, (P, I, P, P)),
    "svo_process_batch": (I, (P, P, P, I, I, P, P, P)),
    "svo_alloc_pinned": (P, (SZ,)),
    "svo_free_pinned": (None, (P,)),
    "svo_process": (I, (P, P, P, I, P, P)),
    "svo_circular_matching": (I, (P, P, P, I, I, P, P, P, P, P, P)),
    "svo_get_lk_registers_left": (I, (P,)),
    "svo_get_last_frame_path": (I, (P,)),
    "svo_submit_batch": (I, (P, P, P, I)),
    "svo_collect": (I, (P, P, P, P)),
    "svo_process_batch_masked": (I, (P, P, P, I, I, P, P, P, P)),
    "svo_submit_batch_masked": (I, (P, P, P, I, P)),
    "svo_reset_sequence": (I, (P, I, P, P)),
    "svo_set_rectification_maps": (I, (P, I, I, I, P, P, P, P)),
    "svo_set_rectification": (I, (P, I, P, P)),
    "svo_clear_rectification": (I, (P,)),
    "svo_set_input_format": (I, (P, I)),
    "svo_set_clahe": (I, (P, I, D, I, I)),
    "svo_set_pose_covariance": (I, (P, I, D)),
    "svo_get_last_pose_covariance": (I, (P, P, P, P)),
    "svo_get_features": (I, (P, I, I, P, P, P)),
    "svo_get_last_tracks": (I, (P, I, I, P, P, P, P, P, P)),
    "svo_set_track_output": (I, (P, I, I)),
    "svo_get_last_track_obs": (I, (P, I, I, P, P)),
    "svo_get_feature_ids": (I, (P, I, I, P)),
    "svo_set_descriptor_output": (I, (P, I)),
    "svo_get_last_track_descriptors": (I, (P, I, I, P, P)),
    "svo_descriptor_pattern": (I, (P, P)),
    "svo_desc_index_create": (I, (I, I, P)),
    "svo_desc_index_destroy": (None, (P,)),
    "svo_desc_index_add": (I, (P, I, P, P, P)),
    "svo_desc_index_add_frame": (I, (P, P, I, U32, P, P)),
    "svo_desc_index_size": (I, (P,)),
    "svo_desc_index_truncate": (I, (P, I)),
    "svo_desc_index_match": (I, (P, I, P, I, I, P)),
    "svo_desc_index_set_chunk_rows": (I, (P, I)),
    "svo_desc_index_get_chunk_rows": (I, (P,)),
    "svo_desc_index_set_timing": (I, (P, I)),
    "svo_desc_index_get_stats": (I, (P, P)),
    "svo_reloc_params_default": (None, (P,)),
    "svo_desc_index_enable_points": (I, (P,)),
    "svo_desc_index_add_points": (I, (P, I, P, P, P, P, P)),
    "svo_desc_index_add_frame_points": (I, (P, P, I, U32, P, I32, P, P)),
    "svo_desc_index_select": (I, (P, I, P, P, P, P, P, P, P, P)),
    "svo_desc_index_localize": (I, (P, P, I, P, P, P, P, P, P, P)),
    "svo_desc_index_project": (I, (P, P, P, I, I, P)),
    "svo_desc_index_match_guided": (I, (P, P, P, I, P, P, I, I, P)),
    "svo_desc_index_select_guided": (I, (P, P, P, I, P, P, P, P, P, P, P, P)),
    "svo_desc_index_localize_guided": (I, (P, P, P, I, P, P, P, P, P, P, P)),
    "svo_desc_index_set_guided_sort": (I, (P, I)),
    "svo_desc_index_retire": (I, (P, P, P, P)),
    "svo_desc_index_transform_points": (I, (P, P, I, I, I32, I32, P, P)),
    "svo_desc_index_set_retire_slab_rows": (I, (P, I)),
    "svo_desc_index_get_retire_slab_rows": (I, (P,)),
    "svo_desc_index_get_retire_stats": (I, (P, P)),
    "svo_desc_index_localize_batch": (I, (P, I, P, P, P, P, P, P, P, P, P, P)),
    "svo_desc_index_get_batch_order": (I, (P, I, P, P)),
    "svo_desc_index_add_frames": (I, (P, P, I, P, U32, P, P, P)),
    "svo_desc_index_add_frames_points": (I, (P, P, I, P, U32, P, P, P, P, P)),
    "svo_desc_index_add_obs": (I, (P, I, P, P, P, U32, P, I, P, P, P, P)),
    "svo_desc_index_get_insert_stats": (I, (P, P)),
    "svo_align_params_default": (None, (P, F)),
    "svo_align_sample": (I, (U32, I32, P)),
    "svo_desc_index_match_rows": (I, (P, I, I, I, I, P)),
    "svo_desc_index_pair_rows": (I, (P, P, P, P, P)),
    "svo_desc_index_align": (I, (P, P, P, P, P, P)),
    "svo_fuse_params_default": (None, (P, F)),
    "svo_desc_index_match_near": (I, (P, I, I, I, I, F, P)),
    "svo_desc_index_pair_near": (I, (P, P, P, P, P)),
    "svo_desc_index_relabel": (I, (P, I, P, P, I, I, P)),
    "svo_desc_index_fuse": (I, (P, P, P, P, P)),
    "svo_place_params_default": (None, (P,)),
    "svo_desc_index_tag_votes": (I, (P, I, P, I, I, I, I, P, P, P, P)),
    "svo_desc_index_places": (I, (P, I, P, P, P, P, P, P)),
    "svo_desc_index_places_from_ids": (I, (P, I, P, P, P, P)),
    "svo_desc_index_set_place_combine": (I, (P, I)),
    "svo_desc_index_tag_votes_batch": (I, (P, I, P, P, I, I, I32, I32, P, P, P, P)),
    "svo_desc_index_places_from_ids_batch": (I, (P, I, P, P, P, P, P)),
    "svo_desc_index_places_batch": (I, (P, I, P, P, P, P, P, P, P)),
    "svo_consolidate_params_default": (None, (P, F)),
    "svo_desc_index_consolidate": (I, (P, P, P, P)),
    "svo_desc_index_read_rows": (I, (P, I, I, P, P, P, P)),
    "svo_set_detection_mask": (I, (P, I, P, I, I)),
    "svo_get_detection_mask": (I, (P, I, P, P)),
    "svo_set_motion_prior": (I, (P, I, P, P)),
    "svo_set_motion_priors": (I, (P, P, P, P)),
    "svo_get_motion_prior": (I, (P, I, P, P, P)),
    "svo_motion_prior_from_rotation": (I, (P, P, P, P)),
    "svo_set_motion_prior_mode": (I, (P, I)),
    "svo_get_motion_prior_mode": (I, (P, P)),
    "svo_get_last_motion_prior": (I, (P, I, P, P, P)),
    "svo_get_pyramid": (I, (P, I, I, I, I, I, P, I64, P, P, P, P)),
    "svo_get_derivatives": (I, (P, I, I, I, I, P, P, I64, P, P, P, P)),
    "svo_get_last_timing": (I, (P, P, P)),
    "svo_set_stage_timing": (I, (P, I)),
    "svo_get_stage_timing": (I, (P, P)),
    "svo_get_stream": (P, (P,)),
    "svo_stage_cache_clear": (None, ()),
    "svo_stage_cache_clear_all": (I, ()),
    "svo_fast_detect": (I, (I, P, I, I, I, I, I, P, P, P)),
    "svo_fast_detect_masked": (I, (I, P, I, I, I, I, P, I, I, P, P, P)),
    "svo_fast_score_map": (I, (I, P, I, I, I, I, P)),
    "svo_bucket_filter": (I, (I, I, I, P, P, P, P, I, I, I, I, I, I)),
    "svo_append_features_from_image": (I, (I, P, P, I, I, I, I, I, P, P, P, P)),
    "svo_append_features_from_image_masked": (I, (I, P, P, I, I, I, I, P, I, I, P, P, P, P)),
    "svo_build_pyramid": (I, (I, P, I, I, I, I, I, P, I64, P)),
    "svo_lk_track": (I, (I, P, P, I, I, I, I, P, P, P, I, I, I, D, D)),
    "svo_lk_track_guess": (I, (I, P, P, I, I, I, I, P, P, P, P, I, I, I, D, D)),
    "svo_circular_match": (I, (I, P, P, P, P, P, I, I, I, I, P, P, P, P, P, P)),
    "svo_circular_match_prior": (I, (I, P, P, P, P, P, I, I, I, I, P, P, P, P, P, P, P, P)),
    "svo_find_close_points": (I, (I, I, P, P, F, P)),
    "svo_triangulate": (I, (I, P, P, I, P, P, P)),
    "svo_camera_to_world": (I, (I, P, I, P, P, P, P, P, P, P, I, F, F, P)),
    "svo_pose_covariance": (I, (I, P, I, P, P, P, P, P, I, D, P, P, P)),
    "svo_init_rectify_map": (I, (P, P, I, P, P, I, I, P, P)),
    "svo_rectify_image": (I, (I, P, P, I, I, P, I, I, I, I, P)),
    "svo_convert_gray": (I, (I, I, P, I, I, I, P)),
    "svo_clahe": (I, (I, I, P, I, I, I, D, I, I, P)),
    "svo_describe_points": (I, (I, P, I, I, I, I, P, P, P)),
    "svo_inverse_transform": (I, (I, P, P, P)),
}
for _name, (_restype, _argtypes) in PROTOTYPES.items():
    _fn = getattr(lib, _name)                         # a symbol the library lacks fails the import here
    _fn.restype, _fn.argtypes = _restype, list(_argtypes)
EXPORTS = list(PROTOTYPES)


def check(rc):
    if rc < 0:
        raise SvoError("libsvo_hip status %d: %s" % (rc, (lib.svo_last_error() or b"").decode()))
    return rc


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def default_config(**over):
    c = SvoConfig()
    lib.svo_config_default(C.byref(c))
    for k, v in over.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def copy_config(cfg):
    c = SvoConfig()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(SvoConfig))
    return c


def device_count():
    return lib.svo_device_count()


def u8img(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim != 2:
        raise ValueError("single-channel 8-bit image expected (the ROS path delivers MONO8, src/stereo_vo.cpp:9)")
    return img


def u8frame(img, bpp=None):
    """A frame for the frame pipeline: (H, W) gray, or (H, W, 3) interleaved BGR as the reference CLI feeds it (svo.h: channels);
    bpp (the bytes per pixel of a context's input format, svo.h SVO_INPUT_*): (H, W, bpp), or (H, W) when bpp is 1."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if bpp is not None and bpp > 1:
        if not (img.ndim == 3 and img.shape[2] == bpp):
            raise ValueError("8-bit (H, W, %d) image expected for the input format that is set" % bpp)
    elif not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
        raise ValueError("8-bit (H, W) or (H, W, 3) image expected")
    return img


def cov_mode(mode):
    """An SVO_COV_* constant or "off" / "residual" / "fixed" -> the constant (the library checks the range)."""
    if isinstance(mode, str):
        if mode not in COV_MODES:
            raise ValueError("unknown pose-covariance mode %r (one of %s)" % (mode, ", ".join(COV_MODES)))
        return COV_MODES[mode]
    return int(mode)


def check_cov(mode, pixel_sigma):
    """(mode, pixel_sigma) as svo_set_pose_covariance checks them -> (constant, float); ValueError otherwise."""
    m, s = cov_mode(mode), float(pixel_sigma)
    if m not in COV_MODES.values():
        raise ValueError("unknown pose-covariance mode %r" % (mode,))
    if m == COV_FIXED_SIGMA and not (s > 0 and np.isfinite(s)):
        raise ValueError("pixel_sigma must be positive and finite")
    return m, s


def input_format(fmt):
    """An SVO_INPUT_* constant or a sensor_msgs encoding name ("mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422" (UYVY),
    "yuv422_yuy2") -> the constant."""
    if isinstance(fmt, str):
        if fmt not in INPUT_ENCODINGS:
            raise ValueError("unknown image encoding %r (one of %s)" % (fmt, ", ".join(INPUT_ENCODINGS)))
        return INPUT_ENCODINGS[fmt]
    fmt = int(fmt)
    if not 0 <= fmt < len(INPUT_BPP):
        raise ValueError("unknown input format %d" % fmt)
    return fmt


def check_clahe(clip_limit, tiles):
    """(clip_limit, tiles) as svo_set_clahe checks them before it looks at a size -> (float, tiles_x, tiles_y); ValueError otherwise."""
    clip = float(clip_limit)
    try:
        tx, ty = (int(t) for t in tiles)
    except (TypeError, ValueError):
        raise ValueError("tiles must be a pair (tiles_x, tiles_y)")
    if not (1 <= tx <= 16 and 1 <= ty <= 16):
        raise ValueError("CLAHE tiles must be 1 .. 16 in both directions")
    if not np.isfinite(clip):
        raise ValueError("CLAHE clip_limit must be finite")
    return clip, tx, ty
