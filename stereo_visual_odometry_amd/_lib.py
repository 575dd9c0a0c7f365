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

SVO_OK, SVO_ERR_ARG, SVO_ERR_HIP, SVO_ERR_CAPACITY, SVO_ERR_STATE = 0, -1, -2, -3, -4


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


lib.svo_last_error.restype = C.c_char_p
lib.svo_alloc_pinned.restype = C.c_void_p
lib.svo_alloc_pinned.argtypes = [C.c_size_t]
lib.svo_free_pinned.restype = None
lib.svo_free_pinned.argtypes = [C.c_void_p]
lib.svo_get_stream.restype = C.c_void_p
lib.svo_stage_cache_clear.restype = None
lib.svo_stage_cache_clear.argtypes = []
lib.svo_get_stream.argtypes = [C.c_void_p]
lib.svo_get_lk_registers_left.restype = C.c_int
lib.svo_get_lk_registers_left.argtypes = [C.c_void_p]
lib.svo_get_last_frame_path.restype = C.c_int
lib.svo_get_last_frame_path.argtypes = [C.c_void_p]
# svo_get_last_frame_path bits (svo.h SVO_PATH_*)
PATH_LEAN, PATH_LK_CHAINED, PATH_INGEST_AHEAD, PATH_FRONT_FUSED, PATH_TRI_EPNP_FUSED, PATH_GRAPH = 1, 2, 4, 8, 16, 32
PATH_INPUT_CONVERTED = 64
PATH_POSE_COV = 128
PATH_DETECT_MASKED = 256
PATH_CLAHE = 512
PATH_TRACK_IDS = 1024
# track ids and observation rows (svo.h svo_track_obs): the 64-byte row as a ctypes structure and as a numpy structured dtype
OBS_INLIER, OBS_HAS_XYZ = 1, 2


class SvoTrackObs(C.Structure):
    _fields_ = [("id", C.c_int64), ("l0", C.c_float * 2), ("r0", C.c_float * 2), ("l1", C.c_float * 2), ("r1", C.c_float * 2),
                ("xyz", C.c_float * 3), ("age", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32)]


TRACK_OBS_DTYPE = np.dtype([("id", "<i8"), ("l0", "<f4", 2), ("r0", "<f4", 2), ("l1", "<f4", 2), ("r1", "<f4", 2),
                            ("xyz", "<f4", 3), ("age", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert TRACK_OBS_DTYPE.itemsize == 64 and C.sizeof(SvoTrackObs) == 64
if hasattr(lib, "svo_set_track_output"):
    lib.svo_set_track_output.restype = C.c_int
    lib.svo_set_track_output.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.svo_get_last_track_obs.restype = C.c_int
    lib.svo_get_last_track_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.svo_get_feature_ids.restype = C.c_int
    lib.svo_get_feature_ids.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
# binary descriptors (svo.h, "Binary descriptors"): rows of DESC_BYTES bytes beside the observation rows
PATH_DESCRIPTORS = 8192
DESC_BYTES = 32
lib.svo_set_descriptor_output.restype = C.c_int
lib.svo_set_descriptor_output.argtypes = [C.c_void_p, C.c_int]
lib.svo_get_last_track_descriptors.restype = C.c_int
lib.svo_get_last_track_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
lib.svo_describe_points.restype = C.c_int
lib.svo_describe_points.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_descriptor_pattern.restype = C.c_int
lib.svo_descriptor_pattern.argtypes = [C.c_void_p, C.c_void_p]
# descriptor index (svo.h, "Descriptor index"): the 32-byte result row as a numpy structured dtype
MATCH_NONE, MATCH_NO_DIST = -1, 257
DESC_MATCH_DTYPE = np.dtype([("id", "<u8"), ("id2", "<u8"), ("row", "<i4"), ("row2", "<i4"), ("dist", "<u2"), ("dist2", "<u2"), ("reserved", "<u4")])
assert DESC_MATCH_DTYPE.itemsize == 32
lib.svo_desc_index_create.restype = C.c_int
lib.svo_desc_index_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
lib.svo_desc_index_destroy.restype = None
lib.svo_desc_index_destroy.argtypes = [C.c_void_p]
lib.svo_desc_index_add.restype = C.c_int
lib.svo_desc_index_add.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
lib.svo_desc_index_add_frame.restype = C.c_int
lib.svo_desc_index_add_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.svo_desc_index_size.restype = C.c_int
lib.svo_desc_index_size.argtypes = [C.c_void_p]
lib.svo_desc_index_truncate.restype = C.c_int
lib.svo_desc_index_truncate.argtypes = [C.c_void_p, C.c_int]
lib.svo_desc_index_match.restype = C.c_int
lib.svo_desc_index_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
lib.svo_desc_index_set_chunk_rows.restype = C.c_int
lib.svo_desc_index_set_chunk_rows.argtypes = [C.c_void_p, C.c_int]
lib.svo_desc_index_get_chunk_rows.restype = C.c_int
lib.svo_desc_index_get_chunk_rows.argtypes = [C.c_void_p]


class SvoDescIndexStats(C.Structure):
    _fields_ = [("last_kernels_ms", C.c_float), ("scratch_allocations", C.c_int32), ("scratch_bytes", C.c_uint64), ("scratch_bytes_outgrown", C.c_uint64)]


lib.svo_desc_index_set_timing.restype = C.c_int
lib.svo_desc_index_set_timing.argtypes = [C.c_void_p, C.c_int]
lib.svo_desc_index_get_stats.restype = C.c_int
lib.svo_desc_index_get_stats.argtypes = [C.c_void_p, C.POINTER(SvoDescIndexStats)]
# relocalisation (svo.h, "Relocalisation"): points in the index, select and localize
POINT_NONE, RELOC_MAX_QUERIES = -1, 4096


class SvoRelocParams(C.Structure):
    _fields_ = [("row_lo", C.c_int32), ("row_hi", C.c_int32), ("max_dist", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32),
                ("min_candidates", C.c_int32), ("ransac_iterations", C.c_int32), ("reproj_error", C.c_float), ("confidence", C.c_float)]


class SvoRelocResult(C.Structure):
    _fields_ = [("success", C.c_int32), ("n_candidates", C.c_int32), ("n_inliers", C.c_int32), ("iters_run", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("T", C.c_double * 16)]


lib.svo_reloc_params_default.restype = None
lib.svo_reloc_params_default.argtypes = [C.POINTER(SvoRelocParams)]
lib.svo_desc_index_enable_points.restype = C.c_int
lib.svo_desc_index_enable_points.argtypes = [C.c_void_p]
lib.svo_desc_index_add_points.restype = C.c_int
lib.svo_desc_index_add_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
lib.svo_desc_index_add_frame_points.restype = C.c_int
lib.svo_desc_index_add_frame_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int32, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.svo_desc_index_select.restype = C.c_int
lib.svo_desc_index_select.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SvoRelocParams), C.POINTER(C.c_int),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_desc_index_localize.restype = C.c_int
lib.svo_desc_index_localize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SvoRelocParams),
                                        C.POINTER(SvoRelocResult), C.c_void_p, C.c_void_p, C.c_void_p]
# guided search (svo.h, "Guided search"): the same calls behind a pose prior's projection gate


class SvoRelocGuide(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("radius", C.c_float), ("reserved", C.c_int32)]


lib.svo_desc_index_project.restype = C.c_int
lib.svo_desc_index_project.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SvoRelocGuide), C.c_int, C.c_int, C.c_void_p]
lib.svo_desc_index_match_guided.restype = C.c_int
lib.svo_desc_index_match_guided.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SvoRelocGuide), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
lib.svo_desc_index_select_guided.restype = C.c_int
lib.svo_desc_index_select_guided.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SvoRelocGuide), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SvoRelocParams),
                                             C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_desc_index_localize_guided.restype = C.c_int
lib.svo_desc_index_localize_guided.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SvoRelocGuide), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(SvoRelocParams),
                                               C.POINTER(SvoRelocResult), C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_desc_index_set_guided_sort.restype = C.c_int
lib.svo_desc_index_set_guided_sort.argtypes = [C.c_void_p, C.c_int]
# motion priors (svo.h): H / Hi are 9 float32 each (n_seq x 9 in the batch setter), has n_seq bytes; R is 9 float64
PATH_MOTION_PRIOR = 2048
lib.svo_set_motion_prior.restype = C.c_int
lib.svo_set_motion_prior.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.svo_set_motion_priors.restype = C.c_int
lib.svo_set_motion_priors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_get_motion_prior.restype = C.c_int
lib.svo_get_motion_prior.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
lib.svo_motion_prior_from_rotation.restype = C.c_int
lib.svo_motion_prior_from_rotation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
PATH_PRIOR_PREDICTED = 4096
PRIOR_EXPLICIT, PRIOR_LAST_ROTATION = 0, 1
PRIOR_MODES = {"explicit": PRIOR_EXPLICIT, "last_rotation": PRIOR_LAST_ROTATION}
lib.svo_set_motion_prior_mode.restype = C.c_int
lib.svo_set_motion_prior_mode.argtypes = [C.c_void_p, C.c_int]
lib.svo_get_motion_prior_mode.restype = C.c_int
lib.svo_get_motion_prior_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
lib.svo_get_last_motion_prior.restype = C.c_int
lib.svo_get_last_motion_prior.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
lib.svo_lk_track_guess.restype = C.c_int
lib.svo_lk_track_guess.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
lib.svo_circular_match_prior.restype = C.c_int
lib.svo_circular_match_prior.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
# CLAHE (svo.h): the equalisation in front of frame ingest, and the stage alone
lib.svo_set_clahe.restype = C.c_int
lib.svo_set_clahe.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int]
lib.svo_clahe.restype = C.c_int
lib.svo_clahe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]
# detection masks (svo.h): mask is a host or device pointer to height rows of width bytes
lib.svo_set_detection_mask.restype = C.c_int
lib.svo_set_detection_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
lib.svo_get_detection_mask.restype = C.c_int
lib.svo_get_detection_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
lib.svo_fast_detect_masked.restype = C.c_int
lib.svo_fast_detect_masked.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_int)]
lib.svo_append_features_from_image_masked.restype = C.c_int
lib.svo_append_features_from_image_masked.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                      C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
# pose covariance (svo.h SVO_COV_*): cov_T / cov_p are n_seq x 36 doubles, valid n_seq ints
COV_OFF, COV_RESIDUAL, COV_FIXED_SIGMA = 0, 1, 2
COV_MODES = {"off": COV_OFF, "residual": COV_RESIDUAL, "fixed": COV_FIXED_SIGMA}
lib.svo_set_pose_covariance.restype = C.c_int
lib.svo_set_pose_covariance.argtypes = [C.c_void_p, C.c_int, C.c_double]
lib.svo_get_last_pose_covariance.restype = C.c_int
lib.svo_get_last_pose_covariance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_pose_covariance.restype = C.c_int
lib.svo_pose_covariance.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
# input formats (svo.h SVO_INPUT_*): what the bytes of the caller's frames are; the sensor_msgs encoding names map onto them
INPUT_MONO8, INPUT_BGR8, INPUT_RGB8, INPUT_BGRA8, INPUT_RGBA8, INPUT_UYVY, INPUT_YUY2 = range(7)
INPUT_ENCODINGS = {"mono8": INPUT_MONO8, "bgr8": INPUT_BGR8, "rgb8": INPUT_RGB8, "bgra8": INPUT_BGRA8, "rgba8": INPUT_RGBA8,
                   "yuv422": INPUT_UYVY, "yuv422_yuy2": INPUT_YUY2}
INPUT_BPP = (1, 3, 3, 4, 4, 2, 2)
lib.svo_set_input_format.restype = C.c_int
lib.svo_set_input_format.argtypes = [C.c_void_p, C.c_int]
lib.svo_convert_gray.restype = C.c_int
lib.svo_convert_gray.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
# ragged / continuous batching (svo.h): active is a host array of n_seq bytes or NULL; Pl / Pr 12 floats each or both NULL
lib.svo_process_batch_masked.restype = C.c_int
lib.svo_process_batch_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_submit_batch_masked.restype = C.c_int
lib.svo_submit_batch_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
lib.svo_reset_sequence.restype = C.c_int
lib.svo_reset_sequence.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
# rectification (svo.h): maps are int16 (h, w, 2) + uint16 (h, w) host arrays
lib.svo_init_rectify_map.restype = C.c_int
lib.svo_init_rectify_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
lib.svo_set_rectification_maps.restype = C.c_int
lib.svo_set_rectification_maps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.svo_set_rectification.restype = C.c_int
lib.svo_set_rectification.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.svo_clear_rectification.restype = C.c_int
lib.svo_clear_rectification.argtypes = [C.c_void_p]
lib.svo_rectify_image.restype = C.c_int
lib.svo_rectify_image.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
# pyramid read-out (svo.h svo_get_pyramid): one level with its stored border, packed
lib.svo_get_pyramid.restype = C.c_int
lib.svo_get_pyramid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
PYR_T1, PYR_LAST_LEFT = 0, 1
# derivative-plane read-out (svo.h svo_get_derivatives): the int16 Ix / Iy planes of one level >= 1 with their zero border
lib.svo_get_derivatives.restype = C.c_int
lib.svo_get_derivatives.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]

# every symbol include/svo.h declares (tests/test_abi.py checks the list against the header)
EXPORTS = [
    "svo_last_error", "svo_device_count", "svo_config_default", "svo_create", "svo_destroy", "svo_set_projection",
    "svo_process_batch", "svo_process_batch_masked", "svo_submit_batch_masked", "svo_reset_sequence", "svo_process", "svo_alloc_pinned", "svo_free_pinned", "svo_circular_matching", "svo_submit_batch", "svo_collect", "svo_get_features", "svo_get_last_tracks",
    "svo_get_pyramid", "svo_get_derivatives",
    "svo_get_lk_registers_left", "svo_get_last_frame_path", "svo_get_last_timing", "svo_set_stage_timing", "svo_get_stage_timing", "svo_get_stream", "svo_fast_detect", "svo_fast_score_map", "svo_bucket_filter",
    "svo_append_features_from_image", "svo_build_pyramid", "svo_lk_track", "svo_circular_match",
    "svo_find_close_points", "svo_stage_cache_clear", "svo_stage_cache_clear_all", "svo_triangulate", "svo_camera_to_world", "svo_inverse_transform",
    "svo_set_rectification_maps", "svo_set_rectification", "svo_clear_rectification", "svo_init_rectify_map", "svo_rectify_image",
    "svo_set_input_format", "svo_convert_gray",
    "svo_set_pose_covariance", "svo_get_last_pose_covariance", "svo_pose_covariance",
    "svo_set_detection_mask", "svo_get_detection_mask", "svo_fast_detect_masked", "svo_append_features_from_image_masked",
    "svo_set_clahe", "svo_clahe",
    "svo_set_track_output", "svo_get_last_track_obs", "svo_get_feature_ids",
    "svo_set_motion_prior", "svo_set_motion_priors", "svo_get_motion_prior", "svo_motion_prior_from_rotation",
    "svo_lk_track_guess", "svo_circular_match_prior",
    "svo_set_motion_prior_mode", "svo_get_motion_prior_mode", "svo_get_last_motion_prior",
    "svo_set_descriptor_output", "svo_get_last_track_descriptors", "svo_describe_points", "svo_descriptor_pattern",
    "svo_desc_index_create", "svo_desc_index_destroy", "svo_desc_index_add", "svo_desc_index_add_frame", "svo_desc_index_size",
    "svo_desc_index_truncate", "svo_desc_index_match", "svo_desc_index_set_chunk_rows", "svo_desc_index_get_chunk_rows",
    "svo_desc_index_set_timing", "svo_desc_index_get_stats",
    "svo_reloc_params_default", "svo_desc_index_enable_points", "svo_desc_index_add_points", "svo_desc_index_add_frame_points",
    "svo_desc_index_select", "svo_desc_index_localize",
    "svo_desc_index_project", "svo_desc_index_match_guided", "svo_desc_index_select_guided", "svo_desc_index_localize_guided",
    "svo_desc_index_set_guided_sort",
]


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
