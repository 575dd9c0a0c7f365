"""Host-side mirror of the reference's C++ surface (include/vo.h) over the C-ABI of libsvo_hip.so.

Same names, argument meaning and failure behaviour as namespace visual_odometry:
VisualOdometry (vo.h:231-380), FeatureSet (vo.h:132-188), Bucket (vo.h:195-229) and the free
functions featureDetectionFast / deletePointsWithFailureStatus / deleteFeaturesWithFailureStatus /
findClosePoints / cameraToWorld / getInverseTransform (vo.h:393-470).  cv::Mat becomes numpy,
std::vector<cv::Point2f> becomes an (N,2) float32 array.  All arithmetic runs on the GPU.
"""
import collections
import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import SvoCameraInfo, SvoConfig, SvoFrameStats, check, default_config, lib, ptr, u8frame, u8img

# the reference's constants (include/vo.h:53-127) for callers that used them by name
BUCKET_START_ROW, BUCKETS_ALONG_HEIGHT, BUCKETS_ALONG_WIDTH, FEATURES_PER_BUCKET = 4, 92, 160, 1
FEATURES_THRESHOLD, PRE_MATCHING_FEATURE_THRESHOLD, AGE_THRESHOLD, FAST_THRESHOLD = 15, 100, 20, 20
RANSAC_REPROJECTION_ERROR, RANSAC_ITERATIONS = 8.0, 100
OPTICAL_FLOW_MIN_EIG_THRESHOLD, CIRCULAR_MATCHING_SUCCESS_THRESHOLD = 0.001, 0.15
MAX_TRANSLATION_NORM, MAX_ROTATION_NORM = 0.1, 0.5


def _pts(p):
    return np.ascontiguousarray(p, np.float32).reshape(-1, 2)


def _K9(K):
    """The camera matrix as 9 float32: a 3x3 (or its 9 values), or the left 3x3 of a 3x4 projection matrix."""
    k = np.asarray(K, np.float32)
    return np.ascontiguousarray(k.reshape(-1) if k.size == 9 else k[:3, :3]).reshape(9).copy()


def _strided_u8(image, f):
    """An image in the format f (an SVO_INPUT_* constant) for the stage calls that take a row stride -> a uint8 (h, w, bpp) array,
    (h, w) for mono8, whose rows may be strided: a view's strides[0] is passed on."""
    bpp = _lib.INPUT_BPP[f]
    img = np.asarray(image)
    if img.dtype != np.uint8 or not ((img.ndim == 3 and img.shape[2] == bpp) or (bpp == 1 and img.ndim == 2)):
        raise ValueError("uint8 (h, w, %d) image expected for this format" % bpp)
    if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != bpp):
        img = np.ascontiguousarray(img)
    return img


# ---------------------------------------------------------------------------- free functions
def _host_mask(mask, height, width):
    """A detection mask as a contiguous (height, width) uint8 array; ValueError for another shape or dtype."""
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.shape != (height, width):
        raise ValueError("detection mask: (%d, %d) uint8 expected, got %s %s" % (height, width, m.shape, m.dtype))
    return np.ascontiguousarray(m)


def featureDetectionFast(image, fast_threshold, device=0, mask=None):
    """vo.h:393-395 — returns (points (N,2) f32, response_strengths (N,) f32), raster order.  mask: an (H, W) uint8 detection
    mask (svo.h: non-zero = allowed), applied to the keypoints that survived non-max suppression, as cv::FeatureDetector does."""
    img = u8img(image)
    h, w = img.shape
    m = _host_mask(mask, h, w) if mask is not None else None
    cap = 4096
    while True:
        xy = np.zeros((cap, 2), np.float32)
        resp = np.zeros(cap, np.float32)
        n = C.c_int(0)
        if m is not None:
            check(lib.svo_fast_detect_masked(device, ptr(img), w, h, w, int(fast_threshold), ptr(m), w, cap, ptr(xy), ptr(resp), C.byref(n)))
        else:
            check(lib.svo_fast_detect(device, ptr(img), w, h, w, int(fast_threshold), cap, ptr(xy), ptr(resp), C.byref(n)))
        if n.value <= cap:
            return xy[:n.value].copy(), resp[:n.value].copy()
        cap = n.value


def fastScoreMap(image, fast_threshold, device=0):
    img = u8img(image)
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    check(lib.svo_fast_score_map(device, ptr(img), w, h, w, int(fast_threshold), ptr(out)))
    return out


def deletePointsWithFailureStatus(point_vector, is_ok):
    """vo.h:406-407 — stable removal of entries whose flag is false (host-side list op)."""
    is_ok = np.asarray(is_ok, bool)
    pv = _pts(point_vector)
    keep = np.ones(len(pv), bool)
    keep[:len(is_ok)] = is_ok
    return pv[keep]


def deleteFeaturesWithFailureStatus(features, is_ok):
    """vo.h:416-417"""
    is_ok = np.asarray(is_ok, bool)
    keep = np.ones(features.size(), bool)
    keep[:len(is_ok)] = is_ok
    features.points = features.points[keep]
    features.ages = features.ages[keep]
    features.strengths = features.strengths[keep]


def findClosePoints(points_1, points_2, threshold, device=0):
    """vo.h:430-432 — v[i] = max(|dx|,|dy|) <= threshold."""
    p1, p2 = _pts(points_1), _pts(points_2)
    ok = np.zeros(len(p1), np.uint8)
    check(lib.svo_find_close_points(device, len(p1), ptr(p1), ptr(p2), C.c_float(threshold), ptr(ok)))
    return ok.astype(bool)


def cameraToWorld(cameraProjection, cameraPoints, worldPoints, rotation, translation,
                  iterations=RANSAC_ITERATIONS, reprojection_error=RANSAC_REPROJECTION_ERROR, confidence=0.98, device=0):
    """vo.h:452-456 — returns ((inliers, success), rotation, translation, iterations_run): the reference's pair, then its two
    in/out arguments (the updated values on success, the inputs on failure, vo.cpp:307-311), then how many RANSAC iterations
    the adaptive loop ran (a counter the reference does not expose)."""
    K = _K9(cameraProjection)
    cam = _pts(cameraPoints)
    world = np.ascontiguousarray(worldPoints, np.float32).reshape(-1, 3)
    n = len(cam)
    R = np.ascontiguousarray(rotation, np.float64).reshape(9).copy()
    t = np.ascontiguousarray(translation, np.float64).reshape(3).copy()
    inl = np.zeros(max(n, 1), np.int32)
    nin, ok, iters = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib.svo_camera_to_world(device, ptr(K), n, ptr(cam), ptr(world), ptr(R), ptr(t), ptr(inl), C.byref(nin), C.byref(ok),
                                  int(iterations), C.c_float(reprojection_error), C.c_float(confidence), C.byref(iters)))
    return (inl[:nin.value].copy(), bool(ok.value)), R.reshape(3, 3), t.reshape(3, 1), iters.value


def poseCovariance(cameraProjection, cameraPoints, worldPoints, rotation, translation, inliers=None, mode="residual",
                   pixel_sigma=1.0, device=0, inlier_indices=None):
    """svo_pose_covariance: the 6x6 covariances of a cameraToWorld result (its inputs, its R and t) -> (cov_p, cov_T, valid).
    The points that count: inliers = n FLAGS, or inlier_indices = the index list cameraToWorld returns (one of the two; neither =
    every point).  cov_p is in the order (r, t) of the cameraToWorld parameters, cov_T in the order (position,
    rotation) of the inverse transform getInverseTransform(R, t), as ROS orders a pose covariance.  A singular system gives
    valid False and zeros."""
    K = _K9(cameraProjection)
    cam = _pts(cameraPoints)
    world = np.ascontiguousarray(worldPoints, np.float32).reshape(-1, 3)
    if len(world) != len(cam):
        raise ValueError("cameraPoints and worldPoints differ in length")
    R = np.ascontiguousarray(rotation, np.float64).reshape(9)
    t = np.ascontiguousarray(translation, np.float64).reshape(3)
    inl = None
    if inlier_indices is not None:
        if inliers is not None:
            raise ValueError("give inliers (flags) or inlier_indices, not both")
        idx = np.asarray(inlier_indices, np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(cam)):
            raise ValueError("inlier_indices out of range")
        inliers = np.zeros(len(cam), bool); inliers[idx] = True
    if inliers is not None:
        inl = np.ascontiguousarray(np.asarray(inliers).astype(bool), np.int32)
        if inl.shape != (len(cam),):
            raise ValueError("inliers must hold one flag per point")
    cov_p, cov_T, valid = np.zeros(36), np.zeros(36), C.c_int(0)
    check(lib.svo_pose_covariance(device, ptr(K), len(cam), ptr(cam), ptr(world), ptr(inl), ptr(R), ptr(t), _lib.cov_mode(mode),
                                  float(pixel_sigma), ptr(cov_p), ptr(cov_T), C.byref(valid)))
    return cov_p.reshape(6, 6), cov_T.reshape(6, 6), bool(valid.value)


def last_stage_path():
    """svo_get_last_frame_path(NULL): the SVO_PATH_* bits of this thread's last triangulatePoints / cameraToWorld call."""
    return lib.svo_get_last_frame_path(None)


def getInverseTransform(rotation, translation, device=0):
    """vo.h:469-470"""
    R = np.ascontiguousarray(rotation, np.float64).reshape(9)
    t = np.ascontiguousarray(translation, np.float64).reshape(3)
    T = np.zeros(16)
    check(lib.svo_inverse_transform(device, ptr(R), ptr(t), ptr(T)))
    return T.reshape(4, 4)


def triangulatePoints(Pl, Pr, pts_l, pts_r, device=0):
    """cv::triangulatePoints + cv::convertPointsFromHomogeneous as used at vo.cpp:89-94 -> (N,3) f32."""
    Pl = np.ascontiguousarray(Pl, np.float32).reshape(12)
    Pr = np.ascontiguousarray(Pr, np.float32).reshape(12)
    a, b = _pts(pts_l), _pts(pts_r)
    xyz = np.zeros((len(a), 3), np.float32)
    check(lib.svo_triangulate(device, ptr(Pl), ptr(Pr), len(a), ptr(a), ptr(b), ptr(xyz)))
    return xyz


def buildOpticalFlowPyramid(image, win, max_level, device=0):
    """cv::buildOpticalFlowPyramid (vo.cpp:50,52,200,201) -> list of u8 level images."""
    img = u8img(image)
    h, w = img.shape
    cap = int(w * h * 1.5) + 64
    buf = np.zeros(cap, np.uint8)
    nl = C.c_int(0)
    check(lib.svo_build_pyramid(device, ptr(img), w, h, w, int(win), int(max_level), ptr(buf), C.c_int64(cap), C.byref(nl)))
    out, off = [], 0
    for _ in range(nl.value):
        out.append(buf[off:off + w * h].reshape(h, w).copy())
        off += w * h
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def calcOpticalFlowPyrLK(prev_img, next_img, prev_pts, win=10, max_level=3, max_count=30, epsilon=1e-4,
                         min_eig_threshold=OPTICAL_FLOW_MIN_EIG_THRESHOLD, device=0, guess=None):
    """cv::calcOpticalFlowPyrLK as called at vo.cpp:203-215 -> (next_pts, status).  guess: (N, 2) points where the top level's
    search starts (OPTFLOW_USE_INITIAL_FLOW, svo_lk_track_guess); None: at the points themselves (flags = 0)."""
    a, b = u8img(prev_img), u8img(next_img)
    h, w = a.shape
    p = _pts(prev_pts)
    out = np.zeros_like(p)
    st = np.zeros(len(p), np.uint8)
    if guess is None:
        check(lib.svo_lk_track(device, ptr(a), ptr(b), w, h, w, len(p), ptr(p), ptr(out), ptr(st), int(win), int(max_level),
                               int(max_count), C.c_double(epsilon), C.c_double(min_eig_threshold)))
        return out, st
    g = _pts(guess)
    if g.shape != p.shape:
        raise ValueError("guess must hold one point per tracked point")
    check(lib.svo_lk_track_guess(device, ptr(a), ptr(b), w, h, w, len(p), ptr(p), ptr(g), ptr(out), ptr(st), int(win), int(max_level),
                                 int(max_count), C.c_double(epsilon), C.c_double(min_eig_threshold)))
    return out, st


lk_track = calcOpticalFlowPyrLK


def _h9(M, what):
    m = np.ascontiguousarray(M, np.float32)
    if m.size != 9:
        raise ValueError("%s: a 3x3 matrix expected" % what)
    return m.reshape(9)


def motion_prior_from_rotation(Pl, R):
    """(H, Hi) = f32(K R K^-1), f32(K R^T K^-1) with K = Pl[:, :3] (svo_motion_prior_from_rotation; host only).  R rotates
    T0-camera coordinates into T1-camera coordinates."""
    pl = np.ascontiguousarray(Pl, np.float32).reshape(12)
    r = np.ascontiguousarray(R, np.float64).reshape(9)
    H, Hi = np.zeros(9, np.float32), np.zeros(9, np.float32)
    check(lib.svo_motion_prior_from_rotation(ptr(pl), ptr(r), ptr(H), ptr(Hi)))
    return H.reshape(3, 3), Hi.reshape(3, 3)


def circular_match_prior(cfg, l0, r0, l1, r1, points_left_t0, H, Hi=None, device=0):
    """circularMatching() with a motion prior (svo_circular_match_prior): the temporal passes start at pred(H, .) / pred(Hi, .);
    Hi = None lets the library invert H -> (pl1, pr1, pr0, pl0_circle, ok)."""
    imgs = [u8img(i) for i in (l0, r0, l1, r1)]
    h, w = imgs[0].shape
    p = _pts(points_left_t0)
    n = len(p)
    hm, him = _h9(H, "H"), (None if Hi is None else _h9(Hi, "Hi"))
    outs = [np.zeros((n, 2), np.float32) for _ in range(4)]
    ok = np.zeros(n, np.uint8)
    check(lib.svo_circular_match_prior(device, C.byref(cfg), ptr(imgs[0]), ptr(imgs[1]), ptr(imgs[2]), ptr(imgs[3]), w, h, w, n,
                                       ptr(p), ptr(hm), ptr(him), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(ok)))
    return outs[0], outs[1], outs[2], outs[3], ok


def circularMatching(cfg, l0, r0, l1, r1, points_left_t0, device=0):
    """The four LK passes + mask of VisualOdometry::circularMatching (vo.cpp:203-230) on four images,
    without the compaction -> (pl1, pr1, pr0, pl0_circle, ok)."""
    imgs = [u8img(i) for i in (l0, r0, l1, r1)]
    h, w = imgs[0].shape
    p = _pts(points_left_t0)
    n = len(p)
    outs = [np.zeros((n, 2), np.float32) for _ in range(4)]
    ok = np.zeros(n, np.uint8)
    check(lib.svo_circular_match(device, C.byref(cfg), ptr(imgs[0]), ptr(imgs[1]), ptr(imgs[2]), ptr(imgs[3]), w, h, w, n,
                                 ptr(p), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(ok)))
    return outs[0], outs[1], outs[2], outs[3], ok


# ---------------------------------------------------------------------------- rectification (svo.h)
def camera_info(info):
    """A ROS camera_info as svo_camera_info: a dict or any object with K (3x3), D (5 plumb_bob or 8 rational_polynomial
    coefficients, or empty), R (3x3), P (3x4), width, height (the raw image size)."""
    get = (lambda k: info[k]) if isinstance(info, dict) else (lambda k: getattr(info, k))
    ci = SvoCameraInfo()
    D = np.asarray(get("D"), np.float64).reshape(-1)
    if len(D) not in (0, 4, 5, 8):
        raise ValueError("D must hold 0, 4, 5 (plumb_bob) or 8 (rational_polynomial) coefficients")
    ci.K[:] = [float(v) for v in np.asarray(get("K"), np.float64).reshape(9)]
    ci.D[:len(D)] = [float(v) for v in D]
    ci.n_d = len(D)
    ci.R[:] = [float(v) for v in np.asarray(get("R"), np.float64).reshape(9)]
    ci.P[:] = [float(v) for v in np.asarray(get("P"), np.float64).reshape(12)]
    ci.width, ci.height = int(get("width")), int(get("height"))
    return ci


def init_rectify_map(K, D, R, P, width, height):
    """cv::initUndistortRectifyMap(K, D, R, P[:, :3], (width, height), CV_16SC2) on the host (svo_init_rectify_map) ->
    (map1 (height, width, 2) int16, map2 (height, width) uint16).  R / P may be None (identity / K)."""
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    D = np.ascontiguousarray(D if D is not None else [], np.float64).reshape(-1)
    R = None if R is None else np.ascontiguousarray(R, np.float64).reshape(9)
    P = None if P is None else np.ascontiguousarray(P, np.float64).reshape(12)
    m1 = np.zeros((height, width, 2), np.int16); m2 = np.zeros((height, width), np.uint16)
    check(lib.svo_init_rectify_map(ptr(K), ptr(D) if len(D) else None, len(D), ptr(R), ptr(P), int(width), int(height), ptr(m1), ptr(m2)))
    return m1, m2


def _maps(map1, map2):
    m1 = np.ascontiguousarray(map1, np.int16); m2 = np.ascontiguousarray(map2, np.uint16)
    if m1.ndim != 3 or m1.shape[2] != 2 or m2.shape != m1.shape[:2]:
        raise ValueError("map1 must be (h, w, 2) int16 and map2 (h, w) uint16")
    return m1, m2


def rectifyImage(raw, map1, map2, device=0):
    """cv::remap(raw, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) on the GPU (svo_rectify_image): the per-frame half of
    image_geometry::PinholeCameraModel::rectifyImage.  raw: (h, w) or (h, w, 3) uint8 -> the map's size, same channels."""
    img = u8frame(raw)
    m1, m2 = _maps(map1, map2)
    h, w = m2.shape
    cn = 3 if img.ndim == 3 else 1
    out = np.zeros((h, w, 3) if cn == 3 else (h, w), np.uint8)
    check(lib.svo_rectify_image(device, ptr(m1), ptr(m2), w, h, ptr(img), img.shape[1], img.shape[0], img.strides[0], cn, ptr(out)))
    return out


def convertGray(image, fmt, device=0):
    """cv::cvtColor(image, ..2GRAY) / cv_bridge's MONO8 conversion on the GPU (svo_convert_gray): the grey conversion of frame
    ingest alone.  image: (h, w, bpp) uint8 in the format `fmt` (an SVO_INPUT_* constant or a sensor_msgs encoding name; (h, w)
    for mono8); rows may be strided (a view's strides[0] is passed on) -> (h, w) uint8."""
    f = _lib.input_format(fmt)
    img = _strided_u8(image, f)
    h, w = img.shape[:2]
    out = np.zeros((h, w), np.uint8)
    check(lib.svo_convert_gray(device, f, C.c_void_p(img.ctypes.data), w, h, img.strides[0], ptr(out)))
    return out


def clahe(image, fmt="mono8", clip_limit=2.0, tiles=(8, 8), device=0):
    """cv::createCLAHE(clip_limit, tiles)->apply() of the grey image of `image` on the GPU (svo_clahe): the equalisation of frame
    ingest alone, on its two kernels.  image: (h, w, bpp) uint8 in the format `fmt` ((h, w) for mono8), rows may be strided ->
    (h, w) uint8.  ValueError for tiles outside 1 .. 16 or a non-finite clip_limit; SvoError when the tiles do not fit the image."""
    f = _lib.input_format(fmt)
    clip, tx, ty = _lib.check_clahe(clip_limit, tiles)
    img = _strided_u8(image, f)
    h, w = img.shape[:2]
    out = np.zeros((h, w), np.uint8)
    check(lib.svo_clahe(device, f, C.c_void_p(img.ctypes.data), w, h, img.strides[0], clip, tx, ty, ptr(out)))
    return out


def describe_points(image, xy, device=0):
    """The steered BRIEF-256 descriptors of the points xy ((n, 2) float32: x, y) of a grey image on the GPU (svo_describe_points):
    the descriptor output of the frame pipeline alone, on its device function.  image: (h, w) uint8, h, w >= 16, rows may be
    strided -> (desc (n, 32) uint8, bins (n,) int32).  Not cv::ORB's descriptors (svo.h, "Binary descriptors")."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("uint8 (h, w) image expected")
    if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img)
    p = _pts(xy)
    n = len(p)
    desc, bins = np.zeros((n, _lib.DESC_BYTES), np.uint8), np.zeros(n, np.int32)
    check(lib.svo_describe_points(device, C.c_void_p(img.ctypes.data), img.shape[1], img.shape[0], img.strides[0], n, ptr(p), ptr(desc), ptr(bins)))
    return desc, bins


def descriptor_pattern():
    """The descriptor's tables (svo_descriptor_pattern; no device needed) -> (pattern (256, 4) int8: ax, ay, bx, by per test,
    C (30,) int32, S (30,) int32)."""
    pat, cs = np.zeros((256, 4), np.int8), np.zeros(60, np.int32)
    check(lib.svo_descriptor_pattern(ptr(pat), ptr(cs)))
    return pat, cs[:30].copy(), cs[30:].copy()


RelocResult = collections.namedtuple("RelocResult", "success n_candidates n_inliers iters_run R t T")
AlignResult = collections.namedtuple("AlignResult", "success n_pairs n_inliers best_hypothesis best_count refit_rounds_run R t T rms")
FuseResult = collections.namedtuple("FuseResult", "n_pairs n_same n_fused n_rows_relabelled")
PlaceResult = collections.namedtuple("PlaceResult", "n_landmarks n_tags_voted n_places")
ConsolidateResult = collections.namedtuple("ConsolidateResult", "n_members n_groups n_dropped n_far_views n_capped_groups n_kept")


class DescriptorIndex:
    """A device-resident index of (descriptor, id) rows with an exact 2-nearest-neighbour Hamming search (svo.h, "Descriptor index"):
    the best row of a range, and the best row with ANOTHER id.  add and match are synchronous and wait for the index's own stream
    only: both are legal while a context has frames in flight."""

    def __init__(self, capacity, device=0, points=False):
        self._h = C.c_void_p()
        check(lib.svo_desc_index_create(int(device), int(capacity), C.byref(self._h)))
        self.capacity = int(capacity)
        if points:
            self.enable_points()

    def enable_points(self):
        """Give the rows 3-D points (svo.h, "Relocalisation"); legal only while the index is empty."""
        check(lib.svo_desc_index_enable_points(self._h))

    def add_points(self, desc, ids, xyz, tags=None):
        """add with a point per row: xyz (n, 3) float32 in the map frame, tags (n,) int32 >= 0 (None: all 0) -> the first row's number."""
        d = self._rows(desc, "desc")
        i = np.ascontiguousarray(ids).astype(np.uint64, copy=False).reshape(-1)
        p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        t = None if tags is None else np.ascontiguousarray(tags, np.int32).reshape(-1)
        if len(i) != len(d) or len(p) != len(d) or (t is not None and len(t) != len(d)):
            raise ValueError("one id, one point and one tag per descriptor row expected")
        first = C.c_int(0)
        check(lib.svo_desc_index_add_points(self._h, len(d), ptr(d), ptr(i), ptr(p), ptr(t), C.byref(first)))
        return first.value

    @staticmethod
    def _frame_handle(vo, what):
        """vo's context, once it has a frame"""
        return vo._need_frame(what, prefix="libsvo_hip status %d: " % _lib.SVO_ERR_STATE)

    def add_frame_points(self, vo, cam_to_map=None, tag=0, seq=0, need_flags=_lib.OBS_INLIER):
        """add_frame with each row's point moved into the map -> (first_row, n_added).  cam_to_map (4, 4) float64 is the pose of the
        PREVIOUS frame's left camera in the map (an observation row's xyz is in the T0 camera frame); None: the identity."""
        h = self._frame_handle(vo, "add_frame_points")
        T = None if cam_to_map is None else np.ascontiguousarray(cam_to_map, np.float64).reshape(16)
        first, n = C.c_int(0), C.c_int(0)
        check(lib.svo_desc_index_add_frame_points(self._h, h, int(seq), int(need_flags), ptr(T), int(tag), C.byref(first), C.byref(n)))
        return first.value, n.value

    @staticmethod
    def reloc_params(**over):
        """svo_reloc_params_default with fields replaced: row_lo, row_hi, max_dist, ratio_num, ratio_den, min_candidates,
        ransac_iterations, reproj_error, confidence"""
        p = _lib.SvoRelocParams()
        lib.svo_reloc_params_default(C.byref(p))
        for k, v in over.items():
            if not hasattr(p, k):
                raise AttributeError("svo_reloc_params has no field %r" % k)
            setattr(p, k, v)
        return p

    def _queries(self, query, xy):
        q = self._rows(query, "query")
        p = _pts(xy)
        if len(p) != len(q):
            raise ValueError("one pixel per query expected")
        return q, p

    def _select(self, query, xy, params, over, guide=None):
        """select's body; guide: None, or (K, R, t, radius) for the guided search"""
        q, p = self._queries(query, xy)
        prm = params if params is not None else self.reloc_params(**over)
        n = len(q)
        cq, cr = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        cxy, cxyz = np.zeros((max(n, 1), 2), np.float32), np.zeros((max(n, 1), 3), np.float32)
        k = C.c_int(0)
        tail = (n, ptr(q), ptr(p), C.byref(prm), C.byref(k), ptr(cq), ptr(cr), ptr(cxy), ptr(cxyz))
        if guide is None:
            check(lib.svo_desc_index_select(self._h, *tail))
        else:
            Kf, g = _K9(guide[0]), self.guide(*guide[1:])
            check(lib.svo_desc_index_select_guided(self._h, ptr(Kf), C.byref(g), *tail))
        k = k.value
        return dict(query=cq[:k].copy(), row=cr[:k].copy(), xy=cxy[:k].copy(), xyz=cxyz[:k].copy())

    def _localize(self, K, query, xy, rotation, translation, params, over, guide=None):
        """localize's body; rotation, translation: the extrinsic guess; guide: None, or (R, t, radius) for the guided search"""
        q, p = self._queries(query, xy)
        prm = params if params is not None else self.reloc_params(**over)
        Kf = _K9(K)
        res = _lib.SvoRelocResult()
        res.R[:] = list(np.asarray(rotation, np.float64).reshape(9))
        res.t[:] = list(np.asarray(translation, np.float64).reshape(3))
        n = len(q)
        cq, cr, ci = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        tail = (n, ptr(q), ptr(p), C.byref(prm), C.byref(res), ptr(cq), ptr(cr), ptr(ci))
        if guide is None:
            check(lib.svo_desc_index_localize(self._h, ptr(Kf), *tail))
        else:
            g = self.guide(*guide)
            check(lib.svo_desc_index_localize_guided(self._h, ptr(Kf), C.byref(g), *tail))
        k = res.n_candidates
        rec = RelocResult(bool(res.success), k, res.n_inliers, res.iters_run, np.array(res.R[:]).reshape(3, 3), np.array(res.t[:]).reshape(3, 1),
                          np.array(res.T[:]).reshape(4, 4))
        return rec, dict(query=cq[:k].copy(), row=cr[:k].copy(), inlier=ci[:k].astype(bool))

    def select(self, query, xy, params=None, **over):
        """The relocaliser's selection alone (svo_desc_index_select): query (n, 32) uint8, xy (n, 2) float32 -> a dict of the candidates'
        query (k,) int32, row (k,) int32, xy (k, 2) float32 and xyz (k, 3) float32, in increasing query."""
        return self._select(query, xy, params, over)

    def localize(self, K, query, xy, rotation=None, translation=None, params=None, **over):
        """Search, select and RANSAC-PnP in one call (svo_desc_index_localize) -> (RelocResult, candidates): the record holds success,
        n_candidates, n_inliers, iters_run, R (3, 3), t (3, 1) with x_cam = R X_map + t (the guess going in, unchanged without
        success) and T (4, 4), the camera in the map; candidates is a dict of query, row (k,) int32 and inlier (k,) bool."""
        return self._localize(K, query, xy, np.eye(3) if rotation is None else rotation, np.zeros(3) if translation is None else translation,
                              params, over)

    # ---- guided search (svo.h, "Guided search"): the same calls behind the projection gate of a pose prior
    @staticmethod
    def guide(R, t, radius):
        """svo_reloc_guide: the prior x_cam = R X_map + t (R (3, 3), t 3 values, float64) and the gate's radius in pixels"""
        g = _lib.SvoRelocGuide()
        g.R[:] = list(np.asarray(R, np.float64).reshape(9))
        g.t[:] = list(np.asarray(t, np.float64).reshape(3))
        g.radius = float(radius)
        return g

    def set_guided_sort(self, on=True):
        """tuning: serve a guided call's queries in image-cell order (the default) or in the caller's; the results do not depend on it"""
        check(lib.svo_desc_index_set_guided_sort(self._h, int(bool(on))))

    def project(self, K, R, t, row_lo=0, row_hi=-1):
        """The projections of the rows [row_lo, row_hi) with the prior (svo_desc_index_project) -> (m, 2) float32; an invisible row
        (no point, not in front of the camera, not finite in float32) is (+inf, +inf)."""
        hi = self.size if row_hi == -1 else int(row_hi)
        uv = np.zeros((max(hi - int(row_lo), 0), 2), np.float32)
        Kf, g = _K9(K), self.guide(R, t, 0.0)
        check(lib.svo_desc_index_project(self._h, ptr(Kf), C.byref(g), int(row_lo), int(row_hi), ptr(uv)))
        return uv

    def match_guided(self, K, R, t, radius, query, xy, row_lo=0, row_hi=-1):
        """match over the rows whose projection lies within radius pixels (per axis, inclusive) of the query's pixel
        (svo_desc_index_match_guided) -> the structured rows match returns"""
        q, p = self._queries(query, xy)
        out = np.zeros(len(q), _lib.DESC_MATCH_DTYPE)
        Kf, g = _K9(K), self.guide(R, t, radius)
        check(lib.svo_desc_index_match_guided(self._h, ptr(Kf), C.byref(g), len(q), ptr(q), ptr(p), int(row_lo), int(row_hi), ptr(out)))
        return out

    def select_guided(self, K, R, t, radius, query, xy, params=None, **over):
        """select over the guided search (svo_desc_index_select_guided) -> the dict select returns"""
        return self._select(query, xy, params, over, guide=(K, R, t, radius))

    def localize_guided(self, K, R, t, radius, query, xy, rotation=None, translation=None, params=None, **over):
        """localize over the guided search (svo_desc_index_localize_guided) -> what localize returns.  rotation, translation: the
        PnP's extrinsic guess; None: the guide's R, t, the usual choice."""
        return self._localize(K, query, xy, R if rotation is None else rotation, t if translation is None else translation, params, over,
                              guide=(R, t, radius))

    # ---- batched relocalisation (svo.h, "Batched relocalisation"): many cameras in one call
    def localize_batch(self, K, queries, xys, guides=None, rotations=None, translations=None, params=None, **over):
        """localize (guides None) or localize_guided for many cameras in one call (svo_desc_index_localize_batch) -> a list with, per
        camera, the (RelocResult, candidates) the single call returns, bit for bit.  K: (B, 3, 3) camera matrices, or one (3, 3) for
        all; queries, xys: per camera an (n_b, 32) uint8 and an (n_b, 2) float32 array; guides: per camera (R, t, radius); rotations,
        translations: per camera the PnP's extrinsic guess (None: the guide's R, t, or the identity and zero without guides)."""
        B = len(queries)
        if len(xys) != B or (guides is not None and len(guides) != B):
            raise ValueError("one pixel array and one guide per camera expected")
        Kf = np.ascontiguousarray(K, np.float32)
        Kf = np.ascontiguousarray(np.broadcast_to(Kf.reshape(-1, 9) if Kf.size != 9 else Kf.reshape(1, 9), (B, 9)))
        pairs = [self._queries(q, p) for q, p in zip(queries, xys)]
        begin = np.zeros(B + 1, np.int32)
        begin[1:] = np.cumsum([len(q) for q, _ in pairs])
        total = int(begin[-1])
        q = np.concatenate([a for a, _ in pairs]) if total else np.zeros((0, _lib.DESC_BYTES), np.uint8)
        p = np.concatenate([b for _, b in pairs]) if total else np.zeros((0, 2), np.float32)
        prm = params if params is not None else self.reloc_params(**over)
        g = None
        if guides is not None:
            g = (_lib.SvoRelocGuide * max(B, 1))()
            for b in range(B):
                g[b] = self.guide(*guides[b])
        res = (_lib.SvoRelocResult * max(B, 1))()
        for b in range(B):
            R0 = rotations[b] if rotations is not None else (guides[b][0] if guides is not None else np.eye(3))
            t0 = translations[b] if translations is not None else (guides[b][1] if guides is not None else np.zeros(3))
            res[b].R[:] = list(np.asarray(R0, np.float64).reshape(9))
            res[b].t[:] = list(np.asarray(t0, np.float64).reshape(3))
        cq, cr, ci = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.uint8)
        check(lib.svo_desc_index_localize_batch(self._h, B, ptr(Kf), g, ptr(begin), ptr(q), ptr(p), C.byref(prm), res, ptr(cq), ptr(cr), ptr(ci)))
        out = []
        for b in range(B):
            r, lo = res[b], int(begin[b])
            k = r.n_candidates
            rec = RelocResult(bool(r.success), k, r.n_inliers, r.iters_run, np.array(r.R[:]).reshape(3, 3), np.array(r.t[:]).reshape(3, 1),
                              np.array(r.T[:]).reshape(4, 4))
            out.append((rec, dict(query=cq[lo:lo + k].copy(), row=cr[lo:lo + k].copy(), inlier=ci[lo:lo + k].astype(bool))))
        return out

    def batch_order(self):
        """diagnostics (svo_desc_index_get_batch_order): the lane order of the last localize_batch as global query numbers, (total,) int32"""
        n = C.c_int(0)
        check(lib.svo_desc_index_get_batch_order(self._h, 0, None, C.byref(n)))
        order = np.zeros(max(n.value, 1), np.int32)
        check(lib.svo_desc_index_get_batch_order(self._h, n.value, ptr(order), C.byref(n)))
        return order[:n.value].copy()

    @staticmethod
    def _rows(desc, what):
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        if d.ndim != 2 or d.shape[1] != _lib.DESC_BYTES:
            raise ValueError("%s: an (n, %d) uint8 array expected" % (what, _lib.DESC_BYTES))
        return d

    def add(self, desc, ids):
        """Append rows: desc (n, 32) uint8, ids (n,) integers -> the row number of the first one.  All or none."""
        d = self._rows(desc, "desc")
        i = np.ascontiguousarray(ids).astype(np.uint64, copy=False).reshape(-1)
        if len(i) != len(d):
            raise ValueError("one id per descriptor row expected")
        first = C.c_int(0)
        check(lib.svo_desc_index_add(self._h, len(d), ptr(d), ptr(i), C.byref(first)))
        return first.value

    def add_frame(self, vo, seq=0, need_flags=_lib.OBS_INLIER):
        """Append the rows of sequence seq of vo's last collected frame whose flags contain need_flags -> (first_row, n_added)."""
        h = self._frame_handle(vo, "add_frame")
        first, n = C.c_int(0), C.c_int(0)
        check(lib.svo_desc_index_add_frame(self._h, h, int(seq), int(need_flags), C.byref(first), C.byref(n)))
        return first.value, n.value

    def match(self, query, row_lo=0, row_hi=-1):
        """query (n, 32) uint8 against the rows [row_lo, row_hi) (row_hi = -1: all) -> a structured array of n rows with the fields of
        svo_desc_match: id, id2, row, row2 (-1: none), dist, dist2 (257 with -1), reserved."""
        q = self._rows(query, "query")
        out = np.zeros(len(q), _lib.DESC_MATCH_DTYPE)
        check(lib.svo_desc_index_match(self._h, len(q), ptr(q), int(row_lo), int(row_hi), ptr(out)))
        return out

    @property
    def size(self):
        return check(lib.svo_desc_index_size(self._h))

    def truncate(self, n_rows):
        check(lib.svo_desc_index_truncate(self._h, int(n_rows)))

    @property
    def chunk_rows(self):
        """tuning: the rows of the index one block of the search walks; assign 0 for the default"""
        return check(lib.svo_desc_index_get_chunk_rows(self._h))

    @chunk_rows.setter
    def chunk_rows(self, rows):
        check(lib.svo_desc_index_set_chunk_rows(self._h, int(rows)))

    def set_timing(self, on=True):
        """diagnostics: record HIP events around the kernels of every later match (off by default)"""
        check(lib.svo_desc_index_set_timing(self._h, int(bool(on))))

    def stats(self):
        """diagnostics (svo_desc_index_get_stats) -> dict: last_kernels_ms (0 unless set_timing), scratch_allocations, scratch_bytes,
        scratch_bytes_outgrown"""
        st = _lib.SvoDescIndexStats()
        check(lib.svo_desc_index_get_stats(self._h, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in st._fields_}

    # ---- index maintenance (svo.h, "Index maintenance"): drop rows anywhere, move points, both on the device
    def retire(self, rows=(0, -1), tags=None, drop_ids=None, latest_per_id=False, scope=False, want_map=True):
        """Drop rows of the scope rows = (row_lo, row_hi) and close the gaps in place (svo_desc_index_retire): tags = (tag_lo, tag_hi)
        keeps the scope's rows whose tag is inside the inclusive window, drop_ids drops those whose id is listed, latest_per_id keeps
        per id only the newest of the survivors, scope drops the whole scope.  -> kept_before (size before + 1,) int32, the remapping
        of every stored row number (its last entry is the new size), or with want_map False the new size alone."""
        rule = _lib.SvoRetireRule()
        rule.row_lo, rule.row_hi = int(rows[0]), int(rows[1])
        ids = None
        if tags is not None:
            rule.flags |= _lib.RETIRE_BY_TAG
            rule.tag_lo, rule.tag_hi = int(tags[0]), int(tags[1])
        if drop_ids is not None:
            rule.flags |= _lib.RETIRE_BY_IDS
            ids = np.ascontiguousarray(drop_ids).astype(np.uint64, copy=False).reshape(-1)
            rule.n_ids, rule.ids = len(ids), (ids.ctypes.data if len(ids) else None)   # ids stays alive until the call returns
        if latest_per_id:
            rule.flags |= _lib.RETIRE_LATEST_PER_ID
        if scope:
            rule.flags |= _lib.RETIRE_SCOPE
        kept_before = np.zeros(self.size + 1, np.int32) if want_map else None
        n_kept = C.c_int(0)
        check(lib.svo_desc_index_retire(self._h, C.byref(rule), ptr(kept_before), C.byref(n_kept)))
        return kept_before if want_map else n_kept.value

    def transform_points(self, T, rows=(0, -1), tags=None):
        """Move the points of the rows of rows = (row_lo, row_hi) whose tag lies in tags = (tag_lo, tag_hi) (None: every row with a
        point) through T (4, 4) float64 (svo_desc_index_transform_points) -> (n_moved, n_skipped); a skipped row's result was not
        finite in float32 and the row is unchanged."""
        M = np.ascontiguousarray(T, np.float64).reshape(16)
        lo, hi = (0, np.iinfo(np.int32).max) if tags is None else (int(tags[0]), int(tags[1]))
        moved, skipped = C.c_int(0), C.c_int(0)
        check(lib.svo_desc_index_transform_points(self._h, ptr(M), int(rows[0]), int(rows[1]), lo, hi, C.byref(moved), C.byref(skipped)))
        return moved.value, skipped.value

    @property
    def retire_slab_rows(self):
        """tuning: the rows of one slab of retire's in-place compaction; assign 0 for the default"""
        return check(lib.svo_desc_index_get_retire_slab_rows(self._h))

    @retire_slab_rows.setter
    def retire_slab_rows(self, rows):
        check(lib.svo_desc_index_set_retire_slab_rows(self._h, int(rows)))

    def retire_stats(self):
        """diagnostics (svo_desc_index_get_retire_stats) -> dict: last_kernels_ms (0 unless set_timing), scratch_allocations,
        scratch_bytes, scratch_bytes_outgrown of the retire scratch"""
        st = _lib.SvoDescRetireStats()
        check(lib.svo_desc_index_get_retire_stats(self._h, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in st._fields_}

    # ---- map alignment (svo.h, "Map alignment"): the rigid transform between two row spans, found on the device
    @staticmethod
    def align_params(src, dst, inlier_dist, **over):
        """svo_align_params_default with the spans src = (lo, hi), dst = (lo, hi) and fields replaced: max_dist, ratio_num, ratio_den,
        min_pairs, hypotheses, refit_rounds.  inlier_dist has no default: none has been measured for any rig."""
        p = _lib.SvoAlignParams()
        lib.svo_align_params_default(C.byref(p), float(inlier_dist))
        p.src_lo, p.src_hi, p.dst_lo, p.dst_hi = int(src[0]), int(src[1]), int(dst[0]), int(dst[1])
        for k, v in over.items():
            if not hasattr(p, k):
                raise AttributeError("svo_align_params has no field %r" % k)
            setattr(p, k, v)
        return p

    def _span_rows(self, span):
        """the rows of a span as the library will resolve it (0 for one it will refuse)"""
        lo, hi, size = int(span[0]), int(span[1]), self.size
        return max(0, (size if hi == -1 or hi > size else hi) - lo) if lo >= 0 else 0

    def match_rows(self, src, dst):
        """match with the descriptors of the rows src = (lo, hi) as the queries, searched in the rows dst = (lo, hi), without a host
        copy of them (svo_desc_index_match_rows) -> match's structured array, one row per source row."""
        out = np.zeros(self._span_rows(src), _lib.DESC_MATCH_DTYPE)
        check(lib.svo_desc_index_match_rows(self._h, int(src[0]), int(src[1]), int(dst[0]), int(dst[1]), ptr(out)))
        return out

    def pair_rows(self, src, dst, inlier_dist=1.0, params=None, **over):
        """Rules 1 - 5 of "Map alignment" (svo_desc_index_pair_rows) -> (pair_src, pair_dst) int32 row numbers, one pair per landmark
        on either side, in increasing source row."""
        p = params if params is not None else self.align_params(src, dst, inlier_dist, **over)
        n = self._span_rows((p.src_lo, p.src_hi))
        ps, pd, k = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int(0)
        check(lib.svo_desc_index_pair_rows(self._h, C.byref(p), C.byref(k), ptr(ps), ptr(pd)))
        return ps[:k.value].copy(), pd[:k.value].copy()

    def align(self, src, dst, inlier_dist, params=None, **over):
        """The rigid transform x_dst = R x_src + t between the landmarks of the rows src and their matches in the rows dst
        (svo_desc_index_align) -> (AlignResult, pairs): pairs is a dict of src, dst (row numbers) and inlier (uint8) per pair.
        result.T is transform_points' argument for the source span."""
        p = params if params is not None else self.align_params(src, dst, inlier_dist, **over)
        n = self._span_rows((p.src_lo, p.src_hi))
        ps, pd, pi = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        r = _lib.SvoAlignResult()
        check(lib.svo_desc_index_align(self._h, C.byref(p), C.byref(r), ptr(ps), ptr(pd), ptr(pi)))
        k = r.n_pairs
        res = AlignResult(bool(r.success), k, r.n_inliers, r.best_hypothesis, r.best_count, r.refit_rounds_run,
                          np.array(r.R, np.float64).reshape(3, 3), np.array(r.t, np.float64), np.array(r.T, np.float64).reshape(4, 4), r.rms)
        return res, {"src": ps[:k].copy(), "dst": pd[:k].copy(), "inlier": pi[:k].copy()}

    # ---- landmark fusion (svo.h, "Landmark fusion"): one id per landmark where two spans of rows overlap, on the device
    @staticmethod
    def fuse_params(src, dst, radius, relabel=(0, -1), **over):
        """svo_fuse_params_default with the spans src, dst, relabel = (lo, hi) and fields replaced: max_dist, ratio_num, ratio_den.
        radius (the map's unit) has no default: none has been measured for any rig."""
        p = _lib.SvoFuseParams()
        lib.svo_fuse_params_default(C.byref(p), float(radius))
        p.src_lo, p.src_hi, p.dst_lo, p.dst_hi = int(src[0]), int(src[1]), int(dst[0]), int(dst[1])
        p.relabel_lo, p.relabel_hi = int(relabel[0]), int(relabel[1])
        for k, v in over.items():
            if not hasattr(p, k):
                raise AttributeError("svo_fuse_params has no field %r" % k)
            setattr(p, k, v)
        return p

    def match_near(self, src, dst, radius):
        """match_rows among the rows of dst whose point lies within radius of the source row's on every axis
        (svo_desc_index_match_near) -> match's structured array, one row per source row."""
        out = np.zeros(self._span_rows(src), _lib.DESC_MATCH_DTYPE)
        check(lib.svo_desc_index_match_near(self._h, int(src[0]), int(src[1]), int(dst[0]), int(dst[1]), float(radius), ptr(out)))
        return out

    def pair_near(self, src, dst, radius, params=None, **over):
        """Rules 1 - 3 of "Landmark fusion", the dry run of fuse (svo_desc_index_pair_near) -> (pair_src, pair_dst) int32 row numbers."""
        p = params if params is not None else self.fuse_params(src, dst, radius, **over)
        n = self._span_rows((p.src_lo, p.src_hi))
        ps, pd, k = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int(0)
        check(lib.svo_desc_index_pair_near(self._h, C.byref(p), C.byref(k), ptr(ps), ptr(pd)))
        return ps[:k.value].copy(), pd[:k.value].copy()

    def relabel(self, from_ids, to_ids, rows=(0, -1)):
        """Every row of rows = (row_lo, row_hi) whose id is from_ids[i] gets the id to_ids[i], in one simultaneous step
        (svo_desc_index_relabel); entries with from == to are ignored, of a repeated `from` the first entry wins -> the rows changed."""
        f = np.ascontiguousarray(from_ids).astype(np.uint64, copy=False).reshape(-1)
        t = np.ascontiguousarray(to_ids).astype(np.uint64, copy=False).reshape(-1)
        if len(f) != len(t):
            raise ValueError("one `to` id per `from` id expected")
        k = C.c_int(0)
        check(lib.svo_desc_index_relabel(self._h, len(f), ptr(f) if len(f) else None, ptr(t) if len(t) else None, int(rows[0]), int(rows[1]), C.byref(k)))
        return k.value

    def fuse(self, src, dst, radius, relabel=(0, -1), params=None, **over):
        """Give the landmarks of the rows src the ids of their partners in the rows dst, in the rows of relabel (svo_desc_index_fuse)
        -> (FuseResult, pairs): pairs is a dict of src and dst row numbers per pair."""
        p = params if params is not None else self.fuse_params(src, dst, radius, relabel, **over)
        n = self._span_rows((p.src_lo, p.src_hi))
        ps, pd = np.zeros(n, np.int32), np.zeros(n, np.int32)
        r = _lib.SvoFuseResult()
        check(lib.svo_desc_index_fuse(self._h, C.byref(p), C.byref(r), ptr(ps), ptr(pd)))
        return FuseResult(r.n_pairs, r.n_same, r.n_fused, r.n_rows_relabelled), {"src": ps[:r.n_pairs].copy(), "dst": pd[:r.n_pairs].copy()}

    # ---- place candidates (svo.h, "Place candidates"): which keyframes (tags) of the map a frame resembles, on the device
    @staticmethod
    def place_params(rows=(0, -1), tags=(0, _lib.PLACE_MAX_TAGS - 1), **over):
        """svo_place_params_default with the rows and the tags = (tag_lo, tag_hi) and fields replaced: max_dist, ratio_num, ratio_den,
        min_votes, separation, max_places"""
        p = _lib.SvoPlaceParams()
        lib.svo_place_params_default(C.byref(p))
        p.row_lo, p.row_hi, p.tag_lo, p.tag_hi = int(rows[0]), int(rows[1]), int(tags[0]), int(tags[1])
        for k, v in over.items():
            if not hasattr(p, k):
                raise AttributeError("svo_place_params has no field %r" % k)
            setattr(p, k, v)
        return p

    @staticmethod
    def _id_list(ids):
        return np.ascontiguousarray(ids).astype(np.uint64, copy=False).reshape(-1)

    def tag_votes(self, ids, rows=(0, -1), tags=(0, 0)):
        """Rule 2 of "Place candidates" with ids as the set M (svo_desc_index_tag_votes): per tag of tags = (tag_lo, tag_hi), over the
        rows of rows = (row_lo, row_hi) -> (votes, rows, row_first, row_end), four int32 arrays indexed tag - tag_lo."""
        i = self._id_list(ids)
        nb = max(0, min(int(tags[1]) - int(tags[0]) + 1, _lib.PLACE_MAX_TAGS)) if int(tags[0]) >= 0 else 0
        out = [np.zeros(max(nb, 1), np.int32) for _ in range(4)]
        check(lib.svo_desc_index_tag_votes(self._h, len(i), ptr(i) if len(i) else None, int(rows[0]), int(rows[1]), int(tags[0]), int(tags[1]),
                                           *(ptr(a) for a in out)))
        return tuple(a[:nb] for a in out)

    def places(self, query, rows=(0, -1), tags=(0, _lib.PLACE_MAX_TAGS - 1), min_votes=1, separation=0, max_places=8, params=None, **over):
        """The keyframes whose rows hold the most landmarks this frame recognises (svo_desc_index_places): query (n, 32) uint8 ->
        (PlaceResult, places, candidates): places is a structured array (tag, votes, rows, row_first, row_end) in rule 3's order,
        candidates a dict of the recognised landmarks' query and row, as select's."""
        q = self._rows(query, "query")
        p = params if params is not None else self.place_params(rows, tags, min_votes=min_votes, separation=separation, max_places=max_places, **over)
        n = len(q)
        res, out = _lib.SvoPlaceResult(), np.zeros(_lib.PLACE_MAX_PLACES, _lib.PLACE_DTYPE)
        cq, cr = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        check(lib.svo_desc_index_places(self._h, n, ptr(q) if n else None, C.byref(p), C.byref(res), ptr(out), ptr(cq), ptr(cr)))
        k = res.n_landmarks if n else 0
        return PlaceResult(res.n_landmarks, res.n_tags_voted, res.n_places), out[:res.n_places].copy(), dict(query=cq[:k].copy(), row=cr[:k].copy())

    def places_from_ids(self, ids, rows=(0, -1), tags=(0, _lib.PLACE_MAX_TAGS - 1), min_votes=1, separation=0, max_places=8, params=None, **over):
        """Rules 2 - 3 of "Place candidates" for landmarks known by id (svo_desc_index_places_from_ids): the keyframes that saw the
        landmarks a tracker holds -> (PlaceResult, places)."""
        i = self._id_list(ids)
        p = params if params is not None else self.place_params(rows, tags, min_votes=min_votes, separation=separation, max_places=max_places, **over)
        res, out = _lib.SvoPlaceResult(), np.zeros(_lib.PLACE_MAX_PLACES, _lib.PLACE_DTYPE)
        check(lib.svo_desc_index_places_from_ids(self._h, len(i), ptr(i) if len(i) else None, C.byref(p), C.byref(res), ptr(out)))
        return PlaceResult(res.n_landmarks, res.n_tags_voted, res.n_places), out[:res.n_places].copy()

    # ---- batched place candidates (svo.h, "Batched place candidates"): every camera's keyframe votes in one call
    @staticmethod
    def _slices(arrays, empty):
        """per-camera arrays -> (the offsets, (B + 1,) int32, and the arrays concatenated)"""
        begin = np.zeros(len(arrays) + 1, np.int32)
        begin[1:] = np.cumsum([len(a) for a in arrays])
        return begin, (np.concatenate(arrays) if int(begin[-1]) else empty)

    def tag_votes_batch(self, ids_list, rows=(0, -1), tags=(0, 0)):
        """tag_votes for many cameras in one call (svo_desc_index_tag_votes_batch): ids_list holds one id list per camera ->
        (votes, rows, row_first, row_end): votes is (B, b) int32, camera b's row what tag_votes returns for its list; the other
        three, (b,) int32 each, are the same for every camera."""
        B = len(ids_list)
        begin, i = self._slices([self._id_list(a) for a in ids_list], np.zeros(0, np.uint64))
        nb = max(0, min(int(tags[1]) - int(tags[0]) + 1, _lib.PLACE_MAX_TAGS)) if int(tags[0]) >= 0 else 0
        if B * nb > _lib.PLACE_BATCH_MAX_BINS:
            nb = 0                                     # a window the library refuses: room for nothing
        votes = np.zeros((B, nb) if B * nb else (1, 1), np.int32)
        out = [np.zeros(max(nb, 1), np.int32) for _ in range(3)]
        check(lib.svo_desc_index_tag_votes_batch(self._h, B, ptr(begin), ptr(i) if len(i) else None, int(rows[0]), int(rows[1]), int(tags[0]), int(tags[1]),
                                                 ptr(votes), *(ptr(a) for a in out)))
        return (votes if B * nb else np.zeros((B, nb), np.int32),) + tuple(a[:nb] for a in out)

    def _places_out(self, B, p):
        return (_lib.SvoPlaceResult * max(B, 1))(), np.zeros((max(B, 1), p.max_places if 1 <= p.max_places <= _lib.PLACE_MAX_PLACES else 1), _lib.PLACE_DTYPE)

    def places_from_ids_batch(self, ids_list, rows=(0, -1), tags=(0, _lib.PLACE_MAX_TAGS - 1), min_votes=1, separation=0, max_places=8, params=None, **over):
        """places_from_ids for many cameras in one call (svo_desc_index_places_from_ids_batch): ids_list holds one id list per camera
        -> a list with, per camera, the (PlaceResult, places) the single call returns, bit for bit."""
        B = len(ids_list)
        begin, i = self._slices([self._id_list(a) for a in ids_list], np.zeros(0, np.uint64))
        p = params if params is not None else self.place_params(rows, tags, min_votes=min_votes, separation=separation, max_places=max_places, **over)
        res, out = self._places_out(B, p)
        check(lib.svo_desc_index_places_from_ids_batch(self._h, B, ptr(begin), ptr(i) if len(i) else None, C.byref(p), res, ptr(out)))
        return [(PlaceResult(res[b].n_landmarks, res[b].n_tags_voted, res[b].n_places), out[b, :res[b].n_places].copy()) for b in range(B)]

    def places_batch(self, queries, rows=(0, -1), tags=(0, _lib.PLACE_MAX_TAGS - 1), min_votes=1, separation=0, max_places=8, params=None, **over):
        """places for many cameras in one call (svo_desc_index_places_batch): queries holds one (n_b, 32) uint8 array per camera -> a
        list with, per camera, the (PlaceResult, places, candidates) the single call returns, bit for bit; candidates' query numbers
        count inside the camera's own array."""
        B = len(queries)
        begin, q = self._slices([self._rows(a, "query") for a in queries], np.zeros((0, _lib.DESC_BYTES), np.uint8))
        p = params if params is not None else self.place_params(rows, tags, min_votes=min_votes, separation=separation, max_places=max_places, **over)
        res, out = self._places_out(B, p)
        total = int(begin[-1])
        cq, cr = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32)
        check(lib.svo_desc_index_places_batch(self._h, B, ptr(begin), ptr(q) if total else None, C.byref(p), res, ptr(out), ptr(cq), ptr(cr)))
        ret = []
        for b in range(B):
            lo = int(begin[b])
            k = res[b].n_landmarks if begin[b + 1] > lo else 0
            ret.append((PlaceResult(res[b].n_landmarks, res[b].n_tags_voted, res[b].n_places), out[b, :res[b].n_places].copy(),
                        dict(query=cq[lo:lo + k].copy(), row=cr[lo:lo + k].copy())))
        return ret

    def set_place_combine(self, on=True):
        """diagnostics: one set of atomics per run of equal tags in a wave (the default) or four per row; the results do not depend on it"""
        check(lib.svo_desc_index_set_place_combine(self._h, int(bool(on))))

    # ---- landmark consolidation (svo.h, "Landmark consolidation"): one row per landmark, and the rows read back
    @staticmethod
    def consolidate_params(radius, rows=(0, -1), tags=None):
        """svo_consolidate_params_default with the scope rows = (row_lo, row_hi) and the window tags = (tag_lo, tag_hi) (None: every
        tag).  radius (the map's unit) has no default: none has been measured for any rig."""
        p = _lib.SvoConsolidateParams()
        lib.svo_consolidate_params_default(C.byref(p), float(radius))
        p.row_lo, p.row_hi = int(rows[0]), int(rows[1])
        if tags is not None:
            p.tag_lo, p.tag_hi = int(tags[0]), int(tags[1])
        return p

    def consolidate(self, radius, rows=(0, -1), tags=None, want_map=True, params=None):
        """Leave one row per landmark among the rows of rows = (row_lo, row_hi) whose tag lies in tags: the group's latest row with the
        medoid descriptor and the mean of the points within radius of the medoid's (svo_desc_index_consolidate) ->
        (ConsolidateResult, kept_before): kept_before is retire's remapping, (size before + 1,) int32, or None with want_map False."""
        p = params if params is not None else self.consolidate_params(radius, rows, tags)
        kept_before = np.zeros(self.size + 1, np.int32) if want_map else None
        r = _lib.SvoConsolidateResult()
        check(lib.svo_desc_index_consolidate(self._h, C.byref(p), C.byref(r), ptr(kept_before)))
        return ConsolidateResult(r.n_members, r.n_groups, r.n_dropped, r.n_far_views, r.n_capped_groups, r.n_kept), kept_before

    def read_rows(self, rows=(0, -1), want=("desc", "ids", "xyz", "tags")):
        """The rows of rows = (row_lo, row_hi) back on the host (svo_desc_index_read_rows) -> (desc (m, 32) uint8, ids (m,) uint64,
        xyz (m, 3) float32, tags (m,) int32); a row without a point reads xyz = +inf and tag = -1.  An output not named in want is
        not read and is None."""
        m = self._span_rows(rows)
        out = dict(desc=np.zeros((m, _lib.DESC_BYTES), np.uint8), ids=np.zeros(m, np.uint64), xyz=np.zeros((m, 3), np.float32),
                   tags=np.zeros(m, np.int32))
        got = [out[k] if k in want else None for k in ("desc", "ids", "xyz", "tags")]
        check(lib.svo_desc_index_read_rows(self._h, int(rows[0]), int(rows[1]), *(ptr(a) for a in got)))
        return tuple(got)

    # ---- batched insertion (svo.h, "Batched insertion"): many sequences' frames, or the caller's own rows, in one call
    @staticmethod
    def _insert_args(n, id_base, cam_to_map, tags):
        """the per-entry arrays of a batched insertion, each None or n entries long"""
        base = None if id_base is None else np.ascontiguousarray(id_base).astype(np.uint64, copy=False).reshape(-1)
        T = None if cam_to_map is None else np.ascontiguousarray(cam_to_map, np.float64).reshape(-1, 16)
        t = None if tags is None else np.ascontiguousarray(tags, np.int32).reshape(-1)
        for a, what in ((base, "id_base"), (T, "cam_to_map"), (t, "tags")):
            if a is not None and len(a) != n:
                raise ValueError("%s: one per entry expected (%d, got %d)" % (what, n, len(a)))
        return base, T, t

    def _add_frames(self, vo, points, seqs, need_flags, id_base, cam_to_map, tags):
        h = self._frame_handle(vo, "add_frames_points" if points else "add_frames")
        s = None if seqs is None else np.ascontiguousarray(seqs, np.int32).reshape(-1)
        n = len(s) if s is not None else int(vo.n_seq)
        base, T, t = self._insert_args(n, id_base, cam_to_map, tags)
        first, added = np.zeros(n, np.int32), np.zeros(n, np.int32)
        if points:
            check(lib.svo_desc_index_add_frames_points(self._h, h, n, ptr(s), int(need_flags), ptr(base), ptr(T), ptr(t), ptr(first), ptr(added)))
        else:
            check(lib.svo_desc_index_add_frames(self._h, h, n, ptr(s), int(need_flags), ptr(base), ptr(first), ptr(added)))
        return first, added

    def add_frames(self, vo, seqs=None, need_flags=_lib.OBS_INLIER, id_base=None):
        """add_frame for many sequences of vo's last collected frame in one call, filtered and packed on the device
        (svo_desc_index_add_frames) -> (first_row, n_added), (n,) int32 each.  seqs: the entries' sequences (None: every sequence of
        vo, in order); id_base (n,) uint64: added to entry b's track ids modulo 2**64 (None: zeros) — seq << 48 keeps the
        sequences' ids apart."""
        return self._add_frames(vo, False, seqs, need_flags, id_base, None, None)

    def add_frames_points(self, vo, cam_to_map=None, tags=None, seqs=None, need_flags=_lib.OBS_INLIER, id_base=None):
        """add_frames with each row's point moved into the map through its entry's cam_to_map ((n, 4, 4) float64; None: as it is)
        and tagged tags[b] >= 0 (None: zeros) -> (first_row, n_added)."""
        return self._add_frames(vo, True, seqs, need_flags, id_base, cam_to_map, tags)

    def add_obs(self, obs_list, desc_list, need_flags=_lib.OBS_INLIER, id_base=None, with_points=False, cam_to_map=None, tags=None):
        """The same stage on the caller's own rows (svo_desc_index_add_obs): entry b is obs_list[b] (TRACK_OBS_DTYPE rows) with
        desc_list[b] ((rows, 32) uint8) -> (first_row, n_added)."""
        n = len(obs_list)
        if len(desc_list) != n:
            raise ValueError("one descriptor block per observation block expected")
        obs = [np.ascontiguousarray(o, _lib.TRACK_OBS_DTYPE).reshape(-1) for o in obs_list]
        desc = [self._rows(d, "desc") if len(d) else np.zeros((0, _lib.DESC_BYTES), np.uint8) for d in desc_list]
        if any(len(o) != len(d) for o, d in zip(obs, desc)):
            raise ValueError("one descriptor row per observation row expected")
        begin = np.zeros(n + 1, np.int64)
        begin[1:] = np.cumsum([len(o) for o in obs])
        if begin[-1] >= 1 << 31:
            raise ValueError("too many rows")
        all_obs = np.concatenate(obs) if n else np.zeros(0, _lib.TRACK_OBS_DTYPE)
        all_desc = np.ascontiguousarray(np.concatenate(desc)) if n else np.zeros((0, _lib.DESC_BYTES), np.uint8)
        base, T, t = self._insert_args(n, id_base, cam_to_map, tags)
        first, added = np.zeros(n, np.int32), np.zeros(n, np.int32)
        begin32 = begin.astype(np.int32)
        check(lib.svo_desc_index_add_obs(self._h, n, ptr(begin32), ptr(all_obs), ptr(all_desc), int(need_flags), ptr(base),
                                         int(bool(with_points)), ptr(T), ptr(t), ptr(first), ptr(added)))
        return first, added

    def insert_stats(self):
        """diagnostics of the last batched insertion (svo_desc_index_get_insert_stats) -> dict: last_kernels_ms (0 unless
        set_timing), last_path (INSERT_PATH_*), rows_scanned, rows_added"""
        st = _lib.SvoDescInsertStats()
        check(lib.svo_desc_index_get_insert_stats(self._h, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in st._fields_}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib.svo_desc_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


# ---------------------------------------------------------------------------- FeatureSet / Bucket
class FeatureSet:
    """vo.h:132-188 — parallel arrays points / ages / strengths."""

    def __init__(self, device=0):
        self.points = np.zeros((0, 2), np.float32)
        self.ages = np.zeros(0, np.int32)
        self.strengths = np.zeros(0, np.int32)
        self.device = device

    def size(self):
        return len(self.points)

    def clear(self):
        self.__init__(self.device)

    def filterByBucketLocationInternal(self, image, buckets_along_height, buckets_along_width, bucket_start_row,
                                       features_per_bucket):
        h, w = np.asarray(image).shape[:2]
        xy = np.ascontiguousarray(self.points, np.float32).reshape(-1, 2).copy()
        ages = np.ascontiguousarray(self.ages, np.int32).copy()
        st = np.ascontiguousarray(self.strengths, np.int32).copy()
        n = C.c_int(len(ages))
        check(lib.svo_bucket_filter(self.device, w, h, C.byref(n), ptr(xy), ptr(ages), ptr(st), buckets_along_height,
                                    buckets_along_width, bucket_start_row, features_per_bucket, AGE_THRESHOLD, FAST_THRESHOLD))
        self.points, self.ages, self.strengths = xy[:n.value].copy(), ages[:n.value].copy(), st[:n.value].copy()

    def filterByBucketLocation(self, image):
        self.filterByBucketLocationInternal(image, BUCKETS_ALONG_HEIGHT, BUCKETS_ALONG_WIDTH, BUCKET_START_ROW, FEATURES_PER_BUCKET)

    def appendFeaturesFromImage(self, image, fast_threshold, cfg=None, mask=None):
        """vo.h:186-187 — FAST + append (age 0) + default-grid bucket filter, fused on the GPU.  mask: an (H, W) uint8 detection
        mask over the whole list, the set's own features included (svo.h)."""
        img = u8img(image)
        h, w = img.shape
        m = _host_mask(mask, h, w) if mask is not None else None
        cfg = cfg if cfg is not None else default_config()
        rows = max(cfg.buckets_along_height - cfg.bucket_start_row, 0)
        cap = max(rows * cfg.buckets_along_width, 64, self.size())
        xy = np.zeros((cap, 2), np.float32); ages = np.zeros(cap, np.int32); st = np.zeros(cap, np.int32)
        n0 = self.size()
        xy[:n0], ages[:n0], st[:n0] = self.points, self.ages, self.strengths
        n = C.c_int(n0)
        if m is not None:
            check(lib.svo_append_features_from_image_masked(self.device, C.byref(cfg), ptr(img), w, h, w, int(fast_threshold), ptr(m), w, cap,
                                                            C.byref(n), ptr(xy), ptr(ages), ptr(st)))
        else:
            check(lib.svo_append_features_from_image(self.device, C.byref(cfg), ptr(img), w, h, w, int(fast_threshold), cap,
                                                     C.byref(n), ptr(xy), ptr(ages), ptr(st)))
        self.points, self.ages, self.strengths = xy[:n.value].copy(), ages[:n.value].copy(), st[:n.value].copy()


class Bucket:
    """vo.h:195-229.  add_feature applies the insertion rule (feature_set.cpp:20-53) on the GPU: the bucket's current content, in
    slot order, followed by the new feature goes through a 1x1 grid of capacity max_size — the stored features refill their
    slots in the same order, then the new one meets exactly the state the reference's bucket is in (at most max_size + 1
    inputs per insertion)."""

    def __init__(self, max_size, device=0):
        self.max_size = max_size
        self.device = device
        self.features = FeatureSet(device)

    def compute_score(self, age, strength):
        q = abs(strength - FAST_THRESHOLD) // 20
        return age + (q if strength >= FAST_THRESHOLD else -q)       # C++ int division truncates toward zero

    def add_feature(self, point, age, strength):
        if not self.max_size:
            return
        fs = self.features
        fs.points = np.concatenate([np.asarray(fs.points, np.float32).reshape(-1, 2), np.array([[point[0], point[1]]], np.float32)])
        fs.ages = np.concatenate([fs.ages, np.array([age], np.int32)]); fs.strengths = np.concatenate([fs.strengths, np.array([strength], np.int32)])
        side = int(max(2, np.ceil(fs.points.max()) + 1))
        fs.filterByBucketLocationInternal(np.zeros((side, side), np.uint8), 1, 1, 0, self.max_size)

    def size(self):
        return self.features.size()


class PinnedImage:
    """An (H, W) or (H, W, 3) uint8 numpy array living in page-locked host memory (svo_alloc_pinned): frames kept in such
    buffers are read by the DMA engines in place instead of being copied to a staging buffer first (include/svo.h)."""

    def __init__(self, shape):
        self._n = int(np.prod(shape))
        self._p = lib.svo_alloc_pinned(self._n)
        if not self._p:
            raise MemoryError("svo_alloc_pinned(%d)" % self._n)
        self.array = np.ctypeslib.as_array((C.c_uint8 * self._n).from_address(self._p)).reshape(shape)

    def __del__(self):
        try:
            if self._p:
                lib.svo_free_pinned(self._p); self._p = None
        except Exception:
            pass


# ---------------------------------------------------------------------------- VisualOdometry
class BatchVisualOdometry:
    """n_seq independent VisualOdometry instances advancing in lock-step on one GPU."""

    def __init__(self, width, height, n_seq=1, cfg=None, device=0):
        self.cfg = cfg if cfg is not None else default_config()
        self.n_seq, self.width, self.height, self.device = n_seq, width, height, device
        self._h = C.c_void_p()
        check(lib.svo_create(C.byref(self.cfg), device, n_seq, width, height, C.byref(self._h)))
        self.stats = None
        self.raw_size = None                          # (raw_w, raw_h) while the context rectifies: frames are then raw
        self.input_format = _lib.INPUT_MONO8          # svo_set_input_format: what the bytes of the caller's frames are

    def _has_context(self):
        """False for a VisualOdometry before its first frame, and for a closed object"""
        return bool(self._h.value)

    def _need_frame(self, what, exc=_lib.SvoError, prefix=""):
        """The context; without one, the error of a call that reads a frame's results"""
        if not self._has_context():
            raise exc("%s%s: no frame yet (call stereo_callback first)" % (prefix, what))
        return self._h

    def _last_rows(self, getter, seq, row_shape, dtype):
        """The rows of sequence seq in the last collected frame through a (ctx, seq, cap, rows, n_tracks) getter: sized by a first
        call, filled by a second -> (rows, n_tracks)."""
        n_tracks = C.c_int(0)
        check(getter(self._h, seq, 0, None, C.byref(n_tracks)))
        rows = np.zeros((max(n_tracks.value, 1),) + row_shape, dtype)
        n = check(getter(self._h, seq, len(rows), ptr(rows), None))
        return rows[:n].copy(), n_tracks.value

    def _in_shape(self):
        """(height, width) of the frames the caller passes: the raw size when rectifying."""
        return (self.raw_size[1], self.raw_size[0]) if self.raw_size else (self.height, self.width)

    def _bpp(self):
        """Bytes per pixel of the frames the caller passes: the channels of a BGR context, else the input format's."""
        return 3 if self.cfg.channels == 3 else _lib.INPUT_BPP[self.input_format]

    def _frame_shape(self):
        bpp = self._bpp()
        return self._in_shape() + ((bpp,) if bpp > 1 else ())

    def _frame(self, img):
        return u8frame(img, None if self.cfg.channels == 3 else self._bpp())

    def set_input_format(self, fmt):
        """The format of the frames passed from now on (svo_set_input_format): an SVO_INPUT_* constant (_lib.INPUT_*) or a
        sensor_msgs encoding name — "mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422" (UYVY), "yuv422_yuy2".  Frames are then
        (H, W, bytes per pixel) arrays; the conversion to grey happens inside frame ingest, before rectification.  Single-channel
        contexts only.  Stream-ordered: legal with frames in flight, from the next frame submitted."""
        f = _lib.input_format(fmt)
        check(lib.svo_set_input_format(self._h, f))
        self.input_format = f

    def set_clahe(self, clip_limit=2.0, tiles=(8, 8)):
        """Equalise both images of every frame submitted from now on (svo_set_clahe): cv::createCLAHE(clip_limit, tiles)->apply()
        of the grey frame, after the input-format conversion and before rectification.  tiles = (tiles_x, tiles_y), each 1 .. 16.
        Single-channel contexts only.  Legal with frames in flight: every frame carries the setting it was issued with.
        ValueError for bad tiles or a non-finite clip_limit; SvoError when the tiles do not fit the frame size."""
        clip, tx, ty = _lib.check_clahe(clip_limit, tiles)
        check(lib.svo_set_clahe(self._h, 1, clip, tx, ty))

    def clear_clahe(self):
        """Frames submitted from now on are not equalised: the context launches what it launched before set_clahe."""
        check(lib.svo_set_clahe(self._h, 0, 0.0, 0, 0))

    def set_pose_covariance(self, mode="residual", pixel_sigma=1.0):
        """A 6x6 covariance with every pose from the next frame submitted on (svo_set_pose_covariance).  mode: "residual" (sigma^2
        from the frame's own reprojection residuals), "fixed" (sigma = pixel_sigma pixels), "off", or an SVO_COV_* constant.
        Legal with frames in flight: every frame carries the mode it was issued with.  Read with last_pose_covariance()."""
        check(lib.svo_set_pose_covariance(self._h, _lib.cov_mode(mode), float(pixel_sigma)))

    def last_pose_covariance(self):
        """Of the last collected frame -> (cov_T (n_seq, 6, 6), cov_p (n_seq, 6, 6), valid (n_seq,) bool).  cov_T: the returned T,
        in the order (position, rotation) of a ROS pose covariance; cov_p: the cameraToWorld parameters (r, t).  Rows without a pose
        (failed frames, idle sequences) are zero with valid False.  SvoError when that frame was issued with the mode off."""
        cov_T, cov_p = np.zeros((self.n_seq, 36)), np.zeros((self.n_seq, 36))
        valid = np.zeros(self.n_seq, np.int32)
        check(lib.svo_get_last_pose_covariance(self._h, ptr(cov_T), ptr(cov_p), ptr(valid)))
        return cov_T.reshape(-1, 6, 6), cov_p.reshape(-1, 6, 6), valid.astype(bool)

    def set_track_output(self, max_rows):
        """Persistent feature ids and per-frame stereo observations from the next frame submitted on (svo_set_track_output):
        every frame then leaves up to max_rows rows (id, the track's four points, its triangulated point, age, flags) per
        sequence in a pinned ring beside the pose; read them with last_track_obs().  The features held now get fresh ids.
        A setup action: SvoError with frames in flight, with features_per_bucket > 1, or for a bad max_rows."""
        check(lib.svo_set_track_output(self._h, 1, int(max_rows)))

    def clear_track_output(self):
        """Frames submitted from now on carry no ids: the context launches what it launched before set_track_output."""
        check(lib.svo_set_track_output(self._h, 0, 0))

    def last_track_obs(self, seq=0, with_count=False):
        """The observation rows of sequence `seq` in the last collected frame -> a numpy structured array (_lib.TRACK_OBS_DTYPE:
        id, l0, r0, l1, r1, xyz, age, flags, pad), the first min(n_tracks, max_rows) tracks in svo_get_last_tracks' order.
        with_count: -> (rows, n_tracks), the frame's full track count.  Host memory only, no synchronisation
        (svo_get_last_track_obs).  SvoError when that frame was issued with the output off."""
        rows, n_tracks = self._last_rows(lib.svo_get_last_track_obs, seq, (), _lib.TRACK_OBS_DTYPE)
        return (rows, n_tracks) if with_count else rows

    def set_descriptor_output(self, on=True):
        """A 32-byte steered BRIEF descriptor beside every observation row, from the next frame submitted on
        (svo_set_descriptor_output); needs the track output, and goes off with it.  SvoError with frames in flight, with the track
        output off, or on a channels = 3 context."""
        check(lib.svo_set_descriptor_output(self._h, 1 if on else 0))

    def last_track_descriptors(self, seq=0):
        """The descriptor rows of sequence seq in the last collected frame -> (n, 32) uint8: row i describes row i of
        last_track_obs(seq).  Host memory only, no synchronisation (svo_get_last_track_descriptors).  SvoError when that frame was
        issued with descriptors off."""
        return self._last_rows(lib.svo_get_last_track_descriptors, seq, (_lib.DESC_BYTES,), np.uint8)[0]

    def feature_ids(self, seq=0):
        """The ids of features(seq)'s entries, in its order (svo_get_feature_ids; synchronises).  SvoError with the output off."""
        cap = 1 << 15
        ids = np.zeros(cap, np.int64)
        n = check(lib.svo_get_feature_ids(self._h, seq, cap, ptr(ids)))
        return ids[:n].copy()

    def set_motion_prior(self, H, Hi=None, seq=-1):
        """Seed the temporal LK passes of the next frame sequence `seq` (-1: every sequence) takes (svo_set_motion_prior): H, a 3x3
        homography, maps pixels of the sequence's previous frame to predicted pixels of the frame submitted next; Hi is its
        inverse (None: the library inverts H).  One-shot: consumed by that frame.  H = None clears a pending prior.  Legal with
        frames in flight.  SvoError for a BGR or float-sums context, a non-finite entry, a singular H."""
        if H is None:
            check(lib.svo_set_motion_prior(self._h, seq, None, None))
            return
        hm, him = _h9(H, "H"), (None if Hi is None else _h9(Hi, "Hi"))
        check(lib.svo_set_motion_prior(self._h, seq, ptr(hm), ptr(him)))

    def set_motion_priors(self, Hs, has=None, His=None):
        """One prior per sequence in one call (svo_set_motion_priors): Hs (n_seq, 3, 3); has: n_seq flags, a false one clears that
        sequence's pending prior (None: every sequence gets its row); His: the inverses (None: inverted by the library)."""
        hs = np.ascontiguousarray(Hs, np.float32)
        if hs.size != 9 * self.n_seq:
            raise ValueError("Hs must hold n_seq = %d 3x3 matrices" % self.n_seq)
        his = None
        if His is not None:
            his = np.ascontiguousarray(His, np.float32)
            if his.size != 9 * self.n_seq:
                raise ValueError("His must hold n_seq = %d 3x3 matrices" % self.n_seq)
        check(lib.svo_set_motion_priors(self._h, ptr(hs), ptr(his), ptr(self._active(has))))

    def set_rotation_prior(self, R, seq=-1, Pl=None):
        """set_motion_prior with the homography of a pure rotation: R (3x3) rotates T0-camera coordinates into T1-camera
        coordinates (a gyro's integrated increment moved into the camera frame).  Pl: the left projection matrix (K = Pl[:, :3]);
        None: the one last passed to initalize_projection_matricies."""
        Pl = Pl if Pl is not None else getattr(self, "_Pl", None)
        if Pl is None:
            raise ValueError("set_rotation_prior: no projection matrix yet (initalize_projection_matricies, or pass Pl)")
        H, Hi = motion_prior_from_rotation(Pl, R)
        self.set_motion_prior(H, Hi, seq)

    def motion_prior(self, seq=0):
        """The prior the next frame of sequence `seq` will use -> (H, Hi) as 3x3 float32 arrays, or None (svo_get_motion_prior;
        host side only)."""
        H, Hi = np.zeros(9, np.float32), np.zeros(9, np.float32)
        pending = C.c_int(0)
        check(lib.svo_get_motion_prior(self._h, seq, ptr(H), ptr(Hi), C.byref(pending)))
        return (H.reshape(3, 3), Hi.reshape(3, 3)) if pending.value else None

    def set_motion_prior_mode(self, mode):
        """"last_rotation": every sequence without an explicit prior for a frame gets one predicted on the device from its own last
        pose (svo_set_motion_prior_mode, SVO_PRIOR_LAST_ROTATION; svo.h has the rule) — the prior for callers without a gyro, and
        the one that works with frames in flight.  "explicit" (the default): only what the setters give.  In force from the next
        submit.  SvoError for a BGR or float-sums context."""
        if mode not in _lib.PRIOR_MODES:
            raise ValueError("motion prior mode: one of %s expected" % sorted(_lib.PRIOR_MODES))
        check(lib.svo_set_motion_prior_mode(self._h, _lib.PRIOR_MODES[mode]))

    def motion_prior_mode(self):
        m = C.c_int(0)
        check(lib.svo_get_motion_prior_mode(self._h, C.byref(m)))
        return {v: k for k, v in _lib.PRIOR_MODES.items()}[m.value]

    def last_motion_prior(self, seq=0):
        """The prior the frame last collected used for sequence `seq` (svo_get_last_motion_prior) -> (H, Hi, source) with source 1
        an explicit prior, 2 a predicted one; None when it used none."""
        H, Hi = np.zeros(9, np.float32), np.zeros(9, np.float32)
        src = C.c_int(0)
        check(lib.svo_get_last_motion_prior(self._h, seq, ptr(H), ptr(Hi), C.byref(src)))
        return (H.reshape(3, 3), Hi.reshape(3, 3), src.value) if src.value else None

    def set_detection_mask(self, mask, seq=-1):
        """Keep features off the zero pixels of `mask` (svo_set_detection_mask): an (height, width) uint8 numpy array, or a torch
        device tensor of that shape and dtype, read through data_ptr() with its own row stride (its producer must have finished,
        or run on stream()).  seq = -1: the shared mask; a sequence's own mask overrides it.  The mask describes the left image of
        the frames submitted from now on and is applied when that image is scanned, in the following call.  mask = None clears.
        Legal with frames in flight.  ValueError for a wrong shape or dtype."""
        if mask is None:
            check(lib.svo_set_detection_mask(self._h, seq, None, 0, 0))
            return
        if hasattr(mask, "data_ptr"):                                 # a torch tensor
            if tuple(mask.shape) != (self.height, self.width) or "uint8" not in str(mask.dtype) or mask.stride(1) != 1:
                raise ValueError("detection mask: (%d, %d) uint8 with unit column stride expected, got %s %s"
                                 % (self.height, self.width, tuple(mask.shape), mask.dtype))
            if mask.is_cuda:
                check(lib.svo_set_detection_mask(self._h, seq, C.c_void_p(mask.data_ptr()), int(mask.stride(0)), 1))
                return
            mask = mask.numpy()
        m = _host_mask(mask, self.height, self.width)
        check(lib.svo_set_detection_mask(self._h, seq, ptr(m), self.width, 0))

    def clear_detection_mask(self, seq=-1):
        """No mask from the next frame submitted on (seq = -1: none at all).  The next call still applies the mask of the image it scans."""
        check(lib.svo_set_detection_mask(self._h, seq, None, 0, 0))

    def detection_mask(self, seq=-1):
        """The mask in force for the frames submitted next: seq's own, else the shared one -> (height, width) uint8, or None."""
        out = np.zeros((self.height, self.width), np.uint8)
        present = C.c_int(0)
        check(lib.svo_get_detection_mask(self._h, seq, ptr(out), C.byref(present)))
        return out if present.value else None

    def set_rectification(self, left_info, right_info, seq=-1):
        """Rectify raw frames with these calibrations (svo_set_rectification): `seq` (-1: the shared maps of every sequence
        without its own).  Frames passed from now on are raw (left_info's width x height).  The projection matrices are NOT
        set here: pass left_info["P"] / right_info["P"] to initalize_projection_matricies."""
        li, ri = camera_info(left_info), camera_info(right_info)
        check(lib.svo_set_rectification(self._h, seq, C.byref(li), C.byref(ri)))
        self.raw_size = (li.width, li.height)

    def set_rectification_maps(self, map1_l, map2_l, map1_r, map2_r, seq=-1, raw_size=None):
        """Install precomputed maps (svo_set_rectification_maps): map1 (height, width, 2) int16 and map2 (height, width) uint16
        at the context's size.  raw_size = (raw_w, raw_h); may be omitted once the context rectifies."""
        raw_size = raw_size or self.raw_size
        if raw_size is None:
            raise ValueError("raw_size = (raw_w, raw_h) is required for the first maps")
        a, b = _maps(map1_l, map2_l); c, d = _maps(map1_r, map2_r)
        if a.shape[:2] != (self.height, self.width) or c.shape[:2] != (self.height, self.width):
            raise ValueError("maps must be (%d, %d)" % (self.height, self.width))
        check(lib.svo_set_rectification_maps(self._h, seq, int(raw_size[0]), int(raw_size[1]), ptr(a), ptr(b), ptr(c), ptr(d)))
        self.raw_size = (int(raw_size[0]), int(raw_size[1]))

    def clear_rectification(self):
        """Back to a plain context (svo_clear_rectification): frames at the context's size again."""
        check(lib.svo_clear_rectification(self._h))
        self.raw_size = None

    def close(self):
        if self._has_context():
            lib.svo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def initalize_projection_matricies(self, leftCameraProjection, rightCameraProjection, seq=-1):
        Pl = np.ascontiguousarray(leftCameraProjection, np.float32).reshape(12)
        Pr = np.ascontiguousarray(rightCameraProjection, np.float32).reshape(12)
        check(lib.svo_set_projection(self._h, seq, ptr(Pl), ptr(Pr)))
        self._Pl = Pl.copy()                          # set_rotation_prior's K

    def _results(self, call):
        """Run call(T_out, ok_out, stats), one of the entry points that hand a frame's results back -> (ok (n_seq,) bool,
        T (n_seq, 4, 4) f64), with the frame's counters in self.stats."""
        T = np.zeros((self.n_seq, 16)); ok = np.zeros(self.n_seq, np.int32)
        st = (SvoFrameStats * self.n_seq)()
        check(call(ptr(T), ptr(ok), st))
        self.stats = list(st)
        return ok.astype(bool), T.reshape(self.n_seq, 4, 4)

    def _active(self, active):
        """None (a null list: every sequence takes the frame), or n_seq truthy flags -> a uint8 array for the masked entry points."""
        if active is None:
            return None
        a = np.ascontiguousarray(np.asarray(active).astype(bool), np.uint8)
        if a.shape != (self.n_seq,):
            raise ValueError("active must hold n_seq = %d flags" % self.n_seq)
        return a

    def stereo_callback_batch(self, lefts, rights, active=None):
        """lists of n_seq host images -> (ok (n_seq,) bool, T (n_seq,4,4) f64).
        active: None (every sequence takes the frame) or n_seq flags; an idle sequence's images may be None, its state is left
        alone and its row is its last good T with ok False and stats.fail_reason 5 (svo_process_batch_masked)."""
        act = self._active(active)
        on = [True] * self.n_seq if act is None else [bool(x) for x in act]
        L = [self._frame(i) if o else None for i, o in zip(lefts, on)]; R = [self._frame(i) if o else None for i, o in zip(rights, on)]
        assert len(L) == self.n_seq and len(R) == self.n_seq
        cn = self._bpp()
        assert all(i.shape == self._frame_shape() for i in L + R if i is not None), "image shape / channels"
        lp = (C.c_void_p * self.n_seq)(*[i.ctypes.data if i is not None else None for i in L])
        rp = (C.c_void_p * self.n_seq)(*[i.ctypes.data if i is not None else None for i in R])
        return self._results(lambda *out: lib.svo_process_batch_masked(self._h, lp, rp, self._in_shape()[1] * cn, 0, ptr(act), *out))

    def process_device(self, left_ptrs, right_ptrs, stride, active=None):
        """device pointers (ints; None for idle sequences) -> same outputs; inputs stay resident in HBM."""
        act = self._active(active)
        lp = (C.c_void_p * self.n_seq)(*left_ptrs); rp = (C.c_void_p * self.n_seq)(*right_ptrs)
        return self._results(lambda *out: lib.svo_process_batch_masked(self._h, lp, rp, stride, 1, ptr(act), *out))

    def submit_device(self, left_ptrs, right_ptrs, stride, active=None):
        act = self._active(active)
        lp = (C.c_void_p * self.n_seq)(*left_ptrs); rp = (C.c_void_p * self.n_seq)(*right_ptrs)
        check(lib.svo_submit_batch_masked(self._h, lp, rp, stride, ptr(act)))

    def reset_sequence(self, seq=-1, Pl=None, Pr=None):
        """Return sequence `seq` (-1: all) to a fresh context's state, optionally with new projection matrices (both or
        neither); its next active frame is a first frame.  Stream-ordered with submit_device, no synchronisation
        (svo_reset_sequence)."""
        if (Pl is None) != (Pr is None):
            raise ValueError("give both Pl and Pr, or neither")
        pl = pr = None
        if Pl is not None:
            pl = np.ascontiguousarray(Pl, np.float32).reshape(12); pr = np.ascontiguousarray(Pr, np.float32).reshape(12)
        check(lib.svo_reset_sequence(self._h, seq, ptr(pl), ptr(pr)))

    def collect(self):
        return self._results(lambda *out: lib.svo_collect(self._h, *out))

    def set_stage_timing(self, on=True):
        """Record the stage-boundary events of every frame from now on (svo_set_stage_timing): last_timing()'s LK time and
        stage_timing() need them; off by default (they cost a lone stream ~10 us per frame)."""
        check(lib.svo_set_stage_timing(self._h, int(bool(on))))

    def last_timing(self):
        lk, fr = C.c_float(0), C.c_float(0)
        check(lib.svo_get_last_timing(self._h, C.byref(lk), C.byref(fr)))
        return lk.value, fr.value

    STAGES = ("ingest+pyramid", "detect", "lk", "compact+triangulate", "pnp")

    def stage_timing(self):
        """HIP-event milliseconds of the last collected frame per pipeline stage (svo_get_stage_timing) -> dict."""
        ms = (C.c_float * 5)()
        check(lib.svo_get_stage_timing(self._h, ms))
        return dict(zip(self.STAGES, [float(x) for x in ms]))

    def stream(self):
        return lib.svo_get_stream(self._h)

    def last_frame_path(self):
        """svo_get_last_frame_path: the SVO_PATH_* bits (_lib.PATH_*) of the most recently issued frame — which builds and
        launch shapes it took; 0 before the first frame."""
        return lib.svo_get_last_frame_path(self._h) if self._has_context() else 0

    def lk_registers_left(self):
        """svo_get_lk_registers_left: VGPRs a SIMD keeps beside this context's LK waves (>= 96: a shared device runs the
        96-register f64 builds)."""
        return lib.svo_get_lk_registers_left(self._h) if self._has_context() else -1

    def features(self, seq=0):
        cap = 1 << 15
        xy = np.zeros((cap, 2), np.float32); ages = np.zeros(cap, np.int32); st = np.zeros(cap, np.int32)
        n = check(lib.svo_get_features(self._h, seq, cap, ptr(xy), ptr(ages), ptr(st)))
        return xy[:n].copy(), ages[:n].copy(), st[:n].copy()

    def last_tracks(self, seq=0):
        cap = 1 << 15
        a = [np.zeros((cap, 2), np.float32) for _ in range(4)]
        world = np.zeros((cap, 3), np.float32); inl = np.zeros(cap, np.uint8)
        n = check(lib.svo_get_last_tracks(self._h, seq, cap, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(world), ptr(inl)))
        return dict(pl0=a[0][:n].copy(), pr0=a[1][:n].copy(), pl1=a[2][:n].copy(), pr1=a[3][:n].copy(),
                    world=world[:n].copy(), inlier=inl[:n].copy())

    PYRAMIDS = {"t1": _lib.PYR_T1, "last_left": _lib.PYR_LAST_LEFT}

    def pyramid(self, seq, which="t1", cam=0, level=0, plane=0):
        """One stored pyramid level of sequence `seq` WITH its REFLECT_101 border (svo_get_pyramid) -> (array, pad): a uint8
        (h + 2 pad, w + 2 pad) array whose [pad:-pad, pad:-pad] is the level.  which: "t1" (the last frame's pyramids) or
        "last_left" (lastLeftPyramid's pair; cam 1 = lastRightPyramid); plane: colour plane of a BGR context."""
        wh = self.PYRAMIDS[which]
        w, h, pad, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib.svo_get_pyramid(self._h, seq, wh, cam, plane, level, None, 0, C.byref(w), C.byref(h), C.byref(pad), C.byref(nl)))
        out = np.zeros((h.value + 2 * pad.value, w.value + 2 * pad.value), np.uint8)
        check(lib.svo_get_pyramid(self._h, seq, wh, cam, plane, level, ptr(out), out.size, None, None, None, None))
        return out, pad.value

    def derivatives(self, seq, which="t1", cam=0, level=1):
        """The Scharr planes the LK kernel loads at pyramid level `level` >= 1 of sequence `seq`, WITH their zero border
        (svo_get_derivatives) -> (ix, iy, pad): int16 (h + 2 pad, w + 2 pad) arrays whose [pad:-pad, pad:-pad] is 4 x the Scharr
        derivative of the level.  which, cam: as pyramid().  SvoError in a context that keeps no planes (has_derivatives())."""
        wh = self.PYRAMIDS[which]
        w, h, pad = C.c_int(), C.c_int(), C.c_int()
        check(lib.svo_get_derivatives(self._h, seq, wh, cam, level, None, None, 0, C.byref(w), C.byref(h), C.byref(pad), None))
        ix = np.zeros((h.value + 2 * pad.value, w.value + 2 * pad.value), np.int16); iy = np.zeros_like(ix)
        check(lib.svo_get_derivatives(self._h, seq, wh, cam, level, ptr(ix), ptr(iy), ix.size, None, None, None, None))
        return ix, iy, pad.value

    def has_derivatives(self):
        """Whether the context keeps derivative planes beside its pyramids (many sequences, grey, exact sums, >= 2 levels)."""
        return lib.svo_get_derivatives(self._h, 0, _lib.PYR_T1, 0, 1, None, None, 0, None, None, None, None) == _lib.SVO_OK

    def pyramid_levels(self):
        """Number of levels the context builds (the buildOpticalFlowPyramid stop rule at its window and max_level)."""
        nl = C.c_int()
        check(lib.svo_get_pyramid(self._h, 0, _lib.PYR_T1, 0, 0, 0, None, 0, None, None, None, C.byref(nl)))
        return nl.value


def _deferrable(slot):
    """A VisualOdometry setter that may come before the first frame.  With a context it is BatchVisualOdometry's setter of the same
    name.  Without one the decorated body checks the arguments as the library would, at once, and returns those to hold for that
    setter in the slot (None: nothing, the slot is emptied); VisualOdometry._apply hands them over when the first frame comes."""
    def wrap(check):
        setter = getattr(BatchVisualOdometry, check.__name__)

        @functools.wraps(setter)
        def method(self, *args, **kw):
            if self._has_context():
                return setter(self, *args, **kw)
            held = check(self, *args, **kw)
            self._held.pop(slot, None)
            if held is not None:
                self._held[slot] = (check.__name__, held)
        return method
    return wrap


def _after_first_frame(getter):
    """A BatchVisualOdometry getter of a frame's results as VisualOdometry has it: SvoError before the first frame."""
    @functools.wraps(getter)
    def method(self, *args, **kw):
        self._need_frame(getter.__name__)
        return getter(self, *args, **kw)
    return method


class VisualOdometry(BatchVisualOdometry):
    """vo.h:231-380 — one stereo stream.  stereo_callback(left, right) -> (success, 4x4 float64)."""

    def __init__(self, width=None, height=None, cfg=None, device=0):
        self._args = (cfg, device)
        self._h = C.c_void_p()                        # no context before the first frame, unless the size is given here
        self._held = {}                               # slot -> (setter's name, its arguments): asked for before the context exists
        self.raw_size = None
        if width is not None:
            super().__init__(width, height, 1, cfg, device)

    # ---- settings before the first frame ("Facades: settings before the first frame").  The slots, in the order _apply
    # hands them to the new context: CLAHE's fit check must see the raw size, so it follows the rectification; the descriptors ride
    # on the track output; the explicit prior is consumed by the first frame.  Below, each slot's setters with their checks.
    _ORDER = ("rectification", "projection", "timing", "format", "covariance", "mask", "clahe", "track", "descriptors", "prior", "prior_mode")

    @_deferrable("rectification")
    def set_rectification(self, left_info, right_info, seq=-1):
        return left_info, right_info                  # the rectified size is then the raw size (as ROS's image_rect)

    @_deferrable("rectification")
    def set_rectification_maps(self, map1_l, map2_l, map1_r, map2_r, seq=-1, raw_size=None):
        if raw_size is None:
            raise ValueError("raw_size = (raw_w, raw_h) is required for the first maps")
        return map1_l, map2_l, map1_r, map2_r, -1, raw_size           # the context's size is then the maps'

    @_deferrable("rectification")
    def clear_rectification(self):
        return None

    @_deferrable("projection")
    def initalize_projection_matricies(self, leftCameraProjection, rightCameraProjection, seq=-1):
        return leftCameraProjection, rightCameraProjection

    @_deferrable("timing")
    def set_stage_timing(self, on=True):
        return (bool(on),)

    @_deferrable("format")
    def set_input_format(self, fmt):
        f = _lib.input_format(fmt)
        return (f,) if f != _lib.INPUT_MONO8 else None                # mono8 is a new context's format (and a BGR context takes no setter)

    @_deferrable("covariance")
    def set_pose_covariance(self, mode="residual", pixel_sigma=1.0):
        return _lib.check_cov(mode, pixel_sigma)

    @_deferrable("mask")
    def set_detection_mask(self, mask, seq=-1):
        if mask is not None and (not hasattr(mask, "ndim") or mask.ndim != 2 or "uint8" not in str(mask.dtype)):
            raise ValueError("detection mask: a 2-D uint8 array expected")
        return (mask,) if mask is not None else None                  # its size is checked against the first frame's

    @_deferrable("mask")
    def clear_detection_mask(self, seq=-1):
        return None

    @_deferrable("clahe")
    def set_clahe(self, clip_limit=2.0, tiles=(8, 8)):
        clip, tx, ty = _lib.check_clahe(clip_limit, tiles)            # the fit to the frame size is checked at the first frame
        return clip, (tx, ty)

    @_deferrable("clahe")
    def clear_clahe(self):
        return None

    @_deferrable("track")
    def set_track_output(self, max_rows):
        if int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        return (int(max_rows),)

    @_deferrable("track")
    def clear_track_output(self):
        self._held.pop("descriptors", None)                           # the descriptors ride on the track output
        return None

    @_deferrable("descriptors")
    def set_descriptor_output(self, on=True):
        if on and "track" not in self._held:
            raise _lib.SvoError("set_descriptor_output: the track output is off (set_track_output first)")
        return (True,) if on else None

    @_deferrable("prior")
    def set_motion_prior(self, H, Hi=None, seq=-1):
        return None if H is None else (_h9(H, "H").copy(), None if Hi is None else _h9(Hi, "Hi").copy())

    @_deferrable("prior_mode")
    def set_motion_prior_mode(self, mode):
        if mode not in _lib.PRIOR_MODES:
            raise ValueError("motion prior mode: one of %s expected" % sorted(_lib.PRIOR_MODES))
        return (mode,)

    def _apply(self, ctx):
        """Hand ctx, a context just created, every held setting in _ORDER.  Like the reference, a first frame needs no projection
        matrices (vo.cpp:47-56 only caches): until initalize_projection_matricies is called they are all-zero, as the reference's
        empty Mats effectively are."""
        zero = np.zeros(12, np.float32)
        held = dict(self._held)
        held.setdefault("projection", ("initalize_projection_matricies", (zero, zero)))
        for slot in self._ORDER:
            if slot in held:
                setter, args = held[slot]
                getattr(ctx, setter)(*args)

    def _first_frame(self, L, colour):
        """The reference learns the image size (and type) from the first frame: create the context at that size, _apply the held
        settings to it, and only then adopt it.  A setting the context refuses (CLAHE tiles that do not fit this size, ...)
        raises with the object still before its first frame and its record intact: correct the setting, pass the frame again."""
        cfg, device = self._args
        cfg = _lib.copy_config(cfg) if cfg is not None else default_config()       # never write into the caller's struct
        cfg.channels = 3 if colour else 1                 # colour Mats, as the reference CLI feeds them (main.cpp:38-46)
        h, w = L.shape[:2]
        setter, args = self._held.get("rectification", (None, None))
        if setter == "set_rectification_maps":
            h, w = np.asarray(args[1]).shape
        ctx = BatchVisualOdometry(w, h, 1, cfg, device)
        try:
            self._apply(ctx)
        except Exception:
            ctx.close()
            raise
        self.__dict__.update(vars(ctx))                   # the context and what BatchVisualOdometry knows about it
        ctx._h = C.c_void_p()                             # (ctx no longer owns it)
        self._held = {}

    def _held_args(self, slot):
        """What the slot holds before the first frame, or None"""
        return self._held[slot][1] if slot in self._held else None

    last_track_obs = _after_first_frame(BatchVisualOdometry.last_track_obs)
    last_track_descriptors = _after_first_frame(BatchVisualOdometry.last_track_descriptors)
    feature_ids = _after_first_frame(BatchVisualOdometry.feature_ids)
    last_pose_covariance = _after_first_frame(BatchVisualOdometry.last_pose_covariance)
    last_motion_prior = _after_first_frame(BatchVisualOdometry.last_motion_prior)

    def pyramid(self, seq=0, which="t1", cam=0, level=0, plane=0):
        self._need_frame("pyramid", RuntimeError)
        return super().pyramid(seq, which, cam, level, plane)

    def detection_mask(self, seq=-1):
        if self._has_context():
            return super().detection_mask(seq)
        m = self._held_args("mask")
        return None if m is None else np.array(m[0].cpu() if hasattr(m[0], "cpu") else m[0], np.uint8)

    def motion_prior_mode(self):
        return super().motion_prior_mode() if self._has_context() else (self._held_args("prior_mode") or ("explicit",))[0]

    def motion_prior(self, seq=0):
        if self._has_context():
            return super().motion_prior(seq)
        p = self._held_args("prior")
        return None if p is None else (p[0].reshape(3, 3), p[1].reshape(3, 3) if p[1] is not None else None)

    def set_rotation_prior(self, R, seq=-1, Pl=None):
        if Pl is None and not self._has_context() and "projection" in self._held:
            Pl = self._held_args("projection")[0]
        return super().set_rotation_prior(R, seq, Pl)

    def stereo_callback(self, image_left, image_right):
        fmt = self.input_format if self._has_context() else (self._held_args("format") or (_lib.INPUT_MONO8,))[0]
        bpp = _lib.INPUT_BPP[fmt] if fmt != _lib.INPUT_MONO8 else None
        if self._has_context() and self.cfg.channels == 3:
            bpp = None
        L, R = u8frame(image_left, bpp), u8frame(image_right, bpp)
        if not self._has_context():
            self._first_frame(L, colour=L.ndim == 3 and bpp is None)
        self._check_frame(L, "left"); self._check_frame(R, "right")
        T = np.zeros(16)
        st = SvoFrameStats()
        rc = check(lib.svo_process(self._h, ptr(L), ptr(R), L.strides[0], ptr(T), C.byref(st)))
        self.stats = st
        return bool(rc), T.reshape(4, 4)

    def reset(self):
        """Start over as a freshly constructed object with the same projection matrices: the next stereo_callback is a first
        frame.  The reference has no counterpart (it constructs a new VisualOdometry); this wraps svo_reset_sequence."""
        if self._has_context():
            self.reset_sequence(0)

    def _check_frame(self, img, which):
        """cv::Mat carries size and type and OpenCV asserts on a mismatch; a raw pointer does not: check before the C call."""
        want = self._frame_shape()
        if img.shape != want:
            raise ValueError("%s image has shape %s, the context was created for %s" % (which, img.shape, want))

    def circularMatching(self, imgLeftT1, imgRightT1, pointsLeftT0, current_features):
        """vo.h:374-379, vo.cpp:169-240.  Tracks pointsLeftT0 around T0-left -> T1-left -> T1-right -> T0-right -> T0-left against
        the pyramid pair this object cached on the device in its previous stereo_callback / circularMatching, removes every point
        (and its feature, in place) that lost an LK status or does not close the loop, and makes the T1 pyramids the cached pair
        (vo.cpp:231-232) — the state stereo_callback itself works on, as in the reference.
        Returns (pointsLeftT0, pointsRightT0, pointsLeftT1, pointsRightT1) — Python has no out-parameters."""
        p0 = _pts(pointsLeftT0)
        empty = np.zeros((0, 2), np.float32)
        if len(p0) == 0:
            return p0, empty, empty, empty                                                  # vo.cpp:179-181
        if not self._has_context():
            raise RuntimeError("circularMatching: no cached pyramids (call stereo_callback first)")
        l1, r1 = self._frame(imgLeftT1), self._frame(imgRightT1)
        self._check_frame(l1, "left"); self._check_frame(r1, "right")
        n = len(p0)
        outs = [np.zeros((n, 2), np.float32) for _ in range(4)]
        ok = np.zeros(n, np.uint8)
        check(lib.svo_circular_matching(self._h, ptr(l1), ptr(r1), l1.strides[0], n, ptr(p0), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                        ptr(outs[3]), ptr(ok)))
        pl1, pr1, pr0 = outs[0], outs[1], outs[2]
        keep = ok.astype(bool)
        deleteFeaturesWithFailureStatus(current_features, keep)                             # :233
        return p0[keep], pr0[keep], pl1[keep], pr1[keep]                                    # :234-238

    def matchingFeatures(self, imageLeftT0, imageRightT0, imageLeftT1, imageRightT1, currentVOFeatures):
        """vo.h:354-362, vo.cpp:315-366 -> (pointsLeftT0, pointsRightT0, pointsLeftT1, pointsRightT1); the feature set is updated in place."""
        currentVOFeatures.appendFeaturesFromImage(imageLeftT0, FAST_THRESHOLD)              # :325
        if currentVOFeatures.size() < PRE_MATCHING_FEATURE_THRESHOLD:                       # :327-332
            currentVOFeatures.appendFeaturesFromImage(imageLeftT0, FAST_THRESHOLD // 4)
        # as in the reference, imageLeftT0 only feeds FAST; the loop's T0 side is the cached pyramid pair (prime with stereo_callback)
        pl0, pr0, pl1, pr1 = self.circularMatching(imageLeftT1, imageRightT1, currentVOFeatures.points.copy(), currentVOFeatures)
        h, w = u8frame(imageLeftT1).shape[:2]
        inside = np.ones(len(pl0), bool)                                                    # :341-359
        for q in (pl0, pl1, pr0, pr1):
            inside &= ~((q[:, 0] < 0) | (q[:, 1] < 0) | (q[:, 1] >= h) | (q[:, 0] >= w))
        deleteFeaturesWithFailureStatus(currentVOFeatures, inside)                          # :360-364
        return pl0[inside], pr0[inside], pl1[inside], pr1[inside]
