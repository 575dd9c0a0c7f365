"""No-GPU checks of rectification (include/svo.h, rectification section): the host map generator equals the numpy
restatement of cv::initUndistortRectifyMap's scalar loop (tests/rectify_ref.py) bit for bit, the identity calibration gives
the identity map, and the new entry points are declared, exported, bound and reject a NULL context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rectify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svo_set_rectification_maps", "svo_set_rectification", "svo_clear_rectification", "svo_init_rectify_map", "svo_rectify_image")


def lib_map(cal, w=None, h=None):
    from stereo_visual_odometry_amd import api
    return api.init_rectify_map(cal["K"], cal["D"], cal["R"], cal["P"], w or cal["width"], h or cal["height"])


def assert_same_map(a, b):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    bad = np.argwhere((a[0] != b[0]).any(-1) | (a[1] != b[1]))
    assert len(bad) == 0, "%d pixels differ, first at %s: %s/%s vs %s/%s" % (
        len(bad), bad[0], a[0][tuple(bad[0])], a[1][tuple(bad[0])], b[0][tuple(bad[0])], b[1][tuple(bad[0])])


@pytest.mark.parametrize("name", ["KITTI00_LEFT", "KITTI00_RIGHT", "ZED_LEFT", "ZED_RIGHT"])
def test_map_equals_numpy_restatement_bit_for_bit(name):
    cal = getattr(ref, name)
    assert_same_map(lib_map(cal), ref.init_rectify_map(cal["K"], cal["D"], cal["R"], cal["P"], cal["width"], cal["height"]))


def test_map_variants_equal_numpy_restatement():
    """P with its own fx / cx (a rectified size other than the raw one), 4 coefficients, R and P left out (identity / K)."""
    z = ref.ZED_RIGHT
    P = [[512.25, 0.0, 300.5, -61.4], [0.0, 530.75, 170.125, 0.0], [0.0, 0.0, 1.0, 0.0]]
    cases = [(z["K"], z["D"], z["R"], P, 640, 360), (z["K"], z["D"][:4], z["R"], P, 333, 201), (z["K"], z["D"], None, None, 257, 143),
             (ref.ZED_LEFT["K"], ref.ZED_LEFT["D"], ref.ZED_LEFT["R"], ref.ZED_LEFT["P"], 97, 61)]
    from stereo_visual_odometry_amd import api
    for K, D, R, P_, w, h in cases:
        assert_same_map(api.init_rectify_map(K, D, R, P_, w, h), ref.init_rectify_map(K, D, R, P_, w, h))


def test_identity_calibration_gives_identity_map():
    cal = ref.KITTI00_LEFT
    m1, m2 = lib_map(cal)
    yy, xx = np.mgrid[0:cal["height"], 0:cal["width"]]
    assert np.array_equal(m1[..., 0], xx) and np.array_equal(m1[..., 1], yy)
    assert not m2.any()


def test_bad_arguments():
    from stereo_visual_odometry_amd import _lib, api
    with pytest.raises(ValueError):
        api.camera_info(dict(ref.ZED_LEFT, D=[0.1, 0.2, 0.3]))
    K = np.eye(3).reshape(9)
    m1 = np.zeros((4, 4, 2), np.int16); m2 = np.zeros((4, 4), np.uint16)
    D = np.zeros(6)
    assert _lib.lib.svo_init_rectify_map(_lib.ptr(K), _lib.ptr(D), 6, None, None, 4, 4, _lib.ptr(m1), _lib.ptr(m2)) == _lib.SVO_ERR_ARG
    Z = np.zeros(12)
    assert _lib.lib.svo_init_rectify_map(_lib.ptr(K), None, 0, None, _lib.ptr(Z), 4, 4, _lib.ptr(m1), _lib.ptr(m2)) == _lib.SVO_ERR_ARG


def test_declared_exported_and_bound():
    from stereo_visual_odometry_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "svo.h does not declare %s" % s
        assert hasattr(_lib.lib, s), "libsvo_hip.so does not export %s" % s
        assert s in _lib.EXPORTS
    assert "svo_camera_info" in txt


def test_camera_info_layout():
    from stereo_visual_odometry_amd import _lib
    ci = _lib.SvoCameraInfo
    assert ci.K.offset == 0 and ci.D.offset == 72 and ci.n_d.offset == 136 and ci.R.offset == 144 and ci.P.offset == 216
    assert ci.width.offset == 312 and ci.height.offset == 316 and C.sizeof(ci) == 320


def test_null_context_is_an_argument_error():
    from stereo_visual_odometry_amd import _lib, api
    lib = _lib.lib
    m1 = np.zeros((4, 4, 2), np.int16); m2 = np.zeros((4, 4), np.uint16)
    p1, p2 = _lib.ptr(m1), _lib.ptr(m2)
    assert lib.svo_set_rectification_maps(None, -1, 4, 4, p1, p2, p1, p2) == _lib.SVO_ERR_ARG
    ci = api.camera_info(ref.KITTI00_LEFT)
    assert lib.svo_set_rectification(None, -1, C.byref(ci), C.byref(ci)) == _lib.SVO_ERR_ARG
    assert lib.svo_clear_rectification(None) == _lib.SVO_ERR_ARG
    raw = np.zeros((4, 4), np.uint8); out = np.zeros((4, 4), np.uint8)
    assert lib.svo_rectify_image(0, None, p2, 4, 4, _lib.ptr(raw), 4, 4, 4, 1, _lib.ptr(out)) == _lib.SVO_ERR_ARG
    assert lib.svo_rectify_image(0, p1, p2, 4, 4, _lib.ptr(raw), 4, 4, 4, 2, _lib.ptr(out)) == _lib.SVO_ERR_ARG
