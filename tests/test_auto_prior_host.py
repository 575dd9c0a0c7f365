"""The predicted motion prior (include/svo.h, SVO_PRIOR_LAST_ROTATION) without a GPU.

tests/cpp/auto_prior_host.cpp is a stand-alone program over stereo_visual_odometry_amd/csrc/svo_prior.hpp — prior_predict_row, the
function k_prior_predict runs per sequence, compiled for the host from the same text — built with AddressSanitizer and UBSan.  The
entry points that need no device are held to their contract.  And the precondition of tests/test_gpu_auto_prior.py's second test is
pinned on the numpy reference: on frame pair (1, 2) of the motion-prior scene the pyramid alone keeps no frame, while the rotation of
frame pair (0, 1) — one frame old, what the predicted prior is — keeps exactly as many tracks as the true one."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
import lk_prior_cases as pc
import auto_prior_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_predict_row_under_sanitizers(tmp_path):
    exe = str(tmp_path / "auto_prior_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "auto_prior_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "AUTO PRIOR HOST OK" in out.stdout, out.stdout + out.stderr


def test_mode_entry_points_need_a_context():
    import ctypes as C
    from stereo_visual_odometry_amd import _lib
    m = C.c_int(0)
    assert _lib.lib.svo_set_motion_prior_mode(None, _lib.PRIOR_LAST_ROTATION) == _lib.SVO_ERR_ARG
    assert _lib.lib.svo_get_motion_prior_mode(None, C.byref(m)) == _lib.SVO_ERR_ARG
    assert _lib.lib.svo_get_last_motion_prior(None, 0, None, None, C.byref(m)) == _lib.SVO_ERR_ARG
    assert (_lib.PRIOR_EXPLICIT, _lib.PRIOR_LAST_ROTATION, _lib.PATH_PRIOR_PREDICTED) == (0, 1, 4096)


def build_facade_test():
    exe = os.path.join(CPP, "auto_prior_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "auto_prior_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())


# (width, height, window) -> points into LK, tracks kept after the circular and bounds masks without a prior / with frame pair
# (0, 1)'s rotation / with the true rotation of frame pair (1, 2): lk_prior_ref.circular on fresh detections of frame 1
COUNTS = {(320, 240, 21): (652, 3, 371, 371), (160, 120, 7): (155, 0, 48, 48), (640, 192, 21): (1045, 7, 704, 704)}


@pytest.mark.parametrize("w,h,win", pc.FRAME_CASES)
def test_a_rotation_one_frame_old_is_as_good_as_the_true_one(w, h, win):
    cfg = orc.default_config(**pc.over(win))
    pts = pc.lk_input(pc.scene(w, h).left[1], cfg)
    kept = []
    for H, Hi in ((None, None), pc.homography(w, h, 1), pc.homography(w, h, 2)):
        c = pc.circular_cached(w, h, win, 2, pts, H, Hi, cfg)
        kept.append(int((c["ok"].astype(bool) & c["inb"]).sum()))
    print(w, h, win, "into LK", len(pts), "kept none / stale / true", kept)
    assert (len(pts),) + tuple(kept) == COUNTS[(w, h, win)]
    assert kept[0] <= max(4, cfg.features_threshold) < kept[1]          # fail_reason 2 without, a frame with (vo.cpp:82-84)
    deg = lambda R: np.degrees(np.arccos((np.trace(R) - 1) / 2))
    assert abs(deg(pc.rotation(w, h, 1)) - 7.65) < 0.01 and abs(deg(pc.rotation(w, h, 2)) - 6.49) < 0.01


def test_the_gap_holds_from_the_carried_feature_set():
    """the same at the state the GPU runs reach frame 2 in — frame 1 played with the ground-truth prior, its inliers carried and topped
    up by detection, the stale rotation the one frame 1's own solve returned — at the small shape (measured when this was written: 177
    points; 0 / 48 / 48 kept; the solved rotation 7.64 degrees against the true 7.65)"""
    w, h, win = 160, 120, 7
    ok, state, st1 = ar.after_frame_one(w, h, win)
    assert ok and st1["fail_reason"] == 0
    stats, stale_deg, true_deg = ar.frame_two(w, h, win)
    print(st1, stats, stale_deg, true_deg)
    assert stats["none"]["fail_reason"] == 2 and stats["stale"]["fail_reason"] == 0 and stats["true"]["fail_reason"] == 0
    assert stats["stale"]["n_after_bounds"] == stats["true"]["n_after_bounds"] >= 15
    assert abs(stale_deg - 7.65) < 0.05 and abs(true_deg - 6.49) < 0.01
