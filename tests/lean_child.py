"""Run in a fresh process with SVO_FORCE_LEAN=1 (test_gpu_shared_device_builds.py::test_forced_lean_takes_the_lean_builds): a
lone context, a many-sequence context alone on the device and the stage entry points must all report the 96-register builds
through svo_get_last_frame_path."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from stereo_visual_odometry_amd import _lib, api, synthetic as syn  # noqa: E402


def main():
    assert os.environ.get("SVO_FORCE_LEAN") == "1", "run with SVO_FORCE_LEAN=1"
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=3, seed=3, step=0.3)
    P = syn.projection_matrices(cal)
    over = dict(max_translation_norm=2.0)

    lone = api.VisualOdometry(cfg=api.default_config(**over)); lone.initalize_projection_matricies(*P)
    for k in range(3):
        lone.stereo_callback(seq.left[k], seq.right[k])
        p = lone.last_frame_path()
        assert p & _lib.PATH_LEAN and not p & _lib.PATH_TRI_EPNP_FUSED, ("lone", k, p)
    assert lone.stats.n_inliers > 0
    lone.close()

    B = 10
    many = api.BatchVisualOdometry(320, 160, B, api.default_config(**over)); many.initalize_projection_matricies(*P)
    for k in range(3):
        ok, _ = many.stereo_callback_batch([seq.left[k]] * B, [seq.right[k]] * B)
        p = many.last_frame_path()
        assert p & _lib.PATH_LEAN and not p & _lib.PATH_LK_CHAINED, ("many", k, p)    # alone on the device: no chaining
    assert ok.all()
    many.close()

    rng = np.random.default_rng(1)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)
    world = np.stack([rng.uniform(-15, 15, 400), rng.uniform(-3, 3, 400), rng.uniform(6, 60, 400)], 1).astype(np.float32)
    cam = np.stack([718.856 * world[:, 0] / world[:, 2] + 607.1928, 718.856 * world[:, 1] / world[:, 2] + 185.2157], 1).astype(np.float32)
    (inl, ok), R, t, _ = api.cameraToWorld(K, cam, world, np.eye(3), np.zeros(3))
    assert ok and len(inl) == 400 and api.last_stage_path() & _lib.PATH_LEAN, ("camera_to_world", api.last_stage_path())
    Pl, Pr = syn.projection_matrices(syn.KITTI00)
    api.triangulatePoints(Pl, Pr, cam, cam - np.float32([5, 0]))
    assert api.last_stage_path() & _lib.PATH_LEAN, ("triangulate", api.last_stage_path())
    print("lean child ok")


if __name__ == "__main__":
    main()
