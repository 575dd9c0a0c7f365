"""The pose stage (svo_kernels_pnp.hip: k_pnp_subsets, k_pnp_epnp, k_tri_epnp, k_pnp_score, k_pnp_decide, k_pnp_final, k_pnp_p3p and
the lean builds) where the other suites do not take it: point counts around the 256-stride of k_pnp_score, the 512 / 256
threads of k_pnp_final and its 2048 register-cached tracks; iteration bounds around the first chunk of 32 (16) hypotheses;
exactly planar, nearly collinear, far, behind-the-camera, duplicated and 90 %-outlier point sets; rotations of pi; three
cameras (KITTI-00, K = I with normalised coordinates, the run1 calibration with fx != fy); and never the guess R = I, t = 0.
The inputs are tests/pnp_ref.py's, each proven fit on the oracle by tests/test_pnp_ref.py.

  stage tests     cameraToWorld per case and camera.  success, iterations run and the inlier index list equal the oracle's
                  EXACTLY (they rest on IEEE-exact operations only, see the header of svo_kernels_pnp.hip); a failure returns the
                  non-identity guess bit-unchanged and no inliers; a success does not depend on the guess.  Class A (the oracle's
                  pose is stationary): the pose is within 1e-6 of the oracle's and, without the oracle, of pnp_ref.minimise on the
                  returned inliers.  Class B (the oracle's 20-step LM stopped short on an ill-conditioned set): no pose
                  tolerance — cost(HIP) - cost* <= 2 (cost(oracle) - cost*) + 1e-9 cost*, cost* the reference minimum.
                  test_gpu_shared_device_builds.py runs these again under SVO_FORCE_LEAN=1 (k_pnp_epnp_lean, k_pnp_final_lean);
                  the path bit each call reports is asserted here, so the child cannot pass on the wrong build.
  pipeline tests  four 480 x 200 scenes (a wall at 30 m, a wall at 8 m that leaves 21-29 tracks and 25-85 RANSAC iterations, a
                  world at 300-400 m, six layers) through a lone context (k_tri_epnp, first chunk 32) and a context of nine
                  sequences that cycle through the scenes (k_triangulate with the spare block, first chunk 16, a different
                  pnp_need per sequence in one k_pnp_decide launch), every frame against the oracle as run_both does.

Class B as measured on the MI355X, full builds (printed per case with -s): cost - cost* of the oracle | of the HIP path, cost*,
and the distance between the two poses.  Two kinds land here: a refine that has nearly arrived when its 20 steps are spent
(near_collinear and bundle_thin under KITTI-00, bundle_thin under run1, pencil_far) and one that stalls hundreds of metres
down the bundle (thin_bundle; near_collinear under the other cameras).  In both the two 20-step schedules take the same
accept / reject decisions and end within 1e-9 m of each other:

  camera case            cost - cost*: oracle | HIP            cost*          oracle <-> HIP
  kitti  near_collinear  1.681913e-06 | 1.681913e-06   2.512553e+01   8.4e-13 rad  9.6e-13 m
  kitti  bundle_thin     1.463829e-08 | 1.463808e-08   2.272907e+01   1.0e-12 rad  4.2e-14 m
  kitti  thin_bundle     1.877205e+02 | 1.877205e+02   1.858980e+03   4.4e-13 rad  1.5e-10 m
  kitti  pencil_far      1.811884e-13 | 7.105427e-14   2.195227e+01   1.9e-15 rad  4.8e-13 m
  ident  near_collinear  1.364243e-02 | 1.364243e-02   5.040745e-05   2.4e-15 rad  2.3e-13 m
  ident  bundle_thin     7.246543e-03 | 7.246543e-03   4.489878e-05   1.0e-15 rad  9.1e-13 m
  ident  thin_bundle     6.781761e-03 | 6.781761e-03   4.656920e-05   3.1e-12 rad  1.0e-09 m
  ident  pencil_far      6.098637e-20 | 6.098637e-20   4.248092e-05   3.2e-16 rad  1.1e-14 m
  run1   near_collinear  1.355063e+03 | 1.355063e+03   2.387610e+01   2.3e-12 rad  2.0e-10 m
  run1   bundle_thin     1.452694e-08 | 1.452665e-08   2.160967e+01   2.3e-12 rad  1.5e-13 m
  run1   thin_bundle     1.681655e+03 | 1.681655e+03   2.154383e+01   1.5e-13 rad  3.4e-12 m
"""
import contextlib
import os

import numpy as np
import pytest

import oracle_lib as orc  # noqa: F401  (the oracle runs inside test_pnp_ref's helpers)
import pnp_ref as ref
from gpu_kit import api, raw_bits as bits  # noqa: F401  (the fixture is found by name)
from test_pnp_ref import GUESS_R, GUESS_T, POSE_TOL_R, POSE_TOL_T, oracle_case, oracle_pipeline

pytestmark = pytest.mark.gpu

FORCED_LEAN = os.environ.get("SVO_FORCE_LEAN") == "1"

def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@contextlib.contextmanager
def device_errors_end_the_session(api):
    """a HIP error is no test failure to collect and move on from: nothing more is started on the device after one"""
    try:
        yield
    except api._lib.SvoError as e:
        pytest.exit("HIP error, session ended: %s" % e, 3)


def gpu_case(api, o, R0, t0):
    with device_errors_end_the_session(api):
        (inl, ok), R, t, iters = api.cameraToWorld(o["K"], o["cam"], o["world"], R0, t0, iterations=o["iters"])
    lean = bool(api.last_stage_path() & api._lib.PATH_LEAN)
    assert lean == (FORCED_LEAN and len(o["world"]) > 4), (o["name"], api.last_stage_path())     # P3P has one build
    return ok, R, t.reshape(3), inl, iters


STAGE_CASES = [(intr, name) for intr in ref.INTRINSICS for name in ref.cases(intr)]


# ------------------------------------------------------------------------------------------------ stage entry
@pytest.mark.parametrize("intr,name", STAGE_CASES, ids=["%s-%s" % c for c in STAGE_CASES])
def test_stage_case_against_the_oracle_and_the_reference(api, intr, name):
    o = oracle_case(name, intr)
    n = len(o["world"])
    ok, R, t, inl, iters = gpu_case(api, o, GUESS_R, GUESS_T)
    assert ok == o["ok"] and iters == o["iters_run"], (ok, o["ok"], iters, o["iters_run"])
    assert np.array_equal(inl, o["inl"]), (len(inl), len(o["inl"]))
    if not ok:
        assert len(inl) == 0 and np.array_equal(bits64(R), bits64(GUESS_R)) and np.array_equal(bits64(t), bits64(GUESS_T))
        return
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert np.all(np.diff(inl) > 0) and inl[0] >= 0 and inl[-1] < n
    ok2, R2, t2, inl2, iters2 = gpu_case(api, o, np.eye(3), np.zeros(3))                          # the guess is ignored
    assert ok2 and iters2 == iters and np.array_equal(inl2, inl)
    assert np.array_equal(bits64(R2), bits64(R)) and np.array_equal(bits64(t2), bits64(t))
    if name in ref.DIRECT_CASES:                                                                 # no refine: the tolerances of test_gpu_parity.py
        assert np.abs(R - o["R"]).max() < 1e-9 and np.abs(t - o["t"]).max() < (1e-8 if n == 4 else 1e-9)
        if name in ref.WELL_POSED_DIRECT:
            assert np.abs(R - o["R_true"]).max() < 2e-4 and np.abs(t - o["t_true"]).max() < 2e-3
        return
    dr, dt = ref.rot_angle(R, o["R"]), float(np.abs(t - o["t"]).max())
    if o["cls"] == "A":
        assert dr < POSE_TOL_R and dt < POSE_TOL_T, (dr, dt)
        Rm, tm, _, _, _ = ref.minimise(o["K"], R, t, o["X"], o["uv"])                            # from the HIP pose, on the inliers it returned
        assert ref.rot_angle(R, Rm) < POSE_TOL_R and np.abs(t - tm).max() < POSE_TOL_T, (ref.rot_angle(R, Rm), np.abs(t - tm).max())
    else:
        assert o["cls"] == "B"
        c_hip = ref.cost(o["K"], R, t, o["X"], o["uv"])
        d_hip, d_orc = c_hip - o["cost_min"], o["cost"] - o["cost_min"]
        print("class B %s %s: cost - cost* oracle %.6e | HIP %.6e (cost* %.6e); oracle <-> HIP %.3e rad %.3e m" % (intr, name, d_orc, d_hip, o["cost_min"], dr, dt))
        print("   oracle r|t", orc.rodrigues_to_vector(o["R"]).tolist(), o["t"].tolist())
        print("   HIP    r|t", orc.rodrigues_to_vector(R).tolist(), t.tolist())
        assert d_hip <= 2 * d_orc + 1e-9 * o["cost_min"], (d_hip, d_orc)


# ------------------------------------------------------------------------------------------------ frame pipeline
SCENES = tuple(ref.PIPE_SCENES)


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def check_frame(want, k, ok, T, stats, feats, tracks, tag):
    """run_both's bar (test_gpu_parity.py)"""
    ok_o, T_o, so, fo, to = want[k]
    assert bool(ok) == ok_o and stats == so, (tag, k, stats, so)
    assert not ok or np.isfinite(T).all(), (tag, k)
    assert np.array_equal(bits(feats[0]), bits(fo[0])) and np.array_equal(feats[1], fo[1]) and np.array_equal(feats[2], fo[2]), (tag, k)
    if k > 0:
        for key in ("pl0", "pr0", "pl1", "pr1"):
            assert np.array_equal(bits(to[key]), bits(tracks[key])), (tag, k, key)
        if so["fail_reason"] in (0, 3, 4) and so["n_after_bounds"] > 15:
            assert np.array_equal(bits(to["world"]), bits(tracks["world"])), (tag, k)
            assert np.array_equal(to["inlier"], tracks["inlier"]), (tag, k)
    assert np.abs(T[:3, 3] - T_o[:3, 3]).max() < POSE_TOL_T and rot_angle(T[:3, :3], T_o[:3, :3]) < POSE_TOL_R, (tag, k, T, T_o)


@pytest.mark.parametrize("scene", SCENES)
def test_pipeline_lone_context(api, scene):
    """B = 1: the first 32 hypotheses share a launch with the triangulation (k_tri_epnp); the 8 m wall needs 28, 25 and 85"""
    seq, P, want = oracle_pipeline(scene)
    g = api.VisualOdometry(cfg=api.default_config(**ref.PIPE_OVER)); g.initalize_projection_matricies(*P)
    try:
        for k in range(ref.PIPE_FRAMES):
            with device_errors_end_the_session(api):
                ok, T = g.stereo_callback(seq.left[k], seq.right[k])
            if k and not FORCED_LEAN and "SVO_TRI_EPNP_FUSED" not in os.environ:
                assert g.last_frame_path() & api._lib.PATH_TRI_EPNP_FUSED, (k, g.last_frame_path())
            check_frame(want, k, ok, T, g.stats.as_dict(), g.features(), g.last_tracks() if k else None, scene)
    finally:
        g.close()


def test_pipeline_nine_sequences_cycle_through_the_scenes(api):
    """B = 9: k_triangulate with the spare block, a first chunk of 16, and one k_pnp_decide launch whose neighbouring sequences
    need 1, about 25 and 85 hypotheses"""
    runs = [oracle_pipeline(s) for s in SCENES]
    B = 9
    g = api.BatchVisualOdometry(ref.PIPE_W, ref.PIPE_H, B, api.default_config(**ref.PIPE_OVER)); g.initalize_projection_matricies(*runs[0][1])
    try:
        for k in range(ref.PIPE_FRAMES):
            L = [runs[i % 4][0].left[k] for i in range(B)]; R = [runs[i % 4][0].right[k] for i in range(B)]
            with device_errors_end_the_session(api):
                ok, T = g.stereo_callback_batch(L, R)
            assert not g.last_frame_path() & api._lib.PATH_TRI_EPNP_FUSED
            for i in range(B):
                check_frame(runs[i % 4][2], k, ok[i], T[i], g.stats[i].as_dict(), g.features(i), g.last_tracks(i) if k else None, "%d %s" % (i, SCENES[i % 4]))
            if k:
                need = sorted({g.stats[i].as_dict()["ransac_iters"] for i in range(B)})
                assert need[0] == 1 and need[-1] > 16, need
    finally:
        g.close()
