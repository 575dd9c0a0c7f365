"""The pose covariance (svo.h, svo_set_pose_covariance) on a real GPU against its definition in numpy (pose_cov_ref.py): the stage
entry on synthetic point sets around every partition boundary of the kernel, the frame pipeline on its lone-stream and
many-sequence paths and with frames in flight, the rows of frames without a pose, and that switching it on moves nothing else.

Tolerance (derived, pose_cov_ref.tolerance): |cov_gpu - cov_ref|_F <= 8 (kappa2(H) (m + 64) + 2^20) 2^-53 |cov_ref|_F for cov_p and
cov_T alike; every compared case must have kappa2(H) <= 1e7 in the reference, asserted first."""
import ctypes as C
import os

import numpy as np
import pytest

import pose_cov_ref as ref
import pose_cov_child as child
from gpu_kit import api, calib, run_child  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = child.W, child.H
PC_THREADS = 256                  # k_pose_cov's block: thread v takes points v, v + 256, ...; n = 257 is the first second point
KAPPA_MAX = 1e7
MODES = {"residual": ref.COV_RESIDUAL, "fixed": ref.COV_FIXED_SIGMA}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else np.uint8)


def check_against_ref(got_p, got_T, got_valid, c, what):
    """c: pose_cov_ref.pose_cov's result for the same inputs."""
    assert bool(got_valid) == c["valid"], (what, got_valid, c["valid"], c["m"])
    if not c["valid"]:
        assert not np.asarray(got_p).any() and not np.asarray(got_T).any(), what
        return
    assert c["kappa"] <= KAPPA_MAX, (what, c["kappa"])
    tol = ref.tolerance(c["kappa"], c["m"])
    for name, g, r in (("cov_p", got_p, c["cov_p"]), ("cov_T", got_T, c["cov_T"])):
        err = np.linalg.norm(np.asarray(g) - r) / np.linalg.norm(r)
        print("%s %s m=%d kappa=%.3g err=%.3g tol=%.3g" % (what, name, c["m"], c["kappa"], err, tol))
        assert err <= tol, (what, name, err, tol)


# ---------------------------------------------------------------------------------------------------- 1. stage entry
def masks(n):
    """name -> inlier flags: holes, only the last point of the last wave, none"""
    rng = np.random.default_rng(n)
    holes = rng.random(n) < 0.6
    last = np.zeros(n, bool); last[-1] = True
    return {"all": None, "holes": holes, "last_only": last, "none": np.zeros(n, bool)}


STAGE_N = [1, 2, 3, 4, 63, 64, 65, PC_THREADS - 1, PC_THREADS, PC_THREADS + 1, 2 * PC_THREADS + 1]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", STAGE_N)
def test_stage_entry_matches_the_reference(api, n, mode):
    K, world, img, R, t = ref.synthetic_points(n, 100 + n)
    for name, mask in masks(n).items():
        cov_p, cov_T, valid = api.poseCovariance(K, img, world, R, t, inliers=mask, mode=mode, pixel_sigma=0.5)
        c = ref.pose_cov(K, world, img, mask, R, t, MODES[mode], 0.5)
        m = n if mask is None else int(mask.sum())
        if m < 3 or (m == 3 and mode == "residual"):
            assert not c["valid"], (n, name, mode)                   # singular H / no redundancy: the reference agrees by construction
        check_against_ref(cov_p, cov_T, valid, c, "n=%d %s %s" % (n, name, mode))
    assert api.last_stage_path() & api._lib.PATH_POSE_COV


def test_stage_entry_small_sets(api):
    """n = 1, 2: singular; n = 3: valid with a fixed sigma only."""
    K, world, img, R, t = ref.synthetic_points(3, 103)
    for n, mode, want in ((1, "residual", False), (1, "fixed", False), (2, "residual", False), (2, "fixed", False),
                          (3, "residual", False), (3, "fixed", True)):
        cov_p, cov_T, valid = api.poseCovariance(K, img[:n], world[:n], R, t, mode=mode)
        assert valid == want, (n, mode)
        assert cov_p.any() == want and cov_T.any() == want, (n, mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_stage_entry_all_far_points(api, mode):
    K, world, img, R, t = ref.synthetic_points(200, 7, depth=(30.0, 40.0))
    cov_p, cov_T, valid = api.poseCovariance(K, img, world, R, t, mode=mode, pixel_sigma=0.5)
    check_against_ref(cov_p, cov_T, valid, ref.pose_cov(K, world, img, None, R, t, MODES[mode], 0.5), "far " + mode)


def test_stage_entry_takes_the_index_list_of_camera_to_world(api):
    K, world, img, R, t = ref.synthetic_points(64, 9)
    mask = np.zeros(64, bool); mask[[0, 5, 6, 20, 41, 63]] = True
    a = api.poseCovariance(K, img, world, R, t, inliers=mask, mode="fixed")
    b = api.poseCovariance(K, img, world, R, t, inlier_indices=np.flatnonzero(mask), mode="fixed")
    assert a[2] and b[2] and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    with pytest.raises(ValueError):
        api.poseCovariance(K, img, world, R, t, inliers=mask, inlier_indices=[1, 2, 3])
    with pytest.raises(ValueError):
        api.poseCovariance(K, img, world, R, t, inlier_indices=[64])


def test_stage_entry_identity_pose(api):
    K, world, img, R, t = ref.synthetic_points(90, 8, r=(0, 0, 0), t=(0, 0, 0))
    cov_p, cov_T, valid = api.poseCovariance(K, img, world, np.eye(3), np.zeros(3), mode="residual")
    check_against_ref(cov_p, cov_T, valid, ref.pose_cov(K, world, img, None, np.eye(3), np.zeros(3), ref.COV_RESIDUAL), "identity")


# ---------------------------------------------------------------------------------------------------- 2. pipeline
@pytest.fixture(scope="module")
def frames():
    from stereo_visual_odometry_amd import synthetic as syn
    s = syn.StereoSequence(cal=calib(W, H), n_frames=5, seed=3, step=0.3)
    return list(s.left), list(s.right), syn.projection_matrices(calib(W, H))


def ref_of_frame(vo, i, T, Pl, mode, sigma=1.0):
    t = vo.last_tracks(i)
    R = T[:3, :3].T
    return ref.pose_cov(np.asarray(Pl, np.float32)[:3, :3], t["world"], t["pl1"], t["inlier"], R, -R @ T[:3, 3], mode, sigma)


def check_frame(vo, n_seq, ok, T, Pl, mode, sigma, what):
    cov_T, cov_p, valid = vo.last_pose_covariance()
    for i in range(n_seq):
        if not ok[i]:
            assert not valid[i] and not cov_T[i].any() and not cov_p[i].any(), (what, i)
            continue
        c = ref_of_frame(vo, i, T[i], Pl, mode, sigma)
        assert c["valid"], (what, i)
        check_against_ref(cov_p[i], cov_T[i], valid[i], c, "%s seq %d" % (what, i))
    return cov_T, cov_p, valid


def test_lone_stream_matches_the_reference(api, frames):
    L, R, (Pl, Pr) = frames
    vo = api.VisualOdometry(cfg=api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
    vo.set_pose_covariance("residual")
    n_ok = 0
    for k in range(4):
        ok, T = vo.stereo_callback(L[k], R[k])
        assert vo.last_frame_path() & api._lib.PATH_POSE_COV
        assert not ok or k > 0
        check_frame(vo, 1, [ok], [T], Pl, ref.COV_RESIDUAL, 1.0, "lone frame %d" % k)
        n_ok += ok
    assert n_ok >= 2
    vo.close()


def device_frames(L, R):
    import torch
    dev = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in zip(L, R)]
    torch.cuda.synchronize()
    return dev


def test_many_sequences_and_frames_in_flight(api, frames):
    """Ten sequences (the many-sequence path), synchronously against the reference; then the same frames with three submitted
    before the first collect: each collect's covariance is its own frame's, bit for bit."""
    L, R, (Pl, Pr) = frames
    B = 10
    dev = device_frames(L, R)                                           # the sequences differ by one frame of offset
    ptrs = lambda k, cam: [dev[(k + (i % 2)) % 5][cam].data_ptr() for i in range(B)]
    sync = []
    vo = api.BatchVisualOdometry(W, H, B, api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
    vo.set_pose_covariance("fixed", 0.5)
    for k in range(4):
        ok, T = vo.process_device(ptrs(k, 0), ptrs(k, 1), W)
        assert ok.any() == (k > 0)
        sync.append((ok, T) + check_frame(vo, B, ok, T, Pl, ref.COV_FIXED_SIGMA, 0.5, "many frame %d" % k))
    vo.close()
    vo = api.BatchVisualOdometry(W, H, B, api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
    vo.set_pose_covariance("fixed", 0.5)
    for k in range(3):
        vo.submit_device(ptrs(k, 0), ptrs(k, 1), W)
    for k in range(4):
        if k == 3:
            vo.submit_device(ptrs(3, 0), ptrs(3, 1), W)
        ok, T = vo.collect()
        got = vo.last_pose_covariance()
        assert np.array_equal(ok, sync[k][0]) and np.array_equal(bits(T), bits(sync[k][1])), k
        for a, b in zip(got, sync[k][2:]):
            assert np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b), k
    vo.close()


# ---------------------------------------------------------------------------------------------------- 3. failure rows
def assert_zero_rows(vo, rows):
    cov_T, cov_p, valid = vo.last_pose_covariance()
    for i in rows:
        assert not valid[i] and not cov_T[i].any() and not cov_p[i].any(), i


def test_failed_frames_give_zero_rows(api, frames):
    L, R, (Pl, Pr) = frames
    vo = api.VisualOdometry(cfg=api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
    vo.set_pose_covariance("residual")
    ok, _ = vo.stereo_callback(L[0], R[0])                              # the first frame
    assert not ok and vo.stats.fail_reason == 1
    assert_zero_rows(vo, [0])
    ok, _ = vo.stereo_callback(L[1], R[1])
    assert ok and vo.last_pose_covariance()[2][0]
    black = np.zeros_like(L[0])
    ok, _ = vo.stereo_callback(black, black)                            # a black pair
    assert not ok and 1 < vo.stats.fail_reason < 5
    assert_zero_rows(vo, [0])
    vo.close()
    gate = api.VisualOdometry(cfg=api.default_config(max_translation_norm=1e-9)); gate.initalize_projection_matricies(Pl, Pr)
    gate.set_pose_covariance("fixed", 1.0)
    gate.stereo_callback(L[0], R[0])
    ok, _ = gate.stereo_callback(L[1], R[1])                            # the motion gate
    assert not ok and gate.stats.fail_reason == 4
    assert_zero_rows(gate, [0])
    gate.close()


def test_masked_frames(api, frames):
    L, R, (Pl, Pr) = frames
    B = 10
    vo = api.BatchVisualOdometry(W, H, B, api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
    vo.set_pose_covariance("residual")
    vo.stereo_callback_batch([L[0]] * B, [R[0]] * B)
    act = np.array([i % 3 != 1 for i in range(B)])
    ok, T = vo.stereo_callback_batch([L[1] if a else None for a in act], [R[1] if a else None for a in act], active=act)
    assert ok[act].any() and not ok[~act].any()
    assert [s.fail_reason == 5 for s in vo.stats] == [not a for a in act]
    cov_T, cov_p, valid = check_frame(vo, B, ok, T, Pl, ref.COV_RESIDUAL, 1.0, "masked")
    assert np.array_equal(valid, ok)
    ok, T = vo.stereo_callback_batch([None] * B, [None] * B, active=np.zeros(B, bool))      # all idle: no launch at all
    assert not ok.any()
    assert_zero_rows(vo, range(B))
    vo.close()


# ---------------------------------------------------------------------------------------------------- 4. nothing else moves
def everything(vo, ok, T):
    f = vo.features(0); t = vo.last_tracks(0)
    st = vo.stats if not isinstance(vo.stats, list) else vo.stats[0]
    return [np.array([ok]), bits(np.asarray(T)), np.array(list(st.as_dict().values())), bits(f[0]), f[1], f[2]] + \
           [bits(t[k]) for k in ("pl0", "pr0", "pl1", "pr1", "world", "inlier")]


def test_mode_moves_nothing_else(api, frames):
    L, R, (Pl, Pr) = frames
    runs = {}
    for mode in ("off", "residual"):
        vo = api.VisualOdometry(cfg=api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
        vo.set_pose_covariance(mode)
        out = []
        for k in range(4):
            ok, T = vo.stereo_callback(L[k], R[k])
            assert bool(vo.last_frame_path() & api._lib.PATH_POSE_COV) == (mode != "off")
            out.append(everything(vo, ok, T))
        if mode == "off":
            rc = api.lib.svo_get_last_pose_covariance(vo._h, None, None, None)
            assert rc == api._lib.SVO_ERR_STATE
            with pytest.raises(api._lib.SvoError):
                vo.last_pose_covariance()
        runs[mode] = out
        vo.close()
    for a, b in zip(runs["off"], runs["residual"]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_mode_switches_with_frames_in_flight(api, frames):
    """on (residual), off, on (fixed) while the frames queue: each collected frame reports what it was issued with — the numbers
    of the same frames run one by one with the same modes, bit for bit."""
    L, R, (Pl, Pr) = frames
    dev = device_frames(L, R)
    one = lambda k, cam: [dev[k][cam].data_ptr()]
    modes = ["residual", "off", "fixed"]

    def context():
        vo = api.BatchVisualOdometry(W, H, 1, api.default_config(max_translation_norm=2.0)); vo.initalize_projection_matricies(Pl, Pr)
        vo.process_device(one(0, 0), one(0, 1), W)                      # the first frame, mode off
        return vo

    def covariance(vo, mode):
        if mode == "off":
            with pytest.raises(api._lib.SvoError):
                vo.last_pose_covariance()
            return None
        return vo.last_pose_covariance()

    vo = context()
    sync = []
    for k, mode in enumerate(modes):
        vo.set_pose_covariance(mode, 0.5)
        ok, T = vo.process_device(one(k + 1, 0), one(k + 1, 1), W)
        assert ok[0]
        if mode != "off":
            check_frame(vo, 1, ok, T, Pl, MODES[mode], 0.5, "one by one, " + mode)
        sync.append((T, covariance(vo, mode)))
    vo.close()
    assert not np.array_equal(sync[0][1][0], sync[2][1][0])
    vo = context()
    for k, mode in enumerate(modes):
        vo.set_pose_covariance(mode, 0.5)
        vo.submit_device(one(k + 1, 0), one(k + 1, 1), W)
        assert bool(vo.last_frame_path() & api._lib.PATH_POSE_COV) == (mode != "off")
    for k, mode in enumerate(modes):
        ok, T = vo.collect()
        assert ok[0] and np.array_equal(bits(T), bits(sync[k][0])), k
        got = covariance(vo, mode)
        if mode != "off":
            assert got[2][0]
            for a, b in zip(got[:2], sync[k][1][:2]):
                assert np.array_equal(bits(a), bits(b)), (k, mode)
    vo.close()


# ---------------------------------------------------------------------------------------------------- 5. graph and lean builds
@pytest.fixture(scope="module")
def launch_list_cases(api):
    assert not os.environ.get("SVO_GRAPH") and not os.environ.get("SVO_FORCE_LEAN")
    return child.run_cases()


@pytest.mark.parametrize("knob", ["SVO_GRAPH", "SVO_FORCE_LEAN"])
def test_graph_and_lean_builds_give_the_same_bits(launch_list_cases, knob, tmp_path):
    env = dict(os.environ)
    env.pop("SVO_GRAPH", None); env.pop("SVO_FORCE_LEAN", None)
    env[knob] = "1"
    out = str(tmp_path / "cases.npz")
    r = run_child("pose_cov_child.py", out, cwd=ROOT, env=env)
    assert "pose cov child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    from stereo_visual_odometry_amd import _lib
    bit = _lib.PATH_GRAPH if knob == "SVO_GRAPH" else _lib.PATH_LEAN
    for name in ("lone", "many", "stage"):
        assert launch_list_cases[name].any()
        assert np.array_equal(bits(got[name]), bits(launch_list_cases[name])), name
        if name != "stage" or knob == "SVO_FORCE_LEAN":
            assert (got[name + "_path"] & bit).all() and not (launch_list_cases[name + "_path"] & bit).any(), name
        assert (got[name + "_path"] & _lib.PATH_POSE_COV).all(), name


# ---------------------------------------------------------------------------------------------------- 6. errors
def test_errors(api):
    lib, ERR = api.lib, api._lib.SVO_ERR_ARG
    vo = api.BatchVisualOdometry(W, H, 1)
    for mode, sigma in ((3, 1.0), (-1, 1.0), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        assert lib.svo_set_pose_covariance(vo._h, mode, sigma) == ERR, (mode, sigma)
    assert lib.svo_set_pose_covariance(None, 1, 1.0) == ERR
    assert lib.svo_set_pose_covariance(vo._h, 1, float("nan")) == 0      # sigma is not looked at outside the fixed mode
    assert lib.svo_get_last_pose_covariance(vo._h, None, None, None) == api._lib.SVO_ERR_STATE      # nothing collected yet
    with pytest.raises(ValueError):
        vo.set_pose_covariance("sometimes")
    vo.close()
    lazy = api.VisualOdometry()                                         # no context yet: checked at once all the same
    for mode, sigma in ((3, 1.0), ("fixed", 0.0), ("fixed", float("nan"))):
        with pytest.raises(ValueError):
            lazy.set_pose_covariance(mode, sigma)
    lazy.set_pose_covariance("residual", float("nan"))
    K, world, img, R, t = ref.synthetic_points(8, 1)
    Rf, tf = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t)
    p = api.ptr
    call = lambda n, mode, sigma: lib.svo_pose_covariance(0, p(K.reshape(9)), n, p(img), p(world), None, p(Rf), p(tf), mode, sigma, None, None, None)
    assert call(0, 1, 1.0) == ERR and call(-1, 1, 1.0) == ERR
    assert call(8, 0, 1.0) == ERR and call(8, 3, 1.0) == ERR and call(8, 2, 0.0) == ERR and call(8, 2, float("nan")) == ERR
    assert call(8, 1, 1.0) == 0                                         # null outputs are allowed
    valid = C.c_int(-1)
    assert lib.svo_pose_covariance(0, p(K.reshape(9)), 8, p(img), p(world), None, p(Rf), p(tf), 2, 1.0, None, None, C.byref(valid)) == 0
    assert valid.value == 1
