"""The triangulation kernels (triangulate_point / svd4_null_vector in svo_kernels_pnp.hip) where real tracks sit and the other
suites do not: disparities of 2^-6 and 2^-12 px, zero and negative, vertical mismatch up to 5 px, points at and beyond the image
corners and at the principal point (where the fourth homogeneous coordinate is exactly zero and the `scale = 1` rule of
convertPointsFromHomogeneous applies), four calibrations — one of them without a baseline: sigma_4 = 0 for every pair there, and
at its seven pairs with d = dy = 0 sigma_3 = sigma_4 = 0 exactly, so only the stable order of the closing sort decides which row of
Vt is "last" (the calibrations with a baseline never come closer than sigma_3 = 16 sigma_4).  The fixture is
tests/triangulate_ref.py's.

  stage tests     svo_triangulate (k_triangulate, 16 lanes per wave) on the whole fixture and on prefixes around the 16- and
                  64-lane wave shapes, against the oracle bit for bit; then, without the oracle, against the f64 reference: the
                  residual of (x, y, z, 1) under the DLT matrix and the depth rule, with the bounds test_oracle_triangulate.py
                  derives.  test_gpu_shared_device_builds.py runs these again under SVO_FORCE_LEAN=1 (k_triangulate_lean); the
                  path bit each call reports is asserted here, so the child cannot pass on the wrong build.
  pipeline tests  a stereo pair whose right image IS the left image: every track reaches the triangulation with |d| <~ 0.1 px,
                  through a lone context (k_tri_epnp, 16 lanes) and a context of nine sequences (k_triangulate, 64 lanes,
                  spare block).
"""
import os

import numpy as np
import pytest

import oracle_lib as orc
import triangulate_ref as ref
from gpu_kit import api, raw_bits as bits  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6                         # as test_gpu_parity.py
PREFIXES = (1, 15, 16, 17, 63, 64, 65)  # the 16- and 64-lane wave shapes of triangulate_body and their neighbours
FORCED_LEAN = os.environ.get("SVO_FORCE_LEAN") == "1"


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


_full = {}


def stage_full(api, name):
    """(Pl, Pr, fixture, xyz of the whole fixture through svo_triangulate) — one GPU call per calibration for the whole file."""
    if name not in _full:
        Pl, Pr, f = ref.fixture(name)
        xyz = api.triangulatePoints(Pl, Pr, f["pl"], f["pr"])
        assert bool(api.last_stage_path() & api._lib.PATH_LEAN) == FORCED_LEAN, api.last_stage_path()
        xyz.setflags(write=False)
        _full[name] = (Pl, Pr, f, xyz)
    return _full[name]


# ------------------------------------------------------------------------------------------------ stage entry
@pytest.mark.parametrize("name", ["kitti", "run1", "general", "zero_baseline"])
def test_stage_equals_the_oracle_on_the_fixture_and_its_prefixes(api, name):
    Pl, Pr, f, full = stage_full(api, name)
    want, _ = orc.triangulate(Pl, Pr, f["pl"], f["pr"])
    diff = np.flatnonzero((bits(full) != bits(want)).any(1))
    assert len(diff) == 0, [(int(i), f["d"][i], f["dy"][i], int(f["pos"][i]), full[i].tolist(), want[i].tolist()) for i in diff[:5]]
    for n in PREFIXES:
        got = api.triangulatePoints(Pl, Pr, f["pl"][:n], f["pr"][:n])
        assert bool(api.last_stage_path() & api._lib.PATH_LEAN) == FORCED_LEAN, (n, api.last_stage_path())
        assert got.shape == (n, 3) and np.array_equal(bits(got), bits(full[:n])), n


@pytest.mark.parametrize("name", list(ref.WITH_BASELINE))
def test_stage_alone_against_the_f64_reference(api, name):
    """No oracle here.  v = (x, y, z, 1) of every finite result must leave the residual a correct null vector leaves (bound
    derived in test_oracle_triangulate.py).  A result the `Wh == 0` rule produced is a direction, not a point: it is the unit
    vector (X, Y, Z) itself, to be read with a fourth coordinate of 0 — such rows are recognised by their unit norm, must pass
    the same bound as (x, y, z, 0), and at least one exists (the principal point at zero disparity)."""
    Pl, Pr, f, xyz = stage_full(api, name)
    A = ref.dlt_matrix(Pl, Pr, f["pl"], f["pr"])
    sv = ref.singular_values(A)
    bound = ref.residual_bound(sv)
    finite = np.isfinite(xyz).all(1)
    print("%s: %d of %d results finite" % (name, finite.sum(), len(xyz)))
    assert finite.mean() > 0.95
    r1 = ref.residual(A, np.concatenate([xyz, np.ones((len(xyz), 1), np.float32)], 1))
    r0 = ref.residual(A, np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1))
    direction = finite & ~(r1 <= bound) & (np.abs(np.linalg.norm(xyz.astype(np.float64), axis=1) - 1) < 1e-6)
    print("%s: residual / bound max %.6f; rows returned as directions: %s" % (name, (r1 / bound)[finite & ~direction].max(), np.flatnonzero(direction).tolist()))
    assert direction.sum() >= 1 and (f["pos"][direction] == 2).all() and (f["d"][direction] == 0).all()
    bad = np.flatnonzero(finite & ~np.where(direction, r0 <= bound, r1 <= bound))
    assert len(bad) == 0, [(int(i), f["d"][i], f["dy"][i], int(f["pos"][i]), sv[i].tolist(), r1[i], xyz[i].tolist()) for i in bad[:5]]
    assert (sv[:, 2] > 100 * bound).mean() >= 0.60
    if name in ref.RECTIFIED:
        sel, d, tol = ref.depth_check(Pr, f)
        z = xyz[sel, 2].astype(np.float64)
        err = np.abs(z * d / -float(np.asarray(Pr).reshape(3, 4)[0, 3]) - 1)
        print("%s: depth error / allowed, max %.3f" % (name, (err / tol).max()))
        assert len(sel) == 35 and (err <= tol).all(), (err / tol).max()
        assert np.array_equal(np.sign(z), np.sign(d))


def test_stage_with_no_points_is_ok_and_writes_nothing(api):
    """svo_triangulate returns before any launch when n == 0: SVO_OK, the output untouched, NULL arrays accepted, no error left
    behind for the next call."""
    lib = api._lib.lib
    Pl, Pr, f, full = stage_full(api, "kitti")
    pl32, pr32 = np.ascontiguousarray(Pl, np.float32).reshape(12), np.ascontiguousarray(Pr, np.float32).reshape(12)
    sentinel = np.full((4, 3), -7.25, np.float32)
    pts = np.ascontiguousarray(f["pl"][:4])
    rc = lib.svo_triangulate(0, api.ptr(pl32), api.ptr(pr32), 0, api.ptr(pts), api.ptr(pts), api.ptr(sentinel))
    assert rc == api._lib.SVO_OK and (sentinel == -7.25).all()
    assert lib.svo_triangulate(0, api.ptr(pl32), api.ptr(pr32), 0, None, None, None) == api._lib.SVO_OK
    assert lib.svo_triangulate(0, api.ptr(pl32), api.ptr(pr32), -1, None, None, None) == api._lib.SVO_ERR_ARG
    empty = api.triangulatePoints(Pl, Pr, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert empty.shape == (0, 3)
    again = api.triangulatePoints(Pl, Pr, f["pl"][:17], f["pr"][:17])
    assert np.array_equal(bits(again), bits(full[:17]))


# ------------------------------------------------------------------------------------------------ frame pipeline
W, H, N_FRAMES = 320, 160, 3
OVER = dict(win_w=21, win_h=21, max_translation_norm=2.0)
SEEDS = (3, 21)


def zero_disparity_streams():
    """Per seed: (frames, what the oracle does on them per frame).  The right image is the left image."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=W, height=H, cx=W / 2.0, cy=H / 2.0)
    P = syn.projection_matrices(cal)
    out = []
    for seed in SEEDS:
        frames = syn.StereoSequence(cal=cal, n_frames=N_FRAMES, seed=seed, step=0.3).left
        o = orc.VisualOdometry(orc.default_config(**OVER)); o.initalize_projection_matricies(*P)
        per = []
        for k in range(N_FRAMES):
            ok, T = o.stereo_callback(frames[k], frames[k])
            st = {fl[0]: getattr(o.stats, fl[0]) for fl in o.stats._fields_}
            per.append((ok, T.copy(), st, [a.copy() for a in o.features()], o.last_tracks() if k else None))
        out.append((frames, per))
    return P, out


@pytest.fixture(scope="module")
def zero_disparity():
    return zero_disparity_streams()


def check_frame(P, want, k, ok, T, stats, feats, tracks, tag):
    ok_o, T_o, so, fo, to = want[k]
    assert bool(ok) == ok_o and stats == so, (tag, k, stats, so)
    assert np.array_equal(bits(feats[0]), bits(fo[0])) and np.array_equal(feats[1], fo[1]) and np.array_equal(feats[2], fo[2]), (tag, k)
    if k > 0:
        for key in ("pl0", "pr0", "pl1", "pr1"):
            assert np.array_equal(bits(to[key]), bits(tracks[key])), (tag, k, key)
        assert so["n_after_bounds"] > 15 and so["fail_reason"] in (0, 3, 4), (tag, k, so)          # the triangulation ran
        assert np.array_equal(bits(to["world"]), bits(tracks["world"])), (tag, k)
        again, _ = orc.triangulate(P[0], P[1], tracks["pl0"], tracks["pr0"])
        assert np.array_equal(bits(again), bits(tracks["world"])), (tag, k)
        assert np.array_equal(to["inlier"], tracks["inlier"]), (tag, k)
    if ok_o:
        assert np.abs(T[:3, 3] - T_o[:3, 3]).max() < POSE_TOL and rot_angle(T[:3, :3], T_o[:3, :3]) < POSE_TOL, (tag, k)


def test_zero_disparity_oracle_behaviour(zero_disparity):
    """What the docstrings below rely on, held on the oracle alone: frame 0 is the first frame (fail_reason 1); on frames 1 and 2
    hundreds of tracks reach the triangulation (seed 3: 447 and 644, seed 21: 416 and 599), all with |xl - xr| < 0.2 px, up to
    2 % of them exactly 0 and about half negative; NO world point is non-finite (0 %) — they are finite and huge (median |.|
    ~1e5 m, largest ~4e15 m), half of them behind the camera; RANSAC still finds a consensus of 370 - 540 "inliers" among them,
    and the motion gate (max_translation_norm = 2 m) then rejects the pose: fail_reason 4 on both frames, ok on none."""
    P, streams = zero_disparity
    for frames, per in streams:
        assert [p[2]["fail_reason"] for p in per] == [1, 4, 4] and not any(p[0] for p in per)
        for k in (1, 2):
            t = per[k][4]
            d = t["pl0"][:, 0].astype(np.float64) - t["pr0"][:, 0]
            assert len(d) == per[k][2]["n_after_bounds"] >= 50 and np.abs(d).max() < 0.2 and (d == 0).any() and (d < 0).any()
            assert np.isfinite(t["world"]).all() and np.abs(t["world"]).max() > 1e9
            assert per[k][2]["n_inliers"] > 100


def test_zero_disparity_lone_context(api, zero_disparity):
    """B = 1: the triangulation of all tracks shares a launch with the first EPnP chunk (k_tri_epnp, 16 tracks per wave), and
    the five points of each hypothesis are triangulated a second time inside it.  Oracle behaviour on this sequence:
    test_zero_disparity_oracle_behaviour."""
    P, streams = zero_disparity
    for s, (frames, want) in enumerate(streams):
        g = api.VisualOdometry(cfg=api.default_config(**OVER)); g.initalize_projection_matricies(*P)
        try:
            for k in range(N_FRAMES):
                ok, T = g.stereo_callback(frames[k], frames[k])
                if k and not FORCED_LEAN and "SVO_TRI_EPNP_FUSED" not in os.environ:
                    assert g.last_frame_path() & api._lib.PATH_TRI_EPNP_FUSED, (k, g.last_frame_path())
                check_frame(P, want, k, ok, T, g.stats.as_dict(), g.features(), g.last_tracks() if k else None, "lone %d" % s)
        finally:
            g.close()


def test_zero_disparity_many_sequence_context(api, zero_disparity):
    """B = 9: k_triangulate with 64 tracks per wave and the spare block that draws the RANSAC subsets; the sequences alternate
    between the two streams, so neighbouring grid rows hold different track counts."""
    P, streams = zero_disparity
    B = 9
    g = api.BatchVisualOdometry(W, H, B, api.default_config(**OVER)); g.initalize_projection_matricies(*P)
    try:
        for k in range(N_FRAMES):
            imgs = [streams[i % 2][0][k] for i in range(B)]
            ok, T = g.stereo_callback_batch(imgs, imgs)
            assert not g.last_frame_path() & api._lib.PATH_TRI_EPNP_FUSED
            for i in range(B):
                check_frame(P, streams[i % 2][1], k, ok[i], T[i], g.stats[i].as_dict(), g.features(i), g.last_tracks(i) if k else None, "many %d" % i)
    finally:
        g.close()
