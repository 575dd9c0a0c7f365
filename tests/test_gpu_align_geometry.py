"""svo_desc_index_align on a real GPU where the f64 part of rules 7 - 10 does the work — Horn's closed form, the 4 x 4 Jacobi, the
pick among equal eigenvalues, the refit's block-wide sums, the search for the best hypothesis — on the scenes of
tests/align_cases.py (geometry_scene) against the numpy reference (tests/align_ref.py); tests/test_gpu_align.py holds rules 1 - 5 and
one generic motion.

Well-posed scenes (a unique rotation) take the full comparison.  Each test first asserts the scene's conditions on the CPU, on the
reference alone: success, every row paired, no final residual within 10 % of inlier_dist of the threshold, and Horn's quaternion
(eigh) and the SVD Kabsch fit of the final inliers within 1e-7 rad and 1e-7 m of each other — a tenth of what is then asked of the
kernels: the sets and the counts to equality, the angle of R_gpu R_ref^T to 1e-6 rad, the two transforms' images of the inliers'
source centroid to 1e-6 m (t itself carries a harmless 1e-10 rad over 8 km in the far scenes), rms to 1e-6.  best_hypothesis,
best_count and refit_rounds_run to equality where the reference's margin over ALL hypotheses is above 1e-6.
Ill-posed scenes (a line, a point, two points) have no unique rotation: neither side is compared with the other, and the result is
held to rule 10's invariants, recomputed in f64 from the returned R and t (align_ref.check_model).

As measured on an MI355X (no kernel or header line changed for these tests; best_hypothesis equal on both sides everywhere):
  scene         n   the reference's margin, margin_final, disagreement (rad, m) | the library's dt (m), dR (rad), best_hypothesis
  identity     64  0.56     1     1.6e-16  0.0e+00  | 0        0        9
  identity    257  0.00034  0.64  6.7e-17  0.0e+00  | 0        8.94e-17 0
  pi_x         64  0.045    1     8.4e-16  2.2e-16  | 0        7.15e-16 5
  pi_x        257  7.8e-05  0.59  6.5e-16  0.0e+00  | 0        5.83e-16 0
  pi_y         64  0.22     1     1.7e-15  0.0e+00  | 0        1.27e-16 3
  pi_y        257  0.0046   0.67  3.6e-17  2.2e-16  | 0        1.6e-16  0
  pi_z         64  0.092    1     1.8e-16  0.0e+00  | 0        4.33e-17 16
  pi_z        257  3.7e-05  0.63  9.2e-17  0.0e+00  | 2.22e-16 3.16e-17 0
  pi_axis      64  1        1     2.3e-16  0.0e+00  | 1.78e-15 7.4e-16  0
  pi_axis     257  0.00039  0.61  4.2e-16  0.0e+00  | 0        1.82e-16 0
  near_pi      64  0.47     1     2.9e-16  0.0e+00  | 0        4.07e-16 1
  near_pi     257  0.016    0.7   2.5e-16  0.0e+00  | 0        5.2e-16  8
  perm         64  1        1     8.9e-16  0.0e+00  | 0        9.07e-16 3
  perm        257  0.005    0.65  4.1e-16  7.1e-15  | 0        5.03e-16 2
  quarter_z    64  0.07     1     3.8e-16  0.0e+00  | 0        4.2e-16  5
  quarter_z   257  0.0066   0.64  1.8e-16  2.2e-16  | 2.22e-16 1.92e-16 1
  tiny         64  0.95     1     1.9e-16  0.0e+00  | 0        1.62e-17 0
  tiny        257  0.6      1     1.3e-16  2.2e-16  | 4.44e-16 4.3e-17  1
  planar       64  0.034    1     2.9e-16  0.0e+00  | 0        2.84e-16 9
  planar      257  0.0035   0.66  1.9e-16  1.8e-15  | 0        4.32e-16 5
  planar_pi    64  0.52     1     4.7e-16  0.0e+00  | 0        2.55e-16 2
  planar_pi   257  0.0038   0.61  6.5e-16  0.0e+00  | 0        7.36e-16 9
  slab         64  1        1     8.7e-17  0.0e+00  | 0        3.44e-16 4
  slab        257  5.3e-05  0.64  5.5e-16  2.2e-16  | 0        7.9e-16  0
  far          64  0.31     0.99  1.1e-16  0.0e+00  | 0        2.29e-16 24
  far         257  0.0016   0.62  4.1e-16  0.0e+00  | 9.09e-13 2.08e-16 2
  far_planar   64  0.75     0.99  3.4e-16  0.0e+00  | 2.27e-13 4.98e-16 9
  far_planar  257  0.00078  0.59  5.9e-16  0.0e+00  | 9.17e-13 6.55e-16 3
  clumped      64  0.32     1     6.7e-16  0.0e+00  | 0        9.16e-16 2
  clumped     257  0.00065  0.63  1.5e-16  0.0e+00  | 0        3.04e-16 1
  far        4095  2.4e-05  0.56  1.5e-16  0.0e+00  | 1.02e-12 5.06e-16 5
  planar     4095  1.4e-06  0.57  4.4e-16  0.0e+00  | 4.44e-16 7.28e-16 17
  pi_axis    4095  1.3e-05  0.61  5.1e-16  0.0e+00  | 0        7.09e-16 10
The round trip: far (n 4095) comes back to 3.3e-7 rad and 2.8e-6 m at the centroid (half an ulp at 6.6 km: 2.4e-4 m), planar_pi
(n 257) to 5.1e-9 rad and 2.9e-8 m (half an ulp at 63 m: 1.9e-6 m)."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import align_ref as aref
from stereo_visual_odometry_amd import _lib, api

pytestmark = pytest.mark.gpu

T_TOL, R_TOL, RMS_TOL, DIS_TOL = 1e-6, 1e-6, 1e-6, 1e-7


def conditions(want, n):
    """the scene's conditions, on the reference alone: a scene that misses them is a bug in the scene"""
    assert want["success"] and want["n_pairs"] == n and want["margin_final"] > 0.1
    assert want["disagreement"][0] <= DIS_TOL and want["disagreement"][1] <= DIS_TOL


def check_against_reference(label, res, pairs, want, xyz, assert_best, assert_best_h=True):
    assert res.n_pairs == want["n_pairs"] and np.array_equal(pairs["src"], want["pair_src"]) and np.array_equal(pairs["dst"], want["pair_dst"])
    assert np.array_equal(pairs["inlier"], want["inlier"]) and res.n_inliers == want["n_inliers"] and res.success == want["success"]
    if want["success"]:
        c = np.asarray(xyz, np.float64)[want["pair_src"]][want["inlier"].astype(bool)].mean(0)
        dt, dr = float(np.linalg.norm(res.R @ c + res.t - (want["R"] @ c + want["t"]))), aref.rotation_angle(res.R, want["R"])
    else:                                             # rule 10: zeros
        assert not res.R.any() and not res.t.any() and not res.T.any() and res.rms == 0.0
        dt = dr = 0.0
    print("%s: dt %.3g m, dR %.3g rad, rms %.6g / %.6g, best_hypothesis %d (%d) / %d (%d), rounds %d / %d, margin %.3g, margin_final %.3g" % (
        label, dt, dr, res.rms, want["rms"], res.best_hypothesis, res.best_count, want["best_hypothesis"], want["best_count"],
        res.refit_rounds_run, want["refit_rounds_run"], want["margin"], want["margin_final"]))
    assert dt <= T_TOL and dr <= R_TOL and abs(res.rms - want["rms"]) <= RMS_TOL
    if assert_best:
        assert (res.best_count, res.refit_rounds_run) == (want["best_count"], want["refit_rounds_run"])
        if assert_best_h:
            assert res.best_hypothesis == want["best_hypothesis"]
    info = aref.check_model(res, pairs, xyz, ac.INLIER_DIST)
    assert info["n_band"] == 0                        # margin_final > 0.1, or margin > 1e-6: no pair is near the threshold
    return info


def result_bytes(res, pairs):
    return b"".join([np.array(res[:6], np.int64).tobytes(), res.R.tobytes(), res.t.tobytes(), res.T.tobytes(), np.float64(res.rms).tobytes(),
                     pairs["src"].tobytes(), pairs["dst"].tobytes(), pairs["inlier"].tobytes()])


# ---- 1. well-posed geometry
@pytest.mark.parametrize("name, n, share, H, sigma", ac.GEOMETRY_CASES)
def test_well_posed_geometry_against_the_reference(name, n, share, H, sigma):
    case, want = ac.geometry_scene(name, n, share, sigma), ac.geometry_reference(name, n, share, H, sigma)
    conditions(want, n)
    index = ac.build_index(api, case)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H)
    # clumped: many hypotheses draw a coincident or collinear triple, where the two sides may pick different rotations and count
    # differently; the winner is a generic one, but which h it is is printed, not asserted
    check_against_reference("%s n %d" % (name, n), res, pairs, want, case["xyz"], assert_best=want["margin"] > 1e-6, assert_best_h=name != "clumped")
    assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"])             # exactly the true inliers
    if name in ac.EXACT_R:
        # Without noise the least-squares rotation IS the exact matrix, to the f32 rounding of the points (1e-8 rad over 32
        # inliers).  With N(0, 5 mm) on 180 inliers it is not, for any estimator: it lies sigma / (17.3 m x sqrt(2 x 180)) = 1.5e-5
        # rad from it, the reference's f64 fit included, so there the library may be no further from the exact matrix than the
        # reference is, plus the 1e-6.
        E = np.array(ac.EXACT_R[name], np.float64)
        exact, exact_ref = aref.rotation_angle(res.R, E), aref.rotation_angle(want["R"], E)
        print("against the exact matrix: %.3g rad (the reference: %.3g rad)" % (exact, exact_ref))
        assert exact <= R_TOL + (exact_ref if sigma > 0 else 0.0)


@pytest.mark.parametrize("name, n, share, H, sigma", (("far", 4095, 0.6, 512, 0.005), ("planar_pi", 257, 0.3, 64, 0.005)))
def test_round_trip_through_transform_points(name, n, share, H, sigma):
    """align, move the source span by T, align again: the identity, with the same inliers.  The moved points are rounded to f32 — at
    8 km half an ulp is 0.5 mm a coordinate — and the least-squares fit of the inliers averages that: over 1638 inliers spread
    over +-30 m to some 3e-7 rad (tests/test_align_geometry_ref.py makes the same trip on the reference), which is why `far` makes
    the trip at its largest size.  At the centroid the fit is held to half an ulp of the largest moved coordinate."""
    case, want = ac.geometry_scene(name, n, share, sigma), ac.geometry_reference(name, n, share, H, sigma)
    conditions(want, n)
    index = ac.build_index(api, case)
    args = (case["src"], case["dst"], ac.INLIER_DIST)
    res, pairs = index.align(*args, min_pairs=3, hypotheses=H)
    check_against_reference("%s n %d" % (name, n), res, pairs, want, case["xyz"], assert_best=want["margin"] > 1e-6)
    assert index.transform_points(res.T, rows=case["src"]) == (n, 0)
    again, pairs2 = index.align(*args, min_pairs=3, hypotheses=H)
    moved = case["xyz"][pairs["src"]][pairs["inlier"].astype(bool)].astype(np.float64) @ res.R.T + res.t
    c, half_ulp = moved.mean(0), float(np.spacing(np.float32(np.abs(moved).max()))) / 2
    dr, dt = aref.rotation_angle(again.R, np.eye(3)), float(np.linalg.norm(again.R @ c + again.t - c))
    print("%s again: dR %.3g rad, at the centroid %.3g m (half an ulp at %.0f m: %.3g m)" % (name, dr, dt, np.abs(moved).max(), half_ulp))
    assert again.success and again.n_inliers == res.n_inliers and np.array_equal(pairs2["inlier"], pairs["inlier"])
    assert np.array_equal(pairs2["src"], pairs["src"]) and np.array_equal(pairs2["dst"], pairs["dst"])
    assert dr <= R_TOL and dt <= half_ulp
    orth = np.abs(again.R.T @ again.R - np.eye(3)).max()
    assert orth <= 1e-12 and abs(np.linalg.det(again.R) - 1) <= 1e-12 and np.array_equal(again.T[:3, :3], again.R)


# ---- 2. ill-posed geometry: invariants
@pytest.mark.parametrize("n", (64, 257))
@pytest.mark.parametrize("name", ac.ILL_POSED)
def test_ill_posed_geometry_keeps_the_invariants(name, n):
    case = ac.geometry_scene(name, n, 0.0, 0.0)
    index = ac.build_index(api, case)
    args = (case["src"], case["dst"], ac.INLIER_DIST)
    res, pairs = index.align(*args, min_pairs=3, hypotheses=16)                      # SVO_OK, or align raises
    info = aref.check_model(res, pairs, case["xyz"], ac.INLIER_DIST, min_pairs=3)
    print("%s n %d: n_inliers %d, best_hypothesis %d (%d), rounds %d, rms %.3g, %s" % (
        name, n, res.n_inliers, res.best_hypothesis, res.best_count, res.refit_rounds_run, res.rms, info))
    assert res.n_pairs == n and np.array_equal(pairs["src"], np.arange(n, 2 * n)) and info["n_band"] == 0
    assert res.success == (res.n_inliers >= 3) and res.n_inliers == int(pairs["inlier"].sum())
    if name != "needle":                              # any rotation of the top eigenspace maps a line onto its image
        assert res.n_inliers == n and res.success
    if name == "coincident":                          # a zero matrix, the Jacobi's immediate return, the first of equal eigenvalues
        cp, cq = case["xyz"][n].astype(np.float64), case["xyz"][0].astype(np.float64)
        assert res.R.tobytes() == np.eye(3).tobytes() and np.array_equal(res.t, cq - cp) and res.rms == 0.0
        assert (res.best_hypothesis, res.best_count, res.refit_rounds_run) == (0, n, 1)
    first = result_bytes(res, pairs)
    assert result_bytes(*index.align(*args, min_pairs=3, hypotheses=16)) == first
    index.chunk_rows = 1
    assert result_bytes(*index.align(*args, min_pairs=3, hypotheses=16)) == first


# ---- 3. kernel seams: the default motion on a uniform cloud
def seam_run(n, share, H, sigma, seed=0, inliers=None, **kw):
    case = ac.geometry_scene("default", n, share, sigma, seed, inliers)
    want = ac.geometry_reference("default", n, share, H, sigma, seed, inliers, **kw)
    return case, want, ac.build_index(api, case)


@pytest.mark.parametrize("name, n, share, H, sigma", ac.N_SEAMS)
def test_n_at_the_fit_kernels_strides(name, n, share, H, sigma):
    """n at 255, 256, 257 (k_align_fit's thread count) and 4095 (its last pair but one)"""
    case, want, index = seam_run(n, share, H, sigma)
    conditions(want, n)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H)
    check_against_reference("n %d" % n, res, pairs, want, case["xyz"], assert_best=want["margin"] > 1e-6)
    assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"])


def align_into_marked_outputs(index, params, n):
    """svo_desc_index_align into a result filled with 0x5A and lists filled with 77, 8 entries longer than the call may write"""
    r = _lib.SvoAlignResult()
    C.memset(C.byref(r), 0x5A, C.sizeof(r))
    ps, pd, pi = np.full(n + 8, 77, np.int32), np.full(n + 8, 77, np.int32), np.full(n + 8, 77, np.uint8)
    assert _lib.lib.svo_desc_index_align(index._h, C.byref(params), C.byref(r), _lib.ptr(ps), _lib.ptr(pd), _lib.ptr(pi)) == _lib.SVO_OK
    k = r.n_pairs
    assert 0 <= k <= n and (ps[k:] == 77).all() and (pd[k:] == 77).all() and (pi[k:] == 77).all()
    res = api.AlignResult(bool(r.success), k, r.n_inliers, r.best_hypothesis, r.best_count, r.refit_rounds_run,
                          np.array(r.R, np.float64).reshape(3, 3), np.array(r.t, np.float64), np.array(r.T, np.float64).reshape(4, 4), r.rms)
    return res, {"src": ps[:k].copy(), "dst": pd[:k].copy(), "inlier": pi[:k].copy()}


def test_h_at_the_score_and_fit_kernels_strides():
    """H at 1, 3, 4, 5 (k_align_score's four hypotheses a block) and 255, 256, 257, 1023 (k_align_fit's search), from the largest to
    the smallest on ONE index: the counts and models of every larger call are still in the device block.  In this scene hypothesis
    4 is the first that counts anything, so H <= 4 must fail with best_hypothesis 0 and count 0 — a call that read past its H
    would find 4's 33 — and H >= 5 must succeed with 4."""
    n, share, sigma = 65, 0.5, 0.0
    case = ac.geometry_scene("default", n, share, sigma, ac.H_SEAM_SEED)
    index = ac.build_index(api, case)
    for H in ac.H_SEAMS:
        want = ac.geometry_reference("default", n, share, H, sigma, ac.H_SEAM_SEED)
        assert want["n_pairs"] == n and want["margin"] > 1e-6 and want["margin_final"] > 0.1
        if H > ac.H_SEAM_FIRST:
            conditions(want, n)
        else:
            assert not want["success"] and want["best_count"] == 0
        p = api.DescriptorIndex.align_params(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H)
        res, pairs = align_into_marked_outputs(index, p, n)
        check_against_reference("H %d" % H, res, pairs, want, case["xyz"], assert_best=True)
        if H > ac.H_SEAM_FIRST:
            assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"]) and res.best_hypothesis == ac.H_SEAM_FIRST


@pytest.mark.parametrize("what, seed, best, tie", ac.LATE_WINNERS)
def test_late_winner(what, seed, best, tie):
    """the best hypothesis in slot 1, 2, 3 of k_align_fit's search and in its last wave, a later hypothesis tying its count"""
    n, share, H, sigma = ac.LATE
    case, want, index = seam_run(n, share, H, sigma, seed)
    conditions(want, n)
    assert want["margin"] > 1e-6 and want["best_hypothesis"] == best
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H)
    check_against_reference(what, res, pairs, want, case["xyz"], assert_best=True)
    assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"]) and res.best_hypothesis == best


@pytest.mark.parametrize("inliers, H, sigma", ac.ONE_PLACE)
def test_inliers_in_one_wave_or_one_slot(inliers, H, sigma):
    """n = 4096 with every inlier in the fit kernel's last wave (c % 256 >= 192: three of the four wave sums are zero in every refit
    round), or in ONE of every thread's 16 slots (15 are empty).  Slot 15 (c >= 3840) is drawn by none of the 1024 hypotheses, so
    there both sides end without a model, which is compared as it is; slot 13 is drawn by hypothesis 849 alone."""
    n = 4096
    case, want, index = seam_run(n, 0.0, H, sigma, 0, inliers)
    assert np.array_equal(want["pair_src"], np.arange(n, 2 * n)) and np.array_equal(~case["outlier"], ac.kept_pairs(inliers, n))
    if inliers == "slot15":
        assert not want["success"] and want["margin"] > 1e-6
    else:
        conditions(want, n)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H)
    check_against_reference(inliers, res, pairs, want, case["xyz"], assert_best=want["margin"] > 1e-6)
    if inliers != "slot15":
        assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"])


def test_success_boundary():
    """n_inliers exactly min_pairs: success; one below: failure, R, t, T and rms zero, everything else as before (rule 10)"""
    _, seed, best, _ = ac.LATE_WINNERS[0]
    n, share, H, sigma = ac.LATE
    k = 10
    case, at, index = seam_run(n, share, H, sigma, seed, min_pairs=k)
    above = ac.geometry_reference("default", n, share, H, sigma, seed, min_pairs=k + 1)
    conditions(at, n)
    assert at["n_inliers"] == k and 6 <= k <= 20 and at["margin"] > 1e-6 and not above["success"] and above["n_inliers"] == k
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=k, hypotheses=H)
    check_against_reference("min_pairs = n_inliers", res, pairs, at, case["xyz"], assert_best=True)
    assert res.success and res.n_inliers == k
    res2, pairs2 = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=k + 1, hypotheses=H)
    check_against_reference("min_pairs = n_inliers + 1", res2, pairs2, above, case["xyz"], assert_best=True)
    assert not res2.success and not res2.R.any() and not res2.t.any() and not res2.T.any() and res2.rms == 0.0
    assert res2[1:6] == res[1:6] and np.array_equal(pairs2["inlier"], pairs["inlier"])


def test_three_inliers_among_64():
    """the smallest set the refit fits: exactly the three pairs of hypothesis 700 are inliers"""
    n, H = 64, 1024
    case, want, index = seam_run(n, 0.0, H, 0.0, 0, "h700", min_pairs=3, refit_rounds=8)
    conditions(want, n)
    assert want["margin"] > 1e-6 and want["n_inliers"] == 3 and want["refit_rounds_run"] >= 1
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H, refit_rounds=8)
    check_against_reference("three inliers", res, pairs, want, case["xyz"], assert_best=True)
    assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"])


@pytest.mark.parametrize("rounds", (1, 8))
def test_refit_rounds(rounds):
    n, share, H, sigma = 257, 0.3, 64, 0.005
    case, want, index = seam_run(n, share, H, sigma, refit_rounds=rounds)
    conditions(want, n)
    res, pairs = index.align(case["src"], case["dst"], ac.INLIER_DIST, min_pairs=3, hypotheses=H, refit_rounds=rounds)
    check_against_reference("refit_rounds %d" % rounds, res, pairs, want, case["xyz"], assert_best=want["margin"] > 1e-6)
    assert np.array_equal(pairs["inlier"].astype(bool), ~case["outlier"])
