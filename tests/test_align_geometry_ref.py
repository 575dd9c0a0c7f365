"""The hard-geometry scenes of tests/align_cases.py (geometry_scene) and the additions to the reference (tests/align_ref.py: kabsch,
disagreement, check_model), without a GPU: every scene has the shape, the motion and the offset it is named for; every well-posed
case meets, on the reference alone, the conditions tests/test_gpu_align_geometry.py rests on (success, every row paired, no final
residual within 10 % of the threshold, the two f64 methods within 1e-7 rad and 1e-7 m of each other, exactly the true inliers); the
pinned seam scenes have the late winners, ties and empty places they were searched for; and check_model refuses a model that is
slightly wrong."""
import numpy as np
import pytest

import align_cases as ac
import align_ref as aref

DIS_TOL = 1e-7                                        # a tenth of what the GPU tests ask of the kernels


def ref_pairs(want):
    return dict(src=want["pair_src"], dst=want["pair_dst"], inlier=want["inlier"])


def meets_conditions(want, n):
    """the conditions of a well-posed case, on the reference alone"""
    return bool(want["success"] and want["n_pairs"] == n and want["margin_final"] > 0.1 and want["disagreement"] is not None
                and want["disagreement"][0] <= DIS_TOL and want["disagreement"][1] <= DIS_TOL)


def describe(want):
    return "margin %.3g, margin_final %.3g, disagreement %.3g rad %.3g m, best %d (%d), rounds %d, inliers %d" % (
        (want["margin"], want["margin_final"]) + (want["disagreement"] or (np.nan, np.nan)) +
        (want["best_hypothesis"], want["best_count"], want["refit_rounds_run"], want["n_inliers"]))


# ---- 1. the scenes are what they are named for
@pytest.mark.parametrize("n", (64, 257))
@pytest.mark.parametrize("name", list(ac.GEOMETRY))
def test_scene_has_its_shape_motion_and_offset(name, n):
    angle, axis, shift, cloud, offset = ac.GEOMETRY[name]
    case = ac.geometry_scene(name, n, 0.0, 0.0)
    P = case["xyz"][n:].astype(np.float64)
    s = np.linalg.svd(P - P.mean(0), compute_uv=False) / np.sqrt(n)
    (lo2, hi2), (lo3, hi3) = ac.SHAPE[cloud + "_far" if cloud == "plane" and offset else cloud]
    print(name, n, "extents", s)
    assert lo2 <= s[1] <= hi2 and lo3 <= s[2] <= hi3
    if cloud == "point":
        assert s[0] == 0.0 and (case["xyz"][n:] == case["xyz"][n]).all() and (case["xyz"][:n] == case["xyz"][0]).all()
    else:
        assert s[0] > 10.0
    if cloud == "two_points":
        assert len(np.unique(case["xyz"][n:], axis=0)) == 2 and abs(int((case["xyz"][n:] == case["xyz"][n]).all(1).sum()) - n / 2) <= 0.5
    if cloud == "clumped":
        _, counts = np.unique(case["xyz"][n:], axis=0, return_counts=True)
        assert sorted(counts)[-2:] == [int(round(0.3 * n)) // 2 + 1, (int(round(0.3 * n)) + 1) // 2 + 1]   # two points, their copies
    assert np.abs(P - offset).max() <= 62.0           # +-30 m about the offset; the line's y = 2 s + 1 reaches 61
    R = case["R"]
    assert abs(aref.rotation_angle(R, np.eye(3)) - angle) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() < 1e-15
    q0 = 0.5 * np.sqrt(max(0.0, 1.0 + np.trace(R)))
    assert abs(q0 - abs(np.cos(angle / 2))) <= 1e-7, q0                # 0 at a rotation by pi, 1 at the identity
    assert np.array_equal(case["t"], shift)
    if name in ac.EXACT_R:
        assert np.array_equal(R, np.array(ac.EXACT_R[name], np.float64))
    # the rows pair up one to one, as motion_scene's: pair c is source row n + c
    Q = case["xyz"][:n].astype(np.float64)
    ps, pd = aref.pairs(case["desc"], case["ids"], case["tags"], case["src"], case["dst"])
    assert np.array_equal(ps, np.arange(n, 2 * n)) and len(set(pd.tolist())) == n
    assert np.abs(P @ R.T + case["t"] - Q[pd]).max() <= np.spacing(np.float32(np.abs(Q).max()))   # and are the motion's images
    assert not case["xyz"].flags.writeable and not case["outlier"].flags.writeable


def test_the_scene_is_cached_and_the_lists_are_complete():
    assert ac.geometry_scene("far", 64, 0.5, 0.0) is ac.geometry_scene("far", 64, 0.5, 0.0)
    assert ac.geometry_reference("far", 64, 0.5, 128, 0.0) is ac.geometry_reference("far", 64, 0.5, 128, 0.0)
    assert sorted(ac.WELL_POSED + ac.ILL_POSED + ("default",)) == sorted(ac.GEOMETRY) and len(ac.WELL_POSED) == 15 and len(ac.ILL_POSED) == 4
    assert len(ac.GEOMETRY_CASES) == 33 and (ac.ANGLE, ac.AXIS, ac.SHIFT) == (0.7, (1.0, 2.0, 3.0), (12.0, -3.0, 40.0))
    assert np.array_equal(ac.rotation(ac.ANGLE, ac.AXIS), ac.true_motion()[0])


# ---- 2. every well-posed case meets its conditions
@pytest.mark.parametrize("name, n, share, H, sigma", ac.GEOMETRY_CASES + ac.N_SEAMS)
def test_well_posed_case_meets_its_conditions(name, n, share, H, sigma):
    case, want = ac.geometry_scene(name, n, share, sigma), ac.geometry_reference(name, n, share, H, sigma)
    print(name, n, share, H, sigma, describe(want))
    assert meets_conditions(want, n)
    assert np.array_equal(want["inlier"].astype(bool), ~case["outlier"])
    assert aref.rotation_angle(want["R"], case["R"]) < 1e-3
    c = case["xyz"][want["pair_src"]][want["inlier"].astype(bool)].astype(np.float64).mean(0)
    assert np.linalg.norm(want["R"] @ c + want["t"] - (case["R"] @ c + case["t"])) < 0.02
    if sigma == 0 and name != "clumped":
        assert want["margin"] > 1e-6                  # the cases whose best hypothesis the GPU tests assert
    if name in ac.EXACT_R:                            # the exact matrix is what a noise-free fit gives, and only that
        exact = aref.rotation_angle(want["R"], np.array(ac.EXACT_R[name], np.float64))
        print("against the exact matrix: %.3g rad" % exact)
        assert exact <= (1e-7 if sigma == 0 else 4 * sigma / (17.3 * np.sqrt(2 * want["n_inliers"])))
    info = aref.check_model(want, ref_pairs(want), case["xyz"], ac.INLIER_DIST, min_pairs=3)
    assert info["n_band"] == 0


@pytest.mark.parametrize("name, n, share, H, sigma", (("far", 4095, 0.6, 512, 0.005), ("planar_pi", 257, 0.3, 64, 0.005)))
def test_round_trip_on_the_reference(name, n, share, H, sigma):
    """the GPU test's round trip with the reference on both legs: the source points moved by T as transform_points moves them (f64,
    rounded to f32 once), fitted again on the same inliers -> the identity to 1e-6 rad, and at the inliers' centroid to half an ulp
    of the largest moved coordinate: what rounding the moved points leaves after a least-squares fit of that many pairs"""
    case, want = ac.geometry_scene(name, n, share, sigma), ac.geometry_reference(name, n, share, H, sigma)
    inl = want["inlier"].astype(bool)
    P, Q = case["xyz"][want["pair_src"]][inl].astype(np.float64), case["xyz"][want["pair_dst"]][inl].astype(np.float64)
    moved = (P @ want["R"].T + want["t"]).astype(np.float32)
    R, t = aref.horn(moved.astype(np.float64), Q)
    c = moved.astype(np.float64).mean(0)
    half_ulp = float(np.spacing(np.float32(np.abs(moved).max()))) / 2
    print(name, "angle %.3g rad, at the centroid %.3g m, half an ulp %.3g m" % (aref.rotation_angle(R, np.eye(3)), np.linalg.norm(R @ c + t - c), half_ulp))
    assert aref.rotation_angle(R, np.eye(3)) <= 1e-6 and np.linalg.norm(R @ c + t - c) <= half_ulp


# ---- 3. the ill-posed scenes: the reference runs through, and its own result keeps the invariants
@pytest.mark.parametrize("n", (64, 257))
@pytest.mark.parametrize("name", ac.ILL_POSED)
def test_ill_posed_scene_on_the_reference(name, n):
    case, want = ac.geometry_scene(name, n, 0.0, 0.0), ac.geometry_reference(name, n, 0.0, 16, 0.0)
    info = aref.check_model(want, ref_pairs(want), case["xyz"], ac.INLIER_DIST, min_pairs=3)
    print(name, n, describe(want), info)
    assert want["n_pairs"] == n and want["success"] and info["n_band"] == 0 and not case["outlier"].any()
    if name != "needle":
        assert want["n_inliers"] == n


# ---- 4. the pinned seam scenes
def test_h_seam_scene():
    n, share, sigma = 65, 0.5, 0.0
    case = ac.geometry_scene("default", n, share, sigma, ac.H_SEAM_SEED)
    clean = [h for h in range(1024) if not case["outlier"][aref.sample(h, n)].any()]
    assert clean[0] == ac.H_SEAM_FIRST == 4 and sorted(ac.H_SEAMS, reverse=True) == list(ac.H_SEAMS)
    for H in ac.H_SEAMS:
        want = ac.geometry_reference("default", n, share, H, sigma, ac.H_SEAM_SEED)
        print(H, describe(want))
        assert want["n_pairs"] == n and want["margin"] > 1e-6 and want["margin_final"] > 0.1
        if H > ac.H_SEAM_FIRST:
            assert meets_conditions(want, n) and (want["best_hypothesis"], want["best_count"]) == (4, 33)
            assert np.array_equal(want["inlier"].astype(bool), ~case["outlier"])
        else:                                         # no hypothesis below H counts a pair: the first stays, nothing is fitted
            assert not want["success"] and (want["best_hypothesis"], want["best_count"], want["n_inliers"], want["refit_rounds_run"]) == (0, 0, 0, 0)


def count_of(case, want, h):
    """rule 8's count of hypothesis h on the reference's pairs"""
    P, Q = case["xyz"][want["pair_src"]].astype(np.float64), case["xyz"][want["pair_dst"]].astype(np.float64)
    pick = aref.sample(h, len(P))
    R, t = aref.horn(P[pick], Q[pick])
    d = float(np.float32(ac.INLIER_DIST))
    return int((aref.residual2(R, t, P, Q) <= d * d).sum())


@pytest.mark.parametrize("what, seed, best, tie", ac.LATE_WINNERS)
def test_late_winner_scene(what, seed, best, tie):
    n, share, H, sigma = ac.LATE
    case, want = ac.geometry_scene("default", n, share, sigma, seed), ac.geometry_reference("default", n, share, H, sigma, seed)
    print(what, seed, describe(want))
    assert meets_conditions(want, n) and want["margin"] > 1e-6
    assert want["best_hypothesis"] == best and want["best_count"] == 10 == want["n_inliers"]
    assert best // 256 == int(what[4:]) if what.startswith("slot") else best % 256 >= 192
    assert best < tie < H and count_of(case, want, tie) == want["best_count"]       # "the smallest h at equal counts" decides
    assert all(count_of(case, want, h) < 10 for h in range(0, best, 7))             # and nothing early comes near (a sample of them)
    assert np.array_equal(want["inlier"].astype(bool), ~case["outlier"])


def test_the_sampler_reaches_wave_3_and_slot_13_and_never_slot_15():
    inside = lambda keep: [h for h in range(1024) if keep[aref.sample(h, 4096)].all()]
    wave3, slot15, slot13 = (inside(ac.kept_pairs(k, 4096)) for k in ("wave3", "slot15", "slot13"))
    assert wave3[0] == 103 and len([h for h in wave3 if h < 512]) >= 2 and slot15 == [] and slot13 == [849]
    assert ac.kept_pairs("slot15", 4096).sum() == 256 and (np.flatnonzero(ac.kept_pairs("slot15", 4096)) >= 3840).all()
    assert ac.kept_pairs("wave3", 4096).sum() == 1024 and ac.kept_pairs("h700", 64).sum() == 3


@pytest.mark.parametrize("inliers, H, sigma", ac.ONE_PLACE)
def test_one_place_scene(inliers, H, sigma):
    n = 4096
    case, want = ac.geometry_scene("default", n, 0.0, sigma, 0, inliers), ac.geometry_reference("default", n, 0.0, H, sigma, 0, inliers)
    print(inliers, describe(want))
    assert np.array_equal(want["pair_src"], np.arange(n, 2 * n))                    # pair c is source row n + c: the places are k_align_fit's
    assert np.array_equal(~case["outlier"], ac.kept_pairs(inliers, n)) and want["n_pairs"] == n
    if inliers == "slot15":
        # no hypothesis draws inside the slot: the best one is a chance hit, nothing is fitted, and the call fails.  Its model is no
        # map's, so some of 4096 residuals of metres fall near the threshold: the condition here is that none, in any hypothesis,
        # falls within 1e-6 of it, which is what equality of counts and flags needs
        assert not want["success"] and want["n_inliers"] < 3 and want["best_count"] < 3 and want["refit_rounds_run"] == 0 and want["margin"] > 1e-6
    else:
        assert meets_conditions(want, n) and np.array_equal(want["inlier"].astype(bool), ~case["outlier"])
        assert want["best_hypothesis"] == (103 if inliers == "wave3" else 849) and want["refit_rounds_run"] >= 1


def test_boundary_and_minimum_scenes():
    _, seed, best, _ = ac.LATE_WINNERS[0]
    n, share, H, sigma = ac.LATE
    at, above = (ac.geometry_reference("default", n, share, H, sigma, seed, min_pairs=k) for k in (10, 11))
    assert at["success"] and at["n_inliers"] == 10 and 6 <= at["n_inliers"] <= 20 and at["margin"] > 1e-6 and at["margin_final"] > 0.1
    assert not above["success"] and not above["R"].any() and not above["T"].any() and above["rms"] == 0.0
    for k in ("n_inliers", "best_hypothesis", "best_count", "refit_rounds_run"):
        assert at[k] == above[k]
    assert np.array_equal(at["inlier"], above["inlier"])
    three = ac.geometry_reference("default", 64, 0.0, 1024, 0.0, 0, "h700", min_pairs=3, refit_rounds=8)
    case = ac.geometry_scene("default", 64, 0.0, 0.0, 0, "h700")
    print("three inliers:", describe(three))
    assert meets_conditions(three, 64) and three["margin"] > 1e-6 and three["n_inliers"] == 3 == three["best_count"]
    assert three["best_hypothesis"] <= 700 and three["refit_rounds_run"] >= 1 and np.array_equal(three["inlier"].astype(bool), ~case["outlier"])


@pytest.mark.parametrize("rounds", (1, 8))
def test_refit_rounds_scene(rounds):
    want = ac.geometry_reference("default", 257, 0.3, 64, 0.005, refit_rounds=rounds)
    print(rounds, describe(want))
    assert meets_conditions(want, 257) and 1 <= want["refit_rounds_run"] <= rounds


# ---- 5. the two f64 methods on the existing scenes, and check_model's teeth
@pytest.mark.parametrize("n, share, H, sigma", ac.MOTION_CASES)
def test_kabsch_and_horn_agree_on_motion_scene(n, share, H, sigma):
    case, want = ac.motion_scene(n, share, sigma), ac.motion_reference(n, share, H, sigma)
    inl = want["inlier"].astype(bool)
    angle, dist = aref.disagreement(case["xyz"][want["pair_src"]][inl], case["xyz"][want["pair_dst"]][inl])
    print(n, "disagreement %.3g rad %.3g m" % (angle, dist))
    assert angle <= DIS_TOL and dist <= DIS_TOL


def test_check_model_refuses_a_model_that_is_slightly_wrong(monkeypatch):
    name, n, share, H, sigma = "planar", 64, 0.5, 128, 0.0
    case, want = ac.geometry_scene(name, n, share, sigma), ac.geometry_reference(name, n, share, H, sigma)
    pairs = ref_pairs(want)
    aref.check_model(want, pairs, case["xyz"], ac.INLIER_DIST, min_pairs=3)

    def with_R(R):
        T = want["T"].copy()
        T[:3, :3] = R
        return dict(want, R=R, T=T)
    bent = with_R(want["R"] + 1e-11 * np.arange(9).reshape(3, 3))                   # not orthonormal to 1e-12
    mirrored = with_R(want["R"] * np.array([1, 1, -1.0]))                           # det -1
    turned = with_R(ac.rotation(0.01, (0, 0, 1)) @ want["R"])                       # a rotation, but not this map's: 0.3 m at 30 m
    loose_T = dict(want, T=want["T"] + 1e-9)
    off_rms = dict(want, rms=want["rms"] + 1e-8)
    for bad in (bent, mirrored, turned, loose_T, off_rms):
        with pytest.raises(AssertionError):
            aref.check_model(bad, pairs, case["xyz"], ac.INLIER_DIST, min_pairs=3)
    flipped = want["inlier"].copy(); flipped[0] ^= 1
    with pytest.raises(AssertionError):
        aref.check_model(want, dict(pairs, inlier=flipped), case["xyz"], ac.INLIER_DIST, min_pairs=3)
    with pytest.raises(AssertionError):
        aref.check_model(want, pairs, case["xyz"], ac.INLIER_DIST, min_pairs=want["n_inliers"] + 1)
    # a pair inside the band may carry either flag, and is counted
    inl = want["inlier"].astype(bool)
    r = np.sqrt(aref.residual2(want["R"], want["t"], case["xyz"][pairs["src"]].astype(np.float64), case["xyz"][pairs["dst"]].astype(np.float64)))
    at = np.float32(r[~inl].min())                    # a threshold within f32 rounding (6e-8) of the nearest outlier's residual
    monkeypatch.setattr(aref, "BAND", 1e-6)           # and, for this check alone, a band that holds that
    for flag in (0, 1):
        flags = want["inlier"].copy(); flags[np.flatnonzero(~inl)[r[~inl].argmin()]] = flag
        k = int(flags.sum())
        rms = float(np.sqrt((r[flags.astype(bool)] ** 2).sum() / k))
        info = aref.check_model(dict(want, n_inliers=k, rms=rms), dict(pairs, inlier=flags), case["xyz"], at)
        assert info["n_band"] == 1
