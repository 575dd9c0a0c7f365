"""The numpy reference of the motion prior (tests/lk_prior_ref.py), checked on the CPU as far as it can be: its LK loop against the
oracle wherever the guess must not matter, pred and the host inverse against their definitions, and the precondition of the GPU
frame test (tests/test_gpu_motion_prior.py): on its scene the oracle, which has no prior, loses frame 1 for lack of tracks
(fail_reason 2), while the reference given the rotation homography keeps enough of them for a pose."""
import numpy as np
import pytest

import oracle_lib as orc
import lk_prior_cases as pc
import lk_prior_ref as ref

W, H = 320, 240


@pytest.mark.parametrize("win", [7, 10, 21])
@pytest.mark.parametrize("pair", ["turn", "stereo"])
def test_track_without_a_guess_and_with_the_points_is_the_oracle(pair, win):
    """init = None and init = pts: points, statuses, level visits and Newton steps of the oracle, bit for bit — on the turning
    pair (left 0 -> left 1: most tracks leave their levels) and on a stereo pair (left 1 -> right 1: most converge)"""
    A, B = (pc.levels(W, H, win, 0, 0), pc.levels(W, H, win, 1, 0)) if pair == "turn" else (pc.levels(W, H, win, 1, 0), pc.levels(W, H, win, 1, 1))
    rng = np.random.default_rng(win)
    pts = np.concatenate([pc.fast_points(W, H, 60), np.stack([rng.uniform(-3, W + 3, 20), rng.uniform(-3, H + 3, 20)], 1).astype(np.float32)])
    a = ref.same_as_oracle(A, B, pts, pc.MAX_LEVEL)
    b = ref.same_as_oracle(A, B, pts, pc.MAX_LEVEL, init=pts)
    assert a["steps"].sum() > 500 and 0 < a["status"].sum() < len(pts)
    assert np.array_equal(a["steps"], b["steps"]) and np.array_equal(a["visits"], b["visits"])


def test_a_guess_changes_the_track_and_the_template_stays():
    """the guess is not ignored: with the rotation homography more tracks end at status 1 where the scene says, in fewer steps"""
    P, G, kind = pc.track_case(W, H, 21)
    A, B = pc.levels(W, H, 21, 0, 0), pc.levels(W, H, 21, 1, 0)
    sel = kind == 0
    none, with_g = ref.track(A, B, P[sel], pc.MAX_LEVEL), ref.track(A, B, P[sel], pc.MAX_LEVEL, init=G[sel])
    near = lambda r: (r["status"] == 1) & (np.abs(r["next"] - G[sel]).max(1) < 4)        # ended within 4 px of the rotation's prediction
    assert near(with_g).sum() > 2 * near(none).sum() and near(with_g).sum() > 60, (near(with_g).sum(), near(none).sum())
    assert with_g["steps"].sum() < none["steps"].sum()
    assert np.array_equal(with_g["visits"] > 0, none["visits"] > 0)                     # the template (and its eigenvalue test) is the point's


def test_pred_of_the_identity_is_the_point_in_bits():
    """(a coordinate of -0.0 comes back as +0.0 — the sum with the zero product — which no later operation can tell apart)"""
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-50, 700, (200, 2)), [[0, 0], [1e-40, 5], [3e38, 1], [0.1, 0.7]]]).astype(np.float32)
    out, used = ref.pred_points(np.eye(3, dtype=np.float32), pts)
    assert used.all()
    assert np.array_equal(out.view(np.uint32), pts.view(np.uint32))


def test_pred_falls_back_to_the_point():
    p = np.array([[10.5, 20.25]], np.float32)
    for M in ([[1, 0, 0], [0, 1, 0], [0, 0, 0]], [[1, 0, 0], [0, 1, 0], [0, 0, -1]], [[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]],
              [[1, 0, 0], [0, 1, 0], [0, 0, np.nan]], [[3e38, 3e38, 0], [0, 1, 0], [0, 0, 1e-3]], [[1, 0, 0], [0, np.inf, 0], [0, 0, 1]]):
        out, used = ref.pred_points(np.array(M, np.float32), p)
        assert not used[0] and np.array_equal(out.view(np.uint32), p.view(np.uint32)), M
    out, used = ref.pred_points(np.array([[2, 0, 1], [0, 2, -1], [0, 0, 2]], np.float32), p)
    assert used[0] and out.tolist() == [[11.0, 19.75]]


def test_adjugate_inverse_of_a_rotation_homography():
    Pl, _ = pc.projections(W, H)
    K = Pl.reshape(3, 4)[:, :3].astype(np.float64)
    for k in (1, 2):
        R = pc.rotation(W, H, k)
        Hm, _ = pc.homography(W, H, k)
        want = K @ R.T @ np.linalg.inv(K)
        got = ref.adjugate_inverse(Hm).astype(np.float64)
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (k, np.abs(got - want).max())
    with pytest.raises(ValueError):
        ref.adjugate_inverse(np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], np.float32))


def oracle_frames(win, n):
    cfg = orc.default_config(**pc.over(win))
    o = orc.VisualOdometry(cfg); o.initalize_projection_matricies(*pc.projections(W, H))
    out = []
    for k in range(n):
        ok, _ = o.stereo_callback(pc.scene(W, H).left[k], pc.scene(W, H).right[k])
        out.append((ok, {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}))
    return out


def test_the_turn_loses_the_frame_without_a_prior_and_keeps_it_with_one():
    """Frame 1 of the GPU frame test's scene at w = 21 (measured when this was written: 6 tracks without the prior, 323 with it)"""
    win = 21
    cfg = orc.default_config(**pc.over(win))
    fr = oracle_frames(win, 2)
    assert fr[0][1]["fail_reason"] == 1 and fr[1][1]["fail_reason"] == 2, fr
    pts = pc.lk_input(pc.scene(W, H).left[0], cfg)
    assert len(pts) == fr[1][1]["n_into_lk"], (len(pts), fr[1][1]["n_into_lk"])
    assert fr[1][1]["n_after_bounds"] < cfg.features_threshold
    Hm, Hi = pc.homography(W, H, 1)
    c = pc.circular_cached(W, H, win, 1, pts, Hm, Hi, cfg)
    keep = c["ok"].astype(bool) & c["inb"]
    print("into LK %d; the oracle, no prior: %d after circular, %d after bounds; the reference with the prior: %d after circular, %d after bounds, "
          "%d Newton steps" % (len(pts), fr[1][1]["n_after_circular"], fr[1][1]["n_after_bounds"], c["ok"].sum(), keep.sum(), c["steps"]))
    assert keep.sum() >= cfg.features_threshold
    Pl, Pr = pc.projections(W, H)
    world, _ = orc.triangulate(Pl, Pr, pts[keep], c["pr0"][keep])
    ok, R, t, inl, _ = orc.camera_to_world(Pl.reshape(3, 4)[:, :3], c["pl1"][keep], world, np.eye(3), np.zeros(3), cfg.ransac_iterations,
                                           cfg.ransac_reprojection_error, cfg.ransac_confidence)
    assert ok and len(inl) >= cfg.features_threshold, (ok, len(inl))
    yaw = np.degrees(np.arctan2(R[0, 2], R[2, 2]))
    true = np.degrees(np.arctan2(pc.rotation(W, H, 1)[0, 2], pc.rotation(W, H, 1)[2, 2]))
    assert abs(yaw - true) < 0.5, (yaw, true)
