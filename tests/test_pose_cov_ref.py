"""The numpy reference of the pose covariance (pose_cov_ref.py) against central differences of its own functions, so that the
definition in include/svo.h, the reference and the GPU tests built on it cannot drift apart: J against the residual function, G
against p -> (c, Log(R(p)t R_hat)), and the properties a covariance has."""
import numpy as np
import pytest

import pose_cov_ref as ref

POSES = {"small": ((0.01, -0.02, 0.015), (0.05, -0.02, 0.3)), "large": ((0.4, -0.7, 0.9), (-1.0, 0.5, 2.0)),
         "tiny_angle": ((3e-10, -2e-10, 1e-10), (0.02, 0.01, -0.1)), "identity": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))}
SIZES = (3, 15, 300)


def central(f, p, h):
    cols = []
    for k in range(len(p)):
        d = np.zeros(len(p)); d[k] = h
        cols.append((f(p + d) - f(p - d)) / (2 * h))
    return np.stack(cols, -1)


@pytest.fixture(scope="module", params=sorted(POSES))
def pose(request):
    return request.param


@pytest.mark.parametrize("m", SIZES)
def test_jacobian_matches_central_differences(pose, m):
    r, t = POSES[pose]
    K, world, img, R, t = ref.synthetic_points(m, 10 + m, r=r, t=t)
    K, X, u = K.astype(np.float64), world.astype(np.float64), img.astype(np.float64)
    p = np.concatenate([ref.log_so3(R), t])
    J = ref.jacobian(p, K, X)
    Jn = central(lambda q: ref.residuals(q, K, X, u).reshape(-1), p, 1e-6)
    # truncation h^2 |e'''| / 6 and rounding u |e| / h with |e| <= 2^11 px: both ~1e-7 of |J| at h = 1e-6
    assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max(), (np.abs(J - Jn).max(), np.abs(J).max())


def test_G_matches_central_differences(pose):
    r, t = POSES[pose]
    R, t = ref.exp_so3(np.asarray(r)), np.asarray(t, np.float64)
    p = np.concatenate([ref.log_so3(R), t])
    G = ref.G_matrix(p[:3], R, t)
    Gn = central(lambda q: ref.transform_params(q, R), p, 1e-5)
    assert np.abs(G - Gn).max() <= 1e-9 * max(1.0, np.abs(G).max()), np.abs(G - Gn).max()


def test_accumulating_rotates_both_blocks_by_the_pose_before(pose):
    """for pose = pose * T the increment's covariance maps with blockdiag(R_w, R_w) — no lever arm in p_w."""
    r, t = POSES[pose]
    R, t = ref.exp_so3(np.asarray(r)), np.asarray(t, np.float64)
    p = np.concatenate([ref.log_so3(R), t])
    R_w, p_w = ref.exp_so3(np.array([0.3, -1.1, 0.6])), np.array([40.0, -3.0, 30.0])
    M = np.block([[R_w, np.zeros((3, 3))], [np.zeros((3, 3)), R_w]])
    An = central(lambda q: ref.accumulated_params(q, R, R_w, p_w), p, 1e-5)
    A = M @ ref.G_matrix(p[:3], R, t)
    assert np.abs(A - An).max() <= 1e-8 * max(1.0, np.abs(A).max()), np.abs(A - An).max()      # rounding u |p_w| / h = 5e-10


def test_validity_rule_agrees_with_the_rank_of_J():
    """The reference's eigenvalue rule against a third view, the numerical rank of J itself, on singular and regular sets."""
    for n, seed in ((1, 1), (2, 2), (3, 3), (4, 4), (40, 5)):
        K, world, img, R, t = ref.synthetic_points(n, seed)
        for degenerate in (False, True):
            if degenerate:
                world[:] = world[0]
            p = np.concatenate([ref.log_so3(R), t])
            J = ref.jacobian(p, K.astype(np.float64), world.astype(np.float64), R)
            full = np.linalg.matrix_rank(J) == 6
            assert ref.pose_cov(K, world, img, None, R, t, ref.COV_FIXED_SIGMA)["valid"] == full, (n, degenerate)


@pytest.mark.parametrize("m", SIZES)
def test_covariances_are_symmetric_positive_definite(pose, m):
    r, t = POSES[pose]
    K, world, img, R, t = ref.synthetic_points(m, 20 + m, r=r, t=t)
    for mode in (ref.COV_RESIDUAL, ref.COV_FIXED_SIGMA):
        c = ref.pose_cov(K, world, img, None, R, t, mode, 0.7)
        if m == 3 and mode == ref.COV_RESIDUAL:                      # 2m - 6 = 0: no redundancy to estimate sigma from
            assert not c["valid"] and not c["cov_p"].any() and not c["cov_T"].any()
            continue
        assert c["valid"] and c["m"] == m
        for S in (c["cov_p"], c["cov_T"]):
            assert np.abs(S - S.T).max() <= 1e-9 * np.abs(S).max()
            assert np.linalg.eigvalsh(0.5 * (S + S.T)).min() > 0


@pytest.mark.parametrize("m", SIZES)
def test_fixed_unit_sigma_is_the_inverse_of_H(m):
    K, world, img, R, t = ref.synthetic_points(m, 30 + m)
    c = ref.pose_cov(K, world, img, None, R, t, ref.COV_FIXED_SIGMA, 1.0)
    assert c["valid"]
    assert np.array_equal(c["cov_p"], np.linalg.inv(c["H"]))
    e = c["cov_p"] @ c["H"] - np.eye(6)
    assert np.abs(e).max() <= 64 * c["kappa"] * 2.0 ** -53


def test_rank_deficient_sets_are_invalid():
    K, world, img, R, t = ref.synthetic_points(2, 5)
    for n in (1, 2):
        for mode in (ref.COV_RESIDUAL, ref.COV_FIXED_SIGMA):
            assert not ref.pose_cov(K, world[:n], img[:n], None, R, t, mode)["valid"]
    K, world, img, R, t = ref.synthetic_points(40, 6)
    world[:] = world[0]                                               # forty copies of one point: rank 2
    assert not ref.pose_cov(K, world, img, None, R, t, ref.COV_FIXED_SIGMA)["valid"]


def test_inlier_mask_selects_the_rows():
    K, world, img, R, t = ref.synthetic_points(64, 7)
    mask = np.zeros(64, bool); mask[::3] = True
    a = ref.pose_cov(K, world, img, mask, R, t, ref.COV_RESIDUAL)
    b = ref.pose_cov(K, world[mask], img[mask], None, R, t, ref.COV_RESIDUAL)
    assert a["valid"] and a["m"] == int(mask.sum()) and np.array_equal(a["cov_T"], b["cov_T"])
