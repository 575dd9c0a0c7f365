"""The pose covariance of include/svo.h (svo_set_pose_covariance) in numpy f64, written from its definition: residuals
e_i = pi(R X_i + t) - u_i over the inliers, J = de/d(r, t) at the refined pose with a closed-form derivative of the exponential map
(Gallego & Yezzi 2015, not the kernel's dR/dr table), H = Jt J inverted by numpy.linalg.inv, cov_p = sigma^2 H^-1,
cov_T = G cov_p Gt with G the Jacobian of (c, phi) — T's translation column and the left perturbation of its rotation block —
with respect to (r, t).  Also the synthetic point sets the tests share."""
import numpy as np

COV_RESIDUAL, COV_FIXED_SIGMA = 1, 2
PIVOT_FLOOR = 2.0 ** -40          # svo.h: a Cholesky pivot counts when more than this fraction of its diagonal entry is left
ZED_K = np.array([[684.37, 0, 689.89], [0, 684.37, 406.87], [0, 0, 1]], np.float64)      # synthetic.ZED


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def exp_so3(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    K = hat(r)
    if th < 1e-9:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + 2 * np.sin(th / 2) ** 2 / th ** 2 * K @ K


def log_so3(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1)
    return v * (np.arctan2(s, c) / s if s > 1e-8 else 1.0)


def d_exp_so3(r):
    """[dR/dr_0, dR/dr_1, dR/dr_2] of R = exp([r]x): (r_k [r]x + [r x (I - R) e_k]x) R / theta^2; the generators at r = 0."""
    r = np.asarray(r, np.float64)
    th2 = r @ r
    if th2 < 1e-18:
        return [hat(e) for e in np.eye(3)]
    R = exp_so3(r)
    return [(r[k] * hat(r) + hat(np.cross(r, (np.eye(3) - R)[:, k]))) @ R / th2 for k in range(3)]


def right_jacobian(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    K = hat(r)
    if th < 1e-9:
        return np.eye(3) - 0.5 * K
    return np.eye(3) - 2 * np.sin(th / 2) ** 2 / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K


def residuals(p, K, X, u, R=None):
    """(m, 2): pi(R(r) X + t) - u;  R overrides R(p[:3]) (the pipeline's own matrix of the same rotation)."""
    R = exp_so3(p[:3]) if R is None else R
    Xc = X @ R.T + p[3:]
    return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1) - u


def jacobian(p, K, X, R=None):
    """(2m, 6), rows (ex_0, ey_0, ex_1, ...)."""
    R = exp_so3(p[:3]) if R is None else R
    dR = d_exp_so3(p[:3])
    Xc = X @ R.T + p[3:]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    fx, fy = K[0, 0], K[1, 1]
    dXc = [X @ dR[k].T for k in range(3)] + [np.tile(e, (len(X), 1)) for e in np.eye(3)]      # d Xc / d p_k, (m, 3) each
    J = np.zeros((len(X), 2, 6))
    for k in range(6):
        J[:, 0, k] = fx * (dXc[k][:, 0] / z - x * dXc[k][:, 2] / z ** 2)
        J[:, 1, k] = fy * (dXc[k][:, 1] / z - y * dXc[k][:, 2] / z ** 2)
    return J.reshape(-1, 6)


def transform_params(p, R_hat):
    """(c, phi) of the inverse transform at p: c = -R(p)t t, phi = Log(R(p)t R_hat)."""
    R = exp_so3(p[:3])
    return np.concatenate([-R.T @ p[3:], log_so3(R.T @ R_hat)])


def G_matrix(r, R, t):
    Jr = right_jacobian(r)
    c = -R.T @ t
    return np.block([[hat(c) @ Jr, -R.T], [-Jr, np.zeros((3, 3))]])


def positive_definite(H):
    """svo.h's pivot rule, decided WITHOUT a Cholesky factorisation (the kernel's recurrence is not restated here): with C = H
    scaled to a unit diagonal, pivot_k / H_kk = 1 / (C_k^-1)_kk >= lambda_min(C_k) >= lambda_min(C) for every leading block C_k
    (interlacing), so lambda_min(C) > 2^-40 implies every pivot passes, and a singular H has lambda_min(C) = O(2^-53) of either
    sign.  The two rules can only differ for lambda_min(C) within a factor 6 below the floor (1 / (C^-1)_kk <= 6 lambda_min):
    kappa ~ 1e11 and beyond, far from anything the tests compare (kappa <= 1e7) or expect to be singular."""
    d = np.diag(H)
    if not (d > 0).all():
        return False
    s = 1 / np.sqrt(d)
    return bool(np.linalg.eigvalsh(H * np.outer(s, s)).min() > PIVOT_FLOOR)


def accumulated_params(p, R_hat, R_w, p_w):
    """(position, left rotation perturbation) of the accumulated pose [R_w p_w] * T(p) about its value at R(p) = R_hat."""
    R = exp_so3(p[:3])
    return np.concatenate([p_w + R_w @ (-R.T @ p[3:]), log_so3(R_w @ R.T @ R_hat @ R_w.T)])


def pose_cov(K, world, img, inlier, R, t, mode, pixel_sigma=1.0):
    """-> dict(valid, cov_p, cov_T, kappa, m, H).  world (n, 3), img (n, 2): the f32 values widened; inlier: n flags or None;
    R, t: the cameraToWorld result.  Invalid: zeros and kappa = inf."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    sel = np.ones(len(world), bool) if inlier is None else np.asarray(inlier).astype(bool)
    X, u = np.asarray(world, np.float64)[sel], np.asarray(img, np.float64)[sel]
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    m = len(X)
    out = dict(valid=False, cov_p=np.zeros((6, 6)), cov_T=np.zeros((6, 6)), kappa=np.inf, m=m, H=None)
    if m < 3 or (mode == COV_RESIDUAL and 2 * m - 6 <= 0):
        return out
    p = np.concatenate([log_so3(R), t])
    J = jacobian(p, K, X, R)
    H = J.T @ J
    out["H"] = H
    if not positive_definite(H):
        return out
    e = residuals(p, K, X, u, R)
    s2 = (e ** 2).sum() / (2 * m - 6) if mode == COV_RESIDUAL else pixel_sigma ** 2
    cov_p = s2 * np.linalg.inv(H)
    G = G_matrix(p[:3], R, t)
    out.update(valid=True, cov_p=cov_p, cov_T=G @ cov_p @ G.T, kappa=np.linalg.cond(H))
    return out


def tolerance(kappa, m):
    """Relative Frobenius bound on cov_gpu - cov_ref: the normwise bound of inverting H (summation order m u, factorisation a
    small multiple of u, times kappa) plus the cancellation in the residuals (pixel coordinates up to 2^11, residuals down to 2^-2)."""
    return 8 * (kappa * (m + 64) + 2.0 ** 20) * 2.0 ** -53


def synthetic_points(n, seed, depth=(2.0, 40.0), noise=0.3, r=(0.01, -0.02, 0.015), t=(0.05, -0.02, 0.3)):
    """n world points in front of a ZED camera at pose (r, t), their projections with `noise` px of Gaussian noise, every value
    rounded through f32 as the stage entry takes them -> (K f32 (3, 3), world f32, img f32, R f64, t f64)."""
    rng = np.random.default_rng(seed)
    K = ZED_K
    R, t = exp_so3(np.asarray(r, np.float64)), np.asarray(t, np.float64)
    z = rng.uniform(depth[0], depth[1], n)
    px = np.stack([rng.uniform(40, 1880, n), rng.uniform(40, 1040, n)], 1)
    Xc = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1)
    world = ((Xc - t) @ R).astype(np.float32)                                         # R^t (Xc - t)
    img = (residuals(np.concatenate([log_so3(R), t]), K, world.astype(np.float64), np.zeros((n, 2)), R)
           + rng.normal(0, noise, (n, 2))).astype(np.float32)
    return K.astype(np.float32), world, img, R, t
