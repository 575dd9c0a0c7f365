"""A definitional f64 reference of what the pose stage (cameraToWorld: RANSAC over 5-point EPnP, then a refine on the inliers)
is FOR, next to its oracle parity tests: the pose that minimises the sum of squared reprojection errors over a given point set,
found by Gauss-Newton on (left-multiplied rotation increment, translation) run to a step of 1e-13 — not by the 20-step
Levenberg-Marquardt schedule of the oracle and the kernels — and RANSACUpdateNumIters as its definition reads.  Plain numpy;
nothing here knows the oracle or the library.

The second half builds the inputs of tests/test_pnp_ref.py (CPU: every input is proven fit on the oracle there) and
tests/test_gpu_pnp_edges.py: fixed-seed point sets at the counts, iteration bounds and geometries where the stage's kernels take
another path than on a comfortable scene.  case(name, intr) -> (K, world f32, cam f32, true R, true t, K_iters, expect).
"""
import os
import re
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DBL_MIN = float(np.finfo(np.float64).tiny)
CONFIDENCE = float(np.float32(0.98))          # the stage's default, as the f32 argument reaches the f64 formula
THRESHOLD = 8.0


# ------------------------------------------------------------------------------------------------ geometry
def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def rodrigues(r):
    """exp of the rotation vector r"""
    r = np.asarray(r, np.float64).reshape(3)
    th = float(np.linalg.norm(r))
    S = skew(r)
    if th < 1e-8:
        return np.eye(3) + S + 0.5 * S @ S
    return np.eye(3) + (np.sin(th) / th) * S + ((1 - np.cos(th)) / (th * th)) * S @ S


def rot_angle(Ra, Rb):
    """the angle of Ra^T Rb, from the antisymmetric part where that is the accurate one (small angles)"""
    D = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    c = 0.5 * (np.trace(D) - 1)
    return float(np.arctan2(s, c))


def project(K, R, t, X):
    K = np.asarray(K, np.float64).reshape(3, 3)
    Xc = np.asarray(X, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64).reshape(3)
    return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)


def residuals(K, R, t, X, uv):
    return (project(K, R, t, X) - np.asarray(uv, np.float64)).reshape(-1)


def cost(K, R, t, X, uv):
    """the sum of squared reprojection errors"""
    r = residuals(K, R, t, X, uv)
    return float(r @ r)


def apply_step(R, t, d):
    """pose after the increment d = (w, dt): R <- exp(w) R, t <- t + dt"""
    return rodrigues(d[:3]) @ np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3) + d[3:]


def jacobian(K, R, t, X):
    """d residuals / d (w, dt) at w = dt = 0, analytic: Xc' = exp(w) (R X) + t + dt, so dXc/dw = -[R X]x and dXc/dt = I"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    RX = np.asarray(X, np.float64) @ np.asarray(R, np.float64).T
    Xc = RX + np.asarray(t, np.float64).reshape(3)
    n = len(Xc)
    iz = 1.0 / Xc[:, 2]
    dp = np.zeros((n, 2, 3))                                   # d (u, v) / d Xc
    dp[:, 0, 0] = K[0, 0] * iz; dp[:, 0, 2] = -K[0, 0] * Xc[:, 0] * iz * iz
    dp[:, 1, 1] = K[1, 1] * iz; dp[:, 1, 2] = -K[1, 1] * Xc[:, 1] * iz * iz
    dw = np.zeros((n, 3, 3))                                   # -[R X]x
    dw[:, 0, 1] = RX[:, 2]; dw[:, 0, 2] = -RX[:, 1]
    dw[:, 1, 0] = -RX[:, 2]; dw[:, 1, 2] = RX[:, 0]
    dw[:, 2, 0] = RX[:, 1]; dw[:, 2, 1] = -RX[:, 0]
    J = np.concatenate([dp @ dw, dp], 2)
    return J.reshape(2 * n, 6)


def gn_step(K, R, t, X, uv):
    """the Gauss-Newton step at (R, t) by an SVD least-squares solve -> (d, cond(J))"""
    J = jacobian(K, R, t, X)
    r = residuals(K, R, t, X, uv)
    d, _, _, sv = np.linalg.lstsq(J, -r, rcond=None)
    cond = float(sv[0] / sv[-1]) if sv[-1] > 0 else float("inf")
    return d, cond


def remaining_step(K, R, t, X, uv):
    """How far (R, t) is from stationary: the first Gauss-Newton step from it -> (|w| rad, |dt| m, cond(J))."""
    d, cond = gn_step(K, R, t, X, uv)
    return float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:])), cond


def minimise(K, R, t, X, uv, max_iter=500, tol=1e-13):
    """Gauss-Newton with a Levenberg fallback from (R, t), until the step is below tol in rad and in m.
    -> (R, t, cost, (|w|, |dt|) of the last step, cond(J))."""
    R, t = np.asarray(R, np.float64).copy(), np.asarray(t, np.float64).reshape(3).copy()
    c = cost(K, R, t, X, uv)
    last, cond = (np.inf, np.inf), np.inf
    for _ in range(max_iter):
        d, cond = gn_step(K, R, t, X, uv)
        last = (float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:])))
        if last[0] < tol and last[1] < tol:
            break
        R1, t1 = apply_step(R, t, d)
        c1 = cost(K, R1, t1, X, uv)
        if not c1 <= c:                                        # Levenberg: damp until the cost stops rising
            J = jacobian(K, R, t, X); r = residuals(K, R, t, X, uv)
            A, g = J.T @ J, J.T @ r
            lam, found = 1e-6, False
            while lam < 1e12:
                dd = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
                R1, t1 = apply_step(R, t, dd)
                c1 = cost(K, R1, t1, X, uv)
                if c1 < c:
                    found = True
                    break
                lam *= 10
            if not found:                                      # no descent left in f64: this is the minimum to rounding
                break
        R, t, c = R1, t1, c1
    return R, t, c, last, cond


def iterations_needed(confidence, n, good, K):
    """RANSACUpdateNumIters(confidence, ep = (n - good) / n, model_points = 5, max_iters = K) as its definition reads
    -> (iterations, distance of log(1-p) / log(1 - (1-ep)^5) from the nearest half-integer: where that is ~0, the rounding of
    rint is not decided by f64 and two correct implementations may differ by one)."""
    p = min(max(float(confidence), 0.0), 1.0)
    ep = min(max((n - good) / float(n), 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** 5
    if denom < DBL_MIN:
        return 0, 0.5
    num, denom = np.log(num), np.log(denom)
    if denom >= 0 or -num >= K * (-denom):
        return int(K), 0.5
    q = float(num / denom)
    return int(np.rint(q)), abs(abs(q - np.floor(q)) - 0.5)


# ------------------------------------------------------------------------------------------------ intrinsics
KITTI00_K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float64)


def run1_K():
    """camera_matrix of tests/golden/camera_info_left.yaml (fx != fy)"""
    with open(os.path.join(HERE, "golden", "camera_info_left.yaml")) as f:
        m = re.search(r"camera_matrix:.*?data:\s*\[([^\]]*)\]", f.read(), re.S)
    return np.array([float(v) for v in m.group(1).split(",")], np.float64).reshape(3, 3)


INTRINSICS = ("kitti", "ident", "run1")


def intrinsics(intr):
    """-> (K, px): px is how many of this camera's image units one KITTI-00 pixel is (noise and outlier offsets scale with it).
    ident: K = I and normalised image coordinates, as the reference's own known-answer test; the 8-"pixel" threshold admits
    everything there."""
    K = {"kitti": KITTI00_K, "ident": np.eye(3), "run1": run1_K()}[intr]
    return K, K[0, 0] / KITTI00_K[0, 0]


# ------------------------------------------------------------------------------------------------ case builders
MILD_R, MILD_T = (0.01, -0.02, 0.005), (0.05, -0.02, -0.6)


# Cases whose seed had to be chosen to keep a condition tests/test_pnp_ref.py sets (the name alone seeds every other case).
# A refine that is still moving when it reaches its 20th step, but has nearly arrived, is rare: most thin bundles either converge
# in a few steps or stall hundreds of metres away.  The three seeds below were found by search, on the oracle.
SEEDS = {"near_collinear": 1, "bundle_thin": 23, "pencil_far": 71,
         "thin_bundle": zlib.crc32(b"thin_bundle#1"),          # by its name it converges (class A) under KITTI-00 and run1
         "p3p_collinear3": zlib.crc32(b"p3p_collinear3#10")}   # 0 / 0 in the P3P: most seeds fail under one camera, "succeed" under another


def _seed(name):
    return SEEDS.get(name, zlib.crc32(name.encode()))


def _cloud(rng, n, x=15.0, y=3.0, z=(6.0, 60.0)):
    return np.stack([rng.uniform(-x, x, n), rng.uniform(-y, y, n), rng.uniform(z[0], z[1], n)], 1)


def _finish(intr, rng, world, rvec, tvec, K_iters, expect, outliers=0.0, noise=0.2):
    """world (f64) -> the case tuple: f32 world points, their f32 projections under (rvec, tvec) with `noise` KITTI pixels of
    Gaussian noise, a fraction `outliers` of them moved by up to 80 KITTI pixels."""
    K, px = intrinsics(intr)
    R, t = rodrigues(rvec), np.asarray(tvec, np.float64)
    world = world.astype(np.float32)
    cam = project(K, R, t, world)
    n = len(world)
    cam = cam + rng.normal(0, 1, cam.shape) * (noise * px)
    bad = rng.random(n) < outliers
    cam[bad] += rng.uniform(-80, 80, (int(bad.sum()), 2)) * px
    return K.astype(np.float32), world, cam.astype(np.float32), R, t, K_iters, expect


def _small(rng, n):
    """n points of the small well-posed scene of the direct branches (as test_gpu_parity.py's): 4-9 m deep, +-2 m wide"""
    return np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1)


SMALL_R, SMALL_T = (0.12, -0.2, 0.07), (0.2, -0.1, 1.1)

RANSAC_CASES = (
    ["mild", "wall_slanted", "wall_frontal", "ground_plane", "far", "near", "rot_1rad_behind", "rot_pi", "rot_near_pi", "behind_40",
     "zero_motion_exact", "near_collinear", "bundle_thin", "thin_bundle", "narrow_fov_far", "pencil_far", "duplicates_12x25", "few_6", "few_7", "few_8", "few_16"]
    + ["n_%d" % n for n in (255, 256, 257, 511, 512, 513, 2047, 2048, 2049)]
    + ["iters_%d" % k for k in (1, 2, 15, 16, 17, 31, 32, 33, 100)]
    + ["outliers_90", "all_outliers"])
DIRECT_CASES = ["p3p_mild", "p3p_coplanar", "p3p_rot_pi", "p3p_duplicate", "p3p_collinear3",
                "e5_mild", "e5_coplanar", "e5_rot_pi", "e5_duplicate"]
CASES = RANSAC_CASES + DIRECT_CASES
# expect: "pose" = succeeds and the true pose is recovered; "ok" = succeeds (the pose is held to the reference minimum, not to
# the truth: too few inliers, too few hypotheses or an ill-posed set); "fail" = no consensus, R and t untouched;
# "nonfinite" = the solve's own arithmetic breaks down: a failure by the finite-pose rule (orc.h)
# K-bound and outlier cases say nothing where the threshold admits every point
IDENT_LEFT_OUT = tuple(c for c in RANSAC_CASES if c.startswith("iters_")) + ("outliers_90", "all_outliers")


def cases(intr):
    return [c for c in CASES if not (intr == "ident" and c in IDENT_LEFT_OUT)]


WELL_POSED_DIRECT = ("p3p_mild", "p3p_coplanar", "p3p_rot_pi", "e5_mild", "e5_rot_pi")


def case(name, intr="kitti"):
    rng = np.random.default_rng(_seed(name))
    fin = lambda *a, **k: _finish(intr, rng, *a, **k)
    n = 300
    if name == "mild":
        return fin(_cloud(rng, n), MILD_R, MILD_T, 100, "pose")
    if name == "wall_slanted":
        w = _cloud(rng, n); w[:, 2] = 20 + 0.5 * w[:, 0]
        return fin(w, MILD_R, MILD_T, 100, "pose")
    if name == "wall_frontal":                                  # exactly planar: every 5-point EPnP hypothesis is useless
        w = _cloud(rng, n); w[:, 2] = 20
        return fin(w, MILD_R, MILD_T, 100, "fail")
    if name == "ground_plane":
        w = _cloud(rng, n); w[:, 1] = 1.65
        return fin(w, MILD_R, MILD_T, 100, "fail")
    if name == "far":
        return fin(_cloud(rng, n, 80, 20, (200, 400)), MILD_R, MILD_T, 100, "ok")
    if name == "near":
        return fin(_cloud(rng, n, 1.5, 0.5, (1.5, 4)), MILD_R, (0.05, -0.02, -0.3), 100, "pose")
    if name == "rot_1rad_behind":                               # points all around the camera; those behind it project too
        w = rng.uniform(-30, 30, (4 * n, 3))
        R, t = rodrigues((0, 1.0, 0)), np.asarray(MILD_T)
        z0, z1 = w[:, 2], (w @ R.T + t)[:, 2]
        w = w[(np.abs(z0) > 3) & (np.abs(z1) > 3)][:n]
        return fin(w, (0, 1.0, 0), MILD_T, 100, "pose")
    if name == "rot_pi":
        return fin(_cloud(rng, n), (0, 0, np.pi), MILD_T, 100, "pose")
    if name == "rot_near_pi":
        a = np.array([0.05, 0.03, 1.0]); a *= 3.1 / np.linalg.norm(a)
        return fin(_cloud(rng, n), a, (0.05, -0.02, 2.0), 100, "pose")
    if name == "behind_40":                                     # 40 of 300 points with negative depth, before and after
        w = _cloud(rng, n); w[:40, 2] = -w[:40, 2]
        return fin(w, MILD_R, MILD_T, 100, "pose")
    if name == "zero_motion_exact":                             # R = I, t = 0 and no noise: the refine starts at |param| ~ 0
        return fin(_cloud(rng, n), (0, 0, 0), (0, 0, 0), 100, "pose", noise=0.0)
    if name in ("near_collinear", "bundle_thin"):               # a fan in the plane x = 0.3 z, 0.002 (0.001) rad wide about y = 0.1 z
        z = rng.uniform(6, 60, n); s = 0.001 if name == "near_collinear" else 0.0005
        w = np.stack([0.3 * z, (0.1 + rng.uniform(-s, s, n)) * z, z], 1)
        return fin(w, MILD_R, MILD_T, 100, "ok")
    if name == "thin_bundle":                                   # a bundle of 5 cm about the ray x = 0.3 z, y = 0.1 z
        z = rng.uniform(6, 60, n)
        w = np.stack([0.3 * z, 0.1 * z + rng.uniform(-0.05, 0.05, n), z], 1)
        return fin(w, MILD_R, MILD_T, 100, "ok")
    if name in ("narrow_fov_far", "pencil_far"):                # a 4 (0.2) degree field of view at 150-160 m
        z = rng.uniform(150, 160, n); h = np.tan(np.deg2rad(2.0 if name == "narrow_fov_far" else 0.1))
        w = np.stack([rng.uniform(-h, h, n) * z, rng.uniform(-h, h, n) * z, z], 1)
        return fin(w, MILD_R, MILD_T, 100, "ok")
    if name == "duplicates_12x25":                              # 12 distinct correspondences, each 25 times
        K, w, c, R, t, it, e = fin(_cloud(rng, 12), MILD_R, MILD_T, 100, "ok")
        idx = rng.permutation(np.repeat(np.arange(12), 25))
        return K, np.ascontiguousarray(w[idx]), np.ascontiguousarray(c[idx]), R, t, it, e
    if name.startswith("few_"):
        return fin(_cloud(rng, int(name[4:])), MILD_R, MILD_T, 100, "pose")
    if name.startswith("n_"):
        return fin(_cloud(rng, int(name[2:])), MILD_R, MILD_T, 100, "pose", outliers=0.3)
    if name.startswith("iters_"):
        k = int(name[6:])
        return fin(_cloud(rng, 200), MILD_R, MILD_T, k, "fail" if k == 1 else "ok", outliers=0.5)
    if name == "outliers_90":
        return fin(_cloud(rng, n), MILD_R, MILD_T, 1000, "ok", outliers=0.9)
    if name == "all_outliers":                                  # image points that have nothing to do with the world points
        K, w, c, R, t, it, e = fin(_cloud(rng, 200), MILD_R, MILD_T, 100, "fail")
        c = (project(K, np.eye(3), np.zeros(3), _cloud(rng, 200))).astype(np.float32)
        return K, w, c, R, t, it, e
    # ---- the direct branches: n = 4 is one P3P, n = 5 one EPnP; no noise (no refine follows)
    if name in ("p3p_mild", "e5_mild"):
        return fin(_small(rng, 4 if name[0] == "p" else 5), SMALL_R, SMALL_T, 100, "pose", noise=0.0)
    if name in ("p3p_coplanar", "e5_coplanar"):                 # exactly coplanar in f32: z = 6 (P3P is at home there)
        w = _small(rng, 4 if name[0] == "p" else 5); w[:, 2] = 6
        return fin(w, SMALL_R, SMALL_T, 100, "pose" if name[0] == "p" else "nonfinite", noise=0.0)
    if name in ("p3p_rot_pi", "e5_rot_pi"):
        return fin(_small(rng, 4 if name[0] == "p" else 5), (0, 0, np.pi), SMALL_T, 100, "pose", noise=0.0)
    if name in ("p3p_duplicate", "e5_duplicate"):               # two equal correspondences
        w = _small(rng, 4 if name[0] == "p" else 5); w[-1] = w[1]
        return fin(w, SMALL_R, SMALL_T, 100, "ok", noise=0.0)
    if name == "p3p_collinear3":                                # the triangle of the P3P has no area
        w = np.round(_small(rng, 4) * 64) / 64                 # multiples of 1/64: the quarter point is exact in f32 too
        w[2] = w[0] + 0.25 * (w[1] - w[0])
        return fin(w, SMALL_R, SMALL_T, 100, "fail", noise=0.0)
    raise KeyError(name)


def classify(step_r, step_t, cond):
    """A: the pose is stationary (the remaining Gauss-Newton step is at most 1e-7 rad and m); B: it is not, on an ill-conditioned
    problem (cond(J) >= 1e3), where a 20-step Levenberg-Marquardt schedule may stop in a flat valley; anything else: None."""
    if step_r <= 1e-7 and step_t <= 1e-7:
        return "A"
    return "B" if cond >= 1e3 else None


# ------------------------------------------------------------------------------------------------ pipeline scenes
PIPE_W, PIPE_H, PIPE_FRAMES = 480, 200, 4
PIPE_OVER = dict(win_w=10, win_h=10, max_translation_norm=5.0)
PIPE_SCENES = {                                               # StereoSequence arguments beside cal, n_frames, step
    "wall_30": dict(seed=31, n_layers=1, depth=(30.0, 30.0)),  # a near-planar world
    "wall_8": dict(seed=31, n_layers=1, depth=(8.0, 8.0)),     # 20-30 tracks, many at negative depth, RANSAC past both first chunks
    "far_300": dict(seed=31, n_layers=2, depth=(300.0, 400.0)),
    "layers_6": dict(seed=31),                                 # the default six-layer scene
}


def pipe_sequence(name):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=PIPE_W, height=PIPE_H, cx=PIPE_W / 2.0, cy=PIPE_H / 2.0)
    return syn.StereoSequence(cal=cal, n_frames=PIPE_FRAMES, step=0.3, **PIPE_SCENES[name])
