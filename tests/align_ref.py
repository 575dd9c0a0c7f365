"""Reference for the descriptor index's map alignment (include/svo.h, "Map alignment"), straight from rules 1 - 10.  Rule 1 through
desc_match_ref.match; rules 2 - 5 and the sampler on Python integers; rules 7 - 9 in f64 with Horn's quaternion through
numpy.linalg.eigh.  It knows nothing of the kernels' LDS lists, ballots, Jacobi sweeps or summation trees, so its models differ
from the library's in their last bits: `margin` says how far every residual it compared stayed from the threshold, and a test asserts
a set only where that margin leaves no room for those bits."""
import numpy as np

import desc_match_ref as mref
import reloc_ref as rref

MAX_ROWS, MAX_HYPOTHESES, MAX_DRAWS = 4096, 1024, 64
M64 = (1 << 64) - 1


def mix64(x):
    """splitmix64's finaliser, modulo 2^64"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample(h, n_pairs, max_draws=MAX_DRAWS, with_draws=False):
    """rule 6: three distinct pair numbers below n_pairs for hypothesis h (-> also the draws made, with_draws)"""
    assert n_pairs >= 3
    out, k = [], 0
    while k < max_draws and len(out) < 3:
        d = (mix64((h << 32) | k) >> 32) % n_pairs
        k += 1
        if d not in out:
            out.append(d)
    c = 0
    while len(out) < 3:                               # the fallback: the smallest numbers not yet used
        if c not in out:
            out.append(c)
        c += 1
    return (out, k) if with_draws else out


def pairs(desc, ids, tags, src, dst, max_dist=40, ratio_num=7, ratio_den=10, matches=None):
    """rules 1 - 5 on the host's copies of an index's arrays: src = (lo, hi), dst = (lo, hi) -> (pair_src, pair_dst) int32 row numbers.
    Sorting, not dictionaries: per destination id, then per source id, the first of the rows ordered by (dist, j)."""
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    tags = np.asarray(tags).reshape(-1)
    (s0, s1), (d0, d1) = src, dst
    m = mref.match(np.asarray(desc, np.uint8).reshape(-1, 32)[s0:s1], desc, ids, d0, d1) if matches is None else matches
    acc = [j for j in range(s1 - s0) if int(tags[s0 + j]) != rref.POINT_NONE and
           rref.accept(m[j], tags[int(m[j]["row"])] if int(m[j]["row"]) >= 0 else rref.POINT_NONE, max_dist, ratio_num, ratio_den)]
    for key_of in (lambda j: int(m[j]["id"]), lambda j: int(ids[s0 + j])):           # rule 3, then rule 4
        order = sorted(acc, key=lambda j: (key_of(j), int(m[j]["dist"]), j))
        acc = sorted(j for i, j in enumerate(order) if i == 0 or key_of(order[i - 1]) != key_of(j))
    return np.array([s0 + j for j in acc], np.int32), np.array([int(m[j]["row"]) for j in acc], np.int32)


def horn(P, Q):
    """rule 7 on the pairs (P[i], Q[i]), f64: the centred cross-covariance, Horn's symmetric 4 x 4 matrix, the eigenvector of its
    largest eigenvalue (numpy.linalg.eigh) as a quaternion -> R, t with Q ~ R P + t"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    cp, cq = P.mean(0), Q.mean(0)
    S = (P - cp).T @ (Q - cq)                         # S[i, j] = sum p_i q_j
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[2, 2] - S[0, 0], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
    w, V = np.linalg.eigh(N)
    q0, q1, q2, q3 = V[:, 3]
    R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                  [2 * (q1 * q2 + q0 * q3), q0 * q0 + q2 * q2 - q1 * q1 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                  [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 + q3 * q3 - q1 * q1 - q2 * q2]])
    return R, cq - R @ cp


def kabsch(P, Q):
    """the same least-squares problem as horn through the SVD of the centred cross-covariance, the determinant's sign set right"""
    cp, cq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - cq).T @ (P - cp))
    D = np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cq - R @ cp


def disagreement(P, Q):
    """how far the two f64 methods, horn and kabsch, are apart on the same pairs -> (the angle between their rotations in radians,
    the distance in metres between their images of the pairs' source centroid): what a test may ask of a third f64 method at most"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    (Rh, th), (Rk, tk) = horn(P, Q), kabsch(P, Q)
    c = P.mean(0)
    return rotation_angle(Rh, Rk), float(np.linalg.norm((Rh @ c + th) - (Rk @ c + tk)))


def residual2(R, t, P, Q):
    r = P @ R.T + t - Q
    return (r * r).sum(1)


def fit(P, Q, inlier_dist, min_pairs=6, hypotheses=256, refit_rounds=4):
    """rules 5 - 10 on the pairs' points P, Q (n_pairs, 3) float32 -> dict: success, n_pairs, n_inliers, best_hypothesis, best_count,
    refit_rounds_run, inlier (uint8 per pair), R, t, T, rms, and the margins: `margin` = the smallest ||r| - d| / d over every
    residual compared in any hypothesis or refit round, `margin_final` = the same for the final model alone."""
    P, Q = np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(Q, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(P)
    d = float(np.float32(inlier_dist))
    d2 = d * d
    out = dict(success=False, n_pairs=n, n_inliers=0, best_hypothesis=-1, best_count=0, refit_rounds_run=0, inlier=np.zeros(n, np.uint8),
               R=np.zeros((3, 3)), t=np.zeros(3), T=np.zeros((4, 4)), rms=0.0, margin=np.inf, margin_final=np.inf)
    if n < min_pairs:
        return out

    def margin(r2):
        r2 = r2[np.isfinite(r2)]
        return float(np.abs(np.sqrt(r2) - d).min() / d) if len(r2) else np.inf

    best, model = (-1, 0), None
    for h in range(hypotheses):
        pick = sample(h, n)
        R, t = horn(P[pick], Q[pick])
        r2 = residual2(R, t, P, Q)
        count = int((r2 <= d2).sum()) if np.isfinite(R).all() and np.isfinite(t).all() else 0
        out["margin"] = min(out["margin"], margin(r2))
        if count > best[0]:                           # at equal counts the smallest h stays
            best, model = (count, h), (R, t)
    R, t = model
    r2 = residual2(R, t, P, Q)
    inl = r2 <= d2
    rounds = 0
    for _ in range(refit_rounds):
        if inl.sum() < 3:
            break
        R, t = horn(P[inl], Q[inl])
        r2 = residual2(R, t, P, Q)
        out["margin"] = min(out["margin"], margin(r2))
        new = r2 <= d2
        rounds += 1
        same = np.array_equal(new, inl)
        inl = new
        if same:
            break
    k = int(inl.sum())
    out.update(n_inliers=k, best_hypothesis=best[1], best_count=best[0], refit_rounds_run=rounds, inlier=inl.astype(np.uint8),
               success=k >= min_pairs, margin_final=margin(r2))
    if out["success"]:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        out.update(R=R, t=t, T=T, rms=float(np.sqrt(r2[inl].sum() / k)))
    return out


def align(desc, ids, xyz, tags, src, dst, inlier_dist, max_dist=40, ratio_num=7, ratio_den=10, **kw):
    """all of it on the host's copies of an index's arrays -> fit's dict with pair_src, pair_dst"""
    ps, pd = pairs(desc, ids, tags, src, dst, max_dist, ratio_num, ratio_den)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = fit(xyz[ps], xyz[pd], inlier_dist, **kw)
    out.update(pair_src=ps, pair_dst=pd)
    return out


def rotation_angle(Ra, Rb):
    """the angle of Ra Rb^T in radians, from the skew part (accurate near zero, where arccos of the trace is not)"""
    D = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


BAND = 1e-9                                           # check_model: residuals this close to the threshold (relative) may fall on either side


def check_model(res, pairs, xyz, inlier_dist, min_pairs=None):
    """Rule 10's invariants of one result, recomputed in f64 from the returned R and t alone — no second model is involved, so they
    hold wherever the rotation is ambiguous.  res: the library's AlignResult or fit's dict; pairs: src, dst (row numbers) and inlier
    per pair; xyz: the index's points.  Asserts: every entry finite; on success |R^T R - I| <= 1e-12, |det R - 1| <= 1e-12, T is R and
    t over the row 0 0 0 1, every flagged pair's residual <= inlier_dist and every other pair's above it (pairs within BAND x
    inlier_dist of the threshold excepted, and counted), rms the flagged pairs' to 1e-9; on failure R, t, T and rms zero; always
    n_inliers == the flags' sum and, with min_pairs, success == (n_inliers >= min_pairs).
    -> dict: n_band (the pairs excepted), ortho, det (the two errors), rms, nearest (the smallest | |r| - d | / d)."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    R, t, T, rms = (np.asarray(get(k), np.float64) for k in ("R", "t", "T", "rms"))
    flags = np.asarray(pairs["inlier"]).astype(bool)
    assert np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(T).all() and np.isfinite(rms)
    assert len(flags) == get("n_pairs") and int(get("n_inliers")) == int(flags.sum())
    if min_pairs is not None:
        assert bool(get("success")) == (int(get("n_inliers")) >= min_pairs)
    if not get("success"):
        assert not R.any() and not t.any() and not T.any() and rms == 0.0
        return dict(n_band=0, ortho=0.0, det=0.0, rms=0.0, nearest=np.inf)
    ortho, det = float(np.abs(R.T @ R - np.eye(3)).max()), float(abs(np.linalg.det(R) - 1.0))
    assert ortho <= 1e-12 and det <= 1e-12, (ortho, det)
    assert np.array_equal(T[:3, :3], R) and np.array_equal(T[:3, 3], t) and np.array_equal(T[3], [0, 0, 0, 1])
    xyz = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    d = float(np.float32(inlier_dist))
    r = np.sqrt(residual2(R, t, xyz[np.asarray(pairs["src"])], xyz[np.asarray(pairs["dst"])]))
    band = np.abs(r - d) <= BAND * d
    assert ((r <= d) == flags)[~band].all(), "a flag disagrees with its pair's recomputed residual"
    want_rms = float(np.sqrt((r[flags] ** 2).sum() / flags.sum())) if flags.any() else 0.0
    assert abs(float(rms) - want_rms) <= 1e-9, (float(rms), want_rms)
    return dict(n_band=int(band.sum()), ortho=ortho, det=det, rms=want_rms, nearest=float((np.abs(r - d) / d).min()) if len(r) else np.inf)
