"""The motion prior of include/svo.h ("Motion prior") in numpy: LK with an initial guess, the prediction of a homography, the host
inverse, and circular matching with a prior.  The reference of tests/test_gpu_motion_prior.py.

`track` is the loop of lk_tail_ref.track (itself an operation-for-operation copy of the oracle's lk_level) with ONE change: at the
top level the search starts at init * 2^-top instead of the point's own position there (OpenCV's OPTFLOW_USE_INITIAL_FLOW).  It is
trusted as far as tests/test_lk_prior_ref.py checks it: with init = None and with init = the points it must return the oracle's
points, statuses, level visits and Newton steps bit for bit — everything else of the loop is then the oracle's."""
import numpy as np

import lk_tail_ref as lt
from lk_tail_ref import F, FLT_EPSILON, FLT_SCALE, W_BITS, _bilinear, _f32_of_int, _weights

Levels = lt.Levels


def track(A, B, pts, max_level, init=None, max_count=30, epsilon=1e-4, min_eig=1e-3):
    """cv::calcOpticalFlowPyrLK of the points from Levels A to Levels B; init: (n, 2) guesses (OPTFLOW_USE_INITIAL_FLOW) or None
    (flags = 0) -> dict: next (n, 2) float32, status (n,) uint8, visits / steps (n,) per feature."""
    w = A.win
    half = F(w - 1) * F(0.5)
    top = min(max_level, A.n - 1, B.n - 1)
    max_count = min(max(max_count, 0), 100)
    eps2 = min(max(epsilon, 0.0), 10.0) ** 2
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    if init is not None:
        init = np.ascontiguousarray(init, np.float32).reshape(-1, 2)
        assert init.shape == pts.shape
    nxt = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    visits, steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
    den = F(2 * w * w)
    for level in range(top, -1, -1):
        scale = F(1.0 / (1 << level))
        cols, rows = A.size[level]
        for i in range(n):
            ppx, ppy = pts[i, 0] * scale, pts[i, 1] * scale
            if level == top:
                npx, npy = (ppx, ppy) if init is None else (init[i, 0] * scale, init[i, 1] * scale)     # the one change
            else:
                npx, npy = nxt[i, 0] * F(2.0), nxt[i, 1] * F(2.0)
            nxt[i] = (npx, npy)
            ppx, ppy = ppx - half, ppy - half
            ipx, ipy = int(np.floor(ppx)), int(np.floor(ppy))
            if ipx < -w or ipx >= cols or ipy < -w or ipy >= rows:
                if level == 0:
                    status[i] = 0
                continue
            wts = _weights(ppx - F(ipx), ppy - F(ipy))
            I = _bilinear(A, A.img[level], ipx, ipy, w, wts, W_BITS - 5)
            d = A.der[level]
            Ix = _bilinear(A, d[:, :, 0], ipx, ipy, w, wts, W_BITS)
            Iy = _bilinear(A, d[:, :, 1], ipx, ipy, w, wts, W_BITS)
            A11 = _f32_of_int((Ix * Ix).sum()) * FLT_SCALE
            A12 = _f32_of_int((Ix * Iy).sum()) * FLT_SCALE
            A22 = _f32_of_int((Iy * Iy).sum()) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            min_e = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4.0) * A12 * A12)) / den
            if float(min_e) < min_eig or D < FLT_EPSILON:
                if level == 0:
                    status[i] = 0
                continue
            D = F(1.0) / D
            visits[i] += 1
            npx, npy = npx - half, npy - half
            pdx = pdy = F(0.0)
            for j in range(max_count):
                fx, fy = np.floor(npx), np.floor(npy)
                # a guess may lie anywhere: compare as floats first, so that the integer conversion only sees origins in reach
                if not (fx >= -w and fx < cols and fy >= -w and fy < rows):
                    if level == 0:
                        status[i] = 0
                    break
                inx, iny = int(fx), int(fy)
                steps[i] += 1
                wj = _weights(npx - F(inx), npy - F(iny))
                diff = _bilinear(B, B.img[level], inx, iny, w, wj, W_BITS - 5) - I
                b1 = _f32_of_int((diff * Ix).sum()) * FLT_SCALE
                b2 = _f32_of_int((diff * Iy).sum()) * FLT_SCALE
                dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                npx, npy = npx + dx, npy + dy
                nxt[i] = (npx + half, npy + half)
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                    break
                if j > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                    nxt[i] = (nxt[i, 0] - dx * F(0.5), nxt[i, 1] - dy * F(0.5))
                    break
                pdx, pdy = dx, dy
            if status[i] and level == 0:
                fx, fy = np.floor(nxt[i, 0] - half), np.floor(nxt[i, 1] - half)
                if not (fx >= -w and fx < cols and fy >= -w and fy < rows):
                    status[i] = 0
    return dict(next=nxt, status=status, visits=visits, steps=steps)


def same_as_oracle(A, B, pts, max_level, init=None, **kw):
    """track() with a guess that must not matter (None, or the points themselves), checked against the oracle as
    lk_tail_ref.same_as_oracle checks its own copy: points and statuses bit for bit, the visit and step totals; returns track()'s dict"""
    r = track(A, B, pts, max_level, init=init, **kw)
    ok = dict(max_count=kw.get("max_count", 30), epsilon=kw.get("epsilon", 1e-4), min_eig=kw.get("min_eig", 1e-3))
    out, st, nv, ns = lt.oracle_track_counted(A, B, pts, max_level, **ok)
    assert np.array_equal(st, r["status"]), np.flatnonzero(st != r["status"])
    assert np.array_equal(out.view(np.uint32), r["next"].view(np.uint32)), np.flatnonzero((out.view(np.uint32) != r["next"].view(np.uint32)).any(1))
    assert (nv, ns) == (int(r["visits"].sum()), int(r["steps"].sum())), (nv, ns, int(r["visits"].sum()), int(r["steps"].sum()))
    return r


def pred(M, p):
    """pred(M, (x, y)) of svo.h: every operation float32 and rounded once, IEEE division; the point itself where D <= 0 or a
    quotient is not finite (NaN included) -> (x', y', predicted?)"""
    m = np.asarray(M, np.float32).reshape(9)
    x, y = F(p[0]), F(p[1])
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        D = (m[6] * x + m[7] * y) + m[8]
        if D > 0:
            u, v = X / D, Y / D
            if np.isfinite(u) and np.isfinite(v):
                return u, v, True
    return x, y, False


def pred_points(M, pts):
    """pred over (n, 2) points -> ((n, 2) float32 guesses, (n,) bool: the homography was used, not the fallback)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out, used = np.zeros_like(pts), np.zeros(len(pts), bool)
    for i, p in enumerate(pts):
        out[i, 0], out[i, 1], used[i] = pred(M, p)
    return out, used


def adjugate_inverse(H):
    """Hi of svo.h when the caller passes none: adj(H) / det in float64 (each cofactor a d - b c, det = h0 C00 + h1 C01 + h2 C02),
    each entry rounded to float32 -> (3, 3) float32; ValueError for a det that is 0 or not finite"""
    m = [float(v) for v in np.asarray(H, np.float32).reshape(9)]
    C00, C01, C02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    C10, C11, C12 = m[2] * m[7] - m[1] * m[8], m[0] * m[8] - m[2] * m[6], m[1] * m[6] - m[0] * m[7]
    C20, C21, C22 = m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]
    det = m[0] * C00 + m[1] * C01 + m[2] * C02
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("singular H")
    adj = np.array([C00, C10, C20, C01, C11, C21, C02, C12, C22], np.float64)
    return (adj / det).astype(np.float32).reshape(3, 3)


def rotation_homography(Pl, R):
    """f32(K R K^-1), f32(K R^T K^-1) with K = Pl[:, :3], in float64: what svo_motion_prior_from_rotation computes (to rounding)"""
    K = np.asarray(Pl, np.float32).reshape(3, 4)[:, :3].astype(np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    Ki = np.linalg.inv(K)
    return (K @ R @ Ki).astype(np.float32), (K @ R.T @ Ki).astype(np.float32)


def in_image(p, W, H):
    """vo.cpp:344-359 for one point list -> (n,) bool"""
    return ~((p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 1] >= F(H)) | (p[:, 0] >= F(W)))


def circular(levels4, pts, H, Hi, cfg):
    """Circular matching with a prior (svo.h): levels4 = the Levels of (left T0, right T0, left T1, right T1); pass 0 (L0 -> L1)
    starts from pred(H, pl0), pass 2 (R1 -> R0) from pred(Hi, pr1), the stereo passes at their points; H = None: no prior at all.
    All four passes run for every point -> dict: pl1, pr1, pr0, plc (n, 2) float32; status (4, n); ok (n,) uint8 = every status and
    the loop closure; inb (n,) bool = pl0, pl1, pr1, pr0 inside the image; used (2, n) bool: pred did not fall back (passes 0, 2);
    steps / visits: totals over the four passes."""
    L0, R0, L1, R1 = levels4
    kw = dict(max_count=cfg.lk_max_count, epsilon=cfg.lk_epsilon, min_eig=cfg.optical_flow_min_eig_threshold)
    ml = cfg.max_level
    pl0 = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pl0)
    g0, u0 = pred_points(H, pl0) if H is not None else (None, np.zeros(n, bool))
    a = track(L0, L1, pl0, ml, init=g0, **kw)
    b = track(L1, R1, a["next"], ml, **kw)
    g2, u2 = pred_points(Hi, b["next"]) if H is not None else (None, np.zeros(n, bool))
    c = track(R1, R0, b["next"], ml, init=g2, **kw)
    d = track(R0, L0, c["next"], ml, **kw)
    status = np.stack([a["status"], b["status"], c["status"], d["status"]])
    thr = F(cfg.circular_matching_success_threshold)
    ex, ey = np.abs(pl0[:, 0] - d["next"][:, 0]), np.abs(pl0[:, 1] - d["next"][:, 1])
    off = np.where(ex < ey, ey, ex)
    ok = (status.all(0) & ~(off > thr)).astype(np.uint8)
    W, Hh = L0.size[0]
    inb = in_image(pl0, W, Hh) & in_image(a["next"], W, Hh) & in_image(b["next"], W, Hh) & in_image(c["next"], W, Hh)
    return dict(pl1=a["next"], pr1=b["next"], pr0=c["next"], plc=d["next"], status=status, ok=ok, inb=inb, used=np.stack([u0, u2]),
                steps=int(sum(r["steps"].sum() for r in (a, b, c, d))), visits=int(sum(r["visits"].sum() for r in (a, b, c, d))))
