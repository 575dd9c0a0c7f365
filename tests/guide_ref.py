"""Reference for the guided search (include/svo.h, "Guided search"), straight from rules 1 - 3, in numpy: the projection in f64 with
every product, quotient and sum an operation of its own (numpy rounds each; nothing is fused), .astype(np.float32), and the gate in
f32.  The search over the admissible rows is desc_match_ref's definition with the other rows masked out; selection and everything
behind it are reloc_ref's.  It knows nothing of chunks, ballots or the order in which the kernel serves the queries."""
import numpy as np

import desc_match_ref as mref
import descriptor_ref as dref
import reloc_ref as rref

POINT_NONE = -1


def project(K, R, t, xyz, tags):
    """rule 1: K (3, 3) or 9 values (K[0], K[2], K[4], K[5] are used, as float32 widened), R (3, 3), t (3,) float64, xyz (m, 3)
    float32, tags (m,) -> uv (m, 2) float32, (+inf, +inf) for an invisible row"""
    K = np.asarray(K, np.float32).reshape(-1)
    fx, cx, fy, cy = (np.float64(K[i]) for i in (0, 2, 4, 5))
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    tags = np.asarray(tags).reshape(-1)
    with np.errstate(all="ignore"):
        c = []
        for r in range(3):
            s = R[3 * r] * p[:, 0]
            s = s + R[3 * r + 1] * p[:, 1]
            s = s + R[3 * r + 2] * p[:, 2]
            c.append(s + t[r])
        u = fx * (c[0] / c[2])
        u = (u + cx).astype(np.float32)
        v = fy * (c[1] / c[2])
        v = (v + cy).astype(np.float32)
        visible = (tags != POINT_NONE) & (c[2] > 0) & np.isfinite(u) & np.isfinite(v)
    uv = np.full((len(p), 2), np.inf, np.float32)
    uv[visible, 0] = u[visible]
    uv[visible, 1] = v[visible]
    return uv


def admissible(uv, xy, radius):
    """rule 2: uv (m, 2) float32 projections, xy (n, 2) float32 pixels -> (n, m) bool.  f32 subtraction, absolute value and compare;
    inf - inf and anything with NaN give NaN, which fails the compare."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    rad = np.float32(radius)
    with np.errstate(all="ignore"):
        du = np.abs(uv[None, :, 0] - xy[:, None, 0])
        dv = np.abs(uv[None, :, 1] - xy[:, None, 1])
        assert du.dtype == np.float32
        return (du <= rad) & (dv <= rad)


def match(query, xy, desc, ids, uv, radius, lo=0, hi=-1):
    """rule 3: desc_match_ref.match's definition over the admissible rows of [lo, hi) -> (n,) rows of desc_match_ref.DTYPE"""
    query = np.asarray(query, np.uint8).reshape(-1, 32)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    hi = len(desc) if hi == -1 else hi
    assert 0 <= lo <= hi <= len(desc) == len(ids) == len(uv)
    n = len(query)
    out = np.zeros(n, mref.DTYPE)
    out["row"] = out["row2"] = mref.NONE
    out["dist"] = out["dist2"] = mref.NO_DIST
    if hi == lo or n == 0:
        return out
    rows = np.arange(lo, hi, dtype=np.int64)
    big = np.iinfo(np.int64).max
    for q0 in range(0, n, mref.BLOCK):                                  # blocks only bound the memory
        q1 = min(n, q0 + mref.BLOCK)
        adm = admissible(uv[lo:hi], np.asarray(xy, np.float32).reshape(-1, 2)[q0:q1], radius)
        D = dref.hamming(query[q0:q1], desc[lo:hi]).astype(np.int64)
        key = np.where(adm, D * (1 << 32) + rows[None, :], big)
        best = key.argmin(1)
        has = adm.any(1)
        o = out[q0:q1]
        j = np.flatnonzero(has)
        o["row"][j] = rows[best[j]]
        o["dist"][j] = D[j, best[j]]
        o["id"][j] = ids[lo:hi][best[j]]
        other = adm & (ids[lo:hi][None, :] != o["id"][:, None]) & has[:, None]
        key2 = np.where(other, key, big)
        second = key2.argmin(1)
        j2 = np.flatnonzero(other.any(1))
        o["row2"][j2] = rows[second[j2]]
        o["dist2"][j2] = D[j2, second[j2]]
        o["id2"][j2] = ids[lo:hi][second[j2]]
        out[q0:q1] = o
    return out


def select_index(K, R, t, radius, query, xy, desc, ids, xyz, tags, row_lo=0, row_hi=-1, max_dist=40, ratio_num=7, ratio_den=10):
    """rules 1 - 4 on the host's copies of an index's arrays -> dict(query, row, xy, xyz) as api.DescriptorIndex.select_guided gives"""
    uv = project(K, R, t, xyz, tags)
    m = match(query, xy, desc, ids, uv, radius, row_lo, row_hi)
    q, r = rref.select(m, tags, max_dist, ratio_num, ratio_den)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return dict(query=q, row=r, xy=xy[q], xyz=xyz[r])
