"""Synthetic index rows for the map alignment's tests (include/svo.h, "Map alignment"), shared by the reference's own tests and the
GPU tests.  A case is a dict of the arrays an index is built from — desc (m, 32) uint8, ids (m,) uint64, xyz (m, 3) float32, tags
(m,) int32 (-1: a row without a point) — and the two spans src, dst.  Every case is built once and never changed."""
import functools

import numpy as np

ANGLE, AXIS, SHIFT = 0.7, (1.0, 2.0, 3.0), (12.0, -3.0, 40.0)        # the relation of the two map frames: x_dst = R x_src + t
INLIER_DIST = 0.05


def flip_bits(rng, desc, n_bits):
    """each row with n_bits[i] distinct bits flipped"""
    out = desc.copy()
    for i, b in enumerate(np.broadcast_to(n_bits, len(desc))):
        for bit in rng.choice(256, int(b), replace=False):
            out[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def true_motion():
    a = np.array(AXIS) / np.linalg.norm(AXIS)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ANGLE) * K + (1 - np.cos(ANGLE)) * K @ K, np.array(SHIFT)


def _case(desc, ids, xyz, tags, src, dst):
    for a in (desc, ids, xyz, tags):
        a.setflags(write=False)
    return dict(desc=desc, ids=ids, xyz=xyz, tags=tags, src=src, dst=dst)


# ---- scenes for rules 2 - 5: what matters is which rows pair up, not where the points are
@functools.lru_cache(maxsize=None)
def pair_scene(name):
    """"k_rows": every landmark has 1 .. 3 rows on both sides, each a few bits from the landmark's descriptor; "equal": the rows of a
    landmark are bit-identical copies, so every distance ties and (dist, j) decides by j alone, and rows tie across landmarks;
    "no_points": a third of the rows on either side carry no point; "lone": the destination holds ONE landmark (dist2 = 257
    everywhere), in several rows; "before": k_rows with the source span in front of the destination; "empty": no source rows."""
    rng = np.random.default_rng({"k_rows": 1, "equal": 2, "no_points": 3, "lone": 4, "before": 5, "empty": 6}[name])
    L = 1 if name == "lone" else 150
    base = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    rows = {}
    for side, first_id in (("dst", 10_000), ("src", 50_000)):
        k = rng.integers(1, 4, L)                                        # rows per landmark
        if name == "lone" and side == "src":
            k = np.array([5])
        lm = rng.permutation(np.repeat(np.arange(L), k))                 # the landmark of every row
        d = base[lm] if name == "equal" else flip_bits(rng, base[lm], rng.integers(0, 9, len(lm)))
        if name == "equal":
            d[lm % 5 == 0] = base[0]                                     # a fifth of the landmarks look alike entirely
        tags = rng.integers(0, 7, len(lm)).astype(np.int32)
        if name == "no_points":
            tags[rng.random(len(lm)) < 1 / 3] = -1
        rows[side] = (d, (first_id + lm).astype(np.uint64), rng.uniform(-30, 30, (len(lm), 3)).astype(np.float32), tags)
    if name == "lone":                                                   # each source row its own landmark: all five match the one destination id
        rows["src"] = (rows["src"][0], np.arange(50_000, 50_005, dtype=np.uint64)) + rows["src"][2:]
    order = ("src", "dst") if name == "before" else ("dst", "src")
    n0 = len(rows[order[0]][0])
    cat = [np.concatenate([rows[order[0]][i], rows[order[1]][i]]) for i in range(4)]
    span = {order[0]: (0, n0), order[1]: (n0, len(cat[0]))}
    if name == "empty":
        span["src"] = (len(cat[0]), len(cat[0]))
    return _case(cat[0], cat[1], cat[2], cat[3], span["src"], span["dst"])


PAIR_SCENES = ("k_rows", "equal", "no_points", "lone", "before", "empty")


# ---- scenes for rules 6 - 10: n rows on either side that pair up one to one, their points related by the true motion
@functools.lru_cache(maxsize=None)
def motion_scene(n, outlier_share, sigma, seed=0, identity=False):
    """n destination rows, then n source rows; source row j matches destination row perm[j] (0 .. 8 bits apart, every id its own).
    Points in +-30 m; the destination's are R p + t, plus N(0, sigma) per axis, and for an outlier_share of them a displacement of
    1 .. 5 m per axis with a random sign.  -> the case, with `outlier` (per source row) and the true R, t."""
    rng = np.random.default_rng(1000 + seed + n)
    R, t = (np.eye(3), np.zeros(3)) if identity else true_motion()
    d_src = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    d_dst = np.zeros_like(d_src)
    d_dst[perm] = flip_bits(rng, d_src, rng.integers(0, 9, n))
    P = rng.uniform(-30, 30, (n, 3))
    Q = P.astype(np.float32).astype(np.float64) @ R.T + t + (rng.normal(0, sigma, (n, 3)) if sigma > 0 else 0)
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:int(round(outlier_share * n))]] = True
    Q[outlier] += rng.uniform(1, 5, (int(outlier.sum()), 3)) * rng.choice([-1.0, 1.0], (int(outlier.sum()), 3))
    xyz = np.zeros((2 * n, 3), np.float32)
    xyz[perm] = Q[np.arange(n)].astype(np.float32)
    xyz[n:] = P.astype(np.float32)
    ids = np.concatenate([500_000 + np.arange(n), 1_000 + np.arange(n)]).astype(np.uint64)
    case = _case(np.concatenate([d_dst, d_src]), ids, xyz, np.zeros(2 * n, np.int32), (n, 2 * n), (0, n))
    outlier.setflags(write=False)
    case.update(outlier=outlier, R=R, t=t)
    return case


# (n_pairs, outlier share, hypotheses, sigma): every n the issue names, every share, H from 8 to 1024, with and without noise
MOTION_CASES = ((3, 0.0, 8, 0.0), (4, 0.0, 8, 0.0), (6, 0.0, 16, 0.005), (63, 0.3, 64, 0.005), (64, 0.5, 128, 0.0), (65, 0.5, 128, 0.005),
                (1024, 0.6, 512, 0.005), (1025, 0.6, 512, 0.0), (4096, 0.7, 1024, 0.005), (4096, 0.0, 8, 0.0))


@functools.lru_cache(maxsize=None)
def motion_reference(n, outlier_share, hypotheses, sigma, refit_rounds=4):
    """the reference's result on motion_scene(n, outlier_share, sigma) with min_pairs = 3: computed once, shared, never changed"""
    import align_ref as aref
    c = motion_scene(n, outlier_share, sigma)
    return aref.align(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], INLIER_DIST, min_pairs=3, hypotheses=hypotheses,
                      refit_rounds=refit_rounds)


def build_index(api, case, extra=0, chunk_rows=None):
    """an index with points holding the case's rows"""
    index = api.DescriptorIndex(len(case["desc"]) + extra, points=True)
    if chunk_rows is not None:
        index.chunk_rows = chunk_rows
    has = case["tags"] >= 0
    cuts = [0] + [i for i in range(1, len(has)) if has[i] != has[i - 1]] + [len(has)]
    for a, b in zip(cuts[:-1], cuts[1:]):                                # runs of rows with a point, and of rows without
        if b > a and has[a]:
            index.add_points(case["desc"][a:b], case["ids"][a:b], case["xyz"][a:b], case["tags"][a:b])
        elif b > a:
            index.add(case["desc"][a:b], case["ids"][a:b])
    return index
