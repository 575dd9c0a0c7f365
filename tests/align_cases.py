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


# ---- scenes for the f64 part of rules 7 - 9 at hard geometry: motion_scene's rows with another motion, cloud or offset
PLANE = (0.3, -0.2, 1.0)                              # z = 0.3 x - 0.2 y + 1: a floor seen at a slant
FAR = 5000.0                                          # metres, on every axis: a map after a long sequence
LINE = ((1.0, 2.0, -1.0), (0.0, 1.0, 3.0))            # p = s (1, 2, -1) + (0, 1, 3)
PI = float(np.pi)
# name: (angle, axis, shift, cloud, offset)
GEOMETRY = {
    "default": (ANGLE, AXIS, SHIFT, "uniform", 0.0),
    "identity": (0.0, AXIS, (0.0, 0.0, 0.0), "uniform", 0.0),
    "pi_x": (PI, (1.0, 0.0, 0.0), SHIFT, "uniform", 0.0),
    "pi_y": (PI, (0.0, 1.0, 0.0), SHIFT, "uniform", 0.0),
    "pi_z": (PI, (0.0, 0.0, 1.0), SHIFT, "uniform", 0.0),
    "pi_axis": (PI, AXIS, SHIFT, "uniform", 0.0),
    "near_pi": (PI - 1e-9, AXIS, SHIFT, "uniform", 0.0),
    "perm": (2 * PI / 3, (1.0, 1.0, 1.0), SHIFT, "uniform", 0.0),
    "quarter_z": (PI / 2, (0.0, 0.0, 1.0), SHIFT, "uniform", 0.0),
    "tiny": (1e-7, AXIS, SHIFT, "uniform", 0.0),
    "planar": (ANGLE, AXIS, SHIFT, "plane", 0.0),
    "planar_pi": (PI, (3.0, -1.0, 2.0), SHIFT, "plane", 0.0),
    "slab": (ANGLE, AXIS, SHIFT, "slab", 0.0),
    "far": (ANGLE, AXIS, SHIFT, "uniform", FAR),
    "far_planar": (2.9, AXIS, SHIFT, "plane", FAR),
    "clumped": (ANGLE, AXIS, SHIFT, "clumped", 0.0),
    "collinear": (ANGLE, AXIS, SHIFT, "line", 0.0),
    "needle": (ANGLE, AXIS, SHIFT, "needle", 0.0),
    "coincident": (ANGLE, AXIS, SHIFT, "point", 0.0),
    "two_points": (ANGLE, AXIS, SHIFT, "two_points", 0.0),
}
WELL_POSED = ("identity", "pi_x", "pi_y", "pi_z", "pi_axis", "near_pi", "perm", "quarter_z", "tiny", "planar", "planar_pi", "slab", "far",
              "far_planar", "clumped")
ILL_POSED = ("collinear", "needle", "coincident", "two_points")
# The motions that are matrices of 0 and +-1: what the library's R is held to, and what the scene's points are made with
EXACT_R = {
    "identity": ((1, 0, 0), (0, 1, 0), (0, 0, 1)), "pi_x": ((1, 0, 0), (0, -1, 0), (0, 0, -1)), "pi_y": ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    "pi_z": ((-1, 0, 0), (0, -1, 0), (0, 0, 1)), "perm": ((0, 0, 1), (1, 0, 0), (0, 1, 0)), "quarter_z": ((0, -1, 0), (1, 0, 0), (0, 0, 1)),
}
# The shape a cloud is named for, as bounds on the singular values s1 >= s2 >= s3 of the centred source cloud (f32 points widened)
# over sqrt(n), i.e. its rms extent along its principal axes in metres: cloud -> ((lowest s2, highest s2), (lowest s3, highest s3)).
# uniform +-30 m has 17.3 m a side; a plane and a line are exact in f64 and keep the f32 rounding of their points, 2e-6 m at 30 m and
# 5e-4 m at 5000 m; the slab's +-1 mm is 5.8e-4 m rms and the needle's +-1 cm 5.8e-3 m; two points have no second extent at all.
SHAPE = {
    "uniform": ((10.0, 30.0), (10.0, 30.0)), "plane": ((10.0, 30.0), (0.0, 1e-5)), "plane_far": ((10.0, 30.0), (0.0, 5e-4)),
    "slab": ((10.0, 30.0), (1e-4, 1e-3)), "clumped": ((5.0, 30.0), (0.0, 1e-5)), "line": ((0.0, 1e-5), (0.0, 1e-5)),
    "needle": ((1e-3, 1e-2), (1e-3, 1e-2)), "point": ((0.0, 0.0), (0.0, 0.0)), "two_points": ((0.0, 1e-12), (0.0, 1e-12)),
}


def rotation(angle, axis):
    """Rodrigues' formula; where the result is a matrix of 0 and +-1 to rounding, exactly that matrix"""
    a = np.array(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    return np.round(R) if np.abs(R - np.round(R)).max() < 1e-12 else R


def _cloud(rng, kind, n):
    """n source points in f64, before the offset and the rounding to f32"""
    if kind == "uniform":
        return rng.uniform(-30, 30, (n, 3))
    if kind in ("plane", "slab", "clumped"):
        xy = rng.uniform(-30, 30, (n, 2))
        P = np.column_stack([xy, PLANE[0] * xy[:, 0] + PLANE[1] * xy[:, 1] + PLANE[2]])
        if kind == "slab":
            P[:, 2] += rng.uniform(-1e-3, 1e-3, n)
        if kind == "clumped":                         # 30 % of the pairs are copies of two of the others, in turn
            order = rng.permutation(n)
            copies, marks = order[:int(round(0.3 * n))], order[-2:]
            P[copies] = P[marks[np.arange(len(copies)) % 2]]
        return P
    if kind in ("line", "needle"):
        s = rng.uniform(-30, 30, n)
        P = s[:, None] * np.array(LINE[0]) + np.array(LINE[1])
        return P + rng.uniform(-0.01, 0.01, (n, 3)) if kind == "needle" else P
    if kind == "point":
        return np.tile(rng.uniform(-30, 30, 3), (n, 1))
    if kind == "two_points":
        ab = rng.uniform(-30, 30, (2, 3))
        return ab[(rng.permutation(n) < n // 2).astype(int)]
    raise KeyError(kind)


def kept_pairs(inliers, n):
    """the pairs a scene keeps free of the outlier displacement, by name: "wave3", the pairs k_align_fit gives to its last wave
    (c % 256 >= 192); "slot<k>", the pairs of every thread's slot k (c // 256 == k; slot15 is c >= 3840); "h<k>", the three pairs
    hypothesis k draws"""
    import align_ref as aref
    c = np.arange(n)
    if inliers == "wave3":
        return c % 256 >= 192
    if inliers.startswith("slot"):
        return c // 256 == int(inliers[4:])
    assert inliers[0] == "h"
    return np.isin(c, aref.sample(int(inliers[1:]), n))


@functools.lru_cache(maxsize=None)
def geometry_scene(name, n, outlier_share, sigma, seed=0, inliers=None):
    """motion_scene's rows — n destination rows, then n source rows, source row j matching destination row perm[j] 0 .. 8 bits
    apart, every id its own, so pair c is source row n + c — with the motion, the cloud and the offset GEOMETRY[name] fixes:
    x_dst = R x_src + t with the f32 source points, N(0, sigma) per axis, and for an outlier_share of the pairs (or, with `inliers`,
    for every pair kept_pairs does not name) a displacement of 1 .. 5 m per axis with a random sign.  The clouds' shapes are
    bounded in SHAPE and asserted by tests/test_align_geometry_ref.py, with the motions' angles and the offsets.  Seeds: every
    well-posed scene meets its conditions at seed 0 (the margins and disagreements that test prints); the seam scenes' pinned seeds
    are H_SEAM_SEED and LATE_WINNERS below.  -> the case, with `outlier` (per source row) and the true R, t."""
    angle, axis, shift, cloud, offset = GEOMETRY[name]
    rng = np.random.default_rng([2000 + list(GEOMETRY).index(name), seed, n])
    R, t = rotation(angle, axis), np.array(shift)
    d_src = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    d_dst = np.zeros_like(d_src)
    d_dst[perm] = flip_bits(rng, d_src, rng.integers(0, 9, n))
    P = (_cloud(rng, cloud, n) + offset).astype(np.float32)
    Q = P.astype(np.float64) @ R.T + t + (rng.normal(0, sigma, (n, 3)) if sigma > 0 else 0)
    outlier = np.zeros(n, bool)
    if inliers is None:
        outlier[rng.permutation(n)[:int(round(outlier_share * n))]] = True
    else:
        outlier = ~kept_pairs(inliers, n)
    Q[outlier] += rng.uniform(1, 5, (int(outlier.sum()), 3)) * rng.choice([-1.0, 1.0], (int(outlier.sum()), 3))
    xyz = np.zeros((2 * n, 3), np.float32)
    xyz[perm] = Q.astype(np.float32)
    xyz[n:] = P
    ids = np.concatenate([500_000 + np.arange(n), 1_000 + np.arange(n)]).astype(np.uint64)
    case = _case(np.concatenate([d_dst, d_src]), ids, xyz, np.zeros(2 * n, np.int32), (n, 2 * n), (0, n))
    outlier.setflags(write=False)
    case.update(outlier=outlier, R=R, t=t)
    return case


@functools.lru_cache(maxsize=None)
def _geometry_pairs(name, n, outlier_share, sigma, seed, inliers):
    import align_ref as aref
    c = geometry_scene(name, n, outlier_share, sigma, seed, inliers)
    return aref.pairs(c["desc"], c["ids"], c["tags"], c["src"], c["dst"])


@functools.lru_cache(maxsize=None)
def geometry_reference(name, n, outlier_share, hypotheses, sigma, seed=0, inliers=None, min_pairs=3, refit_rounds=4):
    """the reference's result on geometry_scene(name, n, outlier_share, sigma, seed, inliers): computed once, shared, never changed;
    with `disagreement`, align_ref.disagreement on its final inlier set (None with fewer than 3 inliers)"""
    import align_ref as aref
    c = geometry_scene(name, n, outlier_share, sigma, seed, inliers)
    ps, pd = _geometry_pairs(name, n, outlier_share, sigma, seed, inliers)
    out = aref.fit(c["xyz"][ps], c["xyz"][pd], INLIER_DIST, min_pairs=min_pairs, hypotheses=hypotheses, refit_rounds=refit_rounds)
    inl = out["inlier"].astype(bool)
    out.update(pair_src=ps, pair_dst=pd, disagreement=aref.disagreement(c["xyz"][ps][inl], c["xyz"][pd][inl]) if inl.sum() >= 3 else None)
    return out


# (n_pairs, outlier share, hypotheses, sigma) of every well-posed scene, and of three of them at k_align_fit's last pair but one
GEOMETRY_SIZES = ((64, 0.5, 128, 0.0), (257, 0.3, 64, 0.005))
GEOMETRY_CASES = tuple((name, n, share, H, 0.0 if name == "tiny" else sigma) for name in WELL_POSED for n, share, H, sigma in GEOMETRY_SIZES) + \
    tuple((name, 4095, 0.6, 512, 0.005) for name in ("far", "planar", "pi_axis"))
N_SEAMS = tuple(("default", n, 0.4, 64, 0.005) for n in (255, 256, 257, 4095))
H_SEAMS = (1023, 257, 256, 255, 5, 4, 3, 1)          # in the order of the calls on one index: every call after a larger one
# "default" at n = 65, share 0.5, sigma 0 with this seed: hypothesis 4 is the first whose three pairs are all inliers (count 33) and
# hypotheses 0 .. 3 count nothing, so H >= 5 succeeds with best_hypothesis 4 and H <= 4 fails with best_hypothesis 0, count 0 — a
# call that read the counts a larger H left behind would report 4
H_SEAM_SEED, H_SEAM_FIRST = 1, 4
# "default" at n = 64, share 0.85 (10 inliers), sigma 0, H = 1024: (what, seed, the reference's best_hypothesis, a later hypothesis
# that ties its count of 10).  Slot k: best_hypothesis // 256, the k of k_align_fit's search; wave 3: best_hypothesis % 256 >= 192
LATE_WINNERS = (("slot1", 2, 349, 542), ("slot2", 1, 610, 753), ("slot3", 34, 830, 895), ("wave3", 9, 452, 712))
LATE = (64, 0.85, 1024, 0.0)
# n = 4096, every pair an outlier but the named ones: (inliers, H, sigma).  The sampler is a function of h and n alone: at n = 4096
# hypothesis 103 is the first of 21 below 512 that draws inside wave 3; NO hypothesis below 1024 draws three pairs of slot 15, so that
# scene ends without a model on both sides; hypothesis 849 is the only one that draws inside one slot's 256 pairs late in the list
# (slot 13), and that scene is the one whose refit sums have 15 of 16 slots empty
ONE_PLACE = (("wave3", 512, 0.005), ("slot15", 1024, 0.005), ("slot13", 1024, 0.005))


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
