"""Inputs of the relocaliser's GPU tests (tests/test_gpu_reloc_select.py, tests/test_gpu_reloc_facade.py).

clause_case(): 4096 queries and an index in which each clause of the selection rules (include/svo.h, "Relocalisation") decides for
some query.  Query j is a random 256-bit base b_j; its row A_j is b_j with d1[j] bits flipped, and — where a second distance is
planned — a row B_j of another id is b_j with d2[j] bits flipped.  Random descriptors lie ~128 bits apart (84 at least among these),
so (d1, d2) is what the search returns wherever d2 is planned; the tests do not rely on that: the expected values come from the
reference search on the same arrays, and the plan is only asserted where a test names a clause.

scene(): landmarks in front of a camera, their exact projections and noisy copies of their descriptors: a set on which the PnP succeeds."""
import numpy as np

N = 4096
N_B = 1024                                             # queries below this number have a planned second row
# per kind j % 8: (d1, d2 or 0 = none planned, has a point) — at max_dist = 40, ratio 7 / 10
KINDS = [(10, 30, True),                               # 0 accepted
         (40, 60, True),                               # 1 dist == max_dist: accepted
         (41, 70, True),                               # 2 max_dist + 1: rejected
         (7, 10, True),                                # 3 7 * 10 == 10 * 7: rejected (strict)
         (7, 11, True),                                # 4 accepted
         (5, 30, False),                               # 5 the best row has no point: rejected
         (21, 30, True),                               # 6 210 == 210: rejected
         (20, 30, True)]                               # 7 accepted
# (query, the query whose id it takes, d1 override or None)
SHARED = [(4095, 0, None),                             # the ends of the list: 0 (d1 10) beats 4095 (d1 20)
          (72, 8, None),                               # j, j + 64 at equal distances: the smaller j wins
          (16, 80, 12),                                # j, j + 64, the later one closer (16: 12 against 80: 10); 16 was all there was between survivors 15 and 17
          (1028, 4, None),                             # j, j + 1024 at equal distances (7, 7)
          (24, 1048, 12),                              # j, j + 1024, the later one closer (24: 12 against 1048: 10)
          (1500, 100, None), (3000, 100, None)]        # three of one id: 100 (7), 1500 (7), 3000 (10) -> 100


def flip(rng, base, bits):
    out = base.copy()
    for b in rng.choice(256, bits, replace=False):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def clause_case():
    """-> dict: query (N, 32), xy (N, 2); the index's rows in the order they are added: desc, ids, xyz (f32), tags (int32, -1 = a
    row added without a point: these are the rows [n_with, n_with + n_without)), and plan d1, d2, row_a (N,)"""
    rng = np.random.default_rng(2024)
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    d1 = np.array([KINDS[j % 8][0] for j in range(N)])
    d2 = np.array([KINDS[j % 8][1] if j < N_B else 0 for j in range(N)])
    has = np.array([KINDS[j % 8][2] for j in range(N)])
    id_a = (np.arange(N, dtype=np.uint64) + np.uint64(1000)) * np.uint64(0x100000001)
    for j, other, d in SHARED:
        id_a[j] = id_a[other]
        if d is not None:
            d1[j] = d
    a_rows = np.stack([flip(rng, base[j], d1[j]) for j in range(N)])
    with_pt, without = np.flatnonzero(has), np.flatnonzero(~has)
    b_of = np.flatnonzero(d2 > 0)
    b_rows = np.stack([flip(rng, base[j], d2[j]) for j in b_of])
    desc = np.concatenate([a_rows[with_pt], a_rows[without], b_rows])
    ids = np.concatenate([id_a[with_pt], id_a[without], (b_of.astype(np.uint64) + np.uint64(1 << 40))])
    m = len(desc)
    tags = np.concatenate([with_pt % 5, np.full(len(without), -1), b_of % 3]).astype(np.int32)
    row_a = np.zeros(N, np.int64)
    row_a[with_pt] = np.arange(len(with_pt)); row_a[without] = len(with_pt) + np.arange(len(without))
    xyz = rng.normal(size=(m, 3)).astype(np.float32)
    xyz[tags < 0] = 0
    xy = rng.uniform(0, 1000, (N, 2)).astype(np.float32)
    return dict(query=base, xy=xy, desc=desc, ids=ids, xyz=xyz, tags=tags, d1=d1, d2=d2, row_a=row_a,
                n_with=len(with_pt), n_without=len(without))


def fill(index, case):
    """the rows of a case into an api.DescriptorIndex(points=True): add_points, plain add for the rows without a point, add_points"""
    a, b = case["n_with"], case["n_with"] + case["n_without"]
    for lo, hi in ((0, a), (a, b), (b, len(case["desc"]))):
        if case["tags"][lo] < 0:
            index.add(case["desc"][lo:hi], case["ids"][lo:hi])
        else:
            index.add_points(case["desc"][lo:hi], case["ids"][lo:hi], case["xyz"][lo:hi], case["tags"][lo:hi])


def scene(n, seed, noise_bits=3, outliers=0):
    """n landmarks 4 .. 12 m in front of a 640 x 480 camera at a known pose -> dict: K (3, 3) f32, desc (n, 32), ids, xyz (n, 3) f32
    in the map, tags, query (n, 32) = desc with noise_bits flipped, xy (n, 2) f32 the exact projections (the first `outliers` of them
    moved 50 pixels), R, t (x_cam = R X + t)"""
    rng = np.random.default_rng(seed)
    K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], np.float64)
    th = 0.1
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    t = np.array([0.3, -0.1, 0.5])
    cam = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 12, n)], 1)
    xyz = ((cam - t) @ R).astype(np.float32)           # X = R^T (x_cam - t)
    c = xyz.astype(np.float64) @ R.T + t
    xy = (c[:, :2] / c[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)
    xy[:outliers] += 50
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    query = np.stack([flip(rng, d, noise_bits) for d in desc]) if noise_bits else desc.copy()
    return dict(K=K.astype(np.float32), desc=desc, ids=np.arange(n, dtype=np.uint64) + np.uint64(7), xyz=xyz, tags=(np.arange(n) % 4).astype(np.int32),
                query=query, xy=xy, R=R, t=t)
