"""Inputs of the guided search's tests (include/svo.h, "Guided search").

repeated_scene(): the repeated-structure scene.  160 landmarks 4 .. 16 m in front of a 640 x 360 camera (fx = fy = 500), each stored
a second time 4 m to the side with the same descriptor under another id.  The queries are the landmarks' descriptors with 12 bits
flipped at their true projections plus pixel noise (sigma 0.2 px); the prior is the true pose off by about 0.01 rad and 0.1 m.
Unguided, every query finds its landmark and the copy at the same distance and the ratio test rejects it; within 24 px of the
prior's projection only the right copy remains.

clause_rows() / clause_pixels(): rows and query pixels on both sides of every clause of rules 1 and 2, for the host program and the
GPU tests alike.

planned_case(): an index of 2304 rows and 4096 queries in which the planned situations of the guided search occur — see its
docstring."""
import numpy as np

from reloc_cases import flip

RADIUS = 24.0
K_SCENE = np.array([[500, 0, 320], [0, 500, 180], [0, 0, 1]], np.float32)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def repeated_scene(n=160, seed=2501):
    """-> dict: K (3, 3) f32; the index's rows desc (2n, 32), ids, xyz (2n, 3) f32, tags — rows [0, n) the landmarks, [n, 2n) their
    copies 4 m to the side; query (n, 32), xy (n, 2) f32; the true pose R, t and the prior R0, t0 (x_cam = R X + t); radius"""
    rng = np.random.default_rng(seed)
    K = K_SCENE.astype(np.float64)
    R, t = rot(0.02, -0.05, 0.01), np.array([0.2, -0.1, 0.3])
    z = rng.uniform(4, 16, n)
    px = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 340, n)], 1)
    cam = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1)
    xyz = ((cam - t) @ R).astype(np.float32)                           # X = R^T (x_cam - t)
    c = xyz.astype(np.float64) @ R.T + t
    xy = c[:, :2] / c[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    xy = (xy + rng.normal(0, 0.2, (n, 2))).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    query = np.stack([flip(rng, d, 12) for d in desc])
    copy = (xyz.astype(np.float64) + np.array([4.0, 0, 0]) @ R).astype(np.float32)   # 4 m along the camera's x axis
    ids = np.arange(n, dtype=np.uint64) + np.uint64(100)
    R0 = rot(0.006, -0.006, 0.005) @ R                                 # about 0.01 rad in all
    t0 = t + np.array([0.06, -0.05, 0.06])                             # about 0.1 m
    return dict(K=K_SCENE, desc=np.concatenate([desc, desc]), ids=np.concatenate([ids, ids + np.uint64(1 << 20)]),
                xyz=np.concatenate([xyz, copy]), tags=np.zeros(2 * n, np.int32), query=query, xy=xy, R=R, t=t, R0=R0, t0=t0, radius=RADIUS)


# ---- the clauses of rules 1 and 2
# Two priors over the same rows.  I: the identity with fy = 0.  II: t2 = 1e-300 and fx = 0, under which a row with z == 0 has
# Zc = 1e-300 > 0 and, with x = 1e30, an infinite f64 quotient: 0 x inf is NaN, so the row is invisible.
CLAUSE_GUIDES = [(np.array([[400, 0, 300], [0, 0, 200], [0, 0, 1]], np.float32), np.eye(3), np.zeros(3)),
                 (np.array([[0, 0, 300], [0, 250, 200], [0, 0, 1]], np.float32), np.eye(3), np.array([0.0, 0.0, 1e-300]))]
CLAUSE_VISIBLE = [[True, False, False, False, False, False, True, True],
                  [True, False, False, True, False, False, True, True]]


def clause_rows():
    """-> xyz (8, 3) f32, tags (8,) int32.  Under prior I: 0 plain, visible at (400, 200); 1 Zc == 0; 2 Zc < 0; 3 Zc so small that u
    overflows f32 while the f64 value is finite; 4 Zc == 0 (under II: the infinite quotient, NaN; row 1 overflows in v there); 5 no point; 6 visible, since
    fy = 0 times a finite quotient is 0; 7 u = 3.2e38, just inside f32: visible.  CLAUSE_VISIBLE has the plan under both priors."""
    xyz = np.array([[1, 0, 4], [1, 1, 0], [1, 1, -2], [1, 0, 1e-37], [1e30, 1, 0], [1, 0, 4], [1, 3, 4], [1e30, 0, 1.25e-6]], np.float32)
    tags = np.array([0, 0, 0, 0, 0, -1, 2, 0], np.int32)
    return xyz, tags


def clause_pixels(u, v, radius):
    """query pixels against a row that projects to (u, v) for every clause of rule 2 at this radius -> (xy (12, 2) f32, admits (12,)
    bool as planned): |u - x| == radius, the next f32 beyond it, on both sides and both axes, an exact hit, NaN and infinite pixels"""
    r, u, v = np.float32(radius), np.float32(u), np.float32(v)
    inf = np.float32(np.inf)
    xy = [(u + r, v, True), (np.nextafter(np.float32(u + r), inf), v, False), (u - r, v, True), (np.nextafter(np.float32(u - r), -inf), v, False),
          (u, v + r, True), (u, np.nextafter(np.float32(v + r), inf), False), (u, v, True), (np.nan, v, False), (u, np.nan, False),
          (np.inf, v, False), (u, -np.inf, False), (np.inf, np.inf, False)]
    return np.array([(a, b) for a, b, _ in xy], np.float32), np.array([c for _, _, c in xy])


# ---- the planned case of the GPU match test
N_ROWS, N_QUERIES = 2304, 4096


def planned_case():
    """An index of 2304 rows (36 chunks of 64, 2.25 chunks of 1024) seen by the identity prior with K_SCENE, and 4096 queries.

    Rows sit on a lattice: row r projects near pixel (40 + 16 (r % 36), 30 + 5 (r // 36)) — 36 columns, 64 rows of pixels — at
    depths 5 .. 9 m, so with radius 12 a query admits a few dozen rows spread over many chunks.  Queries 0 .. 4095 sit at random
    pixels of the image, their descriptors near one of the rows they admit (or near nothing).  Then the planned situations, each on
    its own query / rows, all far outside the image (|pixel| > 5000) so that the lattice does not interfere:
      A  query 0: no admissible row in the whole range;
      B  query 1: admissible only in row 63 (the last of chunk 0 at 64) and row 64 (the first of the next); likewise rows 1023, 1024;
      C  queries 64 .. 127 (one wave with the sort off): they admit only rows of chunks 30 .. 35 (at 64), nothing in chunk 0 .. 29;
      D  queries 128 .. 191: exactly one lane (query 130) admits row 700, nobody else admits anything near it;
      E  query 2: its best admissible row 200 and the nearest row of all, 201, carry the same id, 201 is inadmissible;
      F  query 3: the best in row 10, the only admissible row of another id is row 2203 (another chunk at 64 and at 1024);
      G  rows 2296 .. 2303 are clause_rows() (the clause priors are applied to them by the tests).
    -> dict: K, R, t, radius; desc, ids, xyz, tags (rows); query, xy"""
    rng = np.random.default_rng(77)
    K = K_SCENE.astype(np.float64)
    m, n = N_ROWS, N_QUERIES
    r = np.arange(m)
    z = rng.uniform(5, 9, m)
    pu, pv = 40 + 16.0 * (r % 36) + rng.uniform(-3, 3, m), 30 + 5.0 * (r // 36) + rng.uniform(-2, 2, m)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    ids = (rng.integers(0, 900, m).astype(np.uint64) + np.uint64(1)) * np.uint64(0x100000001)   # shared ids: the second's rule has work
    tags = (r % 7).astype(np.int32)
    tags[rng.random(m) < 0.03] = -1                                      # some rows without a point
    xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 360, n)], 1)
    query = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    near = rng.integers(0, m, n)
    for j in range(0, n, 2):                                             # every other query: a noisy copy of a row close to its pixel
        d = np.abs(pu - xy[j, 0]) + np.abs(pv - xy[j, 1])
        near[j] = int(np.argmin(d))
        query[j] = flip(rng, desc[near[j]], int(rng.integers(0, 30)))

    def put(row, u, v, depth=6.0):
        pu[row], pv[row], z[row] = u, v, depth
        tags[row] = 1

    far = 6000.0
    xy[0] = (-far, -far)                                                 # A
    put(63, far, far); put(64, far + 5, far); put(1023, far, far + 9); put(1024, far - 4, far + 9); xy[1] = (far, far + 4)   # B
    ids[63], ids[64], ids[1023], ids[1024] = 11, 12, 13, 14
    query[1] = flip(rng, desc[1024], 9)
    for k, j in enumerate(range(64, 128)):                               # C
        row = 30 * 64 + 5 * k
        put(row, 2 * far + 40 * k, -far)
        xy[j] = (2 * far + 40 * k + 1, -far)
        query[j] = flip(rng, desc[row], k % 20)
    for j in range(128, 192):                                            # D
        xy[j] = (-2 * far - 50 * (j - 128), far)
    put(700, -2 * far - 100, far + 3)
    query[130] = flip(rng, desc[700], 5)
    put(200, far, -far); put(201, far + 100, -far); ids[200] = ids[201] = 4242; xy[2] = (far + 2, -far)   # E
    query[2] = flip(rng, desc[200], 20); desc[201] = flip(rng, query[2], 2)
    put(10, -far, far); put(2203, -far + 7, far - 7); ids[10], ids[2203] = 77, 78; xy[3] = (-far + 1, far - 1)   # F
    query[3] = flip(rng, desc[10], 4)
    cam = np.stack([(pu - K[0, 2]) / K[0, 0] * z, (pv - K[1, 2]) / K[1, 1] * z, z], 1)
    xyz = cam.astype(np.float32)
    cx, ct = clause_rows()                                            # G
    xyz[m - len(cx):] = cx
    tags[m - len(cx):] = ct
    xyz[tags < 0] = 0
    return dict(K=K_SCENE, R=np.eye(3), t=np.zeros(3), radius=12.0, desc=desc, ids=ids, xyz=xyz, tags=tags, query=query,
                xy=xy.astype(np.float32))
