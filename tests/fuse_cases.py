"""Synthetic index rows for the landmark fusion's tests (include/svo.h, "Landmark fusion"), shared by the reference's own tests, the
host program's vectors and the GPU tests.  A case is align_cases' dict — desc (m, 32) uint8, ids (m,) uint64, xyz (m, 3) float32,
tags (m,) int32 (-1: a row without a point), the spans src and dst — built once and never changed."""
import functools

import numpy as np

import align_cases as ac
import align_ref as aref

PAD = 37                                              # rows in front of the destination span: dst_lo is no multiple of any chunk size
LATTICE = 0.25                                        # points are multiples of it, so every difference is exact in f32
RADII = (0.0, 0.5, 100.0)                             # coincident points only; two lattice steps; everything


def _freeze(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def near_scene(n_src, n_dst, all_points=False):
    """PAD rows, then the destination span of n_dst rows, then the source span of n_src rows.  Descriptors from a pool of 48 with 0 .. 2
    bits flipped and ids that repeat, so that (dist, row) ties and the other-id rule decide; points on the 0.25 lattice in [0, 4)^3;
    unless all_points, a sixth of the rows on either side carry no point.  With n_src >= 1 and n_dst >= 4 the first destination rows
    sit around source row 0's point p: p + (0.5, 0, 0), exactly at RADII[1]; the next f32 above that on x, one ulp beyond; p - (0, 0,
    0.5); and p itself."""
    rng = np.random.default_rng(100_000 + 17 * n_src + n_dst + (7 if all_points else 0))
    m = PAD + n_dst + n_src
    pool = rng.integers(0, 256, (48, 32), dtype=np.uint8)
    lm = rng.integers(0, 48, m)
    desc = ac.flip_bits(rng, pool[lm], rng.integers(0, 3, m))
    ids = (lm % 20).astype(np.uint64) + np.where(rng.random(m) < 0.5, np.uint64(0), np.uint64(1 << 63))
    xyz = (rng.integers(0, 16, (m, 3)) * LATTICE).astype(np.float32)
    tags = rng.integers(0, 5, m).astype(np.int32)
    if not all_points:
        tags[rng.random(m) < 1 / 6] = -1
    d0, s0 = PAD, PAD + n_dst
    if n_src >= 1 and n_dst >= 4:
        p = np.array([1.25, 2.0, 1.5], np.float32)
        xyz[s0] = p
        xyz[d0] = p + np.array([0.5, 0, 0], np.float32)
        xyz[d0 + 1] = xyz[d0]
        xyz[d0 + 1, 0] = np.nextafter(xyz[d0, 0], np.float32(np.inf))
        xyz[d0 + 2] = p - np.array([0, 0, 0.5], np.float32)
        xyz[d0 + 3] = p
        tags[s0] = tags[d0:d0 + 4] = 1
        desc[d0:d0 + 4] = desc[s0]                                       # all four at distance 0: the gate alone decides
        ids[d0:d0 + 4] = np.array([901, 902, 903, 904], np.uint64)
    return _freeze(dict(desc=desc, ids=ids, xyz=xyz, tags=tags, src=(s0, m), dst=(d0, s0)))


# (source rows, destination rows): every n and every D the tests name, the large ones once each
NEAR_SIZES = ((0, 1000), (1, 0), (1, 1), (63, 7), (64, 8), (65, 9), (200, 1000), (65, 5000), (4096, 1000))


@functools.lru_cache(maxsize=None)
def pair_scene():
    """40 landmarks with k = 3 rows on each side.  A landmark's rows lie within 0.25 of its place, places are 2 apart; descriptors
    are the landmark's with 0 .. 4 bits flipped; every second landmark has the SAME id on both sides, the others their own."""
    rng = np.random.default_rng(4242)
    L, k = 40, 3
    base = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    place = np.stack([2.0 * (np.arange(L) % 8), 2.0 * (np.arange(L) // 8), np.full(L, 6.0)], 1)
    rows = []
    for first_id in (100, 5000):                                         # destination, then source
        lm = rng.permutation(np.repeat(np.arange(L), k))
        d = ac.flip_bits(rng, base[lm], rng.integers(0, 5, len(lm)))
        ids = np.where(lm % 2 == 0, 100 + lm, first_id + lm).astype(np.uint64)
        xyz = (place[lm] + rng.integers(-1, 2, (len(lm), 3)) * LATTICE).astype(np.float32)
        rows.append((d, ids, xyz, np.zeros(len(lm), np.int32)))
    cat = [np.concatenate([rows[0][i], rows[1][i]]) for i in range(4)]
    return _freeze(dict(desc=cat[0], ids=cat[1], xyz=cat[2], tags=cat[3], src=(L * k, 2 * L * k), dst=(0, L * k), radius=0.5))


@functools.lru_cache(maxsize=None)
def merge_scene(n_src, n_dst):
    """Two maps of the same n_dst // 2 landmarks laid over each other: n_dst destination rows, then n_src source rows, each row a
    landmark's descriptor with ONE bit flipped, a different bit for every row of the landmark — so every row's descriptor is its own
    and a search for it returns the row — and its point within 0.25 of the landmark's place (places on a lattice of 1 in [0, 16)^3).
    A third of the source landmarks carry the destination's id already; a tenth of all rows carry no point."""
    rng = np.random.default_rng(9000 + n_src + n_dst)
    L = max(n_dst // 2, 1)
    m = n_dst + n_src
    base = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    place = rng.integers(0, 16, (L, 3)).astype(np.float64)
    lm = rng.integers(0, L, m)
    seen = np.zeros(L, np.int64)
    desc = base[lm]
    for r in range(m):                                                   # row r flips bit (its ordinal among its landmark's rows)
        b = seen[lm[r]]
        seen[lm[r]] += 1
        desc[r, b >> 3] ^= np.uint8(1 << (b & 7))
    assert seen.max() <= 256 and len(np.unique(desc, axis=0)) == m
    ids = (10 + lm).astype(np.uint64)
    own = (lm % 3 != 0) & (np.arange(m) >= n_dst)
    ids[own] += np.uint64(1 << 63)
    xyz = (place[lm] + rng.integers(-1, 2, (m, 3)) * LATTICE).astype(np.float32)
    tags = rng.integers(0, 5, m).astype(np.int32)
    tags[rng.random(m) < 0.1] = -1
    return _freeze(dict(desc=desc, ids=ids, xyz=xyz, tags=tags, src=(n_dst, m), dst=(0, n_dst), radius=0.5))


# ---- the reason for the feature: a map whose overlap exists under two ids
DUP_L, DUP_RADIUS = 160, 0.1
DUP_K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)


@functools.lru_cache(maxsize=None)
def duplicate_scene():
    """DUP_L landmarks 1 apart on x and y (>= 4 x DUP_RADIUS), 8 .. 12 in front of a camera at the origin.  Copy A, ids 1 .. L, is the
    base descriptor with the 8 bits F_A flipped; copy B behind it, ids 1000 + .., the base with F_B flipped and its points 0.03 off
    on every axis; the queries are the base with F_Q flipped, their pixels the exact projections of A's points.  F_A, F_B, F_Q are
    disjoint, so a query is 16 bits from either copy and A's copy 16 bits from B's."""
    rng = np.random.default_rng(20_261_021)
    L = DUP_L
    base = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    bits = rng.permutation(256)[:24]
    flip = []
    for F in (bits[:8], bits[8:16], bits[16:24]):
        d = base.copy()
        for b in F:
            d[:, b >> 3] ^= np.uint8(1 << (b & 7))
        flip.append(d)
    A = np.stack([(np.arange(L) % 16) - 7.5, (np.arange(L) // 16) - 4.5, 8.0 + (np.arange(L) % 5)], 1).astype(np.float32)
    B = (A + np.float32(0.03)).astype(np.float32)
    K = DUP_K.astype(np.float64)
    Ad = A.astype(np.float64)
    xy = np.stack([K[0] * (Ad[:, 0] / Ad[:, 2]) + K[2], K[4] * (Ad[:, 1] / Ad[:, 2]) + K[5]], 1).astype(np.float32)
    ids = np.concatenate([1 + np.arange(L), 1000 + np.arange(L)]).astype(np.uint64)
    return _freeze(dict(base=base, desc=np.concatenate([flip[0], flip[1]]), ids=ids, xyz=np.concatenate([A, B]), tags=np.zeros(2 * L, np.int32),
                        query=flip[2], xy=xy, src=(L, 2 * L), dst=(0, L), radius=DUP_RADIUS))


# ---- relabel: an index of 200 000 rows without points
RELABEL_ROWS = 200_000
RELABEL_N = (0, 1, 4096, 100_000)


@functools.lru_cache(maxsize=None)
def relabel_index():
    """desc (random: every row its own), ids: 50 000 landmark ids, four rows each on average, half of them >= 2^63"""
    rng = np.random.default_rng(77)
    desc = rng.integers(0, 256, (RELABEL_ROWS, 32), dtype=np.uint8)
    universe = rng.permutation(1 << 20)[:50_000].astype(np.uint64) + np.where(np.arange(50_000) % 2 == 0, np.uint64(0), np.uint64(1 << 63))
    ids = universe[rng.integers(0, len(universe), RELABEL_ROWS)]
    return _freeze(dict(desc=desc, ids=ids, universe=universe))


def table_slots(n):
    t = 2
    while t < 2 * n:
        t *= 2
    return t


@functools.lru_cache(maxsize=None)
def relabel_lists(n):
    """(from, to) of n entries over relabel_index()'s ids: `from` drawn with repeats, `to` from the ids in use (chains, and now and
    then from == to) or fresh ones.  From 4096 entries on the first ones are planted: a chain a -> b, b -> c over ids that are all in
    use; a repeated `from` (the first wins); from == to, in front of a later entry with the same `from`, which then wins; and six
    `from` values in use whose probes start at the same slot of the table."""
    rng = np.random.default_rng(500 + n)
    u = relabel_index()["universe"]
    frm = u[rng.integers(0, len(u), n)].copy()
    to = np.where(rng.random(n) < 0.5, u[rng.integers(0, len(u), n)], np.uint64(1 << 40) + rng.integers(0, 1 << 30, n).astype(np.uint64))
    if n == 1:
        frm[0], to[0] = u[3], u[3] + np.uint64(1 << 41)
    if n >= 4096:
        mask = table_slots(n) - 1
        slot = np.array([aref.mix64(int(v)) & mask for v in u[:20_000]])
        vals, counts = np.unique(slot, return_counts=True)
        clash = u[:20_000][slot == vals[counts.argmax()]][:6]
        assert len(clash) >= 3
        plant_f = [u[10], u[11], u[12], u[12], u[13], u[13]] + list(clash)
        plant_t = [u[11], u[14], u[15], u[16], u[13], u[17]] + [np.uint64((1 << 50) + i) for i in range(len(clash))]
        frm[:len(plant_f)] = np.array(plant_f, np.uint64)
        to[:len(plant_t)] = np.array(plant_t, np.uint64)
    frm.setflags(write=False); to.setflags(write=False)
    return frm, to
