"""Synthetic index rows for the place candidates' tests (include/svo.h, "Place candidates"), shared by the reference's own tests, the
host program's vectors and the GPU tests.  A case is align_cases' dict — desc (m, 32) uint8, ids (m,) uint64, xyz (m, 3) float32,
tags (m,) int32 (-1: a row without a point) — built once and never changed."""
import functools

import numpy as np

import align_cases as ac
import align_ref as aref

BIG_TAG = 5_000_000                                   # a tag above every span the tests use but the whole-limit one's


def _freeze(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def table_slots(n):
    t = 2
    while t < 2 * n:
        t *= 2
    return t


# ---- the reason for the feature: 12 keyframes, every landmark seen from three consecutive ones
KEYFRAMES, PER_GROUP, SEEN_IN, QUERIED = 12, 40, 3, 5
PLANTED_K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)


@functools.lru_cache(maxsize=None)
def planted_scene():
    """Group g of 40 landmarks is first seen in keyframe g and again in g + 1 and g + 2 (while those exist); keyframe k's rows — tag
    k, contiguous — are the groups k - 2, k - 1, k.  A row is its landmark's descriptor with 0 .. 4 bits flipped.  The queries are
    group QUERIED's descriptors with 3 bits flipped, their pixels the exact projections of the landmarks' points (8 .. 12 in front
    of a camera at the origin, 1 apart on x and y)."""
    rng = np.random.default_rng(32_000)
    L = KEYFRAMES * PER_GROUP
    base = rng.integers(0, 256, (L, 32), dtype=np.uint8)
    j = np.arange(PER_GROUP)
    lm_rows, tags = [], []
    for k in range(KEYFRAMES):
        for g in range(max(0, k - SEEN_IN + 1), k + 1):
            lm_rows.append(g * PER_GROUP + j)
            tags.append(np.full(PER_GROUP, k))
    lm, tags = np.concatenate(lm_rows), np.concatenate(tags).astype(np.int32)
    desc = ac.flip_bits(rng, base[lm], rng.integers(0, 5, len(lm)))
    i = lm % PER_GROUP
    pts = np.stack([(i % 8) - 3.5, (i // 8) - 2.0, 8.0 + (i % 5)], 1).astype(np.float32)
    q_lm = QUERIED * PER_GROUP + j
    query = ac.flip_bits(rng, base[q_lm], 3)
    P = np.stack([(j % 8) - 3.5, (j // 8) - 2.0, 8.0 + (j % 5)], 1).astype(np.float64)
    K = PLANTED_K.astype(np.float64)
    xy = np.stack([K[0] * (P[:, 0] / P[:, 2]) + K[2], K[4] * (P[:, 1] / P[:, 2]) + K[5]], 1).astype(np.float32)
    return _freeze(dict(desc=desc, ids=(1000 + lm).astype(np.uint64), xyz=pts, tags=tags, query=query, xy=xy, query_ids=(1000 + q_lm).astype(np.uint64)))


# ---- rule 2: rows whose tags come in every pattern the sweep's wave loop meets
VOTE_KINDS = ("runs", "one_tag", "own_tag", "interleaved")
VOTE_ROWS = dict(runs=70_000, one_tag=40_000, own_tag=3_000, interleaved=20_011)


@functools.lru_cache(maxsize=None)
def vote_scene(kind):
    """runs: tag runs of 1, 63, 64, 65, 1, 200 and 700 rows in turn (boundaries inside waves), the tag growing by 1, 2 or 3 a run;
    one_tag: every row tag 7; own_tag: row r has tag r; interleaved: a random tag of 0 .. 49 a row.  But for own_tag a twentieth
    of the rows carry no point (-1) and a twentieth the tag BIG_TAG.  A landmark has four rows on average; half of the ids are
    >= 2^63, and 0 and 2^64 - 1 are among them."""
    rng = np.random.default_rng(600 + VOTE_KINDS.index(kind))
    m = VOTE_ROWS[kind]
    if kind == "runs":
        tags, t, i = np.zeros(m, np.int32), 0, 0
        lens = (1, 63, 64, 65, 1, 200, 700)
        at = 0
        while at < m:
            n = lens[i % len(lens)]
            tags[at:at + n] = t
            at += n; i += 1; t += 1 + i % 3
    elif kind == "one_tag":
        tags = np.full(m, 7, np.int32)
    elif kind == "own_tag":
        tags = np.arange(m, dtype=np.int32)
    else:
        tags = rng.integers(0, 50, m).astype(np.int32)
    if kind != "own_tag":
        u = rng.random(m)
        tags[u < 0.05] = -1
        tags[(u >= 0.05) & (u < 0.10)] = BIG_TAG
    n_lm = m // 4
    universe = rng.permutation(1 << 22)[:n_lm].astype(np.uint64) + np.where(np.arange(n_lm) % 2 == 0, np.uint64(0), np.uint64(1 << 63))
    universe[0], universe[1] = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    ids = universe[rng.integers(0, n_lm, m)]
    ids[:8] = universe[:8]                                               # ids 0 and 2^64 - 1 are in use
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    xyz = rng.integers(0, 16, (m, 3)).astype(np.float32)
    return _freeze(dict(desc=desc, ids=ids, xyz=xyz, tags=tags, universe=universe))


ID_COUNTS = (0, 1, 64, 65, 4096)


@functools.lru_cache(maxsize=None)
def id_list(kind, n):
    """n ids for vote_scene(kind): three quarters drawn from the ids in use with repeats, a quarter absent from the index; from 64
    on the first are planted — 0 and 2^64 - 1, an id three times, and six ids in use whose probes start at one slot of the set
    (fuse_cases' construction, for the set of n entries)."""
    rng = np.random.default_rng(900 + n)
    u = vote_scene(kind)["universe"]
    lst = np.where(rng.random(n) < 0.75, u[rng.integers(0, len(u), n)], np.uint64(1 << 40) + rng.integers(0, 1 << 30, n).astype(np.uint64))
    if n == 1:
        lst[0] = u[0]
    if n >= 64:
        clash = colliding(u, n, 6)
        plant = [u[0], u[1], u[5], u[5], u[5]] + list(clash)
        lst[:len(plant)] = np.array(plant, np.uint64)
    lst.setflags(write=False)
    return lst


def colliding(universe, n, k):
    """up to k values of the universe whose probes start at the same slot of a set of n entries"""
    mask = table_slots(n) - 1
    u = universe[:3000]
    slot = np.array([aref.mix64(int(v)) & mask for v in u])
    vals, counts = np.unique(slot, return_counts=True)
    clash = u[slot == vals[counts.argmax()]][:k]
    assert len(clash) >= 2
    return clash


# ---- rule 3: hand-made histograms.  (name, votes per tag from tag_lo on, tag_lo, min_votes, separation, max_places, the tags expected)
PICK_CASES = (
    ("ties_take_the_smaller_tag", (3, 5, 5, 2, 5), 0, 1, 0, 8, (1, 2, 4, 0, 3)),
    ("separation_1", (3, 5, 5, 2, 5), 0, 1, 1, 8, (1, 4)),
    ("separation_above_the_span", (3, 5, 5, 2, 5), 0, 1, 100, 8, (1,)),
    ("suppression_chain", (1, 2, 3, 4, 5, 6, 7), 0, 1, 1, 8, (6, 4, 2, 0)),       # 5 leaves with 6 and so does not take 4 with it
    ("places_at_both_ends", (9, 0, 0, 0, 8), 10, 1, 0, 8, (10, 14)),
    ("both_ends_with_separation", (9, 1, 0, 1, 8), 10, 1, 1, 8, (10, 14)),
    ("min_votes_above_every_bin", (3, 5, 5, 2, 5), 0, 6, 0, 8, ()),
    ("min_votes_cuts", (3, 5, 5, 2, 5), 0, 3, 0, 8, (1, 2, 4, 0)),
    ("fewer_places_than_max_places", (0, 4, 0, 0, 2), 3, 1, 0, 8, (4, 7)),
    ("max_places_1", (3, 5, 5, 2, 5), 0, 1, 0, 1, (1,)),
    ("max_places_64", tuple(1 + (7 * i) % 11 for i in range(70)), 0, 1, 0, 64, None),      # None: 64 places, the reference's order
)


@functools.lru_cache(maxsize=None)
def histogram_scene(votes, tag_lo):
    """An index whose votes for its own queries are the histogram: tag tag_lo + b holds votes[b] rows, each a landmark of its own
    with a random descriptor, which are the queries (distance 0, every other row far); and one more row per tag that no query
    recognises — a descriptor of its own that is not asked for.  Tags shuffled row by row: not contiguous."""
    rng = np.random.default_rng(7_000 + len(votes) + tag_lo)
    tags = np.concatenate([np.full(v + 1, tag_lo + b) for b, v in enumerate(votes)]).astype(np.int32)
    asked = np.concatenate([np.arange(v + 1) < v for v in votes])
    order = rng.permutation(len(tags))
    tags, asked = tags[order], asked[order]
    m = len(tags)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    ids = (np.uint64(1 << 63) + np.arange(m).astype(np.uint64))
    xyz = rng.integers(0, 16, (m, 3)).astype(np.float32)
    return _freeze(dict(desc=desc, ids=ids, xyz=xyz, tags=tags, query=desc[asked].copy()))
