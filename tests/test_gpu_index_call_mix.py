"""One descriptor index taken through every call family, twice, against fresh indexes (include/svo.h, "Descriptor index" to "Batched
insertion").  The calls of an index share their host side — the stream, the pinned staging, the partial states, the maintenance
scratch, the growable pinned blocks — so a call must not depend on what an earlier call of another family left there.  The worn
index goes through add_points and add_obs; match, match_guided and project; select, localize and localize_guided; localize_batch with
three cameras; match_rows, pair_rows and align; match_near, pair_near, fuse and relabel; tag_votes, places_from_ids and places;
retire by ids, consolidate and transform_points; read_rows — in that order, twice.  Before each call a fresh index is loaded with
read_rows of the worn one, the same call is made on both, and everything the call returns — and, where it changes the index, the
rows it leaves — is compared bit for bit: both sides run the same kernels on the same inputs, poses included.

The shapes are the smallest that cross a wave and a chunk: 300 rows, 65 queries, 64 rows a chunk.  The second pass is larger, so
that each of the four growable buffers grows behind the calls' backs.  Their first sizes are 4096 partial states and 64 KiB:
  the partial states: 260 queries over more than 16 chunks;
  the maintenance scratch and the pinned row staging: add_obs with 1000 rows of 64 + 32 bytes;
  the pinned place block: tag_votes with 5000 bins of 16 bytes.
The two that have stats keep their contract after every call: the size never shrinks and the outgrown bytes stay below it."""
import numpy as np
import pytest

from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

CAPACITY, CHUNK = 4096, 64
FIRST_BYTES, FIRST_STATES = 64 << 10, 4096             # the growable buffers' first sizes
OBS_ROW_BYTES, BIN_BYTES = 64 + 32, 16                # a staged row (observation and descriptor), a tag's bin
K = np.array([[400.0, 0, 320], [0, 400, 240], [0, 0, 1]], np.float32)
R0, T0 = np.eye(3), np.zeros(3)
RADIUS_PX, RADIUS_MAP, INLIER_DIST = 8.0, 0.1, 0.05

# map A: n_a landmarks; map B: the first n_b of them seen again (noisy descriptors, other ids, points through MOVE);
# obs: the entries of add_obs; n_q queries: the first landmarks of A seen at their projections; bins: tag_votes' tag span
PASSES = [dict(n_a=200, n_b=60, obs=(29, 19), n_q=65, bins=8),                 # 300 rows: a seventh of the observation rows is not kept
          dict(n_a=400, n_b=260, obs=(600, 0, 400), n_q=260, bins=5000)]


def rigid(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


MOVE = rigid(0.008, [0.02, -0.01, 0.015])             # B's points: within RADIUS_MAP of A's on every axis


def noisy(rng, desc, flips):
    """each row with `flips` of its 256 bits turned"""
    out = desc.copy()
    for row in out:
        for bit in rng.choice(256, flips, replace=False):
            row[bit >> 3] ^= 1 << (bit & 7)
    return out


def material(api, k, p):
    """what pass k adds and asks for"""
    rng = np.random.default_rng(350 + k)
    n_a, n_b, n_q = p["n_a"], p["n_b"], p["n_q"]
    base, tag0 = np.uint64((k + 1) * 1000000), 100 * k
    a_desc = rng.integers(0, 256, (n_a, 32), dtype=np.uint8)
    a_xyz = np.column_stack([rng.uniform(-2, 2, n_a), rng.uniform(-2, 2, n_a), rng.uniform(4, 8, n_a)]).astype(np.float32)
    b_xyz = (a_xyz[:n_b].astype(np.float64) @ MOVE[:3, :3].T + MOVE[:3, 3]).astype(np.float32)
    m = dict(desc=np.concatenate([a_desc, noisy(rng, a_desc[:n_b], 8)]), xyz=np.concatenate([a_xyz, b_xyz]),
             ids=np.concatenate([base + np.arange(n_a, dtype=np.uint64), base + np.uint64(500000) + np.arange(n_b, dtype=np.uint64)]),
             tags=np.concatenate([tag0 + np.arange(n_a) // 25, tag0 + 20 + np.arange(n_b) // 25]).astype(np.int32))
    m["a_ids"] = m["ids"][:n_a]
    m["query"] = noisy(rng, a_desc[:n_q], 6)
    m["xy"] = (a_xyz[:n_q, :2] / a_xyz[:n_q, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)
    m["obs"], m["obs_desc"] = [], []
    for b, rows in enumerate(p["obs"]):
        o = np.zeros(rows, api._lib.TRACK_OBS_DTYPE)
        o["id"] = 700000 + 10000 * b + np.arange(rows)
        o["xyz"] = np.column_stack([rng.uniform(-2, 2, rows), rng.uniform(-2, 2, rows), rng.uniform(4, 8, rows)])
        o["flags"] = 3                                                      # INLIER | HAS_XYZ ...
        o["flags"][::7] = 2                                                 # ... but for every seventh row, which is not kept
        m["obs"].append(o)
        m["obs_desc"].append(rng.integers(0, 256, (rows, 32), dtype=np.uint8))
    m["obs_T"] = [rigid(0.01 * (b + 1), [0.1 * b, 0.0, 0.05]) for b in range(len(p["obs"]))]
    m["obs_tags"] = [tag0 + 40 + b for b in range(len(p["obs"]))]
    m["obs_base"] = np.full(len(p["obs"]), base, np.uint64)
    return m


def same(a, b):
    """bit for bit, through the tuples, dicts and records the calls return"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def fresh_copy(api, ix):
    """a new index holding the rows of ix, set as ix is"""
    f = api.DescriptorIndex(CAPACITY, points=True)
    f.chunk_rows = CHUNK
    f.set_timing(True)
    desc, ids, xyz, tags = ix.read_rows()
    if len(ids):
        f.add_points(desc, ids, xyz, tags)
    return f


class Worn:
    """the worn index, the stats it has shown so far, and the one way a call is made and compared"""

    def __init__(self, api):
        self.api = api
        self.ix = api.DescriptorIndex(CAPACITY, points=True)
        self.ix.chunk_rows = CHUNK
        self.ix.set_timing(True)
        self.seen = dict(search=0, retire=0)

    def check_stats(self, name):
        for which, st in (("search", self.ix.stats()), ("retire", self.ix.retire_stats())):
            assert st["scratch_bytes"] >= self.seen[which], (name, which, st)
            assert st["scratch_bytes_outgrown"] < st["scratch_bytes"] or st["scratch_bytes"] == st["scratch_bytes_outgrown"] == 0, (name, which, st)
            assert (st["scratch_allocations"] == 0) == (st["scratch_bytes"] == 0), (name, which, st)
            self.seen[which] = st["scratch_bytes"]

    def call(self, name, f, changes=False, timed=None):
        """f(index) on the worn index and on a fresh copy of it -> the worn index's result"""
        fresh = fresh_copy(self.api, self.ix)
        try:
            got, want = f(self.ix), f(fresh)
            assert same(got, want), "%s: the worn index and a fresh one differ\n%r\n%r" % (name, got, want)
            if changes:
                assert self.ix.size == fresh.size and same(self.ix.read_rows(), fresh.read_rows()), "%s: the rows it left differ" % name
            if timed:                                                        # the call timed its span, into its own figure
                ms = dict(search=self.ix.stats, retire=self.ix.retire_stats, insert=self.ix.insert_stats)[timed]()["last_kernels_ms"]
                print(name, timed, ms)
                assert ms > 0, (name, timed)
        finally:
            fresh.close()
        self.check_stats(name)
        return got

    def close(self):
        self.ix.close()


def one_pass(w, k, p):
    m = material(w.api, k, p)
    n_a, n_b, n_q = p["n_a"], p["n_b"], p["n_q"]
    q, xy = m["query"], m["xy"]
    a0 = w.ix.size
    A, B = (a0, a0 + n_a), (a0 + n_a, a0 + n_a + n_b)
    in_a = dict(row_lo=A[0], row_hi=A[1])                                   # B holds the same landmarks under other ids: the ratio test would drop them
    cut = [0, n_q // 2, n_q // 2 + 7, n_q]
    cams = [slice(cut[c], cut[c + 1]) for c in range(3)]
    guides = [(R0, T0, RADIUS_PX)] * 3 if k else None                       # the first pass unguided, the second guided

    # ---- appends
    assert w.call("add_points", lambda ix: ix.add_points(m["desc"], m["ids"], m["xyz"], m["tags"]), changes=True) == a0
    first, added = w.call("add_obs", lambda ix: ix.add_obs(m["obs"], m["obs_desc"], id_base=m["obs_base"], with_points=True, cam_to_map=m["obs_T"],
                                                           tags=m["obs_tags"]), changes=True, timed="insert")
    assert added.tolist() == [r - (r + 6) // 7 for r in p["obs"]] and first[0] == B[1]
    assert w.ix.stats()["last_kernels_ms"] == 0                             # a batched insertion clears the search's figure
    assert k or w.ix.size == 300
    assert (n_q * -(-w.ix.size // CHUNK) > FIRST_STATES) == (k == 1)           # the partial states of the searches below: only the second pass outgrows the first size
    # ---- searches
    out = w.call("match", lambda ix: ix.match(q), timed="search")
    assert (out["row"] == A[0] + np.arange(n_q)).all()
    out = w.call("match_guided", lambda ix: ix.match_guided(K, R0, T0, RADIUS_PX, q, xy, *A), timed="search")
    assert (out["row"] == A[0] + np.arange(n_q)).all()
    assert w.call("project", lambda ix: ix.project(K, R0, T0), timed="search").shape == (w.ix.size, 2)
    # ---- relocalisation
    c = w.call("select", lambda ix: ix.select(q, xy, **in_a), timed="search")
    assert len(c["query"]) == n_q
    res, _ = w.call("localize", lambda ix: ix.localize(K, q, xy, **in_a), timed="search")
    assert res.success and res.n_candidates == n_q
    res, _ = w.call("localize_guided", lambda ix: ix.localize_guided(K, R0, T0, RADIUS_PX, q, xy, **in_a), timed="search")
    assert res.success
    batch = w.call("localize_batch", lambda ix: ix.localize_batch(K, [q[s] for s in cams], [xy[s] for s in cams], guides=guides, **in_a), timed="search")
    assert [r.n_candidates for r, _ in batch] == [s.stop - s.start for s in cams] and batch[0][0].success
    # ---- alignment
    out = w.call("match_rows", lambda ix: ix.match_rows(B, A), timed="search")
    assert (out["row"] == A[0] + np.arange(n_b)).all()
    ps, pd = w.call("pair_rows", lambda ix: ix.pair_rows(B, A), timed="search")
    assert len(ps) == n_b
    res, pairs = w.call("align", lambda ix: ix.align(B, A, INLIER_DIST), timed="search")
    assert res.success and res.n_pairs == n_b and np.abs(res.T - np.linalg.inv(MOVE)).max() < 1e-3
    # ---- fusion
    out = w.call("match_near", lambda ix: ix.match_near(B, A, RADIUS_MAP), timed="search")
    assert (out["row"] == A[0] + np.arange(n_b)).all()
    ps, pd = w.call("pair_near", lambda ix: ix.pair_near(B, A, RADIUS_MAP), timed="search")
    assert len(ps) == n_b
    res, pairs = w.call("fuse", lambda ix: ix.fuse(B, A, RADIUS_MAP), changes=True, timed="search")
    assert res.n_pairs == n_b and res.n_fused == n_b and res.n_rows_relabelled == n_b
    obs_ids = w.ix.read_rows((B[1], -1), want=("ids",))[1]
    moved = obs_ids[:: max(1, len(obs_ids) // 20)]
    assert w.call("relabel", lambda ix: ix.relabel(moved, moved + np.uint64(1 << 40)), changes=True, timed="search") == len(moved)
    # ---- place candidates
    tags = (0, p["bins"] - 1)
    votes, rows, _, _ = w.call("tag_votes", lambda ix: ix.tag_votes(m["a_ids"][:n_q], tags=tags), timed="search")
    assert len(votes) == p["bins"] and rows.sum() > 0
    own = (100 * k, 100 * k + 99)                                           # this pass's tags
    res, places = w.call("places_from_ids", lambda ix: ix.places_from_ids(m["a_ids"][:n_q], rows=(a0, -1), tags=own), timed="search")
    assert res.n_places >= 1 and res.n_landmarks == n_q
    res, places, c = w.call("places", lambda ix: ix.places(q, rows=A, tags=own), timed="search")
    assert res.n_landmarks == n_q and res.n_places >= 1
    # ---- maintenance
    size = w.ix.size
    kept_before = w.call("retire", lambda ix: ix.retire(drop_ids=m["a_ids"][n_q:n_q + 10]), changes=True, timed="retire")
    assert w.ix.size == kept_before[-1] == size - 10
    size = w.ix.size
    res, kept_before = w.call("consolidate", lambda ix: ix.consolidate(2 * RADIUS_MAP), changes=True, timed="retire")
    assert res.n_dropped >= n_b - 10 and res.n_kept == w.ix.size == size - res.n_dropped and kept_before[-1] == w.ix.size
    assert w.call("transform_points", lambda ix: ix.transform_points(rigid(-0.02, [0.05, 0.02, 0.1])), changes=True, timed="retire") == (w.ix.size, 0)
    # ---- the rows back
    assert len(w.call("read_rows", lambda ix: ix.read_rows())[1]) == w.ix.size


def test_a_worn_index_answers_as_a_fresh_one(api):
    small, large = PASSES
    for p in PASSES:                                                        # the sizes that decide which pass grows what
        assert (sum(p["obs"]) * OBS_ROW_BYTES > FIRST_BYTES) == (p is large)
        assert (p["bins"] * BIN_BYTES > FIRST_BYTES) == (p is large)
    w = Worn(api)
    try:
        one_pass(w, 0, small)
        first = w.ix.stats(), w.ix.retire_stats()
        assert first[0]["scratch_allocations"] == 1 and first[0]["scratch_bytes"] == FIRST_STATES * 16
        assert first[1]["scratch_allocations"] >= 1
        one_pass(w, 1, large)
        second = w.ix.stats(), w.ix.retire_stats()
        for a, b in zip(first, second):                                     # each grew, and what it outgrew is kept and counted
            assert b["scratch_allocations"] > a["scratch_allocations"] and b["scratch_bytes"] > a["scratch_bytes"]
            assert b["scratch_bytes_outgrown"] >= a["scratch_bytes"]
    finally:
        w.close()
