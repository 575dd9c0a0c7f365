"""Reference for the descriptor index's maintenance calls (include/svo.h, "Index maintenance"), straight from the two rules, in plain
numpy with Python loops: which rows a retire rule keeps and the remapping kept_before, and the transform of the points in f64 with
every product and sum an operation of its own (numpy rounds each; nothing is fused) and .astype(np.float32).  It knows nothing of
flags arrays, hash tables, scans or slabs.  naive_retire states the retire rule a second time, row against row in O(n^2), for
tests/test_desc_retire_ref.py.  index_case is the generator the CPU and the GPU tests share."""
import numpy as np

POINT_NONE = -1
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def _scope(n0, rows):
    lo, hi = int(rows[0]), int(rows[1])
    hi = n0 if hi == -1 else hi
    assert 0 <= lo <= hi <= n0
    return lo, hi


def retire(ids, tags, rows=(0, -1), tag_window=None, drop_ids=None, latest_per_id=False, scope=False):
    """ids (n0,) uint64, tags (n0,) int32 (None: an index without points) -> (keep (n0,) bool, kept_before (n0 + 1,) int32)"""
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    n0 = len(ids)
    lo, hi = _scope(n0, rows)
    alive = np.zeros(n0, bool)
    listed = set() if drop_ids is None else set(int(v) for v in np.asarray(drop_ids).astype(np.uint64).reshape(-1))
    for r in range(lo, hi):
        a = not scope
        if tag_window is not None:
            a = a and int(tag_window[0]) <= int(tags[r]) <= int(tag_window[1])
        if drop_ids is not None:
            a = a and int(ids[r]) not in listed
        alive[r] = a
    keep = np.ones(n0, bool)
    keep[lo:hi] = alive[lo:hi]
    if latest_per_id:
        rows_alive = np.flatnonzero(alive)
        if len(rows_alive):
            uniq, inverse = np.unique(ids[rows_alive], return_inverse=True)
            last = np.full(len(uniq), -1, np.int64)
            np.maximum.at(last, inverse, rows_alive)
            keep[rows_alive] = last[inverse] == rows_alive
    kept_before = np.zeros(n0 + 1, np.int32)
    kept_before[1:] = np.cumsum(keep)
    return keep, kept_before


def naive_retire(ids, tags, rows=(0, -1), tag_window=None, drop_ids=None, latest_per_id=False, scope=False):
    """the rule once more, as the header words it: alive1 per row, keep by looking at every later row, kept_before by counting"""
    n0 = len(ids)
    lo, hi = _scope(n0, rows)
    drop = [] if drop_ids is None else [int(v) for v in drop_ids]

    def alive1(r):
        if not lo <= r < hi or scope:
            return False
        if tag_window is not None and not (tag_window[0] <= int(tags[r]) <= tag_window[1]):
            return False
        if drop_ids is not None and any(int(ids[r]) == d for d in drop):
            return False
        return True

    def keep(r):
        if not lo <= r < hi:
            return True
        if not alive1(r):
            return False
        return not latest_per_id or not any(alive1(q) and int(ids[q]) == int(ids[r]) for q in range(r + 1, n0))

    k = np.array([keep(r) for r in range(n0)], bool)
    return k, np.array([sum(k[:r]) for r in range(n0 + 1)], np.int32)


def transform(xyz, tags, T, rows=(0, -1), tag_window=None):
    """xyz (n, 3) float32, tags (n,) int32, T (4, 4) float64 -> (xyz after (n, 3) float32, n_moved, n_skipped)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tags = np.asarray(tags, np.int32).reshape(-1)
    T = np.asarray(T, np.float64).reshape(16)
    lo, hi = _scope(len(xyz), rows)
    w_lo, w_hi = (0, np.iinfo(np.int32).max) if tag_window is None else tag_window
    sel = np.zeros(len(xyz), bool)
    sel[lo:hi] = True
    sel &= (tags != POINT_NONE) & (tags >= w_lo) & (tags <= w_hi)
    p = xyz.astype(np.float64)
    out = np.zeros_like(xyz)
    with np.errstate(all="ignore"):
        for c in range(3):
            v = T[4 * c] * p[:, 0]
            v = v + T[4 * c + 1] * p[:, 1]
            v = v + T[4 * c + 2] * p[:, 2]
            v = v + T[4 * c + 3]
            out[:, c] = v.astype(np.float32)
    moved = sel & np.isfinite(out).all(1)
    after = xyz.copy()
    after[moved] = out[moved]
    return after, int(moved.sum()), int((sel & ~moved).sum())


def index_case(n, seed=0, points=True, spread=True):
    """An index of n rows -> dict(desc (n, 32) uint8, ids (n,) uint64, xyz (n, 3) float32, tags (n,) int32).

    Ids come in runs of 1, 2, .. 9, 1, 2, .. rows per id; the first id is 0 and the second 2^64 - 1, the others random 64-bit values.
    With spread the rows of an id lie scattered over the whole index (so that they fall on both sides of any scope edge that is not
    at an end); without, they are adjacent.  tags: the "frame" of a row, r * 8 // n .. (0 .. 7, non-decreasing, so that a window's
    two edges are both met); with points every 11th row has none (tag -1, xyz 0)."""
    rng = np.random.default_rng(1000 + seed)
    ids = np.zeros(n, np.uint64)
    r, k = 0, 0
    while r < n:
        run = k % 9 + 1
        v = np.uint64(0) if k == 0 else U64_MAX if k == 1 else rng.integers(1, 1 << 63, dtype=np.uint64) * np.uint64(2) + np.uint64(k & 1)
        ids[r:r + run] = v
        r += run; k += 1
    if spread:
        ids = ids[rng.permutation(n)]
    tags = (np.arange(n) * 8 // max(n, 1)).astype(np.int32)
    xyz = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    if points:
        none = np.arange(n) % 11 == 5
        tags[none] = POINT_NONE
        xyz[none] = 0
    return dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), ids=ids, xyz=xyz, tags=tags)


def run_lengths(ids):
    """how many rows each id of `ids` has -> the sorted set of those counts"""
    return sorted(set(np.unique(np.asarray(ids), return_counts=True)[1].tolist()))
