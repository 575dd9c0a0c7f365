"""The batched insertion's stage entry on a real GPU (include/svo.h, "Batched insertion": svo_desc_index_add_obs): the caller's
observation rows through the pinned staging and the three kernels of svo_kernels_insert.hip, the index read back with read_rows and
compared byte for byte with tests/insert_ref.py — descriptors, ids, points, tags — beside first_row, n_added and the size.
Entries of 0, 1, 63, 64, 65, 255, 256, 257 and 513 rows (the wave and tile edges, and more than one tile) in one call and alone;
flags that keep nothing, everything, alternate rows, only a tile's last row, only lanes 63 and 64, a seeded random set; need_flags 0
and INLIER; 1, 2, 9, 65 and 1024 entries; with and without points, cam_to_map and id_base absent, id_base near 2^64, a non-empty
index, the plain call on an index with points; the capacity filled exactly and exceeded by one row; a point that is not finite, kept
and not kept; the refusals."""
import numpy as np
import pytest

import insert_ref as ir
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513]
PATTERNS = ["none", "all", "alternate", "tile_last", "lanes_63_64", "random"]
NEAR_TOP = (1 << 64) - 3


def entries_of(sizes, pattern="random", seed=11):
    return [ir.make_entry(r, ir.flag_pattern(pattern, r, seed + b), seed + 50 * b, id0=100 * b) for b, r in enumerate(sizes)]


def prefilled(api, capacity, points, prefill):
    """an index of `capacity` rows holding `prefill` rows -> (index, what read_rows gives for them)"""
    ix = api.DescriptorIndex(capacity, points=points)
    if prefill:
        rng = np.random.default_rng(prefill)
        d, i = rng.integers(0, 256, (prefill, 32), dtype=np.uint8), rng.integers(0, 1 << 62, prefill).astype(np.uint64)
        if points:
            ix.add_points(d, i, rng.uniform(-3, 3, (prefill, 3)).astype(np.float32), rng.integers(0, 9, prefill).astype(np.int32))
        else:
            ix.add(d, i)
    return ix, rows_of(ix, points)


def rows_of(ix, points, lo=0):
    got = ix.read_rows((lo, -1), want=("desc", "ids", "xyz", "tags") if points else ("desc", "ids"))
    return [None if a is None else a.tobytes() for a in got]


def check_call(api, entries, need, id_base=None, with_points=False, T=None, tags=None, index_points=None, prefill=0, slack=5):
    """add_obs onto an index of prefill rows against the reference, byte for byte"""
    points = with_points if index_points is None else index_points
    want = ir.insert(entries, need, id_base, with_points, T, tags, size=prefill, index_has_points=points)
    total = int(want["n_added"].sum())
    ix, before = prefilled(api, prefill + total + slack, points, prefill)
    try:
        first, added = ix.add_obs([o for o, _ in entries], [d for _, d in entries], need, id_base, with_points, T, tags)
        assert first.dtype == np.int32 and added.dtype == np.int32
        assert added.tolist() == want["n_added"].tolist() and first.tolist() == want["first_row"].tolist()
        assert ix.size == prefill + total
        st = ix.insert_stats()
        assert st["last_path"] == api._lib.INSERT_PATH_STAGED and st["rows_added"] == total and st["rows_scanned"] == sum(len(o) for o, _ in entries)
        got = rows_of(ix, points, prefill)
        assert got[0] == want["desc"].tobytes(), "descriptors"
        assert got[1] == want["ids"].tobytes(), "ids"
        if points:
            assert got[2] == want["xyz"].tobytes(), "points"
            assert got[3] == want["tags"].tobytes(), "tags"
        if prefill:
            ix.truncate(prefill)
            assert rows_of(ix, points) == before, "the rows below the old size"
    finally:
        ix.close()
    return total


@pytest.mark.parametrize("with_points", [False, True], ids=["plain", "points"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_size_in_one_call(api, pattern, with_points):
    e = entries_of(SIZES, pattern)
    n = len(e)
    total = check_call(api, e, ir.OBS_INLIER, np.arange(n, dtype=np.uint64) << np.uint64(48), with_points,
                       [ir.pose(b) for b in range(n)] if with_points else None, list(range(n)) if with_points else None, prefill=37)
    assert (total == 0) == (pattern == "none")


@pytest.mark.parametrize("rows", SIZES)
def test_every_size_alone(api, rows):
    for pattern in ("all", "random"):
        check_call(api, entries_of([rows], pattern, seed=rows), ir.OBS_INLIER, None, True, [ir.pose(rows)], [4])


@pytest.mark.parametrize("need", [0, ir.OBS_INLIER])
@pytest.mark.parametrize("n", [1, 2, 9, 65, 1024])
def test_entry_counts_and_need_flags(api, n, need):
    rng = np.random.default_rng(n)
    sizes = [1 + b % 3 for b in range(n)] if n == 1024 else [int(rng.integers(0, 300)) for _ in range(n)]
    e = entries_of(sizes, "random", seed=n)
    for o, _ in e:
        o["flags"][::7] = 0                                                 # rows without any bit: kept by need 0 of the plain call alone
    check_call(api, e, need, None, False)
    check_call(api, e, need, np.full(n, NEAR_TOP, np.uint64), True, [ir.pose(b % 5) for b in range(n)], [b % 11 for b in range(n)], prefill=3)


def test_absent_arrays_and_a_plain_call_on_an_index_with_points(api):
    e = entries_of([70, 0, 300], "alternate")
    check_call(api, e, ir.OBS_INLIER, None, True, None, None, prefill=10)    # cam_to_map NULL: xyz as it is; tags NULL: 0; id_base NULL
    check_call(api, e, ir.OBS_INLIER, None, False, index_points=True, prefill=10)   # SVO_POINT_NONE rows
    check_call(api, e, 0, np.array([NEAR_TOP, 1, NEAR_TOP], np.uint64), False, index_points=True)


def test_no_entries_adds_nothing(api):
    ix = api.DescriptorIndex(8)
    try:
        first, added = ix.add_obs([], [])
        assert len(first) == 0 and len(added) == 0 and ix.size == 0
    finally:
        ix.close()


def test_capacity_filled_exactly_and_exceeded_by_one(api):
    e = entries_of([200, 65, 257], "random", seed=2)
    total = check_call(api, e, ir.OBS_INLIER, None, True, [ir.pose(b) for b in range(3)], [1, 2, 3], prefill=21, slack=0)
    ARG = "status %d" % api._lib.SVO_ERR_ARG
    ix, before = prefilled(api, 21 + total - 1, True, 21)
    try:
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_obs([o for o, _ in e], [d for _, d in e], ir.OBS_INLIER, None, True, [ir.pose(b) for b in range(3)], [1, 2, 3])
        assert ix.size == 21 and rows_of(ix, True) == before
    finally:
        ix.close()


def test_a_point_that_is_not_finite(api):
    """cam_to_map scaled by 1e38: rows of |xyz| = 1e-3 stay finite (1e35), the one row at 10 overflows f32"""
    obs, desc = ir.make_entry(300, ir.flag_pattern("all", 300), 5)
    obs["xyz"] = np.float32(1e-3)
    obs["xyz"][261] = [1e-3, 10.0, 1e-3]
    T = np.eye(4); T[:3, :3] *= 1e38
    ARG = "status %d" % api._lib.SVO_ERR_ARG
    with pytest.raises(ir.Refused):
        ir.insert([(obs, desc)], ir.OBS_INLIER, None, True, [T], [0])
    ix, before = prefilled(api, 400, True, 9)
    try:
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_obs([obs], [desc], ir.OBS_INLIER, None, True, [T], [0])
        assert ix.size == 9 and rows_of(ix, True) == before
    finally:
        ix.close()
    obs["flags"][261] = ir.OBS_HAS_XYZ                                       # the same row, not kept
    assert check_call(api, [(obs, desc)], ir.OBS_INLIER, None, True, [T], [0], prefill=9) == 299


def test_refusals(api):
    ARG, STATE = "status %d" % api._lib.SVO_ERR_ARG, "status %d" % api._lib.SVO_ERR_STATE
    e = entries_of([20, 30], "all")
    obs, desc = [o for o, _ in e], [d for _, d in e]
    ix, before = prefilled(api, 1 << 12, True, 5)
    plain = api.DescriptorIndex(64)
    try:
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_obs(obs, desc, ir.OBS_INLIER, None, True, None, [0, -1])                 # a negative tag
        bad = np.eye(4); bad[2, 3] = np.inf
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_obs(obs, desc, ir.OBS_INLIER, None, True, [np.eye(4), bad], [0, 1])      # a transform that is not finite
        one = ir.make_entry(1, ir.flag_pattern("all", 1), 1)
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_obs([one[0]] * 1025, [one[1]] * 1025)                                    # n = 1025
        big = ir.make_entry((1 << 18) + 1, ir.OBS_HAS_XYZ, 2)
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_obs([big[0]], [big[1]])                                                  # more than 2^18 rows
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.add_obs(obs, desc, ir.OBS_INLIER, None, True)                             # an index without points
        assert ix.size == 5 and rows_of(ix, True) == before and plain.size == 0
    finally:
        ix.close(); plain.close()
