"""Reference for the descriptor index's landmark consolidation (include/svo.h, "Landmark consolidation"), straight from the five
rules, in plain numpy with Python loops: members and groups by a dictionary, the views by slicing, the medoid from the full matrix of
Hamming distances, the gate in float32, the mean as a chain of float64 additions in ascending rows and one float64 division, each
rounded on its own (numpy fuses nothing), .astype(np.float32).  It knows nothing of hash tables, scans, waves or slabs.  `order`
exists for tests/test_consolidate_ref.py alone: it sums the near views in another order, to show that the order rule binds.
group_sizes_case and index_case are the generators the CPU and the GPU tests share."""
import collections

import numpy as np

POINT_NONE = -1
MAX_VIEWS = 64
I32_MAX = int(np.iinfo(np.int32).max)
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
Result = collections.namedtuple("Result", "n_members n_groups n_dropped n_far_views n_capped_groups n_kept")

_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


def hamming(a, b):
    """the search's distance between two descriptors of 32 bytes"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def medoid(rows, desc):
    """rule 3 -> the position among `rows` (ascending) of the view with the least sum of distances, at equal sums the larger row"""
    d = np.asarray(desc)[list(rows)]
    sums = _POP[d[:, None, :] ^ d[None, :, :]].sum((1, 2))         # sums[i] = the sum over j of hamming(d[i], d[j])
    best = 0
    for v in range(1, len(rows)):
        if sums[v] <= sums[best]:                     # ascending rows: `<=` lets the later row win a tie
            best = v
    return best


def mean_point(points, near, order=None):
    """rule 4's arithmetic: points (k, 3) float32 in ascending rows, near (k,) bool -> (3,) float32"""
    out = np.zeros(3, np.float32)
    idx = [j for j in range(len(points)) if near[j]]
    if order == "descending":
        idx = idx[::-1]
    for c in range(3):
        s = np.float64(0.0)
        for j in idx:
            s = s + np.float64(points[j, c])
        out[c] = np.float32(s / np.float64(len(idx)))
    return out


def consolidate(desc, ids, xyz, tags, radius, rows=(0, -1), tag_window=None, order=None):
    """desc (n0, 32) uint8, ids (n0,) uint64, xyz (n0, 3) float32, tags (n0,) int32 -> dict(desc, ids, xyz, tags: the index after the
    call, a row without a point as it was given; kept_before (n0 + 1,) int32; result: the record)"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32).copy()
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3).copy()
    tags = np.asarray(tags, np.int32).reshape(-1)
    n0 = len(ids)
    lo, hi = int(rows[0]), int(rows[1])
    hi = n0 if hi == -1 else hi
    assert 0 <= lo <= hi <= n0 and np.isfinite(radius) and radius >= 0
    w_lo, w_hi = (0, I32_MAX) if tag_window is None else tag_window
    radius = np.float32(radius)
    groups = collections.OrderedDict()
    for r in range(lo, hi):
        if tags[r] != POINT_NONE and w_lo <= int(tags[r]) <= w_hi:
            groups.setdefault(int(ids[r]), []).append(r)
    keep = np.ones(n0, bool)
    n_far = n_capped = 0
    new_desc, new_xyz = {}, {}
    for members in groups.values():
        k = len(members)
        if k == 1:
            continue                                  # rule 5: a group of one row is left as it is
        n_capped += k > MAX_VIEWS
        views = members[-MAX_VIEWS:]
        m = medoid(views, desc)
        p = xyz[views]
        near = (np.abs(p - p[m]) <= radius).all(1)    # float32 differences, float32 compare, inclusive
        assert near[m]
        n_far += int((~near).sum())
        keep[members[:-1]] = False
        new_desc[members[-1]] = desc[views[m]].copy()
        new_xyz[members[-1]] = mean_point(p, near, order)
    for r, d in new_desc.items():
        desc[r] = d
        xyz[r] = new_xyz[r]
    kept_before = np.zeros(n0 + 1, np.int32)
    kept_before[1:] = np.cumsum(keep)
    n_members = sum(len(g) for g in groups.values())
    res = Result(n_members, len(groups), n_members - len(groups), n_far, n_capped, int(keep.sum()))
    return dict(desc=desc[keep], ids=ids[keep], xyz=xyz[keep], tags=tags[keep], kept_before=kept_before, result=res)


def as_read(case):
    """the four arrays of an index as read_rows returns them: a row without a point reads xyz = +inf"""
    xyz = np.asarray(case["xyz"], np.float32).copy()
    xyz[np.asarray(case["tags"]) == POINT_NONE] = np.inf
    return np.asarray(case["desc"], np.uint8), np.asarray(case["ids"]).astype(np.uint64), xyz, np.asarray(case["tags"], np.int32)


def same_rows(got, want):
    """got, want: (desc, ids, xyz, tags) -> the names of the arrays that differ in a byte (xyz compared as bits)"""
    names = ("desc", "ids", "xyz", "tags")
    return [n for n, g, w in zip(names, got, want)
            if g.shape != w.shape or not np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8))]


def group_sizes_case(sizes, seed=0, extra_ids=()):
    """An index whose groups have the given sizes, interleaved row by row (a random permutation of all rows): the descriptors of a
    group are a base with up to 40 random bits flipped per view, the points a centre with offsets of up to 0.05 on most views and up
    to 1.0 on every fifth, tags the row's eighth of the index.  extra_ids: ids for the first groups instead of random ones."""
    rng = np.random.default_rng(7000 + seed)
    ids, desc, xyz = [], [], []
    for g, k in enumerate(sizes):
        v = np.uint64(extra_ids[g]) if g < len(extra_ids) else rng.integers(1, 1 << 63, dtype=np.uint64)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        centre = rng.uniform(-20, 20, 3)
        for j in range(k):
            d = base.copy()
            for b in rng.integers(0, 256, rng.integers(0, 41)):
                d[b >> 3] ^= np.uint8(1 << (b & 7))
            ids.append(v); desc.append(d)
            xyz.append(centre + rng.uniform(-1, 1, 3) * (1.0 if j % 5 == 4 else 0.05))
    n = len(ids)
    perm = rng.permutation(n)
    tags = (np.arange(n) * 8 // max(n, 1)).astype(np.int32)
    return dict(desc=np.array(desc, np.uint8).reshape(n, 32)[perm], ids=np.array(ids, np.uint64)[perm],
                xyz=np.array(xyz, np.float32).reshape(n, 3)[perm], tags=tags)


def index_case(n, views=4, seed=0, none_every=11):
    """An index of n rows of about `views` rows per id, scattered; every none_every-th row has no point (0: none has)"""
    rng = np.random.default_rng(8000 + seed)
    n_ids = max(1, n // views)
    pool = rng.integers(1, 1 << 63, n_ids, dtype=np.uint64)
    if n_ids > 2:
        pool[0], pool[1] = np.uint64(0), U64_MAX
    which = rng.integers(0, n_ids, n)
    base = rng.integers(0, 256, (n_ids, 32), dtype=np.uint8)
    flip = (rng.random((n, 256)) < 0.04)
    desc = base[which] ^ np.packbits(flip, axis=1, bitorder="little")
    centre = rng.uniform(-20, 20, (n_ids, 3))
    xyz = (centre[which] + rng.uniform(-0.05, 0.05, (n, 3)) + (rng.random((n, 1)) < 0.15) * rng.uniform(-1, 1, (n, 3))).astype(np.float32)
    tags = (np.arange(n) * 8 // max(n, 1)).astype(np.int32)
    if none_every:
        none = np.arange(n) % none_every == 5
        tags[none] = POINT_NONE
        xyz[none] = 0
    return dict(desc=desc.astype(np.uint8), ids=pool[which], xyz=xyz, tags=tags)
