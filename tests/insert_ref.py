"""The numpy definition of the descriptor index's batched insertion (include/svo.h, "Batched insertion", rules 1 - 6), vectorised per
entry with boolean masks.  It knows nothing of tiles, ballots or scans.  Points go through reloc_ref.map_points."""
import numpy as np

import reloc_ref as rref

OBS_INLIER, OBS_HAS_XYZ = 1, 2
POINT_NONE = -1
MAX_ENTRIES, MAX_OBS_ROWS = 1024, 1 << 18
OBS_DTYPE = np.dtype([("id", "<i8"), ("l0", "<f4", 2), ("r0", "<f4", 2), ("l1", "<f4", 2), ("r1", "<f4", 2),
                      ("xyz", "<f4", 3), ("age", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert OBS_DTYPE.itemsize == 64


class Refused(Exception):
    """rule 6: the call adds nothing"""


def insert(entries, need_flags, id_base=None, with_points=False, cam_to_map=None, tags=None, size=0, capacity=None, index_has_points=None):
    """entries: [(obs (r,) OBS_DTYPE, desc (r, 32) uint8)] -> dict(desc, ids, xyz, tags, first_row, n_added): the appended rows as
    svo_desc_index_read_rows shows them (xyz, tags None when the index has no points; a plain call on an index with points gives
    +inf and POINT_NONE), first_row and n_added per entry.  Raises Refused where rule 6 refuses."""
    n = len(entries)
    has_points = with_points if index_has_points is None else index_has_points
    need = np.uint32(need_flags | (OBS_HAS_XYZ if with_points else 0))
    if with_points and tags is not None and (np.asarray(tags) < 0).any():
        raise Refused("tag")
    if with_points and cam_to_map is not None and not np.isfinite(np.asarray(cam_to_map, np.float64)).all():
        raise Refused("cam_to_map")
    D, I, X, G, counts = [], [], [], [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for b, (obs, desc) in enumerate(entries):
            obs = np.asarray(obs, OBS_DTYPE).reshape(-1)
            desc = np.asarray(desc, np.uint8).reshape(-1, 32)
            keep = (obs["flags"].astype(np.uint32) & need) == need
            base = np.uint64(0) if id_base is None else np.uint64(id_base[b])
            D.append(desc[keep])
            I.append(obs["id"][keep].astype(np.uint64) + base)                 # uint64 arithmetic wraps modulo 2^64
            counts.append(int(keep.sum()))
            if with_points:
                p = obs["xyz"][keep]
                X.append(p.copy() if cam_to_map is None else rref.map_points(np.asarray(cam_to_map, np.float64).reshape(-1, 16)[b], p))
                G.append(np.full(counts[-1], 0 if tags is None else int(tags[b]), np.int32))
            elif has_points:
                X.append(np.full((counts[-1], 3), np.inf, np.float32)); G.append(np.full(counts[-1], POINT_NONE, np.int32))
    total = sum(counts)
    if capacity is not None and total > capacity - size:
        raise Refused("capacity")
    xyz = np.concatenate(X).reshape(-1, 3) if has_points and n else (np.zeros((0, 3), np.float32) if has_points else None)
    if with_points and not np.isfinite(xyz).all():
        raise Refused("non-finite point")
    n_added = np.array(counts, np.int32).reshape(n)
    first = (size + np.concatenate([[0], np.cumsum(n_added)[:-1]])).astype(np.int32) if n else np.zeros(0, np.int32)
    return dict(desc=np.concatenate(D).reshape(-1, 32) if n else np.zeros((0, 32), np.uint8),
                ids=np.concatenate(I).astype(np.uint64) if n else np.zeros(0, np.uint64), xyz=xyz,
                tags=(np.concatenate(G).astype(np.int32) if n else np.zeros(0, np.int32)) if has_points else None, first_row=first, n_added=n_added)


def make_entry(rows, flags, seed, id0=0):
    """an entry of `rows` observation rows with the given flags ((rows,) or a scalar), random points, ids id0 + 0 .. and descriptors"""
    rng = np.random.default_rng(seed)
    obs = np.zeros(rows, OBS_DTYPE)
    obs["id"] = id0 + np.arange(rows)
    obs["xyz"] = rng.uniform(-20, 20, (rows, 3)).astype(np.float32)
    obs["l1"] = rng.uniform(0, 300, (rows, 2)).astype(np.float32)
    obs["age"] = rng.integers(0, 9, rows)
    obs["flags"] = flags
    return obs, rng.integers(0, 256, (rows, 32), dtype=np.uint8)


def flag_pattern(name, rows, seed=0):
    """the flag patterns of the GPU tests, as flags that keep a row under need = INLIER (| HAS_XYZ): kept rows carry both bits, the
    others HAS_XYZ alone"""
    keep = np.zeros(rows, bool)
    if name == "all":
        keep[:] = True
    elif name == "alternate":
        keep[::2] = True
    elif name == "tile_last":
        keep[255::256] = True
    elif name == "lanes_63_64":
        keep[[i for i in (63, 64) if i < rows]] = True
    elif name == "random":
        keep = np.random.default_rng(seed).random(rows) < 0.4
    elif name != "none":
        raise ValueError(name)
    return np.where(keep, OBS_INLIER | OBS_HAS_XYZ, OBS_HAS_XYZ).astype(np.int32)


def pose(seed, scale=1.0):
    """a rigid cam_to_map with a translation of a few metres, times scale"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4)
    T[:3, :3] = q * scale
    T[:3, 3] = rng.uniform(-5, 5, 3)
    return T
