"""Reference for the descriptor index's landmark fusion (include/svo.h, "Landmark fusion"), straight from rules 1 - 5.  The gate in
numpy float32 (a subtraction, an absolute value and a compare per axis, each rounded to f32 as the rule says); the search as the full
distance matrix of descriptor_ref.hamming with the inadmissible rows struck out and lexicographic arg-mins over (distance, row), as
desc_match_ref does it; rules 2 - 5 of "Map alignment" through align_ref.pairs on those result rows; the map and the relabel on
Python integers with a dictionary.  It knows nothing of the kernels' ballots, groups, chunks or hash table."""
import numpy as np

import align_ref as aref
import desc_match_ref as mref
import descriptor_ref as ref

MAX_ROWS, MAX_LIST, POINT_NONE = 4096, 1 << 20, -1
BLOCK = 128                                           # source rows per distance matrix: bounds the temporaries


def span(s, size):
    lo, hi = int(s[0]), int(s[1])
    return lo, (size if hi == -1 else hi)


def gate(xyz, tags, src_rows, dst_rows, radius):
    """rule 1 -> (len(src_rows), len(dst_rows)) bool: is destination row r admissible for source row s?"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tags = np.asarray(tags).reshape(-1)
    r = np.float32(radius)
    ps, pd = xyz[src_rows], xyz[dst_rows]
    diff = np.abs((pd[None, :, :] - ps[:, None, :]).astype(np.float32))               # f32 - f32 is f32 in numpy; the cast says so
    ok = (diff <= r).all(-1)
    return ok & (tags[src_rows] != POINT_NONE)[:, None] & (tags[dst_rows] != POINT_NONE)[None, :]


def match_near(desc, ids, xyz, tags, src, dst, radius):
    """rules 1 - 2 on the host's copies of an index's arrays -> (n,) rows of desc_match_ref.DTYPE"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    (s0, s1), (d0, d1) = span(src, len(desc)), span(dst, len(desc))
    n = s1 - s0
    out = np.zeros(n, mref.DTYPE)
    out["row"] = out["row2"] = mref.NONE
    out["dist"] = out["dist2"] = mref.NO_DIST
    if n == 0 or d1 == d0:
        return out
    rows = np.arange(d0, d1, dtype=np.int64)
    big = np.iinfo(np.int64).max
    for j0 in range(0, n, BLOCK):
        sr = np.arange(s0 + j0, min(s0 + j0 + BLOCK, s1))
        adm = gate(xyz, tags, sr, rows, radius)
        D = ref.hamming(desc[sr], desc[d0:d1]).astype(np.int64)
        key = np.where(adm, D * (1 << 32) + rows[None, :], big)
        best = key.argmin(1)
        has = adm.any(1)
        o = out[j0:j0 + len(sr)]
        idx = np.arange(len(sr))
        o["row"][has] = rows[best[has]]
        o["dist"][has] = D[idx, best][has]
        o["id"][has] = ids[d0:d1][best[has]]
        other = adm & (ids[d0:d1][None, :] != ids[d0:d1][best][:, None])
        key2 = np.where(other, key, big)
        second = key2.argmin(1)
        has2 = has & other.any(1)
        o["row2"][has2] = rows[second[has2]]
        o["dist2"][has2] = D[idx, second][has2]
        o["id2"][has2] = ids[d0:d1][second[has2]]
        out[j0:j0 + len(sr)] = o
    return out


def pair_near(desc, ids, xyz, tags, src, dst, radius, max_dist=40, ratio_num=7, ratio_den=10):
    """rules 1 - 3 -> (pair_src, pair_dst) int32 row numbers"""
    size = len(np.asarray(ids).reshape(-1))
    src, dst = span(src, size), span(dst, size)
    m = match_near(desc, ids, xyz, tags, src, dst, radius)
    return aref.pairs(desc, ids, tags, src, dst, max_dist, ratio_num, ratio_den, matches=m)


def relabel(ids, from_ids, to_ids, rows=(0, -1)):
    """rule 5 on lists -> (the new ids, the number of rows changed).  Entries with from == to are ignored; of a repeated `from` the
    first remaining entry wins; one simultaneous step on the ids as they were."""
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    lo, hi = span(rows, len(ids))
    table = {}
    for f, t in zip((int(v) for v in from_ids), (int(v) for v in to_ids)):       # Python integers: no id passes through a float
        if f != t and f not in table:
            table[f] = t
    out = ids.copy()
    changed = 0
    for r in range(lo, hi):
        t = table.get(int(ids[r]))
        if t is not None:
            out[r] = t
            changed += 1
    return out, changed


def fuse(desc, ids, xyz, tags, src, dst, radius, relabel_rows=(0, -1), max_dist=40, ratio_num=7, ratio_den=10):
    """all of it -> dict: pair_src, pair_dst, n_pairs, n_same, n_fused, n_rows_relabelled, ids (the index's ids afterwards)"""
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    ps, pd = pair_near(desc, ids, xyz, tags, src, dst, radius, max_dist, ratio_num, ratio_den)
    frm, to = ids[ps], ids[pd]                        # rule 4: read before anything is written
    n_same = int((frm == to).sum())
    new, changed = relabel(ids, frm, to, relabel_rows)
    return dict(pair_src=ps, pair_dst=pd, n_pairs=len(ps), n_same=n_same, n_fused=len(ps) - n_same, n_rows_relabelled=changed, ids=new)
