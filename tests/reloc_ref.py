"""Reference for the relocaliser's selection (include/svo.h, "Relocalisation"), straight from rules 1 - 4, and for the transform of
svo_desc_index_add_frame_points.  Plain Python over the search's result rows (desc_match_ref.match gives them): it knows nothing of
k_reloc_select's passes, ballots or LDS lists."""
import numpy as np

import desc_match_ref as mref

POINT_NONE = -1
MAX_QUERIES = 4096


def accept(m, tag, max_dist, ratio_num, ratio_den):
    """rule 1 for one result row m (a record of desc_match_ref.DTYPE) and the tag of its best row's point"""
    if int(m["row"]) == mref.NONE or int(tag) == POINT_NONE:
        return False
    if int(m["dist"]) > max_dist:
        return False
    return int(m["dist"]) * ratio_den < int(m["dist2"]) * ratio_num     # strict


def select(matches, tags, max_dist, ratio_num, ratio_den):
    """rules 1 - 3: matches (n,) result rows, tags (m,) int per index row -> (cand_query, cand_row) int32 arrays, increasing query"""
    tags = np.asarray(tags).reshape(-1)
    accepted = [j for j in range(len(matches))
                if accept(matches[j], tags[int(matches[j]["row"])] if int(matches[j]["row"]) >= 0 else POINT_NONE, max_dist, ratio_num, ratio_den)]
    best = {}                                          # rule 2: per id the smallest (dist, j)
    for j in accepted:
        k = (int(matches[j]["dist"]), j)
        i = int(matches[j]["id"])
        if i not in best or k < best[i]:
            best[i] = k
    keep = sorted(j for _, j in best.values())         # rule 3: increasing j
    return np.array(keep, np.int32), np.array([int(matches[j]["row"]) for j in keep], np.int32)


def select_index(query, xy, desc, ids, xyz, tags, row_lo=0, row_hi=-1, max_dist=40, ratio_num=7, ratio_den=10):
    """search + rules 1 - 3 on the host's copies of an index's arrays -> dict(query, row, xy, xyz) as api.DescriptorIndex.select gives"""
    m = mref.match(query, desc, ids, row_lo, row_hi)
    q, r = select(m, tags, max_dist, ratio_num, ratio_den)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return dict(query=q, row=r, xy=xy[q], xyz=xyz[r])


def gate(n_candidates, min_candidates):
    """rule 4: does the PnP run?"""
    return n_candidates >= min_candidates


def map_points(T, xyz):
    """svo_desc_index_add_frame_points: per coordinate f32(T[4r] x + T[4r+1] y + T[4r+2] z + T[4r+3]), f64, left to right.  numpy
    rounds every f64 product and sum on its own (no contraction), which is the definition."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.zeros((len(p), 3), np.float32)
    for r in range(3):
        v = T[r, 0] * p[:, 0]
        v = v + T[r, 1] * p[:, 1]
        v = v + T[r, 2] * p[:, 2]
        v = v + T[r, 3]
        out[:, r] = v.astype(np.float32)
    return out
