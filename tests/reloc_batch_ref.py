"""Reference for the batched relocalisation (include/svo.h, "Batched relocalisation"): the contract says a batch is its cameras one
by one, so the reference is a loop of guide_ref.select_index (guided) or reloc_ref.select_index (unguided) over the slices, on the
host's copies of the index's arrays.  It knows nothing of groups, tiles or lane orders."""
import guide_ref as gref
import reloc_ref as rref


def select_batch(rows, cams, guided=True, row_lo=0, row_hi=-1, **rule):
    """rows: dict desc, ids, xyz, tags; cams: [dict K, R, t, radius, query, xy] -> per camera the dict(query, row, xy, xyz) of the
    single call's selection; rule: max_dist, ratio_num, ratio_den"""
    out = []
    for c in cams:
        if guided:
            out.append(gref.select_index(c["K"], c["R"], c["t"], c["radius"], c["query"], c["xy"], rows["desc"], rows["ids"], rows["xyz"], rows["tags"],
                                         row_lo, row_hi, **rule))
        else:
            out.append(rref.select_index(c["query"], c["xy"], rows["desc"], rows["ids"], rows["xyz"], rows["tags"], row_lo, row_hi, **rule))
    return out
