"""Reference for the descriptor index's search (include/svo.h, "Descriptor index"), straight from the definition: the full (n, m)
distance matrix of descriptor_ref.hamming and lexicographic arg-mins over (distance, row).  It knows nothing of the streaming
update or the merge rule of svo_match.hpp.  -> the structured rows api.DescriptorIndex.match returns."""
import numpy as np

import descriptor_ref as ref

NONE, NO_DIST = -1, 257
DTYPE = np.dtype([("id", "<u8"), ("id2", "<u8"), ("row", "<i4"), ("row2", "<i4"), ("dist", "<u2"), ("dist2", "<u2"), ("reserved", "<u4")])


BLOCK = 128                                           # queries per distance matrix: bounds the (block, rows, 32) temporaries


def match(query, desc, ids, lo=0, hi=-1):
    """query (n, 32) uint8 against rows [lo, hi) of desc (m, 32) uint8 with ids (m,) -> (n,) rows of DTYPE"""
    query = np.asarray(query, np.uint8).reshape(-1, 32)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    hi = len(desc) if hi == -1 else hi
    assert 0 <= lo <= hi <= len(desc) == len(ids)
    out = np.zeros(len(query), DTYPE)
    out["row"] = out["row2"] = NONE
    out["dist"] = out["dist2"] = NO_DIST
    if hi == lo:
        return out
    for q0 in range(0, len(query), BLOCK):            # each query on its own: blocks only bound the memory
        out[q0:q0 + BLOCK] = _match_block(query[q0:q0 + BLOCK], desc, ids, lo, hi, out[q0:q0 + BLOCK])
    return out


def _match_block(query, desc, ids, lo, hi, out):
    D = ref.hamming(query, desc[lo:hi]).astype(np.int64)              # (n, hi - lo)
    rows = np.arange(lo, hi, dtype=np.int64)
    key = D * (1 << 32) + rows[None, :]                               # lexicographic (distance, row) as one integer
    best = key.argmin(1)
    out["row"] = rows[best]
    out["dist"] = D[np.arange(len(query)), best]
    out["id"] = ids[lo:hi][best]
    other = ids[lo:hi][None, :] != out["id"][:, None]                 # rows whose id differs from the best's
    big = np.iinfo(np.int64).max
    key2 = np.where(other, key, big)
    second = key2.argmin(1)
    has = other.any(1)
    out["row2"][has] = rows[second[has]]
    out["dist2"][has] = D[np.arange(len(query)), second][has]
    out["id2"][has] = ids[lo:hi][second[has]]
    return out


def plain_second(query, desc, lo=0, hi=-1):
    """the row of the second-smallest key whatever its id (-1 with fewer than two rows): what the id rule replaces"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    hi = len(desc) if hi == -1 else hi
    if hi - lo < 2:
        return np.full(len(query), NONE, np.int64)
    D = ref.hamming(np.asarray(query, np.uint8).reshape(-1, 32), desc[lo:hi]).astype(np.int64)
    key = D * (1 << 32) + np.arange(lo, hi, dtype=np.int64)[None, :]
    return np.argsort(key, 1)[:, 1] + lo
