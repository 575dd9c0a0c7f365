"""Reference for the descriptor index's place candidates (include/svo.h, "Place candidates"), straight from rules 1 - 3.  Rule 1 is
desc_match_ref.match and reloc_ref.select as they are; rule 2 is numpy on the host's copies of the index's ids and tags, with the
set M as a Python set of integers; rule 3 is a loop over a Python list.  It knows nothing of the kernels' LDS set, ballots, bins or
key list."""
import numpy as np

import desc_match_ref as mref
import reloc_ref as rref

MAX_TAGS, MAX_PLACES, MAX_IDS, POINT_NONE = 1 << 20, 64, 4096, -1
PLACE_DTYPE = np.dtype([("tag", "<i4"), ("votes", "<i4"), ("rows", "<i4"), ("row_first", "<i4"), ("row_end", "<i4"), ("reserved", "<i4", 3)])


def span(s, size):
    lo, hi = int(s[0]), int(s[1])
    return lo, (size if hi == -1 else hi)


def tag_votes(ids, tags, m_ids, rows=(0, -1), tag_span=(0, 0)):
    """rule 2 -> (votes, rows, row_first, row_end), int32 arrays of tag_hi - tag_lo + 1 entries; m_ids: M, duplicates legal"""
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    tags = np.asarray(tags).astype(np.int64).reshape(-1)
    lo, hi = span(rows, len(ids))
    t0, t1 = int(tag_span[0]), int(tag_span[1])
    assert 0 <= t0 <= t1 and t1 - t0 + 1 <= MAX_TAGS
    nb = t1 - t0 + 1
    r = np.arange(lo, hi, dtype=np.int64)
    t = tags[lo:hi]
    ok = (t >= t0) & (t <= t1)
    M = set(int(v) for v in np.asarray(m_ids).astype(np.uint64).reshape(-1))        # Python integers: no id passes through a float
    in_m = np.array([int(v) in M for v in ids[lo:hi]], bool) if len(M) else np.zeros(hi - lo, bool)
    b = (t - t0)[ok]
    n_rows = np.bincount(b, minlength=nb).astype(np.int32)
    votes = np.bincount(b, weights=in_m[ok].astype(np.float64), minlength=nb).astype(np.int32)       # counts below 2^24: exact
    first = np.full(nb, np.iinfo(np.int64).max, np.int64)
    end = np.zeros(nb, np.int64)
    np.minimum.at(first, b, r[ok])
    np.maximum.at(end, b, r[ok] + 1)
    first[n_rows == 0] = 0
    return votes, n_rows, first.astype(np.int32), end.astype(np.int32)


def pick(votes, n_rows, row_first, row_end, tag_lo=0, min_votes=1, separation=0, max_places=8):
    """rule 3 -> (n_tags_voted, places) with places a PLACE_DTYPE array in the order of emission"""
    assert min_votes >= 1 and separation >= 0 and 1 <= max_places <= MAX_PLACES
    votes = np.asarray(votes).reshape(-1)
    P = [int(b) for b in np.nonzero(votes >= min_votes)[0]]
    out = []
    while P and len(out) < max_places:
        best = min(P, key=lambda b: (-int(votes[b]), b))                 # the most votes, then the smallest tag
        out.append((tag_lo + best, int(votes[best]), int(n_rows[best]), int(row_first[best]), int(row_end[best]), (0, 0, 0)))
        P = [b for b in P if abs(b - best) > separation]
    return int((votes >= 1).sum()), np.array(out, PLACE_DTYPE)


def places_from_ids(ids, tags, m_ids, rows=(0, -1), tag_span=(0, MAX_TAGS - 1), min_votes=1, separation=0, max_places=8):
    """rules 2 - 3 -> dict: n_landmarks, n_tags_voted, n_places, places"""
    v = tag_votes(ids, tags, m_ids, rows, tag_span)
    voted, pl = pick(*v, tag_lo=int(tag_span[0]), min_votes=min_votes, separation=separation, max_places=max_places)
    n_m = len(set(int(x) for x in np.asarray(m_ids).astype(np.uint64).reshape(-1)))
    return dict(n_landmarks=n_m, n_tags_voted=voted, n_places=len(pl), places=pl)


def recognised(query, desc, ids, tags, rows=(0, -1), max_dist=40, ratio_num=7, ratio_den=10, matches=None):
    """rule 1 -> (cand_query, cand_row), svo_desc_index_select's.  matches: desc_match_ref.match(query, desc, ids, *rows) where the
    caller has it already (it does not depend on the three parameters)"""
    query = np.asarray(query, np.uint8).reshape(-1, 32)
    if len(query) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    lo, hi = span(rows, len(np.asarray(ids).reshape(-1)))
    m = mref.match(query, desc, ids, lo, hi) if matches is None else matches
    assert len(m) == len(query)
    return rref.select(m, tags, max_dist, ratio_num, ratio_den)


def places(query, desc, ids, tags, rows=(0, -1), tag_span=(0, MAX_TAGS - 1), min_votes=1, separation=0, max_places=8, max_dist=40, ratio_num=7,
           ratio_den=10, matches=None):
    """rules 1 - 3 -> places_from_ids' dict with cand_query and cand_row"""
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    cq, cr = recognised(query, desc, ids, tags, rows, max_dist, ratio_num, ratio_den, matches)
    out = places_from_ids(ids, tags, ids[cr], rows, tag_span, min_votes, separation, max_places)
    assert out["n_landmarks"] == len(cq)                                 # one candidate per landmark
    out.update(cand_query=cq, cand_row=cr)
    return out


def best_row_votes(query, desc, ids, tags, rows=(0, -1), tag_span=(0, 0)):
    """the vote this feature replaces: one vote per query for the tag of svo_desc_index_match's best row"""
    lo, hi = span(rows, len(np.asarray(ids).reshape(-1)))
    m = mref.match(np.asarray(query, np.uint8).reshape(-1, 32), desc, ids, lo, hi)
    t = np.asarray(tags).astype(np.int64).reshape(-1)[m["row"][m["row"] >= 0]]
    t = t[(t >= tag_span[0]) & (t <= tag_span[1])]
    return np.bincount(t - tag_span[0], minlength=tag_span[1] - tag_span[0] + 1).astype(np.int32)
