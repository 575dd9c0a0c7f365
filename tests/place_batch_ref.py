"""Reference for the batched place candidates (include/svo.h, "Batched place candidates"): a loop of tests/place_ref.py over the
cameras, which is the definition — camera b's result is the single call's on its slice.  It knows nothing of the kernels' shared
table of (id, camera) pairs, the one sweep or the pick per camera."""
import numpy as np

import place_ref as pr

MAX_CAMERAS, MAX_IDS, MAX_BINS = 1024, 1 << 20, 1 << 24


def tag_votes_batch(ids, tags, lists, rows=(0, -1), tag_span=(0, 0)):
    """-> (votes (B, b), rows, row_first, row_end (b,)), int32; lists: one id list per camera"""
    nb = int(tag_span[1]) - int(tag_span[0]) + 1
    assert len(lists) <= MAX_CAMERAS and len(lists) * nb <= MAX_BINS and sum(len(m) for m in lists) <= MAX_IDS
    shared = pr.tag_votes(ids, tags, [], rows, tag_span)[1:]
    votes = np.zeros((len(lists), nb), np.int32)
    for b, m in enumerate(lists):
        v = pr.tag_votes(ids, tags, m, rows, tag_span)
        votes[b] = v[0]
        assert all(np.array_equal(a, s) for a, s in zip(v[1:], shared))  # the three fields no camera changes
    return (votes,) + tuple(shared)


def places_from_ids_batch(ids, tags, lists, **kw):
    """-> per camera place_ref.places_from_ids' dict"""
    return [pr.places_from_ids(ids, tags, m, **kw) for m in lists]


def places_batch(queries, desc, ids, tags, matches=None, **kw):
    """-> per camera place_ref.places' dict; matches: per camera the reference's search, where the caller has it"""
    return [pr.places(q, desc, ids, tags, matches=None if matches is None else matches[b], **kw) for b, q in enumerate(queries)]
