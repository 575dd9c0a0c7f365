"""Batched place candidates fed from the frame pipeline on a real GPU (include/svo.h: svo_desc_index_add_frame_points,
svo_desc_index_places_batch, places_from_ids_batch, tag_votes_batch): the synthetic sequence's map of
tests/test_gpu_place_frames.py — frames 1 .. 4 as keyframes tagged by their frame number, row_hi keeping the last keyframe's own
rows out.  Several cameras ask in one call: the last keyframe's inlier descriptors, their two halves, every third of them, and
none.  For each camera the batch returns that test's places — the single call's and tests/place_ref.py's on the host's copies of
the rows, every field and all four arrays of tag_votes."""
import numpy as np
import pytest

import place_ref as pr
from gpu_kit import api, projections  # noqa: F401  (the fixture is found by name)
from test_gpu_align_frames import H, INLIER_XYZ, MAP_FRAMES, N_FRAMES, OVER, ROWS, W, map_rows, sequences


@pytest.mark.gpu
def test_the_batch_returns_each_cameras_places_among_the_earlier_keyframes(api):
    A = sequences()[0]
    ix = api.DescriptorIndex(1 << 12, points=True)
    vo = api.BatchVisualOdometry(W, H, 1, api.default_config(**OVER))
    try:
        vo.initalize_projection_matricies(*projections(W, H))
        vo.set_track_output(ROWS)
        vo.set_descriptor_output(True)
        poses, per, first = [np.eye(4)], [], {}
        for k in range(N_FRAMES):
            ok, T = vo.stereo_callback_batch([A.left[k]], [A.right[k]])
            assert bool(ok[0]) == (k > 0), "frame %d" % k
            if k > 0:
                poses.append(poses[-1] @ T[0])
            per.append((vo.last_track_obs(0), vo.last_track_descriptors(0)))
            if k in MAP_FRAMES:
                first[k] = ix.add_frame_points(vo, poses[k - 1], tag=k)[0]
        desc, ids, xyz, tags = map_rows(per, poses, 0)
        assert ix.size == len(desc)
        last = MAP_FRAMES[-1]
        row_hi = first[last]                           # the last keyframe's own rows stay out
        obs, d = per[last]
        query = d[(obs["flags"] & INLIER_XYZ) == INLIER_XYZ]
        assert np.array_equal(query, desc[row_hi:]) and 0 < len(query) <= 4096
        half = len(query) // 2
        queries = [query, query[:half], query[half:], query[::3], query[:0]]
        span = (0, last)
        for kw in (dict(), dict(separation=1), dict(min_votes=5, max_places=2)):
            got = ix.places_batch(queries, rows=(0, row_hi), tags=span, **kw)
            lists = []
            for b, q in enumerate(queries):
                want = pr.places(q, desc, ids, tags, rows=(0, row_hi), tag_span=span, **kw)
                res, places, cand = ix.places(q, rows=(0, row_hi), tags=span, **kw)
                g = got[b]
                print("camera %d, %d queries, %s: %d landmarks, %d tags voted, places (tag, votes, rows): %s" % (
                    b, len(q), kw, g[0].n_landmarks, g[0].n_tags_voted, [(int(p["tag"]), int(p["votes"]), int(p["rows"])) for p in g[1]]))
                assert g[0] == res == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]) and (res.n_landmarks > 0) == (len(q) > 0)
                assert g[1].tobytes() == places.tobytes() == want["places"].tobytes()
                assert np.array_equal(g[2]["query"], want["cand_query"]) and np.array_equal(g[2]["row"], want["cand_row"])
                assert np.array_equal(g[2]["query"], cand["query"]) and np.array_equal(g[2]["row"], cand["row"])
                assert (g[1]["tag"] < last).all()      # nothing of the keyframe kept out
                lists.append(ids[g[2]["row"]])
            by_id = ix.places_from_ids_batch(lists, rows=(0, row_hi), tags=span, **kw)
            assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(by_id, got))
        votes = ix.tag_votes_batch(lists, (0, row_hi), span)
        for b, m in enumerate(lists):
            w = pr.tag_votes(ids, tags, m, (0, row_hi), span)
            assert votes[0][b].tobytes() == w[0].tobytes() and all(g.tobytes() == x.tobytes() for g, x in zip(votes[1:], w[1:]))
        # the local-map query for two trackers at once: the keyframes that saw the tracks each holds, the whole index this time
        tracked = np.unique(ids[row_hi:])
        held = [tracked, tracked[::2]]
        got = ix.places_from_ids_batch(held, tags=span)
        for m, g in zip(held, got):
            want = pr.places_from_ids(ids, tags, m, tag_span=span)
            assert g[0] == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]) and g[1].tobytes() == want["places"].tobytes()
            assert int(g[1]["votes"].max()) == len(m)  # every row of the last keyframe votes for it
    finally:
        vo.close(); ix.close()
