"""Place candidates fed from the frame pipeline on a real GPU (include/svo.h: svo_desc_index_add_frame_points,
svo_desc_index_places, svo_desc_index_places_from_ids, svo_desc_index_tag_votes): the first sequence of
tests/test_gpu_align_frames.py, its frames 1 .. 4 added to one index as keyframes tagged by their frame number, a track keeping its
id from frame to frame.  The queries are the inlier descriptors of the last keyframe, and row_hi keeps that keyframe's own rows out
of the search and of the vote, as a loop closer keeps its most recent keyframes out.

 - asserted, because it holds by construction: the three counts, every place's 32 bytes, the recognised landmarks and all four
   arrays of tag_votes equal tests/place_ref.py on the host's copies of the same rows; places_from_ids with the recognised ids
   gives the same places.
 - printed, not asserted: the places.  Which keyframe leads depends on the tracker's losses frame by frame, which no reference of
   this project predicts."""
import numpy as np
import pytest

import place_ref as pr
from gpu_kit import api, projections  # noqa: F401  (the fixture is found by name)
from test_gpu_align_frames import H, INLIER_XYZ, MAP_FRAMES, N_FRAMES, OVER, ROWS, W, map_rows, sequences


@pytest.mark.gpu
def test_places_of_a_keyframes_descriptors_among_the_earlier_keyframes(api):
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
        span = (0, last)
        for kw in (dict(), dict(separation=1), dict(min_votes=5, max_places=2)):
            want = pr.places(query, desc, ids, tags, rows=(0, row_hi), tag_span=span, **kw)
            res, places, cand = ix.places(query, rows=(0, row_hi), tags=span, **kw)
            print("%d queries, %s: %d landmarks, %d tags voted, places (tag, votes, rows): %s" % (
                len(query), kw, res.n_landmarks, res.n_tags_voted, [(int(p["tag"]), int(p["votes"]), int(p["rows"])) for p in places]))
            assert res == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]) and res.n_landmarks > 0
            assert places.tobytes() == want["places"].tobytes()
            assert np.array_equal(cand["query"], want["cand_query"]) and np.array_equal(cand["row"], want["cand_row"])
            by_id = ix.places_from_ids(ids[cand["row"]], rows=(0, row_hi), tags=span, **kw)
            assert by_id[0] == res and by_id[1].tobytes() == places.tobytes()
            assert (places["tag"] < last).all()        # nothing of the keyframe kept out
        got = ix.tag_votes(ids[want["cand_row"]], (0, row_hi), span)
        for g, w in zip(got, pr.tag_votes(ids, tags, ids[want["cand_row"]], (0, row_hi), span)):
            assert g.tobytes() == w.tobytes()
        # the local-map query: the keyframes that saw the tracks of the last keyframe, the whole index this time
        tracked = np.unique(ids[row_hi:])
        want = pr.places_from_ids(ids, tags, tracked, tag_span=span)
        res, places = ix.places_from_ids(tracked, tags=span)
        assert res == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]) and places.tobytes() == want["places"].tobytes()
        print("local map of %d tracks: (tag, votes) %s" % (len(tracked), [(int(p["tag"]), int(p["votes"])) for p in places]))
        assert int(places["votes"].max()) == len(tracked) == int(ix.tag_votes(tracked, tags=(last, last))[0][0])       # every row of the last keyframe votes for it
    finally:
        vo.close(); ix.close()
