"""Consolidation fed from the frame pipeline on a real GPU (include/svo.h: svo_desc_index_add_frame_points,
svo_desc_index_consolidate, svo_desc_index_read_rows): a synthetic sequence of 13 frames, its frames 1 .. 11 added to one index as
keyframes tagged by their frame number, a track keeping its id from frame to frame; frame 12 is the later frame that is localised
against the map, before and after the consolidation.

 - asserted, because it holds by construction: after consolidate the size is the number of distinct ids, the index equals
   tests/consolidate_ref.py on read_rows' copy of the rows before, byte for byte; localize of the later frame still succeeds.
 - printed, not asserted: the rows, the candidates, the inliers and the distance of the pose from the odometry's, before and after.
   Nobody has measured what they should be.
Measured on an MI355X: 1 629 rows, 519 distinct ids, 1 110 rows dropped, 355 views gated out; localize of frame 12 before: 58
candidates, 55 inliers, largest |T - odometry| entry 0.307; after: 51 candidates, 44 inliers, 0.103 ("Landmark
consolidation")."""
import numpy as np
import pytest

import consolidate_ref as cr
import track_ids_ref as tr
from gpu_kit import api, calib, projections  # noqa: F401  (the fixture is found by name)

W, H, N_FRAMES, ROWS, RADIUS = 320, 160, 13, 150, 0.1
OVER = dict(max_translation_norm=2.0, ransac_reprojection_error=0.25)
INLIER_XYZ = tr.OBS_INLIER | tr.OBS_HAS_XYZ
MAP_FRAMES, QUERY_FRAME = tuple(range(1, 12)), 12


@pytest.mark.gpu
def test_a_map_of_eleven_keyframes_consolidated_still_localises_the_next_frame(api):
    from stereo_visual_odometry_amd import synthetic as syn
    A = syn.StereoSequence(cal=calib(W, H), n_frames=N_FRAMES, seed=900, step=0.3)
    ix = api.DescriptorIndex(1 << 12, points=True)
    vo = api.BatchVisualOdometry(W, H, 1, api.default_config(**OVER))
    try:
        Pl, Pr = projections(W, H)
        vo.initalize_projection_matricies(Pl, Pr)
        vo.set_track_output(ROWS)
        vo.set_descriptor_output(True)
        poses, per = [np.eye(4)], []
        for k in range(N_FRAMES):
            ok, T = vo.stereo_callback_batch([A.left[k]], [A.right[k]])
            assert bool(ok[0]) == (k > 0), "frame %d" % k
            if k > 0:
                poses.append(poses[-1] @ T[0])
            per.append((vo.last_track_obs(0), vo.last_track_descriptors(0)))
            if k in MAP_FRAMES:
                ix.add_frame_points(vo, poses[k - 1], tag=k)
        before = ix.read_rows()
        n0, distinct = ix.size, len(np.unique(before[1]))
        assert n0 > distinct > 0 and (before[3] >= 1).all()
        obs, desc = per[QUERY_FRAME]
        sel = (obs["flags"] & INLIER_XYZ) == INLIER_XYZ
        query, xy = desc[sel], np.ascontiguousarray(obs["l1"][sel])
        inv = np.linalg.inv(poses[QUERY_FRAME])
        K, R0, t0 = Pl[:, :3], np.ascontiguousarray(inv[:3, :3]), np.ascontiguousarray(inv[:3, 3])

        def localise(what):
            res, cand = ix.localize(K, query, xy, R0, t0)
            diff = float(np.abs(res.T - poses[QUERY_FRAME]).max()) if res.success else float("nan")
            print("%s: %d rows, %d queries, %d candidates, %d inliers, success %s, max |T - odometry| = %.3e" % (
                what, ix.size, len(query), res.n_candidates, res.n_inliers, res.success, diff))
            return res

        assert localise("before").success
        want = cr.consolidate(*before, RADIUS)
        res, kept_before = ix.consolidate(RADIUS)
        print("consolidate:", res)
        assert tuple(res) == tuple(want["result"]) and kept_before.tolist() == want["kept_before"].tolist()
        assert ix.size == distinct == res.n_groups
        assert not cr.same_rows(ix.read_rows(), cr.as_read(want))
        assert localise("after").success
    finally:
        vo.close(); ix.close()
