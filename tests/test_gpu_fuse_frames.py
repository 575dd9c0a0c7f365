"""Landmark fusion fed from the frame pipeline on a real GPU (include/svo.h: svo_desc_index_align, svo_desc_index_transform_points,
svo_desc_index_fuse): the two sequences' maps of tests/test_gpu_align_frames.py — one scene seen from two start poses, each map in its
own frame, A's rows first, then B's — aligned, B's rows moved into A's frame, and B's landmarks fused into A's.

 - asserted, because it holds by construction: the pairs, the four counts and every row's id afterwards equal tests/fuse_ref.py on the
   host's copies of the same rows (B's points moved by reloc_ref.map_points with the alignment's T, the formula of
   svo_desc_index_transform_points); the two points of every pair lie within the radius on every axis; ids changed only in B's span.
 - printed, not asserted: n_pairs, n_fused and what svo_desc_index_localize finds for the queries of B's last frame before and after
   the fusion.  Candidates need not grow: rule 2 of "Relocalisation" keeps one query per landmark id, so two former candidates of
   the two copies of one landmark become one.
radius = 0.3 m is the alignment test's inlier_dist, this scene's choice; it is no default.
Measured on an MI355X: see DESIGN.md, "Landmark fusion"."""
import numpy as np
import pytest

import fuse_ref as fr
import reloc_ref as rref
from gpu_kit import api, projections  # noqa: F401  (the fixture is found by name)
from test_gpu_align_frames import H, HYPOTHESES, INLIER_DIST, MAP_FRAMES, MIN_PAIRS, N_FRAMES, OVER, ROWS, W, map_rows, sequences

RADIUS = INLIER_DIST


@pytest.mark.gpu
def test_fuse_after_the_merge_of_two_sequences_maps(api):
    A, B, off = sequences()
    ix = api.DescriptorIndex(1 << 12, points=True)
    rows, spans, last = [], [], None
    try:
        for s, tag0 in ((A, 0), (B, 100)):
            vo = api.BatchVisualOdometry(W, H, 1, api.default_config(**OVER))
            try:
                vo.initalize_projection_matricies(*projections(W, H))
                vo.set_track_output(ROWS)
                vo.set_descriptor_output(True)
                poses, per, lo = [np.eye(4)], [], ix.size
                for k in range(N_FRAMES):
                    ok, T = vo.stereo_callback_batch([s.left[k]], [s.right[k]])
                    assert bool(ok[0]) == (k > 0), "frame %d" % k
                    if k > 0:
                        poses.append(poses[-1] @ T[0])
                    per.append((vo.last_track_obs(0), vo.last_track_descriptors(0)))
                    if k in MAP_FRAMES:
                        ix.add_frame_points(vo, poses[k - 1], tag=tag0 + k)
                rows.append(map_rows(per, poses, tag0)); spans.append((lo, ix.size))
                last = per[-1]
            finally:
                vo.close()
        dst, src = spans
        desc, ids, xyz, tags = (np.concatenate([a, b]) for a, b in zip(*rows))
        # the two contexts numbered their tracks independently: B's ids move out of A's range first, in B's rows only
        own = np.unique(ids[src[0]:src[1]])
        ids = ids.copy()
        ids[src[0]:src[1]] += np.uint64(1 << 40)
        assert ix.relabel(own, own + np.uint64(1 << 40), rows=src) == src[1] - src[0]
        res, _ = ix.align(src, dst, INLIER_DIST, min_pairs=MIN_PAIRS, hypotheses=HYPOTHESES)
        assert res.success and ix.transform_points(res.T, rows=src) == (src[1] - src[0], 0)
        xyz = xyz.copy()
        xyz[src[0]:src[1]] = rref.map_points(res.T, xyz[src[0]:src[1]])
        # the queries: B's last frame, as a camera that relocalises in the merged map would pose them
        K = np.ascontiguousarray(projections(W, H)[0][:, :3], np.float32)
        q_desc, q_xy = last[1], np.ascontiguousarray(last[0]["l1"], np.float32)
        before, _ = ix.localize(K, q_desc, q_xy, np.eye(3), np.zeros(3))
        want = fr.fuse(desc, ids, xyz, tags, src, dst, RADIUS)
        got, pairs = ix.fuse(src, dst, RADIUS)
        after, _ = ix.localize(K, q_desc, q_xy, np.eye(3), np.zeros(3))
        print("fuse: %d pairs, %d same, %d fused, %d rows relabelled of %d + %d rows" % (got + (dst[1] - dst[0], src[1] - src[0])))
        print("localize with %d queries: before %d candidates, %d inliers, success %d; after %d candidates, %d inliers, success %d" % (
            len(q_desc), before.n_candidates, before.n_inliers, before.success, after.n_candidates, after.n_inliers, after.success))
        assert got == (want["n_pairs"], want["n_same"], want["n_fused"], want["n_rows_relabelled"]) and got.n_pairs > 0
        assert np.array_equal(pairs["src"], want["pair_src"]) and np.array_equal(pairs["dst"], want["pair_dst"])
        assert (np.abs(xyz[pairs["src"]] - xyz[pairs["dst"]]) <= np.float32(RADIUS)).all()      # by rule 1
        now = np.array([ix.match(desc[r:r + 1], r, r + 1)[0]["id"] for r in range(ix.size)], np.uint64)    # a row's id: a search of that row alone
        assert np.array_equal(now, want["ids"]) and np.array_equal(now[dst[0]:dst[1]], ids[dst[0]:dst[1]])
        assert int((now != ids).sum()) == got.n_rows_relabelled
    finally:
        ix.close()
