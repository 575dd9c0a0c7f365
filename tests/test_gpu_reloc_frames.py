"""Relocalisation fed from the frame pipeline on a real GPU (include/svo.h: svo_desc_index_add_frame_points, svo_desc_index_select,
svo_desc_index_localize): the 320 x 160 single-sequence stream of tests/test_gpu_desc_index_frames.py, six frames.  The map is the
inliers of frames 1 .. 3, each frame's points moved into the frame of camera 0 with the pose accumulated so far (an observation row's
xyz is in the T0 camera frame, so frame k's rows go through the pose of camera k - 1); the query is frame 5's observation rows
(l1 and descriptors).

 - select equals tests/reloc_ref.py on the host's copies of the same arrays — the points through reloc_ref.map_points, so the
   transform's bits are checked too;
 - localize equals api.cameraToWorld on select's candidate arrays byte for byte: pose, inlier set, iterations;
 - the returned T against the accumulated odometry pose of camera 5.  The bound is twice what the CPU reference chain measures for
   the same difference — the oracle pipeline with ids (track_ids_ref.IdOracleVO), descriptor_ref.describe, reloc_ref, the oracle's
   PnP and inverse transform — computed here from that chain, never from the GPU's numbers.  Measured on the CPU before any GPU run
   with this stream and seed (900): the reference alone gives 59 candidates and a successful PnP with 51 inliers (the condition: at
   least 30 and a success; test_the_reference_alone_meets_the_condition asserts it without a GPU), and
   max |T_reloc - T_odometry| = 6.80e-3, so the bound is 1.36e-2; drift over five frames is the dominant term;
 - with three frames in flight and localize called between submit and collect, poses, observation rows and descriptor rows are bit for
   bit those of a run without an index."""
import functools

import numpy as np
import pytest

import descriptor_ref as dref
import oracle_lib as orc
import reloc_ref as rref
import track_ids_ref as tr
from gpu_kit import api, projections, streams  # noqa: F401  (the fixture is found by name)

W, H, N_FRAMES, SEED0 = 320, 160, 6, 900
ROWS = 150
OVER = dict(max_translation_norm=2.0, ransac_reprojection_error=0.25)
INLIER_XYZ = tr.OBS_INLIER | tr.OBS_HAS_XYZ
MAP_FRAMES, QUERY_FRAME = (1, 2, 3), 5


def frames():
    return streams(1, N_FRAMES, SEED0, W, H)[0]


def build_map(per, poses):
    """the host's copy of the index after add_frame_points on frames 1 .. 3: rows in the order they are added"""
    D, I, X, G = [], [], [], []
    for k in MAP_FRAMES:
        obs, desc = per[k]
        keep = (obs["flags"] & INLIER_XYZ) == INLIER_XYZ
        D.append(desc[keep]); I.append(obs["id"][keep].astype(np.uint64))
        X.append(rref.map_points(poses[k - 1], obs["xyz"][keep])); G.append(np.full(int(keep.sum()), k, np.int32))
    return np.concatenate(D), np.concatenate(I), np.concatenate(X), np.concatenate(G)


@functools.lru_cache(maxsize=None)
def reference_chain():
    """the CPU chain alone -> dict: n_candidates, success, n_inliers, T (camera 5 in the map), P5 (odometry), diff"""
    L, R = frames()
    Pl, Pr = projections(W, H)
    vo = tr.IdOracleVO(orc.default_config(**OVER)); vo.initalize_projection_matricies(Pl, Pr)
    vo.assign_ids()
    poses, per = [np.eye(4)], []
    for k in range(N_FRAMES):
        ok, T = vo.stereo_callback(L[k], R[k])
        assert ok == (k > 0), "frame %d" % k
        if k > 0:
            poses.append(poses[-1] @ T)
        obs = vo.obs()[:ROWS]
        per.append((obs, dref.describe(L[k], np.ascontiguousarray(obs["l1"]))[0] if len(obs) else np.zeros((0, 32), np.uint8)))
    D, I, X, G = build_map(per, poses)
    obs, desc = per[QUERY_FRAME]
    cand = rref.select_index(desc, obs["l1"], D, I, X, G)
    ok, Rm, tm, inl, _ = orc.camera_to_world(Pl[:, :3], cand["xy"], cand["xyz"], np.eye(3), np.zeros(3))
    T = orc.inverse_transform(Rm, tm)
    return dict(n_candidates=len(cand["query"]), success=ok, n_inliers=len(inl), T=T, P5=poses[QUERY_FRAME],
                diff=float(np.abs(T - poses[QUERY_FRAME]).max()))


def test_the_reference_alone_meets_the_condition():
    """no GPU: the stream and the seed give the reference at least 30 candidates and a successful PnP, and the figures of the docstring"""
    ref = reference_chain()
    assert ref["n_candidates"] == 59 and ref["success"] and ref["n_inliers"] == 51
    assert abs(ref["diff"] - 6.80e-3) < 1e-5


def context(api):
    vo = api.BatchVisualOdometry(W, H, 1, api.default_config(**OVER))
    vo.initalize_projection_matricies(*projections(W, H))
    vo.set_track_output(ROWS)
    vo.set_descriptor_output(True)
    return vo


@pytest.fixture(scope="module")
def fed(api):
    """the six frames run synchronously; frames 1 .. 3 go into the index with the pose accumulated before them"""
    L, R = frames()
    vo, ix = context(api), api.DescriptorIndex(1 << 12, points=True)
    poses, per, added = [np.eye(4)], [], {}
    try:
        for k in range(N_FRAMES):
            ok, T = vo.stereo_callback_batch([L[k]], [R[k]])
            assert bool(ok[0]) == (k > 0), "frame %d" % k
            if k > 0:
                poses.append(poses[-1] @ T[0])
            per.append((vo.last_track_obs(0), vo.last_track_descriptors(0)))
            if k in MAP_FRAMES:
                added[k] = ix.add_frame_points(vo, poses[k - 1], tag=k)
        yield dict(ix=ix, per=per, poses=poses, added=added, K=projections(W, H)[0][:, :3])
    finally:
        vo.close(); ix.close()


@pytest.mark.gpu
def test_select_equals_the_reference_on_the_hosts_copies(fed):
    D, I, X, G = build_map(fed["per"], fed["poses"])
    at = 0
    for k in MAP_FRAMES:
        n = int((G == k).sum())
        assert fed["added"][k] == (at, n) and n > 50, "frame %d" % k
        at += n
    assert fed["ix"].size == at
    obs, desc = fed["per"][QUERY_FRAME]
    got = fed["ix"].select(desc, obs["l1"])
    want = rref.select_index(desc, obs["l1"], D, I, X, G)
    assert got["query"].tolist() == want["query"].tolist() and got["row"].tolist() == want["row"].tolist()
    assert got["xy"].tobytes() == want["xy"].tobytes()
    assert got["xyz"].tobytes() == want["xyz"].tobytes()                 # the transform, bit for bit
    assert len(got["query"]) >= 30


@pytest.mark.gpu
def test_localize_equals_camera_to_world_and_the_odometry_pose(api, fed):
    ref = reference_chain()
    print("reference chain: %d candidates, success %s, %d inliers, max |T - odometry| = %.3e" % (ref["n_candidates"], ref["success"], ref["n_inliers"], ref["diff"]))
    assert ref["n_candidates"] >= 30 and ref["success"], "the stream does not meet the test's condition for the reference alone"
    bound = 2 * ref["diff"]
    obs, desc = fed["per"][QUERY_FRAME]
    ix = fed["ix"]
    sel = ix.select(desc, obs["l1"])
    prm = ix.reloc_params()
    (inl, ok), R, t, iters = api.cameraToWorld(fed["K"], sel["xy"], sel["xyz"], np.eye(3), np.zeros(3), prm.ransac_iterations, prm.reproj_error, prm.confidence)
    res, cand = ix.localize(fed["K"], desc, obs["l1"])
    assert ok and res.success and res.n_candidates == len(sel["query"]) >= 30
    assert cand["query"].tolist() == sel["query"].tolist() and cand["row"].tolist() == sel["row"].tolist()
    assert res.R.tobytes() == R.tobytes() and res.t.tobytes() == t.tobytes() and res.iters_run == iters
    assert np.flatnonzero(cand["inlier"]).tolist() == inl.tolist() and res.n_inliers == len(inl)
    diff = float(np.abs(res.T - fed["poses"][QUERY_FRAME]).max())
    print("GPU: %d candidates, %d inliers, max |T - odometry| = %.3e, bound %.3e" % (res.n_candidates, res.n_inliers, diff, bound))
    assert diff <= bound, (diff, bound)


def run_in_flight(api, with_index):
    """the six frames as device frames, three in flight -> per frame (ok, pose, observation rows, descriptor rows) as bytes"""
    import torch
    import reloc_cases as cases
    L, R = frames()
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in zip(L, R)]
    torch.cuda.synchronize()
    vo = context(api)
    s = cases.scene(130, 3, outliers=20)
    ix = api.DescriptorIndex(1 << 12, points=True) if with_index else None
    out, located = [], 0
    try:
        if ix:
            ix.chunk_rows = 64
            ix.add_points(s["desc"], s["ids"], s["xyz"], s["tags"])
        for k0 in range(0, N_FRAMES, 3):
            for k in range(k0, k0 + 3):
                vo.submit_device([dev[k][0].data_ptr()], [dev[k][1].data_ptr()], W)
                if ix:
                    located += ix.localize(s["K"], s["query"], s["xy"])[0].success    # frames in flight: the call waits for its own stream only
            for k in range(k0, k0 + 3):
                if ix:
                    located += len(ix.select(s["query"], s["xy"], row_lo=0, row_hi=ix.size // 2)["query"]) > 0
                ok, T = vo.collect()
                out.append((ok.tobytes(), T.tobytes(), vo.last_track_obs(0).tobytes(), vo.last_track_descriptors(0).tobytes()))
                if ix and k > 0:
                    ix.add_frame_points(vo, None, tag=k)                 # two frames still in flight
        if ix:
            assert located == 12 and ix.size > 130
    finally:
        vo.close()
        if ix:
            ix.close()
        del dev
    return out


@pytest.mark.gpu
def test_localize_beside_frames_in_flight_changes_nothing(api, fed):
    plain, beside = run_in_flight(api, False), run_in_flight(api, True)
    assert len(plain) == len(beside) == N_FRAMES
    for k, (a, b) in enumerate(zip(plain, beside)):
        assert a[0] == b[0] and a[1] == b[1], "frame %d: ok / pose" % k
        assert a[2] == b[2], "frame %d: observation rows" % k
        assert a[3] == b[3], "frame %d: descriptor rows" % k
    assert sum(len(a[3]) for a in plain) > 32 * 500
    for k, p in enumerate(fed["per"]):                                   # and the frames in flight are the synchronous run's
        assert plain[k][2] == p[0].tobytes() and plain[k][3] == p[1].tobytes(), "frame %d" % k


@pytest.mark.gpu
def test_add_frame_points_refusals(api, fed):
    ARG, STATE = "status %d" % api._lib.SVO_ERR_ARG, "status %d" % api._lib.SVO_ERR_STATE
    L, R = frames()
    vo = context(api)
    plain, ix = api.DescriptorIndex(1024), api.DescriptorIndex(1024, points=True)
    try:
        with pytest.raises(api._lib.SvoError, match=STATE):
            ix.add_frame_points(vo)                                      # no frame collected yet
        vo.stereo_callback_batch([L[0]], [R[0]]); vo.stereo_callback_batch([L[1]], [R[1]])
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.add_frame_points(vo)                                   # an index without points
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_frame_points(vo, tag=-1)
        bad = np.eye(4); bad[1, 3] = np.nan
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_frame_points(vo, bad)
        assert ix.size == 0
        first, n = ix.add_frame_points(vo, need_flags=0)                 # HAS_XYZ is required whatever the caller asks for
        obs = vo.last_track_obs(0)
        has = (obs["flags"] & tr.OBS_HAS_XYZ) != 0
        assert (first, n) == (0, int(has.sum())) and n > 50
        # cam_to_map = NULL is the identity: every row found again by its own descriptor carries the observation's own xyz
        desc = vo.last_track_descriptors(0)[has]
        got = ix.select(desc, obs["l1"][has], max_dist=0, ratio_num=1, ratio_den=1)
        assert len(got["query"]) > 50 and got["xyz"].tobytes() == obs["xyz"][has][got["row"]].tobytes()
    finally:
        vo.close(); plain.close(); ix.close()
