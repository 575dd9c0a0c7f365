"""The descriptor index fed from the frame pipeline on a real GPU (include/svo.h: svo_desc_index_add_frame): a 320 x 160
single-sequence context with the track and descriptor outputs on, six frames.  After every collect add_frame(SVO_OBS_INLIER) appends
exactly the ring rows a host filter keeps, in row order, with the right first_row and n_added; frame 5's descriptors matched against
the rows of frames <= 3 equal the reference on the same arrays; with three frames kept in flight and match called between submit and
collect, poses, observation rows and descriptor rows are bit for bit those of a run with no index at all; add_frame before any
collect, or on a frame that ran with descriptors off, is SVO_ERR_STATE."""
import numpy as np
import pytest

import desc_match_ref as mref
from gpu_kit import api, projections, streams  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

W, H, N_FRAMES, SEED0 = 320, 160, 6, 900
ROWS = 150                                            # rows per frame: the first 150 tracks, which keeps the reference's distance matrix small
# a tight RANSAC threshold, so that some of a frame's rows are not inliers and the filter has something to drop
OVER = dict(max_translation_norm=2.0, ransac_reprojection_error=0.25)


def frames():
    return streams(1, N_FRAMES, SEED0, W, H)[0]        # (lefts, rights)


def context(api, desc=True):
    vo = api.BatchVisualOdometry(W, H, 1, api.default_config(**OVER))
    vo.initalize_projection_matricies(*projections(W, H))
    vo.set_track_output(ROWS)
    if desc:
        vo.set_descriptor_output(True)
    return vo


@pytest.fixture(scope="module")
def fed(api):
    """the six frames run synchronously, add_frame after each -> what the ring held and what add_frame reported, per frame"""
    L, R = frames()
    INLIER = api._lib.OBS_INLIER
    vo, ix, everything = context(api), api.DescriptorIndex(1 << 14), api.DescriptorIndex(1 << 14)
    per = []
    try:
        for k in range(N_FRAMES):
            vo.stereo_callback_batch([L[k]], [R[k]])
            obs, desc = vo.last_track_obs(0), vo.last_track_descriptors(0)
            size = ix.size
            first, n = ix.add_frame(vo, 0, INLIER)
            per.append(dict(obs=obs, desc=desc, size_before=size, first=first, n=n, size_after=ix.size, all=everything.add_frame(vo, 0, 0)))
        D = np.concatenate([p["desc"][(p["obs"]["flags"] & INLIER) == INLIER] for p in per])
        I = np.concatenate([p["obs"]["id"][(p["obs"]["flags"] & INLIER) == INLIER] for p in per]).astype(np.uint64)
        yield dict(per=per, ix=ix, everything=everything, D=D, I=I)
    finally:
        vo.close(); ix.close(); everything.close()


def test_add_frame_appends_the_rows_a_host_filter_keeps(api, fed):
    INLIER = api._lib.OBS_INLIER
    at = at_all = 0
    for k, p in enumerate(fed["per"]):
        keep = (p["obs"]["flags"] & INLIER) == INLIER
        assert (p["size_before"], p["first"], p["n"], p["size_after"]) == (at, at, int(keep.sum()), at + int(keep.sum())), "frame %d" % k
        assert p["all"] == (at_all, len(p["obs"])), "frame %d, need_flags = 0" % k
        at += int(keep.sum()); at_all += len(p["obs"])
    D, I, ix = fed["D"], fed["I"], fed["ix"]
    assert ix.size == len(D) == at and at >= 200 and 0 < at < at_all, (at, at_all)
    # the index's rows are the host's rows: each host row finds itself at distance 0, and every field of every result — rows, distances,
    # ids of the best and of the best other landmark — is the reference's on the host's arrays
    got = ix.match(D)
    want = mref.match(D, D, I)
    assert got.tobytes() == want.tobytes()
    # (two tracks that round to one centre pixel share a descriptor: the lower row is then the best, under its own id)
    assert (got["dist"] == 0).all() and (got["row"] <= np.arange(len(D))).all() and (got["id"] == I[got["row"]]).all()
    assert (got["row"] == np.arange(len(D))).mean() > 0.9
    assert (got["row2"] >= 0).all() and (got["id2"] != got["id"]).all()


def test_frame_5_against_the_rows_of_frames_up_to_3(api, fed):
    per, ix, D, I = fed["per"], fed["ix"], fed["D"], fed["I"]
    q = per[5]["desc"]
    old = per[4]["first"]                               # rows of frames 0 .. 3
    assert len(q) > 100 and 100 < old < ix.size
    got = ix.match(q, 0, old)
    assert got.tobytes() == mref.match(q, D, I, 0, old).tobytes()
    assert (got["row"] < old).all() and (got["row2"] < old).all()
    # not vacuous: landmarks of frame 5 were seen in the old rows (how many find their own id again is printed, not asserted)
    ids5 = per[5]["obs"]["id"].astype(np.uint64)
    known = np.isin(ids5, I[:old])
    print("frame 5: %d of %d rows have their id among the %d old rows; %.2f of those find it as their best" %
          (known.sum(), len(q), old, (got["id"][known] == ids5[known]).mean() if known.any() else 0.0))
    assert known.sum() > 50


def run_in_flight(api, with_index):
    """the six frames as device frames, three in flight -> per frame (ok, pose, observation rows, descriptor rows) as bytes"""
    import torch
    L, R = frames()
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in zip(L, R)]
    torch.cuda.synchronize()
    vo = context(api)
    ix = api.DescriptorIndex(1 << 14) if with_index else None
    rng = np.random.default_rng(5)
    probe = rng.integers(0, 256, (130, 32), dtype=np.uint8)
    out, matched = [], 0
    try:
        if ix:
            ix.chunk_rows = 64
            ix.add(rng.integers(0, 256, (300, 32), dtype=np.uint8), np.arange(300) // 3)
        for k0 in range(0, N_FRAMES, 3):
            for k in range(k0, k0 + 3):
                vo.submit_device([dev[k][0].data_ptr()], [dev[k][1].data_ptr()], W)
                if ix:
                    matched += len(ix.match(probe))    # frames in flight: the search waits for its own stream only
            for k in range(k0, k0 + 3):
                if ix:
                    matched += len(ix.match(probe, 0, ix.size // 2))
                ok, T = vo.collect()
                out.append((ok.tobytes(), T.tobytes(), vo.last_track_obs(0).tobytes(), vo.last_track_descriptors(0).tobytes()))
                if ix:
                    ix.add_frame(vo, 0, api._lib.OBS_INLIER)   # two frames still in flight
        if ix:
            assert matched == 12 * 130 and ix.size > 300
    finally:
        vo.close()
        if ix:
            ix.close()
        del dev
    return out


def test_match_beside_frames_in_flight_changes_nothing(api, fed):
    plain, beside = run_in_flight(api, False), run_in_flight(api, True)
    assert len(plain) == len(beside) == N_FRAMES
    for k, (a, b) in enumerate(zip(plain, beside)):
        assert a[0] == b[0] and a[1] == b[1], "frame %d: ok / pose" % k
        assert a[2] == b[2], "frame %d: observation rows" % k
        assert a[3] == b[3], "frame %d: descriptor rows" % k
    assert sum(len(a[3]) for a in plain) > 32 * 500
    # and the frames in flight are the synchronous run's: the same rows reach an index either way
    for k, p in enumerate(fed["per"]):
        assert plain[k][2] == p["obs"].tobytes() and plain[k][3] == p["desc"].tobytes(), "frame %d" % k


def test_add_frame_refusals(api):
    L, R = frames()
    STATE = "status %d" % api._lib.SVO_ERR_STATE
    ix = api.DescriptorIndex(4096)
    vo = context(api)
    try:
        with pytest.raises(api._lib.SvoError, match=STATE):
            ix.add_frame(vo, 0, api._lib.OBS_INLIER)    # no frame collected yet
        vo.stereo_callback_batch([L[0]], [R[0]])
        assert ix.add_frame(vo, 0, 0) == (0, 0)         # a first frame has no tracks
        with pytest.raises(api._lib.SvoError, match="status %d" % api._lib.SVO_ERR_ARG):
            ix.add_frame(vo, 1, 0)                      # no such sequence
    finally:
        vo.close()
    off = context(api, desc=False)
    try:
        off.stereo_callback_batch([L[0]], [R[0]]); off.stereo_callback_batch([L[1]], [R[1]])
        assert len(off.last_track_obs(0)) > 50
        with pytest.raises(api._lib.SvoError, match=STATE):
            ix.add_frame(off, 0, 0)                     # the frame ran with descriptors off
        assert ix.size == 0
    finally:
        off.close(); ix.close()
    lazy = api.VisualOdometry(cfg=api.default_config(**OVER))
    with pytest.raises(api._lib.SvoError, match=STATE):
        api.DescriptorIndex(16).add_frame(lazy)         # the facade that has no context yet
    lazy.close()
