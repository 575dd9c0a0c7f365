"""The batched insertion fed from the frame pipeline on a real GPU (include/svo.h, "Batched insertion": svo_desc_index_add_frames,
svo_desc_index_add_frames_points): 320 x 160 streams and max_rows 150, as tests/test_gpu_reloc_frames.py, in contexts of 1, 2, 9 and
65 sequences, three frames.  The contract is rule 8: one index is filled by the loop of single calls, one by the batch call, and
read_rows, first_row, n_added and the size are compared after every collect, plain and with points.  Then entry selection (a
subset, a permutation, a duplicate), a sequence idle under the mask and a first frame (n_tracks = 0: no rows), id_base = seq << 48,
the call beside two frames in flight, the staged path after eight more submits, and the single calls' refusals.
Sequence i of a context replays stream i % 5: five distinct streams are enough for rows that differ between neighbours."""
import numpy as np
import pytest

import insert_ref as ir
from gpu_kit import api, projections, streams  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

W, H, N_FRAMES, SEED0, ROWS = 320, 160, 3, 900, 150
OVER = dict(max_translation_norm=2.0, ransac_reprojection_error=0.25)
DISTINCT = 5


@pytest.fixture(scope="module")
def five():
    return streams(DISTINCT, N_FRAMES, SEED0, W, H)


def context(api, n, descriptors=True):
    vo = api.BatchVisualOdometry(W, H, n, api.default_config(**OVER))
    vo.initalize_projection_matricies(*projections(W, H))
    vo.set_track_output(ROWS)
    if descriptors:
        vo.set_descriptor_output(True)
    return vo


def feed(vo, five, k, active=None):
    n = vo.n_seq
    return vo.stereo_callback_batch([five[i % DISTINCT][0][k] for i in range(n)], [five[i % DISTINCT][1][k] for i in range(n)], active)


def rows_of(ix, points):
    return [None if a is None else a.tobytes() for a in ix.read_rows(want=("desc", "ids", "xyz", "tags") if points else ("desc", "ids"))]


def loop(ix, vo, seqs, points, T=None, tag=0, need=ir.OBS_INLIER):
    """the loop of single calls over the entries -> (first_row, n_added)"""
    out = [ix.add_frame_points(vo, None if T is None else T[b], tag=tag, seq=s, need_flags=need) if points else ix.add_frame(vo, s, need)
           for b, s in enumerate(seqs)]
    return [f for f, _ in out], [n for _, n in out]


def both(api, vo, seqs, points, T=None, tag=0, need=ir.OBS_INLIER, pair=None, path=None):
    """the loop into pair[0], the batch call into pair[1] -> the batch call's (first_row, n_added), everything compared"""
    a, b = pair
    want = loop(a, vo, seqs if seqs is not None else range(vo.n_seq), points, T, tag, need)
    n = len(want[0])
    got = b.add_frames_points(vo, T, [tag] * n, seqs, need) if points else b.add_frames(vo, seqs, need)
    assert got[0].tolist() == want[0] and got[1].tolist() == want[1], (got, want)
    assert a.size == b.size and rows_of(a, points) == rows_of(b, points)
    if path is not None:
        assert b.insert_stats()["last_path"] == path
    return got


@pytest.mark.parametrize("n", [1, 2, 9, 65])
def test_the_batch_call_equals_the_loop_after_every_collect(api, five, n):
    vo = context(api, n)
    cap = n * ROWS * N_FRAMES
    plain, pts = [api.DescriptorIndex(cap) for _ in range(2)], [api.DescriptorIndex(cap, points=True) for _ in range(2)]
    poses = np.tile(np.eye(4), (n, 1, 1))
    try:
        for k in range(N_FRAMES):
            ok, T = feed(vo, five, k)
            got = both(api, vo, None, False, pair=plain, path=api._lib.INSERT_PATH_RING)
            both(api, vo, None, True, poses, tag=k, pair=pts, path=api._lib.INSERT_PATH_RING)
            counts = [vo.last_track_obs(s, with_count=True)[1] for s in range(n)]
            if k == 0:                                                  # a first frame: n_tracks = 0, no rows, nothing added
                assert counts == [0] * n and got[1].tolist() == [0] * n and plain[1].insert_stats()["rows_scanned"] == 0
            else:
                assert ok.all() and min(counts) > 50 and got[1].min() > 10
                assert plain[1].insert_stats()["rows_scanned"] == sum(min(c, ROWS) for c in counts)
                poses = poses @ T
        assert plain[1].size > n * 60 and pts[1].size > n * 60
    finally:
        vo.close()
        for ix in plain + pts:
            ix.close()


def test_entry_selection_mask_and_id_base(api, five):
    n = 9
    vo = context(api, n)
    cap = 4 * n * ROWS
    pts = [api.DescriptorIndex(cap, points=True) for _ in range(2)]
    based = api.DescriptorIndex(cap)
    T9 = np.stack([ir.pose(s) for s in range(n)])
    try:
        feed(vo, five, 0); feed(vo, five, 1)
        for seqs in ([1, 4, 7], [8, 2, 5, 0, 3, 7, 1, 6, 4], [3, 3, 0, 3]):       # a subset, a permutation, a duplicate
            both(api, vo, seqs, True, T9[seqs], tag=2, pair=pts)
        # id_base = seq << 48: the ids read back are the rows' ids offset, and no two sequences share one
        base = np.arange(n, dtype=np.uint64) << np.uint64(48)
        first, added = based.add_frames(vo, None, 0, base)
        ids = based.read_rows(want=("ids",))[1]
        seen = set()
        for s in range(n):
            obs = vo.last_track_obs(s)
            mine = ids[first[s]:first[s] + added[s]]
            assert added[s] == len(obs) > 50 and mine.tolist() == (obs["id"].astype(np.uint64) + base[s]).tolist()
            assert (mine >> np.uint64(48) == s).all() and not seen & set(mine.tolist())
            seen |= set(mine.tolist())
        # a frame with sequence 4 idle under the mask: its header says no tracks, and it contributes no rows
        active = [s != 4 for s in range(n)]
        feed(vo, five, 2, active)
        assert vo.last_track_obs(4, with_count=True)[1] == 0 and len(vo.last_track_obs(4)) == 0
        got = both(api, vo, None, True, T9, tag=3, pair=pts, need=0)
        assert got[1][4] == 0 and all(got[1][s] > 20 for s in range(n) if s != 4)
        both(api, vo, [4, 4], True, T9[[4, 4]], tag=3, pair=pts)                  # nothing but idle entries: no launch, nothing added
    finally:
        vo.close(); based.close()
        for ix in pts:
            ix.close()


def run_in_flight(api, five, with_index):
    """six frames (the three, twice) of two sequences as device frames, two in flight, the batch call between submit and collect ->
    per frame (ok, poses, observation rows, descriptor rows) as bytes"""
    import torch
    n = 2
    dev = [[(torch.from_numpy(five[i][0][k % N_FRAMES]).cuda(), torch.from_numpy(five[i][1][k % N_FRAMES]).cuda()) for i in range(n)] for k in range(6)]
    torch.cuda.synchronize()
    vo = context(api, n)
    ix = api.DescriptorIndex(1 << 13, points=True) if with_index else None
    out = []

    def collect():
        ok, T = vo.collect()
        out.append((ok.tobytes(), T.tobytes(), b"".join(vo.last_track_obs(i).tobytes() for i in range(n)),
                    b"".join(vo.last_track_descriptors(i).tobytes() for i in range(n))))

    def submit(k):
        vo.submit_device([a.data_ptr() for a, _ in dev[k]], [b.data_ptr() for _, b in dev[k]], W)
    try:
        submit(0); submit(1); collect()
        for k in (2, 4):
            submit(k)                                                   # two frames in flight; the last collected frame's rows are in the ring
            if ix:
                ix.add_frames_points(vo, tags=[k, k])
                assert ix.insert_stats()["last_path"] == api._lib.INSERT_PATH_RING
            collect()
            submit(k + 1)
            if ix:
                ix.add_frames(vo, need_flags=0)
            collect()
        collect()
        if ix:
            assert ix.size > 100
    finally:
        vo.close()
        if ix:
            ix.close()
        del dev
    return out


def test_the_call_beside_frames_in_flight_changes_nothing(api, five):
    plain, beside = run_in_flight(api, five, False), run_in_flight(api, five, True)
    assert len(plain) == len(beside) == 6
    for k, (a, b) in enumerate(zip(plain, beside)):
        assert a[0] == b[0] and a[1] == b[1], "frame %d: ok / pose" % k
        assert a[2] == b[2], "frame %d: observation rows" % k
        assert a[3] == b[3], "frame %d: descriptor rows" % k
    assert sum(len(a[3]) for a in plain) > 2 * 32 * 200


def test_the_staged_path_after_eight_more_submits(api, five):
    """the ring has eight slots: the eighth submit after a collect is about to write the collected frame's slot, so the context keeps
    its rows in copies of its own, and the batch call stages them: the same bits, last_path says staged"""
    import torch
    n = 2
    dev = [[(torch.from_numpy(five[i][0][k % N_FRAMES]).cuda(), torch.from_numpy(five[i][1][k % N_FRAMES]).cuda()) for i in range(n)] for k in range(10)]
    torch.cuda.synchronize()
    vo = context(api, n)
    T2 = np.stack([ir.pose(7), ir.pose(8)])
    ring, staged = [api.DescriptorIndex(2048, points=True) for _ in range(2)], [api.DescriptorIndex(2048, points=True) for _ in range(2)]
    try:
        for k in range(2):
            vo.submit_device([a.data_ptr() for a, _ in dev[k]], [b.data_ptr() for _, b in dev[k]], W)
            vo.collect()
        both(api, vo, None, True, T2, tag=1, pair=ring, path=api._lib.INSERT_PATH_RING)
        for k in range(2, 10):
            vo.submit_device([a.data_ptr() for a, _ in dev[k]], [b.data_ptr() for _, b in dev[k]], W)
        both(api, vo, None, True, T2, tag=1, pair=staged, path=api._lib.INSERT_PATH_STAGED)
        assert staged[1].size > 100 and rows_of(staged[1], True) == rows_of(ring[1], True)
        for k in range(8):
            vo.collect()
    finally:
        vo.close()
        for ix in ring + staged:
            ix.close()
        del dev


def test_refusals(api, five):
    ARG, STATE = "status %d" % api._lib.SVO_ERR_ARG, "status %d" % api._lib.SVO_ERR_STATE
    vo, bare = context(api, 2), context(api, 1, descriptors=False)
    plain, ix = api.DescriptorIndex(1024), api.DescriptorIndex(1024, points=True)
    try:
        for call in (lambda: ix.add_frames(vo), lambda: ix.add_frames_points(vo)):
            with pytest.raises(api._lib.SvoError, match=STATE):
                call()                                                  # no frame collected yet
        feed(vo, five, 0); feed(vo, five, 1); feed(bare, five, 0); feed(bare, five, 1)
        with pytest.raises(api._lib.SvoError, match=STATE):
            ix.add_frames(bare)                                         # the descriptor output was off
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.add_frames_points(vo)                                 # an index without points
        for seqs in ([0, 2], [-1], [0] * 1025):
            with pytest.raises(api._lib.SvoError, match=ARG):
                ix.add_frames(vo, seqs)                                 # a sequence outside the context; too many entries
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_frames_points(vo, tags=[0, -1])
        bad = np.tile(np.eye(4), (2, 1, 1)); bad[1, 0, 0] = np.nan
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.add_frames_points(vo, bad)
        small = api.DescriptorIndex(10, points=True)
        with pytest.raises(api._lib.SvoError, match=ARG):
            small.add_frames_points(vo)                                 # more kept rows than room
        assert ix.size == 0 and plain.size == 0 and small.size == 0
        small.close()
        first, added = ix.add_frames_points(vo, need_flags=0)           # HAS_XYZ is required whatever the caller asks for
        has = [int(((vo.last_track_obs(s)["flags"] & ir.OBS_HAS_XYZ) != 0).sum()) for s in range(2)]
        assert added.tolist() == has and first.tolist() == [0, has[0]] and min(has) > 50
    finally:
        vo.close(); bare.close(); plain.close(); ix.close()
