"""The descriptor output of the frame pipeline on a real GPU (include/svo.h, "Binary descriptors for the observation rows"): in every
case each frame's and each sequence's descriptor rows equal descriptor_ref.describe(the left image of that frame as ingest left it,
the observation rows' l1), bit for bit, and their count is the observation rows' — lone-stream (1, 3 sequences) and many-sequence
(10) launch lists at test_gpu_track_ids.py's sizes, truncation, frames in flight, a ragged frame and a reset, lk_window = 5 (a
stored border of 12 < 15 pixels), CLAHE, a co-resident pair of contexts (the lean build), the host copy of a slot about to be
rewritten, the refusals, "off means off", and the discrimination relation tests/test_descriptor_ref.py pins on the reference."""
import subprocess

import numpy as np
import pytest

import descriptor_ref as ref
import track_ids_ref as tr
from gpu_kit import api, f32_bits as bits, same, snap  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

SIZES = {"even": (320, 160), "odd": (323, 163)}       # tests/test_gpu_track_ids.py's
OVER = dict(max_translation_norm=2.0)
SEED0 = 900
ROWS = 4096                                           # more than any frame here has tracks

_described = {}


def want_rows(key, img, l1):
    """ref.describe(img, l1), computed once per (image, points): sequences that replay one stream ask for the same rows"""
    k = (key, l1.tobytes())
    if k not in _described:
        _described[k] = ref.describe(img, l1)[0]
    return _described[k]


def stream_of(i, n_frames, w, h):
    return tr.stream(n_frames, SEED0 + 31 * (i % 3), w, h)


def check_frame(vo, k, i, img_key, img, max_rows, idle=False):
    """frame k, sequence i: one descriptor row per observation row, each the reference's at the row's l1 -> the rows"""
    obs, n_tracks = vo.last_track_obs(i, with_count=True)
    desc = vo.last_track_descriptors(i)
    assert desc.shape == (len(obs), 32) and len(obs) == min(n_tracks, max_rows), "frame %d seq %d: %s rows for %d observation rows" % (k, i, desc.shape, len(obs))
    if idle:
        assert len(desc) == 0, "frame %d seq %d: an idle sequence has rows" % (k, i)
        return obs, desc
    want = want_rows(img_key, img, np.ascontiguousarray(obs["l1"]))
    assert np.array_equal(desc, want), "frame %d seq %d: rows %s differ" % (k, i, np.nonzero((desc != want).any(1))[0][:8])
    return obs, desc


def run(api, size, n_seq, n_frames, cfg_over=None, max_rows=ROWS, depth=0, schedules=None, vo_hook=None, image_of=None):
    """An n_seq-sequence context with both outputs on over n_frames frames.  depth 0: synchronous host frames; depth > 0: device
    frames, `depth` submitted before each group is collected, every collect checked against its own frame.  schedules: per sequence a
    tuple of "run" / "idle" / "reset" per frame.  image_of(img): the left image as ingest leaves it (CLAHE).  -> (per frame per sequence
    (obs, desc), paths)."""
    w, h = SIZES[size]
    cfg = api.default_config(**dict(OVER, **(cfg_over or {})))
    schedules = schedules or [("run",) * n_frames] * n_seq
    S = [stream_of(i, n_frames, w, h) for i in range(n_seq)]
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg)
    vo.initalize_projection_matricies(*S[0][1])
    vo.set_track_output(max_rows)
    vo.set_descriptor_output(True)
    if vo_hook:
        vo_hook(vo)
    out, paths = [], []
    tag = (size, repr(sorted((cfg_over or {}).items())), image_of is not None)

    def checked(k):
        per = []
        for i in range(n_seq):
            img = S[i][0][0][k]
            per.append(check_frame(vo, k, i, tag + (i % 3, k), image_of(img) if image_of else img, max_rows, idle=schedules[i][k] == "idle"))
        return per

    def prepare(k):
        for i in range(n_seq):
            if schedules[i][k] == "reset":
                vo.reset_sequence(i)
        on = [schedules[i][k] != "idle" for i in range(n_seq)]
        return on, (None if all(on) else on)

    try:
        if depth == 0:
            for k in range(n_frames):
                on, act = prepare(k)
                vo.stereo_callback_batch([S[i][0][0][k] if on[i] else None for i in range(n_seq)],
                                         [S[i][0][1][k] if on[i] else None for i in range(n_seq)], active=act)
                paths.append(vo.last_frame_path())
                out.append(checked(k))
        else:
            import torch
            dev = [[(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in zip(*s[0])] for s in S]
            torch.cuda.synchronize()
            stride = S[0][0][0][0].strides[0]
            for k0 in range(0, n_frames, depth):
                group = list(range(k0, min(k0 + depth, n_frames)))
                for j in group:
                    on, act = prepare(j)
                    vo.submit_device([dev[i][j][0].data_ptr() if on[i] else None for i in range(n_seq)],
                                     [dev[i][j][1].data_ptr() if on[i] else None for i in range(n_seq)], stride, active=act)
                    paths.append(vo.last_frame_path())
                for j in group:
                    vo.collect()
                    out.append(checked(j))
            del dev
    finally:
        vo.close()
    assert all(p & api._lib.PATH_DESCRIPTORS and p & api._lib.PATH_TRACK_IDS for p in paths), paths
    return out, paths


def counts(out, i=0):
    return [len(per[i][1]) for per in out]


# ------------------------------------------------------------------------------------------------ every launch list
@pytest.mark.parametrize("n_seq,size", [(1, "odd"), (3, "even"), (10, "odd"), (10, "even")])
def test_rows_match_the_reference(api, n_seq, size):
    out, paths = run(api, size, n_seq, 4)
    assert bool(paths[-1] & api._lib.PATH_INGEST_AHEAD) == (n_seq > 8), paths
    assert counts(out)[0] == 0 and min(counts(out)[1:]) > 100, counts(out)
    d = out[-1][0][1]
    assert len(np.unique(d, axis=0)) > len(d) // 2, "vacuous descriptors"   # (tracks that round to one centre pixel share a row)


def test_truncation_touches_nothing_beyond_max_rows(api):
    out, _ = run(api, "even", 3, 3, max_rows=100)                    # run() has compared every sequence's rows, the neighbour's first included
    assert all(len(per[i][0]) == 100 and len(per[i][1]) == 100 for per in out[1:] for i in range(3))


def test_frames_in_flight_each_collect_returns_its_own_rows(api):
    out, _ = run(api, "odd", 10, 6, depth=3)
    assert len(set(counts(out)[1:])) > 1, "the frames cannot be told apart"


def test_ragged_frame_and_reset(api):
    sched = [("run",) * 6, ("run", "run", "idle", "idle", "run", "run"), ("run", "run", "run", "reset", "run", "run")]
    out, _ = run(api, "even", 3, 6, depth=1, schedules=sched)
    assert counts(out, 1)[2:4] == [0, 0] and counts(out, 1)[4] > 50 and counts(out, 2)[3] == 0 and counts(out, 2)[4] > 50 and min(counts(out, 0)[1:]) > 100


def test_window_5_stores_a_border_narrower_than_the_patch(api):
    out, _ = run(api, "odd", 1, 3, cfg_over=dict(win_w=5, win_h=5))
    obs = np.concatenate([per[0][0] for per in out[1:]])
    w, h = SIZES["odd"]
    near = (obs["l1"][:, 0] < 15) | (obs["l1"][:, 1] < 15) | (obs["l1"][:, 0] > w - 16) | (obs["l1"][:, 1] > h - 16)
    assert len(obs) > 100 and near.sum() >= 20, "too few rows whose patch crosses the image's edge (%d)" % near.sum()


def test_clahe_frames_are_described_on_the_equalised_image(api):
    from clahe_ref import clahe_ref
    eq = {}

    def image_of(img):
        k = img.tobytes()
        if k not in eq:
            eq[k] = clahe_ref(img, 2.0, (4, 2))
        return eq[k]

    out, paths = run(api, "even", 1, 3, vo_hook=lambda vo: vo.set_clahe(2.0, (4, 2)), image_of=image_of)
    assert all(p & api._lib.PATH_CLAHE for p in paths) and min(counts(out)[1:]) > 50


def test_co_resident_contexts_run_the_lean_build(api):
    """two 9-sequence contexts on one device at w = 22, whose LK build leaves the 96 registers device_sharing() asks for
    (tests/test_gpu_shared_device_builds.py pins that): frames submitted interleaved, every frame on the lean builds"""
    import torch
    L = api._lib
    w, h = SIZES["even"]
    n_seq, n_frames = 9, 3
    cfg = api.default_config(win_w=22, win_h=22, **OVER)
    S = [stream_of(i, n_frames, w, h) for i in range(3)]
    ctx = []
    try:
        for c in range(2):
            vo = api.BatchVisualOdometry(w, h, n_seq, cfg)
            vo.initalize_projection_matricies(*S[0][1])
            vo.set_track_output(ROWS); vo.set_descriptor_output(True)
            ctx.append(vo)
        assert ctx[0].lk_registers_left() >= 96
        dev = [[(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in zip(*s[0])] for s in S]
        torch.cuda.synchronize()
        total = 0
        for k in range(n_frames):
            for c, vo in enumerate(ctx):
                vo.submit_device([dev[(i + c) % 3][k][0].data_ptr() for i in range(n_seq)], [dev[(i + c) % 3][k][1].data_ptr() for i in range(n_seq)], w)
                p = vo.last_frame_path()
                assert p & L.PATH_LEAN and p & L.PATH_DESCRIPTORS, (k, c, p)
            for c, vo in enumerate(ctx):
                vo.collect()
                for i in range(n_seq):
                    s = (i + c) % 3
                    total += len(check_frame(vo, k, i, ("lean", s, k), S[s][0][0][k], ROWS)[1])
        assert total > 2000
    finally:
        for vo in ctx:
            vo.close()


def test_rows_outlive_the_ring_slot_they_were_written_in(api):
    """the last collected frame's rows are read in place until a later submit is about to rewrite their slot — eight frames on —
    and from the host copy made at that moment afterwards"""
    import torch
    w, h = SIZES["even"]
    (Ls, Rs), P = tr.stream(10, SEED0, w, h)
    vo = api.BatchVisualOdometry(w, h, 1, api.default_config(**OVER))
    try:
        vo.initalize_projection_matricies(*P)
        vo.set_track_output(ROWS); vo.set_descriptor_output(True)
        for k in range(2):
            vo.stereo_callback_batch([Ls[k]], [Rs[k]])
        obs, desc = check_frame(vo, 1, 0, ("keep", 1), Ls[1], ROWS)
        assert len(desc) > 100
        dev = [(torch.from_numpy(Ls[k]).cuda(), torch.from_numpy(Rs[k]).cuda()) for k in range(2, 10)]
        torch.cuda.synchronize()
        for l, r in dev:                                             # the eighth of these takes frame 1's slot
            vo.submit_device([l.data_ptr()], [r.data_ptr()], w)
            assert np.array_equal(vo.last_track_descriptors(0), desc) and vo.last_track_obs(0).tobytes() == obs.tobytes()
        for k in range(2, 10):
            vo.collect()
            check_frame(vo, k, 0, ("keep", k), Ls[k], ROWS)
        vo.set_track_output(50)                                      # a new max_rows re-allocates both rings: frame 9's rows survive it
        assert len(vo.last_track_descriptors(0)) == len(vo.last_track_obs(0)) > 50
        check_frame(vo, 9, 0, ("keep", 9), Ls[9], ROWS)
        vo.stereo_callback_batch([Ls[9]], [Rs[9]])
        assert api._lib.PATH_DESCRIPTORS & vo.last_frame_path() and len(vo.last_track_descriptors(0)) == 50
    finally:
        vo.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(api):
    import torch
    L = api._lib
    w, h = SIZES["even"]
    (Ls, Rs), P = tr.stream(3, SEED0, w, h)

    def refused(status, f, *a):
        with pytest.raises(L.SvoError, match="status %d" % status):
            f(*a)

    vo = api.BatchVisualOdometry(w, h, 1, api.default_config(**OVER))
    vo.initalize_projection_matricies(*P)
    refused(L.SVO_ERR_STATE, vo.set_descriptor_output, True)          # the track output is off
    refused(L.SVO_ERR_STATE, vo.last_track_descriptors, 0)            # no frame collected
    vo.set_track_output(100)
    vo.stereo_callback_batch([Ls[0]], [Rs[0]])
    refused(L.SVO_ERR_STATE, vo.last_track_descriptors, 0)            # a frame issued with descriptors off
    dl, dr = torch.from_numpy(Ls[1]).cuda(), torch.from_numpy(Rs[1]).cuda()
    torch.cuda.synchronize()
    vo.submit_device([dl.data_ptr()], [dr.data_ptr()], w)
    refused(L.SVO_ERR_STATE, vo.set_descriptor_output, True)          # switching with a frame in flight
    vo.collect()
    vo.set_descriptor_output(True)
    vo.submit_device([dl.data_ptr()], [dr.data_ptr()], w)
    refused(L.SVO_ERR_STATE, vo.set_descriptor_output, False)
    vo.collect()
    assert len(vo.last_track_descriptors(0)) == len(vo.last_track_obs(0))
    vo.clear_track_output()                                           # switches the descriptors off too
    vo.stereo_callback_batch([Ls[2]], [Rs[2]])
    assert not vo.last_frame_path() & (L.PATH_DESCRIPTORS | L.PATH_TRACK_IDS)
    vo.set_track_output(100)
    vo.stereo_callback_batch([Ls[2]], [Rs[2]])
    assert vo.last_frame_path() & L.PATH_TRACK_IDS and not vo.last_frame_path() & L.PATH_DESCRIPTORS
    vo.close()
    bgr = api.BatchVisualOdometry(w, h, 1, api.default_config(channels=3, **OVER))
    bgr.set_track_output(100)
    refused(L.SVO_ERR_ARG, bgr.set_descriptor_output, True)
    bgr.close()
    one = api.VisualOdometry(cfg=api.default_config(**OVER))           # the lazily created facade takes the setters before its first frame
    with pytest.raises(L.SvoError):
        one.set_descriptor_output(True)                               # the track output first, there too
    one.initalize_projection_matricies(*P)
    one.set_track_output(ROWS); one.set_descriptor_output(True)
    one.stereo_callback(Ls[0], Rs[0]); one.stereo_callback(Ls[1], Rs[1])
    assert one.last_frame_path() & L.PATH_DESCRIPTORS
    check_frame(one, 1, 0, ("one", 1), Ls[1], ROWS)
    one.close()


# ------------------------------------------------------------------------------------------------ off means off
@pytest.mark.parametrize("n_seq", [1, 10])
def test_descriptors_on_change_nothing_else(api, n_seq):
    w, h = SIZES["odd"]
    S = [tr.stream(4, SEED0 + 31 * (i % 3), w, h, (), 0.3) for i in range(n_seq)]
    runs = {}
    for desc_on in (False, True):
        vo = api.BatchVisualOdometry(w, h, n_seq, api.default_config(**OVER))
        vo.initalize_projection_matricies(*S[0][1])
        vo.set_track_output(ROWS)
        if desc_on:
            vo.set_descriptor_output(True)
        per = []
        for k in range(4):
            ok, T = vo.stereo_callback_batch([s[0][0][k] for s in S], [s[0][1][k] for s in S])
            per.append((vo.last_frame_path(), ok.tobytes(), T.tobytes(), [tuple(sorted(s.as_dict().items())) for s in vo.stats],
                        [snap(vo, i) for i in range(n_seq)], [vo.last_track_obs(i).tobytes() for i in range(n_seq)]))
        vo.close()
        runs[desc_on] = per
    for k, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert not a[0] & api._lib.PATH_DESCRIPTORS and b[0] == a[0] | api._lib.PATH_DESCRIPTORS, (k, a[0], b[0])
        assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3], "frame %d: pose / stats" % k
        assert all(same(p, q) for p, q in zip(a[4], b[4])), "frame %d: features / tracks" % k
        assert a[5] == b[5], "frame %d: observation rows" % k
    assert sum(len(x) for x in runs[True][-1][5]) > 64 * 100


# ------------------------------------------------------------------------------------------------ discrimination
def test_same_landmark_is_closer_than_different_landmarks(api):
    """tests/test_descriptor_ref.py's relation on the GPU's own rows, same stream, same frames: the median distance between the
    descriptors of one id in consecutive frames is below the 5th percentile of the distances between different ids of one frame —
    with the reference's own values, since the rows are the reference's bit for bit"""
    (Ls, Rs), P = tr.stream(ref.STREAM["n_frames"], ref.STREAM["seed"], ref.STREAM["w"], ref.STREAM["h"])
    vo = api.BatchVisualOdometry(ref.STREAM["w"], ref.STREAM["h"], 1, api.default_config(**ref.OVER))
    vo.initalize_projection_matricies(*P)
    vo.set_track_output(ROWS); vo.set_descriptor_output(True)
    obs, desc = [], []
    for k in range(ref.STREAM["n_frames"]):
        vo.stereo_callback_batch([Ls[k]], [Rs[k]])
        obs.append(vo.last_track_obs(0)); desc.append(vo.last_track_descriptors(0))
    vo.close()
    same_d, diff_d = ref.discrimination(obs, desc)
    print("same-id pairs %d: median %.1f; different-id pairs %d: 5th percentile %.1f" % (len(same_d), np.median(same_d), len(diff_d), np.percentile(diff_d, 5)))
    assert len(same_d) > 300 and np.median(same_d) < np.percentile(diff_d, 5)
    assert (np.median(same_d), np.percentile(diff_d, 5)) == ref.MEASURED


# ------------------------------------------------------------------------------------------------ the C++ facade
def test_facade_round_trip_from_gxx(tmp_path):
    from test_descriptor_host import build_facade_test
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=4, seed=3, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([seq.n_frames, 160, 320], np.int32).tobytes())
        f.write(np.ascontiguousarray(Pl, np.float32).tobytes()); f.write(np.ascontiguousarray(Pr, np.float32).tobytes())
        for l, r in zip(seq.left, seq.right):
            f.write(l.tobytes()); f.write(r.tobytes())
    out = subprocess.run([build_facade_test(), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "DESCRIPTORS OK" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_descriptors_csv_on_run1(tmp_path):
    """`svo_cli --descriptors` on the committed run1 frames: one `frame,id,64 hex digits` line per observation row, the ids and
    bytes the Python API returns for the same frames"""
    import os
    from test_run1_cli import build_cli
    from stereo_visual_odometry_amd import api, synthetic as syn
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run1_frames_0_7.npz"))
    folder = tmp_path / "run1"
    (folder / "left").mkdir(parents=True); (folder / "right").mkdir()
    for k in range(8):
        for side in ("left", "right"):
            im = d[side][k]
            with open(folder / side / ("frame%06d.pgm" % k), "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0])); f.write(im.tobytes())
    csv = tmp_path / "desc.csv"
    out = subprocess.run([build_cli(), "8", str(folder), "--gray", "1", "--descriptors", str(csv)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "processed 8 frame pairs" in out.stdout, out.stdout + out.stderr
    lines = csv.read_text().splitlines()
    assert lines[0] == "frame,id,descriptor"
    rows = [ln.split(",") for ln in lines[1:]]
    assert all(len(r) == 3 and len(r[2]) == 64 for r in rows)
    vo = api.VisualOdometry(cfg=api.default_config()); vo.initalize_projection_matricies(*syn.projection_matrices(syn.RUN1))
    vo.set_track_output(14080); vo.set_descriptor_output(True)
    for k in range(8):
        vo.stereo_callback(d["left"][k], d["right"][k])
        obs, desc = vo.last_track_obs(), vo.last_track_descriptors()
        mine = [r for r in rows if int(r[0]) == k]
        assert len(mine) == len(obs) == len(desc), k
        assert [int(r[1]) for r in mine] == obs["id"].tolist(), k
        assert [r[2] for r in mine] == [bytes(x).hex() for x in desc], k
        assert np.array_equal(desc, ref.describe(d["left"][k], obs["l1"])[0]), k
    vo.close()
    assert len(rows) > 500
