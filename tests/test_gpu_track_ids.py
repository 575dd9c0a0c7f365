"""Track ids and observation rows on a real GPU (include/svo.h, "Track ids and per-frame stereo observations"): every frame's
headers, ids and whole 64-byte rows — xyz included — bit for bit against IdOracleVO (tests/track_ids_ref.py), svo_get_feature_ids
against the reference's feature ids, poses within 1e-6: lone-stream (1, 3 sequences) and many-sequence (10) launch lists, second
passes, max_features, stale world points, fail_reason 3 and 4, truncation, frames in flight, ragged frames, a reset and an enable
in mid-run, the refusals, and "off means off".  A reference run is computed once per (stream, configuration, schedule) and shared."""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import track_ids_ref as ref
from gpu_kit import api, f32_bits as bits, same, snap, streams as bgr_streams  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

SIZES = {"even": (320, 160), "odd": (323, 163)}       # tests/test_gpu_detect_mask.py's: whole 64 x 16 FAST tiles, and partial ones on every side
OVER = dict(max_translation_norm=2.0)
SEED0 = 900
ROWS = 4096                                           # more than any frame here has tracks


def stream_of(i, n_frames, w, h, movers, blank=()):
    """the stream of sequence i: three distinct ones, reused in turn"""
    return ref.stream(n_frames, SEED0 + 31 * (i % 3), w, h, blank, movers)


@functools.lru_cache(maxsize=None)
def reference(which, n_frames, w, h, movers, blank, cfg_items, schedule, enable_at):
    """One IdOracleVO over stream `which` -> a list of per-frame records (None for an idle frame).  schedule: per frame "run", "idle"
    or "reset" (svo_reset_sequence, then the frame).  enable_at: the frame before which the output is switched on; until then the
    context carries no ids and its next_id does not move."""
    (L, R), P = stream_of(which, n_frames, w, h, movers, blank)
    o = ref.IdOracleVO(orc.default_config(**dict(cfg_items))); o.initalize_projection_matricies(*P)
    out = []
    for k in range(n_frames):
        if k == enable_at:
            o.assign_ids()
        if schedule[k] == "idle":
            out.append(None)
            continue
        if schedule[k] == "reset":
            o.reset()
        keep = o.next_id
        ok, T = o.stereo_callback(L[k], R[k])
        if k < enable_at:
            o.next_id = keep
        out.append(dict(ok=ok, T=T, obs=o.obs(), ids=o.feature_ids().copy(), feats=tuple(a.copy() for a in o.features()), fail=o.fail_reason,
                        next_before=o.next_id_before_detect))
    return out


def check_frame(vo, k, i, rec, ok, T, max_rows, state):
    """frame k, sequence i of the context against its reference record (None: idle)"""
    rows, n_tracks = vo.last_track_obs(i, with_count=True)
    if rec is None:
        assert n_tracks == 0 and len(rows) == 0, "frame %d seq %d: an idle sequence has rows" % (k, i)
        return
    want = rec["obs"]
    assert bool(ok) == rec["ok"], "frame %d seq %d: ok" % (k, i)
    assert np.abs(T - rec["T"]).max() < 1e-6, "frame %d seq %d: pose" % (k, i)
    assert n_tracks == len(want), "frame %d seq %d: n_tracks %d vs %d" % (k, i, n_tracks, len(want))
    assert len(rows) == min(len(want), max_rows), "frame %d seq %d: %d rows" % (k, i, len(rows))
    w = want[:len(rows)]
    if rows.tobytes() != w.tobytes():
        for f in ref.OBS_DTYPE.names:
            assert np.array_equal(rows[f].view(np.uint8), w[f].view(np.uint8)), "frame %d seq %d: field %s differs, first at row %s" % (
                k, i, f, np.nonzero((rows[f] != w[f]).reshape(len(rows), -1).any(1))[0][:5])
    assert rows.tobytes() == w.tobytes(), "frame %d seq %d: rows" % (k, i)
    if state:                                                        # synchronising reads: only where no frame is in flight
        ids = vo.feature_ids(i)
        assert np.array_equal(ids, rec["ids"]), "frame %d seq %d: feature ids" % (k, i)
        f = vo.features(i)
        assert np.array_equal(bits(f[0]), bits(rec["feats"][0])) and np.array_equal(f[1], rec["feats"][1]), "frame %d seq %d: feature set" % (k, i)


def run(api, size, n_seq, n_frames, movers=0.0, blank=(), cfg_over=None, max_rows=ROWS, depth=0, schedules=None, enable_at=0, resets=()):
    """An n_seq-sequence context over n_frames frames against the references.  depth 0: synchronous host frames, everything compared
    after every frame.  depth > 0: device frames, `depth` submitted before each group is collected; every collect must return its own
    frame's rows.  schedules: per sequence a tuple of "run" / "idle" / "reset" per frame.  -> the per-frame reference records."""
    w, h = SIZES[size]
    over = dict(OVER, **(cfg_over or {}))
    cfg_items = tuple(sorted(over.items()))
    schedules = schedules or [("run",) * n_frames] * n_seq
    recs = [reference(i % 3, n_frames, w, h, movers, tuple(blank), cfg_items, tuple(schedules[i]), enable_at) for i in range(n_seq)]
    S = [stream_of(i, n_frames, w, h, movers, blank) for i in range(n_seq)]
    vo = api.BatchVisualOdometry(w, h, n_seq, api.default_config(**over))
    vo.initalize_projection_matricies(*S[0][1])
    paths = []

    def before(k):
        if k == enable_at:
            vo.set_track_output(max_rows)
        for i in range(n_seq):
            if schedules[i][k] == "reset":
                vo.reset_sequence(i)

    def active(k):
        on = [schedules[i][k] != "idle" for i in range(n_seq)]
        return on, (None if all(on) else on)

    if depth == 0:
        for k in range(n_frames):
            before(k)
            on, act = active(k)
            ok, T = vo.stereo_callback_batch([S[i][0][0][k] if on[i] else None for i in range(n_seq)],
                                             [S[i][0][1][k] if on[i] else None for i in range(n_seq)], active=act)
            paths.append(vo.last_frame_path())
            if k >= enable_at:
                for i in range(n_seq):
                    check_frame(vo, k, i, recs[i][k], ok[i], T[i], max_rows, True)
    else:
        import torch
        dev = [[(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in zip(*s[0])] for s in S]
        torch.cuda.synchronize()
        stride = S[0][0][0][0].strides[0]
        k = 0
        while k < n_frames:
            group = list(range(k, min(k + depth, n_frames)))
            for j in group:
                assert j != enable_at or j == group[0], "switching is a setup action: enable before a group's first frame"
                before(j)
                on, act = active(j)
                vo.submit_device([dev[i][j][0].data_ptr() if on[i] else None for i in range(n_seq)],
                                 [dev[i][j][1].data_ptr() if on[i] else None for i in range(n_seq)], stride, active=act)
                paths.append(vo.last_frame_path())
            for j in group:
                ok, T = vo.collect()
                if j >= enable_at:
                    for i in range(n_seq):
                        check_frame(vo, j, i, recs[i][j], ok[i], T[i], max_rows, j == group[-1])
            k += depth
        del dev
    vo.close()
    return recs, paths


def fails(recs, i=0):
    return [r["fail"] if r else None for r in recs[i]]


# ------------------------------------------------------------------------------------------------ the streams on every launch list
@pytest.mark.parametrize("n_seq", [1, 3, 10])
@pytest.mark.parametrize("size", ["odd", "even"])
@pytest.mark.parametrize("movers", [0.0, 0.3], ids=["plain", "movers"])
def test_rows_and_ids_match_the_reference(api, movers, size, n_seq):
    recs, paths = run(api, size, n_seq, 6 if movers == 0 else 5, movers=movers)
    L = api._lib
    assert all(p & L.PATH_TRACK_IDS for p in paths), paths
    assert not any(p & L.PATH_FRONT_FUSED for p in paths), "a lone stream with ids issues the unfused front"
    assert bool(paths[-1] & L.PATH_INGEST_AHEAD) == (n_seq > 8), paths
    last = recs[0][-1]["obs"]
    assert len(last) > 100 and last["age"].max() >= 4, "vacuous stream"
    if movers:
        assert sum(1 for r in recs[0] if r["fail"] == 0 and ((r["obs"]["flags"] & ref.OBS_INLIER) == 0).any()) >= 2, "no non-inlier rows"


@pytest.mark.parametrize("n_seq", [1, 10])
def test_second_pass_every_frame(api, n_seq):
    recs, _ = run(api, "odd", n_seq, 4, cfg_over=dict(pre_matching_feature_threshold=2000))
    assert [len(r["obs"]) for r in recs[0]] == [0, 555, 791, 834], [len(r["obs"]) for r in recs[0]]


def test_max_features_drops_ids_beyond_n_lk(api):
    recs, _ = run(api, "odd", 1, 4, cfg_over=dict(max_features=50))
    assert [len(r["obs"]) for r in recs[0]] == [0, 45, 44, 40] and len(recs[0][3]["ids"]) == 38, [len(r["obs"]) for r in recs[0]]


def test_stale_world_points_are_not_reported(api):
    recs, _ = run(api, "odd", 1, 8, blank=(3,), cfg_over=dict(features_threshold=500))
    r = recs[0]
    assert [len(x["obs"]) for x in r[:7]] == [0, 445, 653, 0, 0, 0, 370] and fails(recs)[1] == 2 and fails(recs)[2] == 0 and fails(recs)[6] == 2
    for k in (1, 6):                                                 # frame 6 follows a frame that triangulated: d.world holds its points
        assert not r[k]["obs"]["xyz"].any() and not (r[k]["obs"]["flags"] & ref.OBS_HAS_XYZ).any()
    assert (r[2]["obs"]["flags"] & ref.OBS_HAS_XYZ).all() and r[2]["obs"]["xyz"].any()


def test_fail_reason_3_rows_without_inlier_flags(api):
    recs, _ = run(api, "odd", 1, 3, movers=0.3, cfg_over=dict(features_threshold=310))
    r = recs[0][1]
    assert r["fail"] == 3 and len(r["obs"]) == 326 and not (r["obs"]["flags"] & ref.OBS_INLIER).any() and (r["obs"]["flags"] & ref.OBS_HAS_XYZ).all()
    assert np.array_equal(r["ids"], r["obs"]["id"]), "the feature set is the compaction's output"


def test_fail_reason_4_rows_with_inlier_flags(api):
    recs, _ = run(api, "odd", 1, 4, movers=0.3, cfg_over=dict(max_translation_norm=0.1))   # the default gate, below the stream's step 0.3
    for r in recs[0][1:]:
        inl = (r["obs"]["flags"] & ref.OBS_INLIER).astype(bool)
        assert r["fail"] == 4 and not r["ok"] and inl.any() and np.array_equal(r["ids"], r["obs"]["id"][inl])
    assert not recs[0][1]["obs"]["flags"][0] & ~3


def test_truncation_keeps_the_first_rows_and_the_full_count(api):
    recs, _ = run(api, "even", 3, 4, max_rows=100)
    assert all(len(r["obs"]) > 100 for r in recs[0][1:])


def test_frames_in_flight_each_collect_returns_its_own_rows(api):
    recs, paths = run(api, "odd", 10, 6, depth=3)
    assert len({len(r["obs"]) for r in recs[0][1:]}) > 1, "the frames cannot be told apart"


def test_ragged_frames_idle_sequence_keeps_its_ids(api):
    sched = [("run",) * 6, ("run", "run", "idle", "idle", "run", "run"), ("run",) * 6]
    recs, _ = run(api, "even", 3, 6, depth=1, schedules=sched)
    a, b = recs[1][1], recs[1][4]
    assert np.isin(b["obs"]["id"], a["ids"]).sum() > 50, "the idle sequence's ids did not continue"


def test_reset_sequence_restarts_its_ids(api):
    sched = [("run",) * 6, ("run", "run", "run", "reset", "run", "run"), ("run",) * 6]
    recs, _ = run(api, "odd", 3, 6, depth=1, schedules=sched)
    assert recs[1][3]["fail"] == 1 and recs[1][4]["obs"]["id"].max() < 1000 and recs[0][4]["obs"]["id"].max() > 1000


@pytest.mark.parametrize("n_seq", [1, 10])
def test_enabling_mid_stream_numbers_the_held_features(api, n_seq):
    recs, _ = run(api, "even", n_seq, 6, enable_at=2)
    r = recs[0][2]
    cont = r["obs"]["id"] < r["next_before"]
    assert r["next_before"] == len(recs[0][1]["feats"][1]) and cont.sum() > 100 and (~cont).sum() > 10


# ------------------------------------------------------------------------------------------------ off means off
def plain_run(api, w, h, S, P, n_seq, cfg, toggle):
    """-> (per-frame (ok, T bytes, stats, snapshots), paths, per-frame feature ids or None).  toggle: "never", "on_off" (enabled and
    disabled before the first frame), "on"."""
    vo = api.BatchVisualOdometry(w, h, n_seq, cfg)
    vo.initalize_projection_matricies(*P)
    if toggle != "never":
        vo.set_track_output(ROWS)
    if toggle == "on_off":
        vo.clear_track_output()
    out, paths, ids = [], [], []
    for k in range(len(S[0][0])):
        ok, T = vo.stereo_callback_batch([s[0][k] for s in S], [s[1][k] for s in S])
        paths.append(vo.last_frame_path())
        out.append((ok.tobytes(), T.tobytes(), [tuple(sorted(s.as_dict().items())) for s in vo.stats], [snap(vo, i) for i in range(n_seq)]))
        if toggle == "on":
            ids.append([vo.feature_ids(i) for i in range(n_seq)])
            for i in range(n_seq):
                rows = vo.last_track_obs(i)
                assert len(np.unique(rows["id"])) == len(rows) and len(np.unique(ids[-1][i])) == len(ids[-1][i]), "frame %d seq %d: ids not unique" % (k, i)
    vo.close()
    return out, paths, ids


def assert_same_runs(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0] and x[1] == y[1] and x[2] == y[2], "%s: frame %d pose / stats" % (what, k)
        assert all(same(p, q) for p, q in zip(x[3], y[3])), "%s: frame %d features / tracks" % (what, k)


@pytest.mark.parametrize("n_seq", [1, 10])
def test_off_means_off_and_on_changes_nothing_else(api, n_seq):
    w, h = SIZES["odd"]
    S = [stream_of(i, 5, w, h, 0.3) for i in range(n_seq)]
    cfg = api.default_config(**OVER)
    runs = {t: plain_run(api, w, h, [s[0] for s in S], S[0][1], n_seq, cfg, t) for t in ("never", "on_off", "on")}
    assert_same_runs(runs["never"][0], runs["on_off"][0], "enabled and disabled")
    assert runs["never"][1] == runs["on_off"][1] and not any(p & api._lib.PATH_TRACK_IDS for p in runs["never"][1])
    assert_same_runs(runs["never"][0], runs["on"][0], "output on")
    assert all(p & api._lib.PATH_TRACK_IDS for p in runs["on"][1])


def test_colour_context_invariance_and_unique_ids(api):
    w, h = SIZES["even"]
    S = bgr_streams(1, 4, SEED0, w, h, cn=3)
    from gpu_kit import projections
    cfg = api.default_config(channels=3, **OVER)
    runs = {t: plain_run(api, w, h, S, projections(w, h), 1, cfg, t) for t in ("never", "on")}
    assert_same_runs(runs["never"][0], runs["on"][0], "channels = 3")
    assert len(runs["on"][2][-1][0]) > 50, "no features"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(api):
    L = api._lib
    w, h = SIZES["even"]
    (Ls, Rs), P = stream_of(0, 3, w, h, 0.0)

    def refused(status, f, *a):
        with pytest.raises(L.SvoError, match="status %d" % status):
            f(*a)

    vo = api.BatchVisualOdometry(w, h, 1, api.default_config(features_per_bucket=2, **OVER))
    refused(L.SVO_ERR_ARG, vo.set_track_output, 100)
    vo.close()
    vo = api.BatchVisualOdometry(w, h, 1, api.default_config(**OVER))
    vo.initalize_projection_matricies(*P)
    refused(L.SVO_ERR_ARG, vo.set_track_output, 0)
    refused(L.SVO_ERR_ARG, vo.set_track_output, 1 << 20)
    refused(L.SVO_ERR_STATE, vo.feature_ids, 0)                       # the getters with the output off
    refused(L.SVO_ERR_STATE, vo.last_track_obs, 0)
    vo.stereo_callback_batch([Ls[0]], [Rs[0]])
    refused(L.SVO_ERR_STATE, vo.last_track_obs, 0)                    # a frame issued with the output off
    import torch
    dl, dr = torch.from_numpy(Ls[1]).cuda(), torch.from_numpy(Rs[1]).cuda()
    torch.cuda.synchronize()
    vo.submit_device([dl.data_ptr()], [dr.data_ptr()], Ls[1].strides[0])
    refused(L.SVO_ERR_STATE, vo.set_track_output, 100)                # switching with a frame in flight
    vo.collect()
    vo.set_track_output(100)
    vo.submit_device([dl.data_ptr()], [dr.data_ptr()], Ls[1].strides[0])
    refused(L.SVO_ERR_STATE, vo.clear_track_output)
    vo.collect()
    vo.close()
    one = api.VisualOdometry(cfg=api.default_config(**OVER))
    one.initalize_projection_matricies(*P)
    one.set_track_output(100)
    one.stereo_callback(Ls[0], Rs[0]); one.stereo_callback(Ls[1], Rs[1])
    pts = one.features()[0]
    assert len(pts) > 10
    refused(L.SVO_ERR_STATE, one.circularMatching, Ls[2], Rs[2], pts, api.FeatureSet())
    one.clear_track_output()
    refused(L.SVO_ERR_STATE, one.feature_ids)
    one.close()
