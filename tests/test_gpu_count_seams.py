"""The per-sequence scan kernels at the end of a frame (k_compact, k_ids_compact, the inlier compaction of pnp_final_body,
k_track_obs) and k_lk_chain's feature loop, at feature counts on their round boundaries: tests/count_seam_cases.py plants the
counts exactly, tests/test_count_seam_cases.py guards on the CPU that they stay there.

After every frame, for every sequence, against the CPU oracle's run of the same stream: ok, every svo_frame_stats field (the LK
work counters included), the feature set (xy bit for bit, ages, strengths), the compacted tracks (all four point lists bit for bit,
world points and inlier flags), the pose within test_gpu_parity's tolerance; with the track output on, headers, ids and whole
64-byte rows byte for byte against IdOracleVO, and svo_get_feature_ids.  An idle sequence reports the idle row and keeps its state.
And from the scene alone, whatever the oracle says: every track starts in a bucket whose patch both right images show, the buckets
are strictly increasing, and there are as many tracks as such buckets.  With frames in flight the synchronising reads wait for the
last frame."""
import os
import pickle

import numpy as np
import pytest

import count_seam_cases as cs
import count_seam_child as child
from gpu_kit import api, f32_bits as bits, raw_bits, run_child, same  # noqa: F401  (the fixture is found by name)
from test_gpu_parity import POSE_TOL_R, POSE_TOL_T, rot_angle
from test_gpu_sequence_lifecycle import check_idle_row

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """The rendered streams and the reference runs are shared by this module's tests and by nobody after them: the process that runs
    the rest of the suite gets the memory back, the device's cached blocks included."""
    yield
    for f in (cs.frames, cs.oracle_run, cs.id_oracle_run):
        f.cache_clear()
    import torch
    torch.cuda.empty_cache()


def snap_of(rec):
    f, t = rec["feats"], rec["tracks"]
    return [raw_bits(f[0]), f[1], f[2]] + [raw_bits(t[k]) for k in ("pl0", "pr0", "pl1", "pr1", "world")] + [t["inlier"]] + ([rec["ids"]] if "ids" in rec else [])


def check_scene(case, i, j, pl0, what):
    """Independent of the oracle: the tracks of image j of sequence i's stream against the scene."""
    s = case.streams[i]
    b = cs.bucket_of(pl0)
    alive = s.allowed(j) if j >= 1 else set()
    assert set(b.tolist()) <= alive, (what, "a track starts in a bucket without a live patch", sorted(set(b.tolist()) - alive)[:8])
    assert (np.diff(b) > 0).all(), (what, "the tracks' buckets are not strictly increasing", np.nonzero(np.diff(b) <= 0)[0][:8])
    assert len(b) == len(alive), (what, "tracks", len(b), "live patches", len(alive))


def check_case(L, case, recs):
    """recs: count_seam_child.run_case's records of `case`."""
    plan, on = case.plan(), case.track_rows is not None
    assert len(recs) == len(plan)
    last_T = [np.eye(4).reshape(16)] * case.B
    prev = [None] * case.B
    for k, (step, row) in enumerate(zip(recs, plan)):
        path = step["path"]
        ahead = case.B > cs.SVO_LONE_MAX_SEQ and case.mode != "graph"     # a captured frame builds nothing ahead (issue_frame)
        assert bool(path & L.PATH_INGEST_AHEAD) == ahead, (case.name, k, "path %#x" % path)
        assert bool(path & L.PATH_TRACK_IDS) == on and (not case.lean or path & L.PATH_LEAN), (case.name, k, "path %#x" % path)
        assert bool(path & L.PATH_GRAPH) == (case.mode == "graph"), (case.name, k, "path %#x" % path)
        for i, j in enumerate(row):
            g, what = step["seqs"][i], (case.name, "call", k, "seq", i, "image", j)
            if j is None:                                             # idle: the idle row, no rows, the state untouched
                check_idle_row((g["ok"], g["T"].reshape(16), g["stats"]), last_T[i])
                assert not on or (g["n_tracks"] == 0 and len(g["obs"]) == 0), what
                if "feats" in g:
                    assert prev[i] is not None and same(snap_of(g), prev[i]), (what, "an idle sequence's state moved")
                continue
            want = cs.oracle_run(case.streams[i])[j]
            assert g["ok"] == want["ok"] and g["stats"] == want["stats"], (what, g["stats"], want["stats"])
            assert np.abs(g["T"][:3, 3] - want["T"][:3, 3]).max() < POSE_TOL_T and rot_angle(g["T"][:3, :3], want["T"][:3, :3]) < POSE_TOL_R, (what, "pose")
            last_T[i] = g["T"].reshape(16)
            fr = want["stats"]["fail_reason"]
            if on:
                ids = cs.id_oracle_run(case.streams[i])[j]
                rows, full = g["obs"], ids["obs"]
                assert g["n_tracks"] == len(full) and len(rows) == min(len(full), case.track_rows), (what, "header", g["n_tracks"], len(rows), len(full))
                assert rows.tobytes() == full[:len(rows)].tobytes(), (what, "rows", [f for f in full.dtype.names if not np.array_equal(rows[f], full[:len(rows)][f])])
                if fr != 1 and len(rows) == len(full):
                    check_scene(case, i, j, rows["l0"], what)
            if "feats" not in g:
                continue
            f, t, wf, wt = g["feats"], g["tracks"], want["feats"], want["tracks"]
            assert np.array_equal(bits(f[0]), bits(wf[0])) and np.array_equal(f[1], wf[1]) and np.array_equal(f[2], wf[2]), (what, "feature set")
            if fr != 1:                                               # a first frame compacts nothing: the tracks are the frame's before
                for key in ("pl0", "pr0", "pl1", "pr1"):
                    assert np.array_equal(bits(t[key]), bits(wt[key])), (what, key)
                if fr in (0, 3, 4):
                    assert np.array_equal(bits(t["world"]), bits(wt["world"])) and np.array_equal(t["inlier"], wt["inlier"]), (what, "world / inlier")
                check_scene(case, i, j, t["pl0"], what)
            if on:
                assert np.array_equal(g["ids"], ids["ids"]), (what, "feature ids")
            prev[i] = snap_of(g)


def run_and_check(api, case, monkeypatch=None):
    assert not os.environ.get("SVO_GRAPH") and not os.environ.get("SVO_FORCE_LEAN") and not case.lean
    if case.mode == "graph":
        monkeypatch.setenv("SVO_GRAPH", "1")
    recs = child.run_case(case)
    if case.mode == "graph":
        monkeypatch.delenv("SVO_GRAPH")
    check_case(api._lib, case, recs)
    return recs


by_name = lambda c: c.name


@pytest.mark.parametrize("case", cs.CASES_A, ids=by_name)
def test_lone_stream_at_the_1024_thread_round(api, case):
    run_and_check(api, case)


def test_nine_sequences_at_the_256_thread_rounds_and_a_ragged_call(api):
    run_and_check(api, cs.CASE_B)


@pytest.mark.parametrize("case", cs.CASES_C1 + [cs.CASE_C9], ids=by_name)
def test_inlier_compaction_at_the_chunk_seam(api, case):
    run_and_check(api, case)


@pytest.mark.parametrize("case", cs.CASES_D, ids=by_name)
def test_lk_grid_hinted_an_order_of_magnitude_too_small(api, case, monkeypatch):
    """An underestimate is only slower: frames 3 and 4 track 1025 features on the grid a hint of 20 gives (sync: frame 3, in flight:
    both; the CPU guard works the schedule out), frame 5 tracks 20 on a grid for 1025; under SVO_GRAPH=1 the grid change re-captures."""
    recs = run_and_check(api, case, monkeypatch)
    j = 0 if case.B == 1 else 4
    assert [r["seqs"][j]["stats"]["n_into_lk"] for r in recs] == [0, 20, 20, 1025, 1025, 20]


@pytest.mark.parametrize("case", cs.CASES_E, ids=by_name)
def test_track_ids_and_rows_at_the_rounds(api, case):
    recs = run_and_check(api, case)
    if case.track_rows == cs.TO_THREADS:                              # max_rows below, at and above a frame's track count
        seen = {(r["seqs"][i]["n_tracks"], len(r["seqs"][i]["obs"])) for r in recs for i in range(case.B)}
        assert {(255, 255), (256, 256), (257, 256)} <= seen, sorted(seen)


def test_lean_builds_at_the_256_thread_seam(api, tmp_path):
    """k_pnp_final_lean (PF_THREADS_LEAN) and k_track_obs_lean: SVO_FORCE_LEAN=1 is read once per process, so a fresh one runs the case."""
    case = cs.CASE_F
    env = dict(os.environ)
    env.pop("SVO_GRAPH", None)
    env["SVO_FORCE_LEAN"] = "1"
    out = str(tmp_path / "recs.pkl")
    r = run_child("count_seam_child.py", case.name, out, cwd=ROOT, env=env, timeout=120)
    assert "count seam child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    with open(out, "rb") as f:
        recs = pickle.load(f)
    check_case(api._lib, case, recs)
    assert {r["seqs"][i]["stats"]["n_after_bounds"] for r in recs[1:] for i in range(case.B)} == {255, 256, 257}
