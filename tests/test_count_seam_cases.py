"""The guard of the case matrix tests/test_gpu_count_seams.py runs (tests/count_seam_cases.py): with the CPU oracle alone, every
case's feature counts sit exactly on the round boundaries it names, the survivors of every frame are exactly the patches the scene
leaves alive, and the few-survivor frames fail the way the case says.  A scene that drifts off its seam fails here, not silently on
the GPU.  No GPU needed."""
import os
import re
import zlib

import numpy as np
import pytest

import count_seam_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_visual_odometry_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_constants_are_the_kernels():
    img, pnp, host, lk, api = src("svo_kernels_img.hip"), src("svo_kernels_pnp.hip"), src("svo_internal.hpp"), src("svo_kernels_lk.hip"), src("svo_api.hip")
    define = lambda text, name: int(re.search(r"^#define %s (\d+)\b" % name, text, re.M).group(1))
    assert define(img, "SCAN_THREADS") == cs.SCAN_THREADS and define(img, "IDC_THREADS") == cs.IDC_THREADS and define(img, "TO_THREADS") == cs.TO_THREADS
    assert define(pnp, "PF_THREADS") == cs.PF_THREADS and define(pnp, "PF_THREADS_LEAN") == cs.PF_THREADS_LEAN
    assert define(host, "SVO_LONE_MAX_SEQ") == cs.SVO_LONE_MAX_SEQ
    m = re.search(r"const int threads = d\.B > SVO_LONE_MAX_SEQ \? (\d+) : SCAN_THREADS;", img)
    assert m and int(m.group(1)) == cs.MANY_COMPACT_THREADS
    assert "const int chunk = (n + THREADS - 1) / THREADS;" in pnp
    # the hint formula, its graph steps and the grid's rounding
    assert "int h = c->lk_hint + c->lk_hint / 3 + 64;" in api and "if (c->use_graph) h = (h + 511) / 512 * 512;" in api
    assert "gx = (gx + 8 * chunk - 1) / (8 * chunk) * (8 * chunk);" in lk
    assert re.search(r'getenv\("SVO_LK_CHUNK"\); v = e \? atoi\(e\) : (\d+);', lk).group(1) == str(cs.LK_CHUNK)
    assert "for (int idx = f; idx < n; idx += slots)" in lk


def test_the_grid_holds_the_counts():
    assert cs.W % cs.BUCKET == 0 and cs.H % cs.BUCKET == 0 and cs.W <= 1000 and cs.H <= 640
    assert len(cs.USABLE) >= cs.SCAN_THREADS + 1 > len(cs.USABLE) - (cs.BAW - 1), "a smaller grid would do"
    assert cs.CAP >= cs.SCAN_THREADS + 1


def test_the_matrix_names_every_seam():
    lone = {c.streams[0].counts()[1] for c in cs.CASES_A}
    assert lone == {cs.SCAN_THREADS - 1, cs.SCAN_THREADS, cs.SCAN_THREADS + 1}
    R = cs.MANY_COMPACT_THREADS
    assert cs.CASE_B.B == cs.SVO_LONE_MAX_SEQ + 1 and set(cs.B_COUNTS) == {R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 1, 1, 64}
    assert len({-(-n // R) for n in cs.B_COUNTS}) == 4, "one, two, three and four rounds in the same launch"
    assert [c.steps[3] for c in (cs.CASE_B,)] == [tuple(i not in (1, 4, 7) for i in range(9))] and cs.CASE_B.steps[4] is None
    assert {p[3] for c in cs.CASES_C1 for p in c.props if p[2] == "n_after_bounds"} == {cs.PF_THREADS - 1, cs.PF_THREADS, cs.PF_THREADS + 1}
    want = {cs.PF_THREADS_LEAN - 1, cs.PF_THREADS_LEAN, cs.PF_THREADS_LEAN + 1}
    for c in (cs.CASE_C9, cs.CASE_F):
        assert c.B == cs.SVO_LONE_MAX_SEQ + 1 and {p[3] for p in c.props if p[2] == "n_after_bounds"} == want
    assert cs.CASE_F.lean and cs.CASE_F.track_rows == cs.TO_THREADS
    assert {(c.B, c.mode) for c in cs.CASES_D} == {(B, m) for B in (1, 9) for m in ("sync", "inflight", "graph")}
    assert all(sum(s == cs.D_JUMP for s in c.streams) == 1 for c in cs.CASES_D)
    assert [c.track_rows for c in cs.CASES_E] == [cs.CAP] * 3 + [cs.TO_THREADS] and all(c.track_rows is None for c in cs.CASES_A + [cs.CASE_B])
    assert [c.name[2:] for c in cs.CASES_E] == [c.name for c in cs.CASES_A + [cs.CASE_B]]


def test_the_frozen_lists_are_the_recorded_ones():
    """The kill lists were fixed against the oracle once; an edit that keeps a count on its seam by luck is still an edit."""
    crc = lambda x: zlib.crc32(repr(x).encode())
    assert crc((cs.THIN_255, cs.THIN_511, cs.THIN_1023, cs.THIN_1024)) == 239576887
    assert crc((cs.C1_PLANTED, cs.C1_MOVERS, sorted(cs.C1_KILLS.items()))) == 3593781592
    assert crc((cs.C9_PLANTED, cs.C9_MOVERS, sorted(cs.C9_KILLS.items()))) == 2607400571
    assert crc((cs.B_COUNTS, sorted(cs.B_KILLS.items()), sorted(cs.B_IDLE.items()), cs.B_SEEDS)) == 2222644626


def test_the_hint_is_an_order_of_magnitude_too_small():
    few, many = 20, 1025
    assert few + few / 3 + 64 < many / 8, "a block really takes at least eight features"
    assert cs.lk_slots(few) == 96 and -(-many // cs.lk_slots(few)) == 11 and many // cs.lk_slots(few) == 10
    assert cs.lk_slots(0) == cs.lk_slots(many) >= many, "the first frames, and the frame after the jump, have a block per feature"
    assert cs.lk_slots(few, graph=True) == 512 != cs.lk_slots(many, graph=True), "the jump crosses a 512 step: the graph is re-captured"
    # what each mode issues the two 1025-feature frames (3 and 4) with: the hint is the last COLLECTED frame's n_after_detect
    nad = [r["stats"]["n_after_detect"] for r in cs.oracle_run(cs.D_JUMP)]
    assert nad == [0, few, few, many, many, few]
    sync = [0, 0] + nad[1:-1]                                         # frame k is issued after frame k - 1 was collected (frame 0 reports 0: no hint)
    flight = [0, 0, 0] + nad[1:-2]                                    # ... after frame k - 2 was collected
    assert (sync[3], sync[4], sync[5]) == (few, many, many) and (flight[3], flight[4], flight[5]) == (few, few, many)


def test_the_scene_is_deterministic_and_a_kill_touches_the_right_image_only():
    a = cs.Stream([300] * 3, seed=5)
    b = cs.Stream([300] * 3, {1: (7, 299)}, seed=5)
    cs.frames.cache_clear()
    La, Ra = cs.frames(a)
    first = [x.copy() for x in La + Ra]
    cs.frames.cache_clear()
    La, Ra = cs.frames(a)
    assert all(np.array_equal(x, y) for x, y in zip(first, La + Ra))
    Lb, Rb = cs.frames(b)
    assert all(np.array_equal(x, y) for x, y in zip(La, Lb)) and np.array_equal(Ra[0], Rb[0]) and np.array_equal(Ra[2], Rb[2])
    diff = np.argwhere(Ra[1] != Rb[1])
    assert set(cs.bucket_of(diff[:, ::-1].astype(np.float32)).tolist()) == {cs.USABLE[7], cs.USABLE[299]}
    assert (Rb[1][Ra[1] != Rb[1]] == cs.BACKGROUND).all()
    assert not La[0].flags.writeable
    for L, R in ((La, Ra),):                                          # every patch stays inside its bucket, off its edges
        for img in L + R:
            ys, xs = np.nonzero(img != cs.BACKGROUND)
            assert (xs % cs.BUCKET).min() >= 0 and (ys % cs.BUCKET).min() >= 3 and (ys % cs.BUCKET).max() <= cs.BUCKET - 4
        for img in L:
            xs = np.nonzero(img != cs.BACKGROUND)[1]
            assert (xs % cs.BUCKET).min() >= 3 and (xs % cs.BUCKET).max() <= cs.BUCKET - 4 and xs.min() >= cs.BUCKET


def holds(stream, run, frame, what, value):
    st, p = run[frame]["stats"], run[frame]["patches"].tolist()
    if what in ("n_into_lk", "n_after_bounds", "n_after_detect", "n_inliers"):
        return st[what] == value
    if what == "fail":
        return st["fail_reason"] == value and run[frame]["ok"] == (value == 0)
    if what == "survivors":
        return p == list(value)
    if what == "none_in":
        return not any(value[0] <= i < value[1] for i in p) and any(i < value[0] for i in p) and any(i >= value[1] for i in p)
    if what == "alone_in_round":
        i, rnd = value
        return i in p and [j for j in p if j // rnd == i // rnd] == [i]
    raise ValueError(what)


@pytest.mark.parametrize("case", cs.CASES, ids=lambda c: c.name)
def test_the_case_sits_on_its_seam(case):
    assert case.props
    for seq, frame, what, value in case.props:
        s = case.streams[seq]
        assert holds(s, cs.oracle_run(s), frame, what, value), (case.name, seq, frame, what, value if np.size(value) < 8 else "...", cs.oracle_run(s)[frame]["stats"])
    for i, s in enumerate(case.streams):
        run = cs.oracle_run(s)
        assert run[0]["stats"]["fail_reason"] == 1
        for k in range(1, len(run)):
            r, st = run[k], run[k]["stats"]
            p = r["patches"]
            assert st["n_after_detect"] == st["n_into_lk"] == len(s.planted[k - 1]), (case.name, i, k, st)
            assert (p >= 0).all() and (np.diff(p) > 0).all(), (case.name, i, k, "the survivors' bucket indices are strictly increasing")
            alive = sorted(s.planted[k - 1].index(b) for b in s.allowed(k))
            assert p.tolist() == alive, (case.name, i, k, "the survivors are the patches both right images show")
            assert st["n_after_bounds"] == st["n_after_circular"] == len(alive)
            assert st["fail_reason"] == (0 if len(alive) > cs.MIN_TRACKS else 2), (case.name, i, k, st)
            if st["fail_reason"] == 0:                               # PnP and the inlier rewrite really run: the movers, and only they, are outliers
                movers = np.array([s.planted[k - 1][j] in s.movers for j in p])
                assert np.array_equal(r["tracks"]["inlier"].astype(bool), ~movers), (case.name, i, k)
                assert st["n_inliers"] == int((~movers).sum()) == len(r["feats"][1])
    if case.track_rows is not None:                                   # E, F: the id reference runs the same frames, and some frame is truncated where the case says so
        for s in case.streams:
            for a, b in zip(cs.id_oracle_run(s), cs.oracle_run(s)):
                assert all(np.array_equal(x, y) for x, y in zip(a["feats"], b["feats"])) and len(a["obs"]) == len(b["tracks"]["pl0"])
                assert len(a["ids"]) == len(a["feats"][1]) and len(np.unique(a["obs"]["id"])) == len(a["obs"])
        counts = {len(r["obs"]) for s in case.streams for r in cs.id_oracle_run(s)}
        if case.track_rows == cs.TO_THREADS:
            assert {cs.TO_THREADS - 1, cs.TO_THREADS, cs.TO_THREADS + 1} <= counts, (case.name, "max_rows against one track fewer, as many, one more")
        else:
            assert max(counts) < case.track_rows


def test_the_ragged_call_follows_a_kill_frame_and_everyone_returns():
    plan = cs.CASE_B.plan()
    assert [row[4] for row in plan] == [0, 1, 2, None, 3] and [row[0] for row in plan] == [0, 1, 2, 3, 4]
    assert cs.CASE_B.streams[8].counts() == [64, 64, 65, 64, 64] and plan[4][8] == 4, "frame 4 tracks fewer features than frame 3 did"
    assert sum(x is None for x in plan[3]) == 3 and all(x is not None for k in (0, 1, 2, 4) for x in plan[k])
