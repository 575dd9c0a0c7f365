"""The motion prior (include/svo.h, "Motion prior") on the GPU, bit for bit against the numpy reference tests/lk_prior_ref.py — which
tests/test_lk_prior_ref.py pins to the oracle wherever a guess must not matter.

All GPU work runs once, in a child process (tests/motion_prior_child.py) that writes what the stage calls and the frame runs returned;
the tests below compute the reference for the same inputs (tests/lk_prior_cases.py) and compare.

 1. svo_lk_track_guess: next points and statuses for w = 5 .. 31, guesses from the rotation homography and adversarial ones.
 2. svo_circular_match_prior: all four point lists and ok, for the rotation homography and for one whose denominator is <= 0 on a part
    of the image (the fallback); H = I gives svo_circular_match's bits.
 3. The frame pipeline, lone stream and nine sequences (derivative planes, batch front): frame 1 completely, every later frame per
    survivor, the same frames without a prior (fail_reason 2 at frame 1: the prior is what saves the frame), a mixed batch, H = I,
    the one-shot scope with frames in flight / an idle frame / a reset, and the errors."""
import os

import numpy as np
import pytest

import oracle_lib as orc
import lk_prior_cases as pc
import lk_prior_ref as ref
import motion_prior_child as child
from gpu_kit import run_child

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6                                  # metres / radians, as tests/test_gpu_parity.py
STAT_NAMES = sorted(f[0] for f in orc.OrcFrameStats._fields_)
PATH_MOTION_PRIOR = 2048


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("motion_prior") / "gpu.npz")
    r = run_child("motion_prior_child.py", out)
    assert "motion prior child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what):
    want = bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1))
    assert bad.size == 0, (what, bad[:10], got[bad[:3]].view(np.float32), want[bad[:3]].view(np.float32))


def stats_of(gpu, key):
    return dict(zip(STAT_NAMES, (int(v) for v in gpu[key + "/stats"])))


# ------------------------------------------------------------------------------------------------ 1. the single pass with a guess
@pytest.mark.parametrize("w,h,win", pc.STAGE_CASES)
def test_lk_track_guess(gpu, w, h, win):
    P, G, kind = pc.track_case(w, h, win)
    A, B = pc.levels(w, h, win, 0, 0), pc.levels(w, h, win, 1, 0)
    r = ref.track(A, B, P, pc.MAX_LEVEL, init=G)
    key = "s/%dx%d/%d" % (w, h, win)
    assert np.array_equal(gpu[key + "/guess/status"], r["status"]), np.flatnonzero(gpu[key + "/guess/status"] != r["status"])
    same_bits(gpu[key + "/guess/next"], r["next"], key)
    # the cases are what they claim to be
    assert 0 < r["status"][kind == 0].sum() and r["steps"][kind == 0].sum() > 1000
    top = 1 << pc.MAX_LEVEL
    far = kind == 2
    assert ((G[far, 0] < -top * win) | (G[far, 1] > h + top * win)).all() and not r["status"][far].any()
    assert np.array_equal(G[kind == 3].view(np.uint32), P[kind == 3].view(np.uint32))
    assert (((G[kind == 4, 0] < 0) | (G[kind == 4, 0] > w - 1)) & (P[kind == 4, 0] >= 0) & (P[kind == 4, 0] <= w - 1)).all()
    # a guess equal to the point is the call without a guess
    assert np.array_equal(gpu[key + "/same/next"], gpu[key + "/plain/next"]) and np.array_equal(gpu[key + "/same/status"], gpu[key + "/plain/status"])
    sel = (kind == 1) | (kind == 3)
    assert np.array_equal(gpu[key + "/guess/next"][sel], gpu[key + "/plain/next"][sel])


# ------------------------------------------------------------------------------------------------ 2. circular matching with a prior
@pytest.mark.parametrize("w,h,win", pc.STAGE_CASES)
def test_circular_match_prior(gpu, w, h, win):
    cfg = orc.default_config(**pc.over(win))
    pts = pc.fast_points(w, h, pc.N_CIRC)
    key = "s/%dx%d/%d" % (w, h, win)
    for j, (k0, k1, H, Hi) in enumerate(pc.circular_cases(w, h)):
        c = ref.circular(pc.levels4(w, h, win, k0, k1), pts, H, Hi, cfg)
        if j == 1:                               # the partial homography: the fallback is taken by some points, not by all
            assert 0 < (~c["used"][0]).sum() < len(pts), c["used"].sum(1)
            assert c["ok"].sum() > 0
        else:
            assert c["used"].all()
        for name in ("pl1", "pr1", "pr0", "plc"):
            same_bits(gpu["%s/circ%d/%s" % (key, j, name)], c[name], (key, j, name))
        assert np.array_equal(gpu["%s/circ%d/ok" % (key, j)], c["ok"]), (key, j, np.flatnonzero(gpu["%s/circ%d/ok" % (key, j)] != c["ok"]))
    for name in ("pl1", "pr1", "pr0", "plc", "ok"):
        assert np.array_equal(gpu[key + "/identity/" + name], gpu[key + "/noprior/" + name]), (key, name)


# ------------------------------------------------------------------------------------------------ 3. the frame pipeline
def frame_reference(w, h, win, k, pts, prior_bits):
    """lk_prior_ref.circular on the frame pair (k - 1, k) with the H, Hi the frame used (svo_get_motion_prior's bits)"""
    H, Hi = prior_bits.view(np.float32).reshape(2, 3, 3)
    return pc.circular_cached(w, h, win, k, pts, H, Hi, orc.default_config(**pc.over(win)))


@pytest.mark.parametrize("n_seq", [1, child.B_MANY])
@pytest.mark.parametrize("w,h,win", pc.FRAME_CASES)
def test_frame_one_completely(gpu, w, h, win, n_seq):
    cfg = orc.default_config(**pc.over(win))
    key = "f/%dx%d/%d/prior" % (w, h, n_seq)
    pts = gpu["append/%dx%d/%d" % (w, h, win)].view(np.float32)
    same_bits(bits(pts), pc.lk_input(pc.scene(w, h).left[0], cfg), "the LK input")
    prior = gpu[key + "/1/prior"]
    Hm, _ = pc.homography(w, h, 1)
    assert np.abs(prior[0].view(np.float32) - Hm.reshape(9)).max() <= 1e-6 * np.abs(Hm).max()       # svo_motion_prior_from_rotation
    assert np.abs(prior[1].view(np.float32) - pc.homography(w, h, 1)[1].reshape(9)).max() <= 1e-6 * np.abs(Hm).max()
    c = frame_reference(w, h, win, 1, pts, prior)
    keep = c["ok"].astype(bool) & c["inb"]
    Pl, Pr = pc.projections(w, h)
    world, _ = orc.triangulate(Pl, Pr, pts[keep], c["pr0"][keep])
    ok, R, t, inl, _ = orc.camera_to_world(Pl.reshape(3, 4)[:, :3], c["pl1"][keep], world, np.eye(3), np.zeros(3), cfg.ransac_iterations,
                                           cfg.ransac_reprojection_error, cfg.ransac_confidence)
    T = orc.inverse_transform(R, t)
    for i in (0, n_seq - 1):
        p = "%s/1/%d" % (key, i)
        st = stats_of(gpu, p)
        print(p, st)
        assert st["n_into_lk"] == len(pts)
        assert (st["n_after_circular"], st["n_after_bounds"]) == (int(c["ok"].sum()), int(keep.sum())), (st, int(c["ok"].sum()), int(keep.sum()))
        for name, want in (("pl0", pts[keep]), ("pr0", c["pr0"][keep]), ("pl1", c["pl1"][keep]), ("pr1", c["pr1"][keep]), ("world", world)):
            same_bits(gpu[p + "/" + name], want, (p, name))
        assert ok and st["fail_reason"] == 0 and gpu[p + "/ok"][0] == 1, (ok, st)
        assert st["n_inliers"] == len(inl)
        assert np.abs(gpu[p + "/T"].reshape(4, 4) - T).max() < POSE_TOL, np.abs(gpu[p + "/T"].reshape(4, 4) - T).max()
    assert all(int(v) & PATH_MOTION_PRIOR for v in gpu[key + "/paths"][1:])
    assert np.array_equal(gpu[key + "/pending"][1:, 0], np.ones((2, n_seq), np.int64)) and not gpu[key + "/pending"][:, 1].any()


@pytest.mark.parametrize("n_seq", [1, child.B_MANY])
@pytest.mark.parametrize("w,h,win", pc.FRAME_CASES)
def test_later_frames_per_survivor(gpu, w, h, win, n_seq):
    key = "f/%dx%d/%d/prior" % (w, h, n_seq)
    for k in range(2, pc.N_FRAMES):
        for i in (0, n_seq - 1):
            p = "%s/%d/%d" % (key, k, i)
            st = stats_of(gpu, p)
            pl0 = gpu[p + "/pl0"].view(np.float32)
            assert st["n_after_circular"] <= st["n_into_lk"] and len(pl0) == st["n_after_bounds"] > 0, st
            c = frame_reference(w, h, win, k, pl0, gpu["%s/%d/prior" % (key, k)])
            assert c["ok"].all() and c["inb"].all(), (p, np.flatnonzero(c["ok"] == 0), np.flatnonzero(~c["inb"]))
            for name in ("pl1", "pr1", "pr0"):
                same_bits(gpu[p + "/" + name], c[name], (p, name))


@pytest.mark.parametrize("n_seq", [1, child.B_MANY])
@pytest.mark.parametrize("w,h,win", pc.FRAME_CASES)
def test_without_a_prior_the_turn_loses_the_frame(gpu, w, h, win, n_seq):
    key = "f/%dx%d/%d/none" % (w, h, n_seq)
    for i in range(n_seq):
        assert stats_of(gpu, "%s/1/%d" % (key, i))["fail_reason"] == 2, (i, stats_of(gpu, "%s/1/%d" % (key, i)))
        assert stats_of(gpu, "f/%dx%d/%d/prior/1/%d" % (w, h, n_seq, i))["fail_reason"] == 0
    assert not any(int(v) & PATH_MOTION_PRIOR for v in gpu[key + "/paths"])
    assert not gpu[key + "/pending"].any()


def records_equal(gpu, a, b):
    names = ("ok", "T", "stats", "xy", "age", "strength", "inlier", "pl0", "pr0", "pl1", "pr1", "world")
    return [n for n in names if not (gpu[a + "/" + n].shape == gpu[b + "/" + n].shape and gpu[a + "/" + n].tobytes() == gpu[b + "/" + n].tobytes())]


@pytest.mark.parametrize("n_seq", [1, child.B_MANY])
@pytest.mark.parametrize("w,h,win", pc.FRAME_CASES)
def test_identity_prior_is_no_prior_in_bits(gpu, w, h, win, n_seq):
    a, b = "f/%dx%d/%d/identity" % (w, h, n_seq), "f/%dx%d/%d/none" % (w, h, n_seq)
    for k in range(pc.N_FRAMES):
        for i in range(n_seq):
            assert records_equal(gpu, "%s/%d/%d" % (a, k, i), "%s/%d/%d" % (b, k, i)) == [], (k, i)
    assert all(int(v) & PATH_MOTION_PRIOR for v in gpu[a + "/paths"][1:])                 # the prior kernel did run


def test_mixed_batch(gpu):
    w, h, win = pc.FRAME_CASES[0]
    n = child.B_MANY
    m, none, prior = ("f/%dx%d/%d/%s" % (w, h, n, mode) for mode in ("mixed", "none", "prior"))
    paths = gpu[m + "/paths"]
    assert int(paths[1]) & PATH_MOTION_PRIOR and not int(paths[2]) & PATH_MOTION_PRIOR and not int(paths[0]) & PATH_MOTION_PRIOR, paths
    assert np.array_equal(gpu[m + "/pending"][1, 0], np.array([i in child.MIXED for i in range(n)], np.int64)) and not gpu[m + "/pending"][:, 1].any()
    for i in range(n):
        if i in child.MIXED:                     # frame 1 is the all-prior context's
            assert records_equal(gpu, "%s/1/%d" % (m, i), "%s/1/%d" % (prior, i)) == [], i
            assert stats_of(gpu, "%s/1/%d" % (m, i))["fail_reason"] == 0
        else:                                    # never touched by a prior: the no-prior context's bits, in the mixed launch and in the frame after it
            for k in range(pc.N_FRAMES):
                assert records_equal(gpu, "%s/%d/%d" % (m, k, i), "%s/%d/%d" % (none, k, i)) == [], (k, i)


def test_one_shot_with_frames_in_flight(gpu):
    """submit, submit, set, submit, collect x 3: the prior reaches the third frame only"""
    assert gpu["o/flight/pending"].tolist() == [1, 0]
    assert [bool(int(v) & PATH_MOTION_PRIOR) for v in gpu["o/flight/paths"]] == [False, False, True]
    for k in range(3):
        assert np.array_equal(gpu["o/flight/%d/stats" % k], gpu["o/sync/%d/stats" % k]) and gpu["o/flight/%d/T" % k].tobytes() == gpu["o/sync/%d/T" % k].tobytes(), k
    assert records_equal(gpu, "o/flight/2/0", "o/sync/2/0") == []
    w, h, win = pc.FRAME_CASES[0]
    assert np.array_equal(gpu["o/flight/1/stats"], gpu["f/%dx%d/1/none/1/0/stats" % (w, h)])       # frame 1 saw no prior
    assert stats_of(gpu, "o/flight/1")["fail_reason"] == 2


def test_idle_frame_and_reset(gpu):
    w, h, win = pc.FRAME_CASES[0]
    # [set for sequence 1] -> [sequence 1 idle] -> [sequence 1 takes the frame] -> [set for all] -> [reset 0] -> [clear 1]
    assert gpu["o/idle/pending"].tolist() == [[0, 1], [0, 1], [0, 0], [1, 1], [0, 1], [0, 0]]
    assert [bool(int(v) & PATH_MOTION_PRIOR) for v in gpu["o/idle/paths"]] == [False, True]
    assert records_equal(gpu, "o/idle/1", "f/%dx%d/1/prior/1/0" % (w, h)) == []                    # sequence 1's frame 1 is the lone stream's with the prior
    assert stats_of(gpu, "o/idle/0")["fail_reason"] == 5


def test_errors(gpu):
    code = lambda k: int(gpu["o/code/" + k][0])
    ERR_ARG, ERR_STATE = -1, -4
    for k in ("bgr", "float_sums", "singular", "non_finite", "non_finite_inverse", "seq_range"):
        assert code(k) == ERR_ARG, (k, code(k))
    assert code("singular_with_inverse") == 0 and code("pending_after_errors") == 0
    assert code("member_with_pending") == ERR_STATE and code("member_after_clear") == 0
