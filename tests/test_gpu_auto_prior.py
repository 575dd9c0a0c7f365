"""SVO_PRIOR_LAST_ROTATION (include/svo.h, "Predicted priors") on the GPU: the prior k_prior_predict makes from a sequence's last pose
is held, bit for bit, to the host restatement the header gives — a context in the default mode whose caller collects every frame and
hands the transposed rotation of the returned transform back through svo_motion_prior_from_rotation and svo_set_motion_prior.

All GPU work runs once, in a child process (tests/auto_prior_child.py: the scene, shapes and record layout of the motion-prior tests);
the tests below compare its runs with each other.  Every run but "none" bootstraps frame 1 with the ground-truth rotation prior —
without one the scene's 7.7 degree turn loses frame 1 (tests/test_gpu_motion_prior.py) and there is no pose to predict from.

 1. auto = host, every record field of every frame and sequence, and the 18 floats the getter reports.
 2. Frame 2 fails for lack of tracks without the predicted prior and gives a pose with it (tests/test_auto_prior_host.py pins the
    same gap on the CPU, for every shape used here).
 3. With frames 1 and 2 both in flight the records are those of the one-call-per-frame run.
 4. A failed frame seeds nothing.  5. An explicit prior wins.  6. An idle frame and a reset.  7. Switching the mode off.  8. Errors."""
import numpy as np
import pytest

import oracle_lib as orc
import lk_prior_cases as pc
import auto_prior_child as child
from gpu_kit import run_child
from test_gpu_motion_prior import records_equal, STAT_NAMES

pytestmark = pytest.mark.gpu

PATH_MOTION_PRIOR, PATH_PRIOR_PREDICTED = 2048, 4096
BOTH = PATH_MOTION_PRIOR | PATH_PRIOR_PREDICTED
MANY = child.B_MANY
# the shapes at which the CPU reference alone shows the gap of test 2 (tests/test_auto_prior_host.py: tracks kept on frame pair
# (1, 2) without a prior / with frame pair (0, 1)'s rotation / with the true one, features_threshold = 15):
#   320 x 240, w = 21:   3 / 371 / 371 of  652        160 x 120, w = 7:   0 / 48 / 48 of 155        640 x 192, w = 21:   7 / 704 / 704 of 1045
GAP_CASES = [(320, 240, 21), (160, 120, 7), (640, 192, 21)]


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("auto_prior") / "gpu.npz")
    r = run_child("auto_prior_child.py", out)
    assert "auto prior child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out))


def stats_of(gpu, key):
    return dict(zip(STAT_NAMES, (int(v) for v in gpu[key + "/stats"])))


def source(gpu, key):
    return int(gpu[key + "/source"][0])


def run_key(w, h, n_seq, mode):
    return "f/%dx%d/%d/%s" % (w, h, n_seq, mode)


# ------------------------------------------------------------------------------------------------ 1. the host restatement
@pytest.mark.parametrize("n_seq", [1, MANY])
@pytest.mark.parametrize("w,h,win", pc.FRAME_CASES)
def test_predicted_prior_is_the_host_restatement_in_bits(gpu, w, h, win, n_seq):
    a, b = run_key(w, h, n_seq, "auto"), run_key(w, h, n_seq, "host")
    for k in range(pc.N_FRAMES):
        for i in range(n_seq):
            assert records_equal(gpu, "%s/%d/%d" % (a, k, i), "%s/%d/%d" % (b, k, i)) == [], (k, i)
    for i in range(n_seq):
        assert gpu["%s/1/%d/ok" % (a, i)][0] == 1                                       # frame 1 gave the pose frame 2 predicts from
        assert source(gpu, "%s/0/%d" % (a, i)) == 0 and source(gpu, "%s/1/%d" % (a, i)) == 1 and source(gpu, "%s/2/%d" % (a, i)) == 2
        assert not gpu["%s/2/%d/pending" % (a, i)].any()                                # nothing came from the host
        want = gpu["%s/2/%d/pending" % (b, i)]                                           # svo_get_motion_prior before B's submit
        assert want.any() and np.array_equal(gpu["%s/2/%d/used" % (a, i)], want), (i, gpu["%s/2/%d/used" % (a, i)].view(np.float32), want.view(np.float32))
        # the getter reports explicit priors too, with the setter's bits
        assert np.array_equal(gpu["%s/1/%d/used" % (a, i)], gpu["%s/1/%d/pending" % (a, i)])
        assert [source(gpu, "%s/%d/%d" % (b, k, i)) for k in range(3)] == [0, 1, 1]
        assert np.array_equal(gpu["%s/2/%d/used" % (b, i)], want)
    assert all(int(v) & BOTH == BOTH for v in gpu[a + "/paths"]), gpu[a + "/paths"]      # every frame of the mode, the first included
    assert [int(v) & BOTH for v in gpu[b + "/paths"]] == [0, PATH_MOTION_PRIOR, PATH_MOTION_PRIOR]
    assert gpu[a + "/mode"][0] == 1 and gpu[b + "/mode"][0] == 0


# ------------------------------------------------------------------------------------------------ 2. what the feature buys
@pytest.mark.parametrize("n_seq", [1, MANY])
@pytest.mark.parametrize("w,h,win", GAP_CASES)
def test_the_predicted_prior_saves_frame_two(gpu, w, h, win, n_seq):
    """CPU reference, tracks kept on frame pair (1, 2) without / with the stale / with the true rotation: 3 / 371 / 371 of 652 at
    320 x 240 (w = 21), 0 / 48 / 48 of 155 at 160 x 120 (w = 7), 7 / 704 / 704 of 1045 at 640 x 192 (w = 21)."""
    cfg = orc.default_config(**pc.over(win))
    a, c = run_key(w, h, n_seq, "auto"), run_key(w, h, n_seq, "plain")
    for i in range(n_seq):
        sa, sc = stats_of(gpu, "%s/2/%d" % (a, i)), stats_of(gpu, "%s/2/%d" % (c, i))
        if i == 0:
            print(w, h, win, n_seq, "auto:", sa, "plain:", sc)
        assert records_equal(gpu, "%s/1/%d" % (a, i), "%s/1/%d" % (c, i)) == []       # the same state before frame 2
        assert sc["fail_reason"] == 2 and gpu["%s/2/%d/ok" % (c, i)][0] == 0, sc
        assert sa["fail_reason"] == 0 and gpu["%s/2/%d/ok" % (a, i)][0] == 1, sa
        assert sa["n_after_bounds"] >= cfg.features_threshold and sa["n_into_lk"] == sc["n_into_lk"], (sa, sc)
        assert source(gpu, "%s/2/%d" % (c, i)) == 0


# ------------------------------------------------------------------------------------------------ 3. frames in flight
@pytest.mark.parametrize("n_seq", [1, MANY])
def test_frames_in_flight(gpu, n_seq):
    w, h, win = pc.FRAME_CASES[0]
    a, f = run_key(w, h, n_seq, "auto"), "o/flight/%d" % n_seq
    for i in range(n_seq):
        for k in (1, 2):
            assert np.array_equal(gpu["%s/%d/%d/stats" % (f, k, i)], gpu["%s/%d/%d/stats" % (a, k, i)]), (k, i)
            assert gpu["%s/%d/%d/T" % (f, k, i)].tobytes() == gpu["%s/%d/%d/T" % (a, k, i)].tobytes(), (k, i)
            assert source(gpu, "%s/%d/%d" % (f, k, i)) == k
            assert np.array_equal(gpu["%s/%d/%d/used" % (f, k, i)], gpu["%s/%d/%d/used" % (a, k, i)])
        assert records_equal(gpu, "%s/2/%d" % (f, i), "%s/2/%d" % (a, i)) == [], i
        assert stats_of(gpu, "%s/2/%d" % (f, i))["fail_reason"] == 0
    assert all(int(v) & BOTH == BOTH for v in gpu[f + "/paths"])


# ------------------------------------------------------------------------------------------------ 4., 5. seeding and precedence
def test_a_failed_frame_does_not_seed_and_an_explicit_prior_wins(gpu):
    w, h, win = pc.FRAME_CASES[0]
    s, a, none, plain = (run_key(w, h, MANY, m) for m in ("seed", "auto", "none", "plain"))
    x, e = child.FAILS, child.EXPLICIT
    # the sequence without a prior at frame 1 fails there, and its frame 2 is the no-prior context's in every bit
    assert stats_of(gpu, "%s/1/%d" % (s, x))["fail_reason"] == 2 and source(gpu, "%s/1/%d" % (s, x)) == 0
    assert source(gpu, "%s/2/%d" % (s, x)) == 0
    for k in range(pc.N_FRAMES):
        assert records_equal(gpu, "%s/%d/%d" % (s, k, x), "%s/%d/%d" % (none, k, x)) == [], k
    # the explicit identity is used as given: source 1, its bits, and the frame of a sequence without a prior from the same state
    assert source(gpu, "%s/2/%d" % (s, e)) == 1
    eye = np.eye(3, dtype=np.float32).reshape(9).view(np.uint32)
    assert np.array_equal(gpu["%s/2/%d/used" % (s, e)], np.stack([eye, eye]))
    assert records_equal(gpu, "%s/1/%d" % (s, e), "%s/1/%d" % (plain, e)) == []
    assert records_equal(gpu, "%s/2/%d" % (s, e), "%s/2/%d" % (plain, e)) == []
    assert stats_of(gpu, "%s/2/%d" % (s, e))["fail_reason"] == 2
    # everyone else predicts, as in the all-auto context
    for i in range(MANY):
        if i in (x, e):
            continue
        assert source(gpu, "%s/2/%d" % (s, i)) == 2
        assert np.array_equal(gpu["%s/2/%d/used" % (s, i)], gpu["%s/2/%d/used" % (a, i)])
        for k in range(pc.N_FRAMES):
            assert records_equal(gpu, "%s/%d/%d" % (s, k, i), "%s/%d/%d" % (a, k, i)) == [], (k, i)


# ------------------------------------------------------------------------------------------------ 6. idle frames and a reset
def test_idle_frame_and_reset(gpu):
    w, h, win = pc.FRAME_CASES[0]
    a, o, x = run_key(w, h, MANY, "auto"), "o/idle", child.IDLE
    # first submit of frame 2: everyone but x.  x reports the row of a frame it did not take and no prior
    assert stats_of(gpu, "%s/first/%d" % (o, x))["fail_reason"] == 5 and source(gpu, "%s/first/%d" % (o, x)) == 0
    for i in range(MANY):
        if i != x:
            assert records_equal(gpu, "%s/first/%d" % (o, i), "%s/2/%d" % (a, i)) == [], i
            assert source(gpu, "%s/first/%d" % (o, i)) == 2
    # second submit: x alone, from the state its last taken frame left
    assert records_equal(gpu, "%s/second/%d" % (o, x), "%s/2/%d" % (a, x)) == []
    assert source(gpu, "%s/second/%d" % (o, x)) == 2
    assert np.array_equal(gpu["%s/second/%d/used" % (o, x)], gpu["%s/2/%d/used" % (a, x)])
    assert all(source(gpu, "%s/second/%d" % (o, i)) == 0 for i in range(MANY) if i != x)
    # a frame nobody takes launches nothing and reports nothing
    assert all(source(gpu, "%s/nobody/%d" % (o, i)) == 0 for i in range(MANY))
    paths = [int(v) for v in gpu[o + "/paths"]]
    assert [p & BOTH for p in paths] == [BOTH, BOTH, 0, BOTH, BOTH] and paths[2] == 0, paths
    # after the reset: frame 0 again, then the first tracked frame — no predicted prior, and without one the turn loses it
    st = dict(zip(STAT_NAMES, (int(v) for v in gpu[o + "/reset0/stats"])))
    assert st["fail_reason"] == 1 and source(gpu, "%s/reset0/%d" % (o, x)) == 0
    st = dict(zip(STAT_NAMES, (int(v) for v in gpu[o + "/reset1/stats"])))
    assert source(gpu, "%s/reset1/%d" % (o, x)) == 0 and st["n_into_lk"] > 0 and st["fail_reason"] == 2, st


# ------------------------------------------------------------------------------------------------ 7. off again, and never on
@pytest.mark.parametrize("n_seq", [1, MANY])
def test_switching_the_mode_off_restores_the_plain_frames(gpu, n_seq):
    w, h, win = pc.FRAME_CASES[0]
    off, plain, none, a = (run_key(w, h, n_seq, m) for m in ("off", "plain", "none", "auto"))
    assert [int(v) & BOTH for v in gpu[off + "/paths"]] == [BOTH, BOTH, 0] and gpu[off + "/mode"][0] == 0
    for k in range(pc.N_FRAMES):
        for i in range(n_seq):
            assert records_equal(gpu, "%s/%d/%d" % (off, k, i), "%s/%d/%d" % (plain, k, i)) == [], (k, i)
    assert all(source(gpu, "%s/2/%d" % (off, i)) == 0 for i in range(n_seq))
    # a context that never set the mode: no prior bit without a prior, the explicit one's alone with one, and every other bit of the
    # frame's path is what the mode's frames report too — the mode adds its two bits to a frame and changes none
    assert [int(v) & BOTH for v in gpu[none + "/paths"]] == [0, 0, 0]
    assert [int(v) & BOTH for v in gpu[plain + "/paths"]] == [0, PATH_MOTION_PRIOR, 0]
    assert [int(v) & ~BOTH for v in gpu[a + "/paths"]] == [int(v) for v in gpu[none + "/paths"]]
    assert int(gpu[off + "/paths"][2]) == int(gpu[none + "/paths"][2])


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors(gpu):
    code = lambda k: int(gpu["o/code/" + k][0])
    ERR_ARG, ERR_STATE = -1, -4
    for k in ("bgr", "float_sums", "unknown_mode", "negative_mode", "getter_seq_range", "getter_null_source"):
        assert code(k) == ERR_ARG, (k, code(k))
    assert code("mode_after_errors") == 0
    assert code("getter_before_collect") == ERR_STATE
    assert code("getter_without_buffers") == 0 and code("source_without_buffers") == 0
    assert code("set_on") == 0 and code("set_off") == 0
