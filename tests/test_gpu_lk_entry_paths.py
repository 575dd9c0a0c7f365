"""What the LK kernels do before their first pass and between features, held to the oracle: the host-computed termination criteria
(LkCrit: lk_max_count = 0, lk_epsilon = 0 -> the exact f64 path of the convergence screen), the scalar feature index, the
wave-per-feature loop over `slots` (feature counts 1, 63, 64, 65 and one above the slot count, so that a block takes a second
feature), at windows 5, 10, 15, 21, 31 and 21 x 21 BGR.  Three entry points: the stage call svo_circular_match, the member call
svo_circular_matching (all four passes of every point, raw points out) and the frame pipeline (early-out build, masks and work
counters in svo_frame_stats).  Points, masks and counters must be EQUAL."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
from gpu_kit import api, calib, f32_bits as bits  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

W, H = 480, 200
WINS = [5, 10, 15, 21, 31]
COUNTS = [1, 63, 64, 65]
LK_SLOTS = 16384                         # LK_MAX_GRID in svo_kernels_lk.hip: blocks per sequence never exceed it
VARIANTS = {"default": {}, "max_count0": dict(lk_max_count=0), "epsilon0": dict(lk_epsilon=0.0)}


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    orc.set_threads(16)                  # the oracle's results do not depend on its thread count
    yield
    orc.set_threads(1)


@pytest.fixture(scope="module")
def seq():
    from stereo_visual_odometry_amd import synthetic as syn
    return syn.StereoSequence(cal=calib(W, H), n_frames=3, seed=21, step=0.4)


def points(seq, n):
    """n start points: bucketed FAST corners first, then seeded random positions that also lie on and outside the image border"""
    xy, resp = orc.fast_detect(seq.left[0], 20)
    fxy, _, _ = orc.bucket_filter(W, H, xy, np.zeros(len(xy), np.int32), resp.astype(np.int32))
    rng = np.random.default_rng(1000 + n)
    extra = np.stack([rng.uniform(-6, W + 6, max(n, 8)), rng.uniform(-6, H + 6, max(n, 8))], 1).astype(np.float32)
    extra[:4] = [[0.0, 0.0], [W - 1.0, H - 1.0], [-3.5, 40.0], [W + 2.0, 10.25]]
    return np.ascontiguousarray(np.concatenate([fxy[:max(n - 8, 1)], extra])[:n], np.float32)


def oracle_loop(seq, win, over, pts):
    ocfg = orc.default_config(win_w=win, win_h=win, **over)
    P = [orc.Pyramid(i, (win, win), ocfg.max_level) for i in (seq.left[0], seq.right[0], seq.left[1], seq.right[1])]
    return orc.circular_match(P[0], P[1], P[2], P[3], pts, ocfg)


def assert_same_loop(got, want, tag):
    for name, g, o in zip(("pl1", "pr1", "pr0", "plc"), got[:4], want[:4]):
        assert np.array_equal(bits(g), bits(o)), (tag, name, int((bits(g) != bits(o)).any(1).sum()))
    assert np.array_equal(got[4], want[4]), tag


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("win", WINS)
def test_stage_circular_match(api, seq, win, variant):
    over = VARIANTS[variant]
    cfg = api.default_config(win_w=win, win_h=win, **over)
    for n in COUNTS + [LK_SLOTS + 1]:
        pts = points(seq, n)
        got = api.circularMatching(cfg, seq.left[0], seq.right[0], seq.left[1], seq.right[1], pts)
        want = oracle_loop(seq, win, over, pts)
        assert_same_loop(got, want, (win, variant, n))
        if n >= 63 and variant != "max_count0":
            assert 0 < want[4].sum() < n, (win, variant, n)          # both outcomes occur


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("win", WINS)
def test_member_circular_matching_raw_points(api, seq, win, variant):
    """svo_circular_matching on a frame context's cached pyramids: every pass's raw points and the mask, before any compaction."""
    from stereo_visual_odometry_amd._lib import lib
    over = VARIANTS[variant]
    for n in COUNTS:
        pts = points(seq, n)
        vo = api.VisualOdometry(cfg=api.default_config(win_w=win, win_h=win, **over))
        vo.stereo_callback(seq.left[0], seq.right[0])               # caches frame 0's pyramid pair
        l1, r1 = np.ascontiguousarray(seq.left[1]), np.ascontiguousarray(seq.right[1])
        outs = [np.zeros((n, 2), np.float32) for _ in range(4)]
        ok = np.zeros(n, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.svo_circular_matching(vo._h, p(l1), p(r1), l1.strides[0], n, p(pts), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(ok))
        assert rc == 0, (win, variant, n, rc)
        assert_same_loop(outs + [ok], oracle_loop(seq, win, over, pts), (win, variant, n))
        vo.close()


def bgr(a):
    return np.ascontiguousarray(np.stack([a, np.roll(a, 1, 0), 255 - a], -1))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("win,cn", [(w, 1) for w in WINS] + [(21, 3)])
def test_frame_pipeline_counts_and_criteria(api, seq, win, cn, variant):
    """max_features = 1, 63, 64, 65 and unlimited through stereo_callback: statistics (LK level visits, Newton steps, the pass each
    dead feature died in, every count), feature sets and track lists equal the oracle's."""
    from stereo_visual_odometry_amd import synthetic as syn
    Pl, Pr = syn.projection_matrices(calib(W, H))
    L = [bgr(a) for a in seq.left] if cn == 3 else list(seq.left)
    R = [bgr(a) for a in seq.right] if cn == 3 else list(seq.right)
    visits = 0
    for mf in COUNTS + [0]:
        over = dict(win_w=win, win_h=win, max_translation_norm=2.0, max_features=mf, **VARIANTS[variant])
        g = api.VisualOdometry(cfg=api.default_config(**over)); g.initalize_projection_matricies(Pl, Pr)
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        for k in range(3):
            ok_g, T_g = g.stereo_callback(L[k], R[k])
            ok_o, T_o = o.stereo_callback(L[k], R[k])
            so = {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}
            sg = g.stats.as_dict()
            tag = (win, cn, variant, mf, k)
            assert ok_g == ok_o and sg == so, (tag, sg, so)
            fg, fo = g.features(), o.features()
            assert np.array_equal(bits(fg[0]), bits(fo[0])) and np.array_equal(fg[1], fo[1]) and np.array_equal(fg[2], fo[2]), tag
            if k > 0:
                tg, to = g.last_tracks(), o.last_tracks()
                for key in ("pl0", "pr0", "pl1", "pr1"):
                    assert np.array_equal(bits(tg[key]), bits(to[key])), (tag, key)
                if mf:
                    assert so["n_into_lk"] <= mf, (tag, so)
                visits += so["lk_level_visits"]
            assert np.abs(T_g - T_o).max() < 1e-6, tag
        g.close()
    assert visits > 0
