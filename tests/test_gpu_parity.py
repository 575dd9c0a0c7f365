"""Parity of the HIP path (through the C-ABI) against the CPU oracle on identical seeded inputs.

Bar: bit-exact for integer / byte / index work and for every validity mask; float point positions are
compared bit-for-bit too (the LK arithmetic is exact-integer + IEEE f32); poses within POSE_TOL.
"""
import os

import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
import scenes
from gpu_kit import api, f32_bits as bits  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

POSE_TOL_T = 1e-6      # metres, per frame  (north_star states 1e-4; the implementation holds 1e-6)
POSE_TOL_R = 1e-6      # radians, per frame


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)))


def images():
    from stereo_visual_odometry_amd import synthetic as syn
    seq = syn.StereoSequence(cal=dict(syn.KITTI00, width=640, height=200, cx=320.0, cy=100.0), n_frames=1, seed=7)
    return {
        "kat_featureset": scenes.featureset_scene(),
        "texture_odd": scenes.random_texture(97, 131, 3, smooth=1),
        "texture": scenes.random_texture(240, 320, 5, smooth=2),
        "layers": seq.left[0],
        "tiny": scenes.random_texture(16, 16, 9, smooth=0),
        "black": np.zeros((64, 80), np.uint8),
    }


# ---------------------------------------------------------------- FAST
@pytest.mark.parametrize("name", ["kat_featureset", "texture_odd", "texture", "layers", "tiny", "black"])
@pytest.mark.parametrize("th", [1, 5, 20, 60])
def test_fast_score_map_bit_exact(api, name, th):
    img = images()[name]
    got = api.fastScoreMap(img, th)
    want = orc.fast_score_map(img, th)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["kat_featureset", "texture", "layers", "black"])
def test_fast_detect_order_and_values(api, name):
    img = images()[name]
    xy, resp = api.featureDetectionFast(img, 20)
    oxy, oresp = orc.fast_detect(img, 20)
    assert np.array_equal(xy, oxy) and np.array_equal(resp, oresp)


# ---------------------------------------------------------------- reference KATs against the product (main.cpp:50-172)
def test_ref_kat_bucket(api):
    b = api.Bucket(0)
    for a, s in zip([6, 2, 3, 4, 5], [60, 20, 30, 40, 50]):
        b.add_feature((1, 1), a, s)
    assert b.max_size == 0 and b.features.size() == 0
    b = api.Bucket(3)
    for a, s in zip([6, 2, 3, 4, 5], [60, 20, 30, 40, 50]):
        b.add_feature((1, 1), a, s)
    f = b.features
    assert f.size() == 3 and f.ages.tolist() == [6, 4, 5] and f.strengths.tolist() == [60, 40, 50]


def test_bucket_incremental_equals_oracle_bucket(api):
    """Bucket::add_feature one call at a time (content + newcomer through the GPU rule) against the oracle's Bucket over random
    insertions: same slots in the same order after every call, incl. aged-out offers and score ties."""
    rng = np.random.default_rng(5)
    for cap in (1, 3, 6):
        g, o = api.Bucket(cap), orc.Bucket(cap)
        for k in range(40):
            pt = (float(rng.integers(0, 50)), float(rng.integers(0, 50)))
            age, st = int(rng.integers(0, 24)), int(rng.integers(0, 130))
            g.add_feature(pt, age, st); o.add_feature(pt[0], pt[1], age, st)
            assert g.size() == o.size()
            assert g.features.ages.tolist() == o.ages and g.features.strengths.tolist() == o.strengths, (cap, k)


def test_ref_kat_featureset(api):
    img = scenes.featureset_scene()
    fs = api.FeatureSet()
    fs.appendFeaturesFromImage(img, 1)
    assert (fs.ages == 0).all() and (fs.strengths <= 128).all() and fs.size() == 11
    fs.filterByBucketLocationInternal(img, 1, 1, 0, 7)
    assert fs.size() == 7


def test_ref_kat_featureset_filter(api):
    rows = cols = 300
    img = np.zeros((rows, cols), np.uint8)
    fs = api.FeatureSet()
    pts = [(cols - 1.0, rows - 1.0)] * 15 + [(cols - 1.0, 0.0)] * 10 + [(0.0, float((rows + 1) // 2))] * 5
    fs.points = np.array(pts, np.float32); fs.ages = np.zeros(30, np.int32); fs.strengths = np.full(30, 40, np.int32)
    fs.filterByBucketLocationInternal(img, 2, 2, 0, 11)
    assert fs.size() == 26
    cp = api.FeatureSet(); cp.points, cp.ages, cp.strengths = fs.points.copy(), fs.ages.copy(), fs.strengths.copy()
    fs.filterByBucketLocationInternal(img, 2, 1, 0, 11)
    assert fs.size() == 21
    cp.filterByBucketLocationInternal(img, 1, 2, 0, 11)
    assert cp.size() == 16


def test_ref_kat_find_unmoved_points(api):
    p1 = np.array([(i, i) for i in range(35)], np.float32)
    p2 = np.array([(i + (0 if i % 5 else 1), i + (0 if i % 7 else 1)) for i in range(35)], np.float32)
    ok = api.findClosePoints(p1, p2, 0.5)
    assert ok.tolist() == [bool((i % 5) and (i % 7)) for i in range(35)]


# ---------------------------------------------------------------- bucketing parity
@pytest.mark.parametrize("per_bucket,grid", [(1, (92, 160, 4)), (3, (10, 12, 1)), (7, (1, 1, 0)), (2, (5, 9, 2))])
def test_bucket_filter_parity(api, per_bucket, grid):
    rng = np.random.default_rng(11 + per_bucket)
    n, w, h = 3000, 640, 360
    xy = np.stack([rng.uniform(0, w - 0.01, n), rng.uniform(0, h - 0.01, n)], 1).astype(np.float32)
    xy[::3] = np.floor(xy[::3])
    ages = rng.integers(0, 25, n).astype(np.int32)
    st = rng.integers(0, 200, n).astype(np.int32)
    want = orc.bucket_filter(w, h, xy, ages, st, grid[0], grid[1], grid[2], per_bucket)
    fs = api.FeatureSet(); fs.points, fs.ages, fs.strengths = xy.copy(), ages.copy(), st.copy()
    fs.filterByBucketLocationInternal(np.zeros((h, w), np.uint8), grid[0], grid[1], grid[2], per_bucket)
    assert np.array_equal(bits(fs.points), bits(want[0])) and np.array_equal(fs.ages, want[1]) and np.array_equal(fs.strengths, want[2])


@pytest.mark.parametrize("name,th", [("texture", 20), ("layers", 20), ("layers", 5), ("black", 20)])
def test_append_features_fused_parity(api, name, th):
    """FAST -> atomicMax bucket keys -> raster emit must equal cv::FAST order + sequential Bucket::add_feature."""
    img = images()[name]
    h, w = img.shape
    rng = np.random.default_rng(5)
    n0 = 400
    oxy = np.stack([rng.uniform(0, w - 0.01, n0), rng.uniform(0, h - 0.01, n0)], 1).astype(np.float32)
    oag = rng.integers(0, 24, n0).astype(np.int32)
    ost = rng.integers(5, 250, n0).astype(np.int32)
    xy, resp = orc.fast_detect(img, th)
    want = orc.bucket_filter(w, h, np.concatenate([oxy, xy]), np.concatenate([oag, np.zeros(len(xy), np.int32)]),
                             np.concatenate([ost, resp.astype(np.int32)]))
    fs = api.FeatureSet(); fs.points, fs.ages, fs.strengths = oxy.copy(), oag.copy(), ost.copy()
    fs.appendFeaturesFromImage(img, th)
    assert fs.size() == len(want[1])
    assert np.array_equal(bits(fs.points), bits(want[0])) and np.array_equal(fs.ages, want[1]) and np.array_equal(fs.strengths, want[2])


def test_append_features_twice_on_sparse_images_same_thread(api):
    """Two calls on one thread, same image size, each image yielding fewer than PRE_MATCHING_FEATURE_THRESHOLD (100) features:
    the cached stage context's first pass offers its survivors for a second pass that this entry point never runs — the grid
    state it leaves behind must not leak into the next call (round-2 advisor finding: phantom / wrong features)."""
    from scenes import make_empty_image, add_triangle
    imgs = []
    for dx in (0, 37):
        im = make_empty_image(300, 200)                              # 300 rows x 200 columns
        for k in range(6):
            add_triangle(im, 30 + dx + 20 * k, 40 + 40 * k, 8)
        imgs.append(im)
    for rep in range(2):
        for im in imgs:
            xy, resp = orc.fast_detect(im, 20)
            assert 0 < len(xy) < 100
            want = orc.bucket_filter(200, 300, xy, np.zeros(len(xy), np.int32), resp.astype(np.int32))
            fs = api.FeatureSet()
            fs.appendFeaturesFromImage(im, 20)
            assert fs.size() == len(want[1]), (rep, fs.size(), len(want[1]))
            assert np.array_equal(bits(fs.points), bits(want[0])) and np.array_equal(fs.ages, want[1]) and np.array_equal(fs.strengths, want[2])
            # and with existing tracks in the set (their order indices are what a stale key would be decoded against)
            fs2 = api.FeatureSet(); fs2.points, fs2.ages, fs2.strengths = want[0][:3].copy(), want[1][:3].copy() + 2, want[2][:3].copy()
            fs2.appendFeaturesFromImage(im, 20)
            w2 = orc.bucket_filter(200, 300, np.concatenate([want[0][:3], xy]), np.concatenate([want[1][:3] + 2, np.zeros(len(xy), np.int32)]),
                                   np.concatenate([want[2][:3], resp.astype(np.int32)]))
            assert np.array_equal(bits(fs2.points), bits(w2[0])) and np.array_equal(fs2.ages, w2[1]) and np.array_equal(fs2.strengths, w2[2])


# ---------------------------------------------------------------- pyramid
@pytest.mark.parametrize("name,win,lv", [("texture", 10, 3), ("texture_odd", 10, 3), ("layers", 21, 3), ("layers", 21, 4), ("tiny", 7, 3)])
def test_pyramid_bit_exact(api, name, win, lv):
    img = images()[name]
    got = api.buildOpticalFlowPyramid(img, win, lv)
    want = orc.Pyramid(img, (win, win), lv)
    assert len(got) == want.nlevels
    for l in range(want.nlevels):
        assert np.array_equal(got[l], want.level(l)), "level %d" % l


# ---------------------------------------------------------------- LK
def lk_points(w, h, n, seed):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1).astype(np.float32)
    p[: n // 4] = np.floor(p[: n // 4])
    p[0] = (0, 0); p[1] = (w - 1, h - 1); p[2] = (-20, 5); p[3] = (w + 30, h + 30); p[4] = (0.5, h - 0.5)
    return p


@pytest.mark.parametrize("win,lv", [(10, 3), (21, 3), (21, 4), (7, 2), (15, 3), (31, 2)])
@pytest.mark.parametrize("shift", [(1, 0), (4, -3), (13, 2)])
def test_lk_track_bit_exact(api, win, lv, shift):
    a = scenes.random_texture(200, 320, 21, smooth=2)
    b = scenes.shift_image(a, *shift)
    b = np.clip(b.astype(np.int32) + np.random.default_rng(1).integers(-2, 3, b.shape), 0, 255).astype(np.uint8)
    pts = lk_points(320, 200, 300, 17)
    got, gst = api.calcOpticalFlowPyrLK(a, b, pts, win, lv)
    pa, pb = orc.Pyramid(a, (win, win), lv), orc.Pyramid(b, (win, win), lv)
    want, wst = orc.lk_track(pa, pb, pts, (win, win), lv)
    assert np.array_equal(gst, wst)
    assert np.array_equal(bits(got), bits(want))
    assert wst.sum() > 100        # the case is not vacuous


def test_stage_calls_reuse_their_device_buffers_and_stay_exact(api):
    """The stage entry points keep one context per calling thread (include/svo.h, svo_stage_cache_clear): calls that alternate
    image sizes, configurations and point counts (capacity grows), a call after an explicit clear and a call from a second
    thread must all give the oracle's bits — nothing of an earlier call may leak into a later one."""
    import threading
    from stereo_visual_odometry_amd._lib import lib
    cases = []
    for k, (h, w, win, lv, n) in enumerate([(120, 200, 10, 2, 40), (200, 320, 21, 3, 700), (120, 200, 10, 2, 40), (120, 200, 10, 3, 3000),
                                            (200, 320, 21, 3, 5)]):
        a = scenes.random_texture(h, w, 90 + k, smooth=2)
        b = scenes.shift_image(a, 2, 1)
        pts = lk_points(w, h, n, 40 + k)
        want = orc.lk_track(orc.Pyramid(a, (win, win), lv), orc.Pyramid(b, (win, win), lv), pts, (win, win), lv)
        cases.append((a, b, pts, win, lv, want))

    def run(case):
        a, b, pts, win, lv, (want, wst) = case
        got, gst = api.calcOpticalFlowPyrLK(a, b, pts, win, lv)
        assert np.array_equal(gst, wst) and np.array_equal(bits(got), bits(want))

    for c in cases:
        run(c)
    for c in cases[:2]:                                            # same shapes again: served from the cache
        run(c)
    lib.svo_stage_cache_clear(); lib.svo_stage_cache_clear()       # idempotent
    run(cases[1])
    err = []

    def other():
        try:
            run(cases[0]); run(cases[1]); lib.svo_stage_cache_clear()
        except BaseException as e:                                 # noqa: BLE001
            err.append(e)
    t = threading.Thread(target=other); t.start(); t.join()
    assert not err, err
    run(cases[0])
    # short-lived worker threads: each one's cached context goes back to a registry when the thread ends and is taken over by
    # the next thread (round-2 advisor finding: one leaked context of GPU memory per thread); clear_all frees what is left
    lib.svo_stage_cache_clear_all.restype = C.c_int

    def worker(case):
        try:
            run(case); run(case)
        except BaseException as e:                                 # noqa: BLE001
            err.append(e)
    for k in range(6):
        t = threading.Thread(target=worker, args=(cases[k % 2],)); t.start(); t.join()
    assert not err, err
    assert lib.svo_stage_cache_clear_all() <= 2                    # this thread's + ONE orphan shared by all six workers, not six
    assert lib.svo_stage_cache_clear_all() == 0
    run(cases[1])
    # parameters that do not shape the buffers are taken over in place: alternating them must not change results
    K = np.eye(3, dtype=np.float32)
    rng = np.random.default_rng(3)
    world = rng.uniform(-1, 1, (40, 3)).astype(np.float32) + np.array([0, 0, 4], np.float32)
    cam = (world[:, :2] / world[:, 2:3]).astype(np.float32)
    for it, conf in ((100, 0.98), (50, 0.9), (100, 0.98), (20, 0.999)):
        (inl_g, ok_g), R_g, t_g, _ = api.cameraToWorld(K, cam, world, np.eye(3), np.zeros(3), iterations=it, confidence=conf)
        ok_o, R_o, t_o, inl_o, _ = orc.camera_to_world(K, cam, world, np.eye(3), np.zeros(3), iterations=it, confidence=conf)
        assert ok_g == ok_o and np.array_equal(inl_g, inl_o) and np.abs(R_g - R_o).max() < 1e-9 and np.abs(t_g.reshape(3) - t_o).max() < 1e-9


@pytest.mark.parametrize("win", [w for w in range(5, 32) if w not in (7, 10, 15, 21, 31)])
def test_lk_any_square_window_bit_exact(api, win):
    """winSize is a mutable member of the reference (vo.h:251): every square window 5..31 is built (the generic
    one-wave-per-feature form for the sizes that are not tuned) and must match the oracle bit for bit — a single LK pass
    with points on and over the borders, and the fused four-pass circular matching."""
    a = scenes.random_texture(160, 256, 30 + win, smooth=2)
    b = scenes.shift_image(a, 3, -2)
    b = np.clip(b.astype(np.int32) + np.random.default_rng(win).integers(-2, 3, b.shape), 0, 255).astype(np.uint8)
    pts = lk_points(256, 160, 160, win)
    got, gst = api.calcOpticalFlowPyrLK(a, b, pts, win, 2)
    pa, pb = orc.Pyramid(a, (win, win), 2), orc.Pyramid(b, (win, win), 2)
    want, wst = orc.lk_track(pa, pb, pts, (win, win), 2)
    assert np.array_equal(gst, wst) and np.array_equal(bits(got), bits(want)) and wst.sum() > 50
    c, d = scenes.shift_image(a, 0, 1), scenes.shift_image(b, 0, 1)              # "right" views: one row lower
    cfg = api.default_config(win_w=win, win_h=win, max_level=2)
    res = api.circularMatching(cfg, a, c, b, d, pts)
    P = [orc.Pyramid(i, (win, win), 2) for i in (a, c, b, d)]
    ref = orc.circular_match(P[0], P[1], P[2], P[3], pts, orc.default_config(win_w=win, win_h=win, max_level=2))
    assert np.array_equal(res[4], ref[4]) and res[4].sum() > 30
    for g, o in zip(res[:4], ref[:4]):
        assert np.array_equal(bits(g), bits(o))


def test_lk_on_a_level_narrower_than_the_border(api):
    """90 x 46 at win 5, max_level 3: the deepest level is 12 x 6 against a stored border of 12 pixels, so its border folds more
    than once (the iterated REFLECT_101 of borderInterpolate).  Points on and beyond that level's edges — a single LK pass against
    orc.lk_track, and whole stereo_callback frames against the oracle."""
    w, h, win, lv = 90, 46, 5, 3
    a = scenes.random_texture(h, w, 61, smooth=1)
    b = scenes.shift_image(a, 2, -1)
    b = np.clip(b.astype(np.int32) + np.random.default_rng(3).integers(-2, 3, b.shape), 0, 255).astype(np.uint8)
    gx, gy = np.meshgrid(np.arange(-44.0, w + 45, 5.5), np.arange(-44.0, h + 45, 5.5))    # level 3: -5.5 .. 16.75 and -5.5 .. 11.1
    pts = np.concatenate([lk_points(w, h, 80, 5), np.stack([gx.ravel(), gy.ravel()], 1)]).astype(np.float32)
    pts[-1] = (8 * 11.5, 8 * 5.5)                                                       # the deepest level's last pixel centre
    got, gst = api.calcOpticalFlowPyrLK(a, b, pts, win, lv)
    pa, pb = orc.Pyramid(a, (win, win), lv), orc.Pyramid(b, (win, win), lv)
    assert pa.nlevels == 4 and (pa.p.w[3], pa.p.h[3]) == (12, 6)
    want, wst = orc.lk_track(pa, pb, pts, (win, win), lv)
    assert np.array_equal(gst, wst)
    assert np.array_equal(bits(got), bits(want))
    assert wst.sum() > 60 and (wst == 0).sum() > 20          # tracked points, and points the bounds test rejects
    from stereo_visual_odometry_amd import synthetic as syn
    seq = syn.StereoSequence(cal=dict(syn.KITTI00, width=w, height=h, cx=w / 2.0, cy=h / 2.0), n_frames=4, seed=5, step=0.2)
    res = run_both(api, seq, dict(win_w=win, win_h=win, max_level=lv, max_translation_norm=2.0), 4)
    assert any(r[2]["n_into_lk"] > 0 for r in res[1:])


def test_odd_window_in_the_frame_pipeline(api):
    """A window that is not one of the tuned sizes through the whole stereo_callback (gray and BGR contexts)."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=3, seed=77, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    for win, cn in ((13, 1), (18, 3), (26, 1)):
        over = dict(win_w=win, win_h=win, max_level=2, max_translation_norm=2.0, channels=cn)
        g = api.VisualOdometry(cfg=api.default_config(**over)); g.initalize_projection_matricies(Pl, Pr)
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        for k in range(3):
            L, R = seq.left[k], seq.right[k]
            if cn == 3:
                L = np.ascontiguousarray(np.stack([L, np.roll(L, 1, 0), 255 - L], -1)); R = np.ascontiguousarray(np.stack([R, np.roll(R, 1, 0), 255 - R], -1))
            ok_g, T_g = g.stereo_callback(L, R); ok_o, T_o = o.stereo_callback(L, R)
            assert ok_g == ok_o and g.stats.as_dict() == {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, (win, cn, k)
            assert np.array_equal(bits(g.features()[0]), bits(o.features()[0])) and np.abs(T_g - T_o).max() < 1e-6
        assert ok_g, (win, cn)


def test_float_sums_mode_window_shapes_gray_and_bgr(api):
    """Float-sums mode over the shapes its chain layout distinguishes (E = W * CN elements per window row, 8 per SIMD step):
    no SIMD part at all (E < 8), no scalar tail (E % 8 == 0), tail longer / shorter than a SIMD lane's share, 3-channel rows —
    through the whole stereo_callback against the oracle, everything a frame produces bit-exact."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=3, seed=78, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    for win, cn in ((5, 1), (16, 1), (24, 1), (29, 1), (6, 3), (8, 3), (13, 3), (21, 3)):
        over = dict(win_w=win, win_h=win, max_level=2, max_translation_norm=2.0, channels=cn, lk_float_sums=1)
        g = api.VisualOdometry(cfg=api.default_config(**over)); g.initalize_projection_matricies(Pl, Pr)
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        for k in range(3):
            L, R = seq.left[k], seq.right[k]
            if cn == 3:
                L = np.ascontiguousarray(np.stack([L, np.roll(L, 1, 0), 255 - L], -1)); R = np.ascontiguousarray(np.stack([R, np.roll(R, 1, 0), 255 - R], -1))
            ok_g, T_g = g.stereo_callback(L, R); ok_o, T_o = o.stereo_callback(L, R)
            assert ok_g == ok_o and g.stats.as_dict() == {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, (win, cn, k)
            assert np.array_equal(bits(g.features()[0]), bits(o.features()[0])) and np.abs(T_g - T_o).max() < 1e-6, (win, cn, k)
            if k > 0:
                to, tg = o.last_tracks(), g.last_tracks()
                for key in ("pl0", "pr0", "pl1", "pr1"):
                    assert np.array_equal(bits(to[key]), bits(tg[key])), (win, cn, k, key)
        assert g.stats.n_into_lk > 50, (win, cn)


def test_lk_flat_image_fails_min_eig(api):
    a = np.full((100, 120), 77, np.uint8)
    pts = lk_points(120, 100, 40, 3)
    got, gst = api.calcOpticalFlowPyrLK(a, a, pts, 10, 3)
    pa = orc.Pyramid(a, (10, 10), 3)
    want, wst = orc.lk_track(pa, pa, pts, (10, 10), 3)
    assert np.array_equal(gst, wst) and np.array_equal(bits(got), bits(want)) and gst.sum() == 0


def test_ref_kat_circular_matching(api):                   # main.cpp:174-209
    iL0, iR0, iL1, iR1 = scenes.circular_scene()
    cfg = api.default_config()
    fs = api.FeatureSet()
    fs.appendFeaturesFromImage(iL0, api.FAST_THRESHOLD)
    assert fs.size() == 121
    pl1, pr1, pr0, plc, ok = api.circularMatching(cfg, iL0, iR0, iL1, iR1, fs.points)
    assert ok.sum() == 121
    pl1b, pr1b, pr0b, plcb, okb = api.circularMatching(cfg, iL1, iR1, iL1, iR1, fs.points)   # what the reference test really runs
    assert okb.sum() == 121
    api.circularMatching(cfg, iL0, iR0, iL1, iR1, np.zeros((0, 2), np.float32))              # boundary conditions
    assert api.circularMatching(cfg, iL0, iR0, iL1, iR1, fs.points[:1])[4].tolist() == [1]
    # and bit-exact against the oracle
    ocfg = orc.default_config()
    P = [orc.Pyramid(i, (10, 10), 3) for i in (iL0, iR0, iL1, iR1)]
    w = orc.circular_match(P[0], P[1], P[2], P[3], fs.points, ocfg)
    for g, o in zip((pl1, pr1, pr0, plc), w[:4]):
        assert np.array_equal(bits(g), bits(o))
    assert np.array_equal(ok, w[4])


def test_ref_kat_circular_matching_member_form(api):        # main.cpp:174-209 as written there: vo.circularMatching(...)
    iL0, iR0, iL1, iR1 = scenes.circular_scene()
    vo = api.VisualOdometry()
    vo.stereo_callback(iL0, iR0)                            # no projection matrices needed for a first frame (vo.cpp:47-56)
    fs = api.FeatureSet(); fs.appendFeaturesFromImage(iL0, api.FAST_THRESHOLD)
    vo.circularMatching(iL1, iR1, np.zeros((0, 2), np.float32), fs)               # boundary conditions, as in the reference test
    vo.circularMatching(iL1, iR1, fs.points[:1].copy(), fs)
    fs = api.FeatureSet(); fs.appendFeaturesFromImage(iL0, api.FAST_THRESHOLD)
    pl0, pr0, pl1, pr1 = vo.circularMatching(iL1, iR1, fs.points.copy(), fs)
    assert fs.size() == 121 and all(len(p) == 121 for p in (pl0, pr0, pl1, pr1))
    # matchingFeatures (vo.h:354-362): the same pipeline from the four images
    vo2 = api.VisualOdometry(); fs2 = api.FeatureSet()
    vo2.stereo_callback(iL0, iR0)                           # primes the cached pyramids (vo.cpp:47-56), as in stereo_callback's own flow
    ql0, qr0, ql1, qr1 = vo2.matchingFeatures(iL0, iR0, iL1, iR1, fs2)
    assert fs2.size() == 121 and np.abs(ql1 - ql0 - [1, 0]).max() < 0.05 and np.abs(qr0 - ql0 - [0, 1]).max() < 0.05


def test_circular_matching_member_shares_the_cached_pyramids(api):
    """vo.cpp:231-232 -> the next :203: the member circularMatching works on the pyramids stereo_callback cached and leaves the
    T1 pyramids cached for the next stereo_callback.  (a) its outputs equal the stage function on (cached pair, T1 pair),
    bit for bit; (b) a stereo_callback after it tracks against the pair it cached, frame by frame equal to the oracle fed the
    equivalent image order."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=4, seed=5, step=0.4)
    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0)
    vo = api.VisualOdometry(cfg=api.default_config(**over)); vo.initalize_projection_matricies(Pl, Pr)
    vo.stereo_callback(seq.left[0], seq.right[0])
    fs = api.FeatureSet(); fs.appendFeaturesFromImage(seq.left[0], api.FAST_THRESHOLD)
    pts = fs.points.copy()
    m = vo.circularMatching(seq.left[1], seq.right[1], pts, fs)                       # T0 = frame 0 (cached), T1 = frame 1
    pl1, pr1, pr0, _, ok = api.circularMatching(api.default_config(**over), seq.left[0], seq.right[0], seq.left[1], seq.right[1], pts)
    keep = ok.astype(bool)
    for got, want in zip(m, (pts[keep], pr0[keep], pl1[keep], pr1[keep])):
        assert np.array_equal(bits(got), bits(want))
    assert 0 < keep.sum() < len(pts) or keep.all()
    # (b) the cached pair is now frame 1's pyramids while imageLeftT0_ is still frame 0: the next callback detects on frame 0
    # and tracks frame-1 pyramids -> frame 2.  The oracle reproduces that state when fed (0), then frame 2 with its pyramid
    # cache swapped to frame 1 — which is what a member circularMatching does in the reference; without such a hook in the
    # oracle, compare against a second product object that gets there through stereo_callback alone on a crafted order:
    # callback(frame 1) after callback(frame 0) caches frame 1's pyramids AND images, so the two objects must differ in
    # what FAST saw (frame 0 vs frame 1) but agree on what LK tracked against.
    ok_a, T_a = vo.stereo_callback(seq.left[2], seq.right[2])
    ref = api.VisualOdometry(cfg=api.default_config(**over)); ref.initalize_projection_matricies(Pl, Pr)
    ref.stereo_callback(seq.left[0], seq.right[0]); ref.stereo_callback(seq.left[1], seq.right[1])
    ok_b, T_b = ref.stereo_callback(seq.left[2], seq.right[2])
    gt = seq.relative_motion(2)
    assert ok_a and ok_b
    # both estimate the motion frame 1 -> frame 2 (the pyramids LK tracked against), to the scene's accuracy
    assert np.linalg.norm(T_a[:3, 3] - gt[:3, 3]) < 0.05 and np.linalg.norm(T_b[:3, 3] - gt[:3, 3]) < 0.05
    # and an object that never called circularMatching still tracks frame 0 -> frame 2: twice the step
    far = api.VisualOdometry(cfg=api.default_config(**over)); far.initalize_projection_matricies(Pl, Pr)
    far.stereo_callback(seq.left[0], seq.right[0])
    ok_c, T_c = far.stereo_callback(seq.left[2], seq.right[2])
    gt02 = np.linalg.inv(seq.poses[0]) @ seq.poses[2]
    assert ok_c and np.linalg.norm(T_c[:3, 3] - gt02[:3, 3]) < 0.08 and np.linalg.norm(T_c[:3, 3]) > 1.5 * np.linalg.norm(T_a[:3, 3])


@pytest.mark.parametrize("win", [10, 21])
def test_circular_match_parity_stereo_scene(api, win):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=2, seed=3)
    cfg = api.default_config(win_w=win, win_h=win)
    ocfg = orc.default_config(win_w=win, win_h=win)
    xy, resp = orc.fast_detect(seq.left[0], 20)
    fxy, _, _ = orc.bucket_filter(480, 200, xy, np.zeros(len(xy), np.int32), resp.astype(np.int32))
    got = api.circularMatching(cfg, seq.left[0], seq.right[0], seq.left[1], seq.right[1], fxy)
    P = [orc.Pyramid(i, (win, win), 3) for i in (seq.left[0], seq.right[0], seq.left[1], seq.right[1])]
    want = orc.circular_match(P[0], P[1], P[2], P[3], fxy, ocfg)
    assert np.array_equal(got[4], want[4])
    for g, o in zip(got[:4], want[:4]):
        assert np.array_equal(bits(g), bits(o))
    assert 0.3 * len(fxy) < want[4].sum() < len(fxy)       # both outcomes occur
    # the same stage call in float-sums mode (oracle: D1 reverted): the member / stage form runs ALL four passes of every point
    # (no early-out: the caller gets every pass's raw points), also for points that die in an early pass
    cfg.lk_float_sums = 1
    pts = np.concatenate([fxy, np.array([[2.0, 3.0], [478.5, 1.5], [-4.0, 50.0]], np.float32)])      # some that leave the image
    got = api.circularMatching(cfg, seq.left[0], seq.right[0], seq.left[1], seq.right[1], pts)
    prev = orc.lib().orc_set_opencv_mode(1)
    try:
        want_fs = orc.circular_match(P[0], P[1], P[2], P[3], pts, ocfg)
    finally:
        orc.lib().orc_set_opencv_mode(prev)
    assert np.array_equal(got[4], want_fs[4])
    for g, o in zip(got[:4], want_fs[:4]):
        assert np.array_equal(bits(g), bits(o))
    assert not all(np.array_equal(bits(a), bits(b)) for a, b in zip(want_fs[:4], [w[:len(pts)] for w in orc.circular_match(P[0], P[1], P[2], P[3], pts, ocfg)[:4]]))


# ---------------------------------------------------------------- triangulation / PnP
def _small_pnp_scene(n, seed):
    rng = np.random.default_rng(seed)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)
    r = rng.normal(0, 0.2, 3); th = np.linalg.norm(r); k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(0, 0.3, 3) + [0, 0, 1.0]
    X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1).astype(np.float32)
    Xc = X.astype(np.float64) @ R.T + t
    uv = ((Xc[:, :2] / Xc[:, 2:]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)
    return K, R, t, X, uv


@pytest.mark.parametrize("seed", range(6))
def test_camera_to_world_four_points_is_one_p3p(api, seed):
    """cv::solvePnPRansac with npoints == 4: one direct P3P, all four inliers, no RANSAC, no refine — against the
    oracle's restatement (pow / acos / cos in the cubic: tolerance, not bits) and against the known pose."""
    K, R, t, X, uv = _small_pnp_scene(4, seed)
    (inl, ok), R_g, t_g, iters = api.cameraToWorld(K, uv, X, np.eye(3), np.zeros(3))
    ok_o, R_o, t_o, inl_o, _ = orc.camera_to_world(K, uv, X, np.eye(3), np.zeros(3))
    assert ok and ok_o and inl.tolist() == [0, 1, 2, 3] == inl_o.tolist() and iters == 0
    assert np.abs(R_g - R_o).max() < 1e-9 and np.abs(t_g.reshape(3) - t_o).max() < 1e-8
    assert np.abs(R_g - R).max() < 2e-4 and np.abs(t_g.reshape(3) - t).max() < 2e-3


@pytest.mark.parametrize("seed", range(4))
def test_camera_to_world_five_points_is_one_epnp(api, seed):
    """npoints == 5 == model_points: one direct EPnP on all points, all inliers, no LM refine."""
    K, R, t, X, uv = _small_pnp_scene(5, 50 + seed)
    (inl, ok), R_g, t_g, iters = api.cameraToWorld(K, uv, X, np.eye(3), np.zeros(3))
    ok_o, R_o, t_o, inl_o, _ = orc.camera_to_world(K, uv, X, np.eye(3), np.zeros(3))
    assert ok and ok_o and inl.tolist() == [0, 1, 2, 3, 4] == inl_o.tolist() and iters == 0
    assert np.abs(R_g - R_o).max() < 1e-9 and np.abs(t_g.reshape(3) - t_o).max() < 1e-9


def test_camera_to_world_fewer_than_four_points_is_an_error(api):
    K, R, t, X, uv = _small_pnp_scene(3, 1)
    with pytest.raises(api._lib.SvoError):
        api.cameraToWorld(K, uv, X, np.eye(3), np.zeros(3))


@pytest.mark.parametrize("per_bucket,grid", [(3, (92, 160)), (2, (20, 30)), (7, (6, 8))])
def test_features_per_bucket_above_one_in_the_frame_pipeline(api, per_bucket, grid):
    """FEATURES_PER_BUCKET is a constant of the reference (vo.h:65) that its own tests vary (main.cpp:125, 152-157): capacities
    above 1 take the general Bucket::add_feature walk inside stereo_callback — feature sets (order included), tracks, masks and
    counters identical to the oracle on every frame, with ages building up so that the replace-the-minimum rule really fires."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=5, seed=31, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=10, win_h=10, max_translation_norm=2.0, features_per_bucket=per_bucket, buckets_along_height=grid[0], buckets_along_width=grid[1],
                bucket_start_row=1)
    g = api.VisualOdometry(cfg=api.default_config(**over)); g.initalize_projection_matricies(Pl, Pr)
    o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
    full = 0
    for k in range(5):
        ok_g, T_g = g.stereo_callback(seq.left[k], seq.right[k]); ok_o, T_o = o.stereo_callback(seq.left[k], seq.right[k])
        sg = g.stats.as_dict(); so = {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}
        assert ok_g == ok_o and sg == so, (k, sg, so)
        fg, fo = g.features(), o.features()
        assert np.array_equal(bits(fg[0]), bits(fo[0])) and np.array_equal(fg[1], fo[1]) and np.array_equal(fg[2], fo[2]), k
        assert np.abs(T_g - T_o).max() < 1e-6
        full += so["n_after_detect"]
    assert ok_g and full > 5 * 100


def test_five_tracks_through_the_frame_pipeline(api):
    """features_threshold below 5 lets a frame reach PnP with exactly five tracks (vo.cpp:82 is max(4, FEATURES_THRESHOLD)):
    the direct 5-point branch then runs inside stereo_callback, identically to the oracle."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=3, seed=11, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=21, win_h=21, max_translation_norm=5.0, max_rotation_norm=3.0, features_threshold=0, max_features=5)
    g = api.VisualOdometry(cfg=api.default_config(**over)); g.initalize_projection_matricies(Pl, Pr)
    o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
    seen5 = False
    for k in range(3):
        ok_g, T_g = g.stereo_callback(seq.left[k], seq.right[k]); ok_o, T_o = o.stereo_callback(seq.left[k], seq.right[k])
        sg = g.stats.as_dict(); so = {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}
        assert ok_g == ok_o and sg == so, (k, sg, so)
        assert np.abs(T_g - T_o).max() < 1e-9
        seen5 |= so["n_after_bounds"] == 5 and so["n_inliers"] == 5
    assert seen5

def test_triangulate_bit_exact_and_analytic(api):
    from stereo_visual_odometry_amd import synthetic as syn
    Pl, Pr = syn.projection_matrices(syn.KITTI00)
    rng = np.random.default_rng(2)
    n = 2000
    Z = rng.uniform(4, 90, n); X = rng.uniform(-20, 20, n); Y = rng.uniform(-3, 3, n)
    ul = 718.856 * X / Z + 607.1928; v = 718.856 * Y / Z + 185.2157; ur = ul - 386.1448 / Z
    pl = np.stack([ul, v], 1).astype(np.float32); pr = np.stack([ur, v + rng.normal(0, 0.05, n)], 1).astype(np.float32)
    got = api.triangulatePoints(Pl, Pr, pl, pr)
    want, _ = orc.triangulate(Pl, Pr, pl, pr)
    assert np.array_equal(bits(got), bits(want))
    # analytic pin (no reference test covers cv::triangulatePoints): Z = -bf / (xl - xr) when yl == yr
    pr2 = np.stack([ur, v], 1).astype(np.float32)
    z = api.triangulatePoints(Pl, Pr, pl, pr2)[:, 2]
    zz = 386.1448 / (pl[:, 0].astype(np.float64) - pr2[:, 0].astype(np.float64))
    assert np.abs(z / zz - 1).max() < 1e-4


def test_ref_kat_camera_to_world(api):                      # main.cpp:211-264
    K, cam, world = scenes.camera_to_world_scene()
    (inl, ok), R, t, iters = api.cameraToWorld(K, cam, world, np.eye(3), np.zeros(3))
    assert ok and len(inl) == 27 and inl.tolist() == list(range(27))
    t = t.ravel()
    assert abs(t[0]) < 1e-6 and abs(t[1]) < 1e-6 and abs(t[2] - 1) < 1e-6
    assert np.abs(R - np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])).max() < 1e-8


@pytest.mark.parametrize("outliers,iters", [(0.0, 100), (0.3, 100), (0.6, 300)])
def test_camera_to_world_parity(api, outliers, iters):
    rng = np.random.default_rng(int(outliers * 10) + 1)
    n = 800
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)
    world = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(6, 60, n)], 1).astype(np.float32)
    rv = np.array([0.01, -0.02, 0.005]); tv = np.array([0.05, -0.02, -0.6])
    Rm, _ = orc.rodrigues_to_matrix(rv)
    pc = world.astype(np.float64) @ Rm.T + tv
    cam = np.stack([718.856 * pc[:, 0] / pc[:, 2] + 607.1928, 718.856 * pc[:, 1] / pc[:, 2] + 185.2157], 1)
    cam += rng.normal(0, 0.2, cam.shape)
    bad = rng.random(n) < outliers
    cam[bad] += rng.uniform(-80, 80, (bad.sum(), 2))
    cam = cam.astype(np.float32)
    ok_o, R_o, t_o, inl_o, dbg = orc.camera_to_world(K, cam, world, np.eye(3), np.zeros(3), iters)
    (inl, ok), R, t, it = api.cameraToWorld(K, cam, world, np.eye(3), np.zeros(3), iterations=iters)
    assert ok == ok_o and it == dbg[0]
    assert np.array_equal(inl, inl_o)                       # inlier mask bit-exact
    assert np.abs(t.ravel() - t_o).max() < POSE_TOL_T and rot_angle(R, R_o) < POSE_TOL_R
    assert np.abs(t.ravel() - tv).max() < 0.05              # and it is the right pose


# ---------------------------------------------------------------- whole frames
def run_both(api, seq, cfg_over, n_frames):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = seq.cal
    Pl, Pr = syn.projection_matrices(cal)
    ovo = orc.VisualOdometry(orc.default_config(**cfg_over)); ovo.initalize_projection_matricies(Pl, Pr)
    gvo = api.VisualOdometry(cfg=api.default_config(**cfg_over)); gvo.initalize_projection_matricies(Pl, Pr)
    out = []
    for k in range(n_frames):
        ok_o, T_o = ovo.stereo_callback(seq.left[k], seq.right[k])
        ok_g, T_g = gvo.stereo_callback(seq.left[k], seq.right[k])
        so = {f[0]: getattr(ovo.stats, f[0]) for f in ovo.stats._fields_}
        sg = gvo.stats.as_dict()
        assert ok_o == ok_g, (k, so, sg)
        assert so == sg, (k, so, sg)
        fo, fg = ovo.features(), gvo.features()
        assert np.array_equal(bits(fo[0]), bits(fg[0])) and np.array_equal(fo[1], fg[1]) and np.array_equal(fo[2], fg[2]), k
        if k > 0:
            to, tg = ovo.last_tracks(), gvo.last_tracks()
            for key in ("pl0", "pr0", "pl1", "pr1"):
                assert np.array_equal(bits(to[key]), bits(tg[key])), (k, key)
            if so["fail_reason"] in (0, 3, 4) and so["n_after_bounds"] > 15:
                assert np.array_equal(bits(to["world"]), bits(tg["world"])), k
                assert np.array_equal(to["inlier"], tg["inlier"]), k
        assert np.abs(T_o[:3, 3] - T_g[:3, 3]).max() < POSE_TOL_T, (k, T_o, T_g)
        assert rot_angle(T_o[:3, :3], T_g[:3, :3]) < POSE_TOL_R, k
        out.append((ok_g, T_g, sg))
    return out


@pytest.mark.parametrize("win,lv", [(10, 3), (21, 3)])
def test_stereo_callback_sequence_parity(api, win, lv):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=5, seed=12, step=0.4)
    res = run_both(api, seq, dict(win_w=win, win_h=win, max_level=lv, max_translation_norm=2.0), 5)
    assert res[0][0] is False and res[0][2]["fail_reason"] == 1
    assert all(r[0] for r in res[1:])
    gt = seq.relative_motion(2)
    assert np.abs(res[2][1][:3, 3] - gt[:3, 3]).max() < 0.03


@pytest.mark.parametrize("win,lv", [(10, 3), (21, 3), (7, 2), (13, 3), (31, 2)])
def test_float_sums_mode_parity(api, win, lv):
    """svo_config.lk_float_sums = 1: the LK sums in FLOAT, in the lane order of OpenCV's SIMD128 code (oracle: deviation D1
    reverted, orc_config.lk_float_sums).  Same bar as the default mode: every counter, feature set, track list, world point
    and inlier mask bit-exact — and the two modes must really differ somewhere (or the switch does nothing)."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=5, seed=12, step=0.4)
    over = dict(win_w=win, win_h=win, max_level=lv, max_translation_norm=2.0)
    fs = run_both(api, seq, dict(over, lk_float_sums=1), 5)
    assert all(r[0] for r in fs[1:])
    ex = run_both(api, seq, over, 5)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(fs[1:], ex[1:])), "float sums and exact sums gave identical poses"
    assert max(np.abs(a[1] - b[1]).max() for a, b in zip(fs[1:], ex[1:])) < 1e-3


def test_float_sums_mode_kitti_frame_and_batch(api):
    """full cfg2-sized frames in float-sums mode, as a batch of two sequences (different frames) against two oracle objects"""
    from stereo_visual_odometry_amd import synthetic as syn
    seq = syn.StereoSequence(n_frames=4, seed=0x5EED0002)
    Pl, Pr = syn.projection_matrices(seq.cal)
    over = dict(win_w=21, win_h=21, max_level=3, max_translation_norm=2.0, lk_float_sums=1)
    b = api.BatchVisualOdometry(seq.cal["width"], seq.cal["height"], 2, api.default_config(**over)); b.initalize_projection_matricies(Pl, Pr)
    os_ = []
    for _ in range(2):
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr); os_.append(o)
    for k in range(3):
        ok, T = b.stereo_callback_batch([seq.left[k], seq.left[k + 1]], [seq.right[k], seq.right[k + 1]])
        for i, o in enumerate(os_):
            ok_o, T_o = o.stereo_callback(seq.left[k + i], seq.right[k + i])
            so = {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}
            assert bool(ok[i]) == ok_o and so == b.stats[i].as_dict(), (k, i, so, b.stats[i].as_dict())
            assert np.abs(T[i] - T_o).max() < 1e-6


def test_stereo_callback_failure_paths_parity(api):
    """too-few-tracks (black frames -> second FAST pass, empty feature set, stale pyramid quirk), then recovery,
    then the motion gate (reference default MAX_TRANSLATION_NORM with a 0.4 m step)."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=4, seed=5, step=0.4)
    black = np.zeros_like(seq.left[0])
    seq.left = [black, black] + seq.left
    seq.right = [black, black] + seq.right
    res = run_both(api, seq, dict(), 6)
    reasons = [r[2]["fail_reason"] for r in res]
    assert reasons[0] == 1 and reasons[1] == 2 and reasons[2] == 2
    assert res[1][2]["second_pass"] == 1
    assert 4 in reasons[3:]                                  # the 0.1 m gate rejects the 0.4 m steps


def test_many_sequence_context_failure_paths_and_second_pass(api):
    """The failure paths inside a context of more than 8 sequences, frames submitted ahead (two in flight): such a context builds
    the next frame's pyramids on a second stream into a fourth pyramid slot (k_pick_next / k_frame_begin) and runs the second
    detection pass with strided kernels.  Sequences 0-4 replay black frames first (second FAST pass, empty feature set, the stale
    lastLeftPyramid of vo.cpp:179-181 next to a fresh imageLeftT0_ — the case that needs all four slots), sequences 5-9 start on
    the scene at once; every sequence must give the oracle's flags, counters, feature sets and pose, frame by frame."""
    from stereo_visual_odometry_amd import synthetic as syn
    import torch
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0)
    sq = syn.StereoSequence(cal=cal, n_frames=5, seed=11, step=0.3)
    black = np.zeros_like(sq.left[0])
    streams = [([black, black] + sq.left[:4], [black, black] + sq.right[:4]),      # black, black, then the scene
               (sq.left + [sq.left[4]], sq.right + [sq.right[4]])]                  # the scene, last frame repeated (zero motion)
    Pl, Pr = syn.projection_matrices(cal)
    want = []
    for L, R in streams:
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        per = []
        for k in range(6):
            ok, T = o.stereo_callback(L[k], R[k])
            per.append((ok, T.copy(), {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, [a.copy() for a in o.features()]))
        want.append(per)
    assert want[0][1][2]["second_pass"] == 1
    B = 10
    vo = api.BatchVisualOdometry(480, 200, B, api.default_config(**over)); vo.initalize_projection_matricies(Pl, Pr)
    which = lambda i: 0 if i < 5 else 1
    dev = [[(torch.from_numpy(np.ascontiguousarray(L[k])).cuda(), torch.from_numpy(np.ascontiguousarray(R[k])).cuda()) for k in range(6)] for L, R in streams]
    torch.cuda.synchronize()
    submit = lambda k: vo.submit_device([dev[which(i)][k][0].data_ptr() for i in range(B)], [dev[which(i)][k][1].data_ptr() for i in range(B)], 480)
    submit(0)
    for k in range(6):
        if k + 1 < 6:
            submit(k + 1)                                            # the next frame is in flight before this one is collected
        ok, T = vo.collect()
        for i in range(B):
            w = want[which(i)][k]
            sg = vo.stats[i].as_dict()
            assert bool(ok[i]) == w[0] and sg == w[2], (k, i, sg, w[2])
            assert np.abs(T[i][:3, 3] - w[1][:3, 3]).max() < POSE_TOL_T and rot_angle(T[i][:3, :3], w[1][:3, :3]) < POSE_TOL_R
    for i in (0, 4, 5, 9):
        f = vo.features(i); w = want[which(i)][5][3]
        assert np.array_equal(bits(f[0]), bits(w[0])) and np.array_equal(f[1], w[1]) and np.array_equal(f[2], w[2])


def test_kitti_shaped_frame_parity(api):
    """full BASELINE cfg2 size (1241x376, 21x21 window, 3 levels), two frames."""
    from stereo_visual_odometry_amd import synthetic as syn
    seq = syn.StereoSequence(n_frames=3, seed=0x5EED0002)
    res = run_both(api, seq, dict(win_w=21, win_h=21, max_level=3, max_translation_norm=2.0), 3)
    assert res[1][0] and res[2][0] and res[2][2]["n_inliers"] > 500


def test_batch_equals_single(api):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seqs = [syn.StereoSequence(cal=cal, n_frames=3, seed=s, step=0.3) for s in (1, 2, 3)]
    Pl, Pr = syn.projection_matrices(cal)
    cfg = api.default_config(win_w=21, win_h=21, max_translation_norm=2.0)
    singles = []
    for s in seqs:
        vo = api.VisualOdometry(cfg=cfg); vo.initalize_projection_matricies(Pl, Pr)
        singles.append([vo.stereo_callback(s.left[k], s.right[k]) + (vo.stats.as_dict(),) for k in range(3)])
    b = api.BatchVisualOdometry(480, 200, 3, cfg); b.initalize_projection_matricies(Pl, Pr)
    for k in range(3):
        ok, T = b.stereo_callback_batch([s.left[k] for s in seqs], [s.right[k] for s in seqs])
        for i in range(3):
            assert ok[i] == singles[i][k][0]
            assert np.array_equal(T[i], singles[i][k][1])           # same kernels, same order: identical bits
            assert b.stats[i].as_dict() == singles[i][k][2]


def test_two_many_sequence_contexts_sharing_the_device(api):
    """Contexts of more than 8 sequences that share a GPU chain their LK launches through an event — the
    configuration bench.py runs.  At w = 21 the LK build leaves 32 registers free, so they keep the FULL builds of triangulate /
    EPnP / refine: the 96-register builds are covered by test_gpu_shared_device_builds.py.  Two contexts of 10 sequences,
    frames submitted interleaved so that their kernels really overlap, an outlier layer so that RANSAC iterates: every
    sequence of both must give the oracle's flags, counters and feature sets, and its pose to the usual tolerance."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0)
    seqs = [syn.StereoSequence(cal=cal, n_frames=4, seed=70 + s, step=0.3, movers=0.3 if s else 0.0) for s in range(3)]
    Pl, Pr = syn.projection_matrices(cal)
    want = []
    for sq in seqs:
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        per = []
        for k in range(4):
            ok, T = o.stereo_callback(sq.left[k], sq.right[k])
            per.append((ok, T.copy(), {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, [a.copy() for a in o.features()]))
        want.append(per)
    B = 10
    ctx = [api.BatchVisualOdometry(480, 200, B, api.default_config(**over)) for _ in range(2)]
    for c in ctx:
        c.initalize_projection_matricies(Pl, Pr)
    pick = lambda c, i: (i + 2 * c) % 3                            # which rendered sequence slot i of context c replays
    import torch
    dev = [[(torch.from_numpy(np.ascontiguousarray(sq.left[k])).cuda(), torch.from_numpy(np.ascontiguousarray(sq.right[k])).cuda())
            for k in range(4)] for sq in seqs]                      # inputs resident in HBM, as in bench.py
    torch.cuda.synchronize()
    seen_iters = 0
    for k in range(4):
        outs = []
        for c, vo in enumerate(ctx):                                # both contexts in flight before either is collected
            vo.submit_device([dev[pick(c, i)][k][0].data_ptr() for i in range(B)], [dev[pick(c, i)][k][1].data_ptr() for i in range(B)], 480)
            path = vo.last_frame_path()
            assert path & api._lib.PATH_LK_CHAINED and not path & api._lib.PATH_LEAN, (k, c, path)   # chained LK, full builds
        for c, vo in enumerate(ctx):
            outs.append(vo.collect())
        for c, vo in enumerate(ctx):
            ok, T = outs[c]
            for i in range(B):
                w = want[pick(c, i)][k]
                sg = vo.stats[i].as_dict()
                assert bool(ok[i]) == w[0] and sg == w[2], (k, c, i, sg, w[2])
                assert np.abs(T[i][:3, 3] - w[1][:3, 3]).max() < POSE_TOL_T and rot_angle(T[i][:3, :3], w[1][:3, :3]) < POSE_TOL_R
                seen_iters = max(seen_iters, sg["ransac_iters"])
        for c, vo in enumerate(ctx):
            for i in (0, B - 1):
                f = vo.features(i); w = want[pick(c, i)][k][3]
                assert np.array_equal(bits(f[0]), bits(w[0])) and np.array_equal(f[1], w[1]) and np.array_equal(f[2], w[2])
    assert seen_iters > 3                                           # the adaptive loop really ran


@pytest.mark.parametrize("win", [7, 10, 15])
def test_many_sequence_context_small_windows(api, win):
    """A many-sequence context (9 sequences) at the small windows against the oracle."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=400, height=176, cx=200.0, cy=88.0)
    over = dict(win_w=win, win_h=win, max_level=2, max_translation_norm=2.0)
    seqs = [syn.StereoSequence(cal=cal, n_frames=3, seed=300 + 7 * win + s, step=0.3) for s in range(2)]
    Pl, Pr = syn.projection_matrices(cal)
    want = []
    for sq in seqs:
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        per = []
        for k in range(3):
            ok, T = o.stereo_callback(sq.left[k], sq.right[k])
            per.append((ok, T.copy(), {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, [a.copy() for a in o.features()], o.last_tracks() if k else None))
        want.append(per)
    B = 9
    vo = api.BatchVisualOdometry(400, 176, B, api.default_config(**over)); vo.initalize_projection_matricies(Pl, Pr)
    for k in range(3):
        ok, T = vo.stereo_callback_batch([seqs[i % 2].left[k] for i in range(B)], [seqs[i % 2].right[k] for i in range(B)])
        for i in range(B):
            w = want[i % 2][k]
            assert bool(ok[i]) == w[0] and vo.stats[i].as_dict() == w[2], (k, i, vo.stats[i].as_dict(), w[2])
            assert np.abs(T[i][:3, 3] - w[1][:3, 3]).max() < POSE_TOL_T
        for i in (0, B - 1):
            f = vo.features(i); w = want[i % 2][k]
            assert np.array_equal(bits(f[0]), bits(w[3][0])) and np.array_equal(f[1], w[3][1]) and np.array_equal(f[2], w[3][2])
            if k:
                tg = vo.last_tracks(i)
                for key in ("pl0", "pr0", "pl1", "pr1"):
                    assert np.array_equal(bits(w[4][key]), bits(tg[key])), (k, i, key)


# ---------------------------------------------------------------- the other BASELINE.json configs as parity cases
def test_max_features_preset_keeps_the_first_n_in_bucket_order(api):
    """The build preset of SURVEY.md 8d cfg2 (not in the reference): only the first max_features of the bucketed set enter
    circularMatching, the rest are dropped from the feature set; oracle and product must agree on every frame."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=480, height=200, cx=240.0, cy=100.0)
    seq = syn.StereoSequence(cal=cal, n_frames=4, seed=31, step=0.4)
    free = run_both(api, seq, dict(win_w=10, win_h=10, max_translation_norm=2.0), 2)
    assert free[1][2]["n_into_lk"] > 250
    res = run_both(api, seq, dict(win_w=10, win_h=10, max_translation_norm=2.0, max_features=200), 4)
    assert all(r[2]["n_into_lk"] == 200 for r in res[1:]) and all(r[0] for r in res[1:])


@pytest.mark.parametrize("over", [
    dict(win_w=15, win_h=15, max_level=2, buckets_along_height=40, buckets_along_width=64, bucket_start_row=2, fast_threshold=30,
         age_threshold=3, features_threshold=10, pre_matching_feature_threshold=50, ransac_reprojection_error=2.0,
         ransac_confidence=0.9, ransac_iterations=40, lk_max_count=10, lk_epsilon=1e-2,
         circular_matching_success_threshold=0.3, optical_flow_min_eig_threshold=1e-2, max_translation_norm=2.0),
    dict(win_w=7, win_h=7, max_level=4, buckets_along_height=23, buckets_along_width=31, bucket_start_row=0, fast_threshold=12,
         age_threshold=2, features_threshold=25, pre_matching_feature_threshold=2000, ransac_reprojection_error=0.7,
         ransac_confidence=0.999, ransac_iterations=300, lk_max_count=100, lk_epsilon=0.0,
         circular_matching_success_threshold=0.05, optical_flow_min_eig_threshold=1e-4, max_translation_norm=0.45,
         max_rotation_norm=0.004),
], ids=["coarse-grid-loose", "fine-grid-strict"])
def test_every_config_knob_away_from_its_default(api, over):
    """All run-time constants of vo.h:53-127 / :251-252 moved off the reference values at once (the second set forces the
    second FAST pass every frame, a tight RANSAC threshold and motion gates that trip on some frames)."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=512, height=224, cx=256.0, cy=112.0)
    seq = syn.StereoSequence(cal=cal, n_frames=7, seed=77, step=0.4, yaw_amp_deg=0.3)
    res = run_both(api, seq, over, 7)
    assert any(r[0] for r in res[1:])                            # not vacuous: poses were produced


def test_cfg3_four_levels_1000_ransac_iterations(api):
    """configs[2]: KITTI-00 shaped, maxLevel 4 (5 levels), 1000 RANSAC-PnP iterations, denser features."""
    from stereo_visual_odometry_amd import synthetic as syn
    seq = syn.StereoSequence(n_frames=3, seed=0x5EED0003, cell_px=12.0)
    res = run_both(api, seq, dict(win_w=21, win_h=21, max_level=4, ransac_iterations=1000, max_translation_norm=2.0), 3)
    assert res[2][0] and res[2][2]["n_into_lk"] > 3000


def test_cfg5_zed_hd_frame(api):
    """configs[4]: ZED calibration, 1920x1080, 21x21 window: HD-resolution stress (bucket size 12x12)."""
    from stereo_visual_odometry_amd import synthetic as syn
    seq = syn.StereoSequence(cal=syn.ZED, n_frames=3, seed=0x5EED0005, cell_px=14.0, depth=(6.0, 40.0), step=0.2)
    res = run_both(api, seq, dict(win_w=21, win_h=21, max_level=3, max_translation_norm=2.0), 3)
    assert res[2][0] and res[2][2]["n_into_lk"] > 5000


def test_outlier_scene_exercises_adaptive_ransac(api):
    """A moving foreground (frames from a second scene pasted in) makes RANSAC run more than one iteration."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=640, height=240, cx=320.0, cy=120.0)
    a = syn.StereoSequence(cal=cal, n_frames=3, seed=21, step=0.4)
    b = syn.StereoSequence(cal=cal, n_frames=3, seed=22, step=-0.9, yaw_amp_deg=1.5)     # a differently moving world
    for k in range(3):
        for im_a, im_b in ((a.left[k], b.left[k]), (a.right[k], b.right[k])):
            im_a[60:200, 380:640] = im_b[60:200, 380:640]
    res = run_both(api, a, dict(win_w=21, win_h=21, max_translation_norm=2.0, ransac_reprojection_error=1.0), 3)
    assert any(r[2]["ransac_iters"] > 1 for r in res[1:])


def test_long_sequence_parity_crosses_age_threshold(api):
    """26 frames of slow motion: tracks survive long enough to reach AGE_THRESHOLD = 20 and get dropped at bucketing
    (feature_set.cpp:26, SURVEY B-8); every frame must stay bit-exact against the oracle."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=400, height=180, cx=200.0, cy=90.0)
    seq = syn.StereoSequence(cal=cal, n_frames=26, seed=77, step=0.05, yaw_amp_deg=0.05)
    Pl, Pr = syn.projection_matrices(cal)
    ovo = orc.VisualOdometry(orc.default_config(win_w=21, win_h=21)); ovo.initalize_projection_matricies(Pl, Pr)
    gvo = api.VisualOdometry(cfg=api.default_config(win_w=21, win_h=21)); gvo.initalize_projection_matricies(Pl, Pr)
    max_age, dropped_old = 0, False
    prev_ages = None
    for k in range(26):
        ok_o, T_o = ovo.stereo_callback(seq.left[k], seq.right[k])
        ok_g, T_g = gvo.stereo_callback(seq.left[k], seq.right[k])
        assert ok_o == ok_g, k
        assert {f[0]: getattr(ovo.stats, f[0]) for f in ovo.stats._fields_} == gvo.stats.as_dict(), k
        fo, fg = ovo.features(), gvo.features()
        assert np.array_equal(bits(fo[0]), bits(fg[0])) and np.array_equal(fo[1], fg[1]) and np.array_equal(fo[2], fg[2]), k
        assert np.abs(T_o - T_g).max() < 1e-6, k
        if len(fg[1]):
            max_age = max(max_age, int(fg[1].max()))
        if prev_ages is not None and (prev_ages >= 19).any():
            dropped_old = True
        prev_ages = fg[1].copy()
    assert max_age >= 20 and dropped_old          # the age gate was really exercised
    assert int(fg[1].max()) <= 20                  # nothing older than the threshold survives a bucketing


@pytest.mark.parametrize("seed,step,yaw,win", [(101, 0.25, 0.6, 21), (202, 0.6, 0.2, 10), (303, 0.1, 1.0, 15)])
def test_soak_sequences_stay_bit_exact(api, seed, step, yaw, win):
    """40 frames per seed with different speeds / yaw rates / windows, batched 2-wide on the GPU against two oracle
    instances: ok flags, counters and the whole feature set must match on every frame, poses within tolerance."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=416, height=176, cx=208.0, cy=88.0)
    seqs = [syn.StereoSequence(cal=cal, n_frames=40, seed=seed + i, step=step, yaw_amp_deg=yaw) for i in range(2)]
    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=win, win_h=win, max_translation_norm=2.0)
    ovos = []
    for _ in seqs:
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr); ovos.append(o)
    g = api.BatchVisualOdometry(416, 176, 2, api.default_config(**over)); g.initalize_projection_matricies(Pl, Pr)
    n_ok = 0
    for k in range(40):
        ok, T = g.stereo_callback_batch([s.left[k] for s in seqs], [s.right[k] for s in seqs])
        for i, o in enumerate(ovos):
            ok_o, T_o = o.stereo_callback(seqs[i].left[k], seqs[i].right[k])
            assert ok_o == bool(ok[i]), (k, i)
            assert {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_} == g.stats[i].as_dict(), (k, i)
            fo, fg = o.features(), g.features(i)
            assert np.array_equal(bits(fo[0]), bits(fg[0])) and np.array_equal(fo[1], fg[1]) and np.array_equal(fo[2], fg[2]), (k, i)
            assert np.abs(T_o[:3, 3] - T[i][:3, 3]).max() < POSE_TOL_T and rot_angle(T_o[:3, :3], T[i][:3, :3]) < POSE_TOL_R, (k, i)
            n_ok += int(ok_o)
    assert n_ok > 40                                    # the sequences really produce poses most of the time


class _Frames:
    """A rendered sequence with its images post-processed (contrast, noise, black bars) — same interface run_both uses."""
    def __init__(self, seq, left, right):
        self.cal, self.left, self.right = seq.cal, left, right


def test_full_size_properties_determinism_and_slot_independence(api):
    """Size-independent properties at BASELINE cfg2's full size, where the oracle is too slow to sit beside every frame:
      * determinism — the same frames through two fresh contexts give identical bits (poses, counters), run to run;
      * slot independence — a sequence's results do not depend on which slot of a batch it occupies or on what its neighbours
        are (the permuted batch returns the permuted results), nor on the batch size (1 vs 5);
      * a context that sees frame k twice in a row reports (numerically) no motion the second time."""
    from stereo_visual_odometry_amd import synthetic as syn
    cal = syn.KITTI00
    W, H = cal["width"], cal["height"]
    P = syn.projection_matrices(cal)
    seqs = [syn.StereoSequence(cal=cal, n_frames=4, seed=0x5EED0100 + s, step=0.5, cell_px=17.6, movers=0.3 if s % 2 else 0.0) for s in range(3)]
    over = dict(win_w=21, win_h=21, max_level=3, max_translation_norm=2.0)

    def run(order, n_frames=4):
        vo = api.BatchVisualOdometry(W, H, len(order), api.default_config(**over)); vo.initalize_projection_matricies(*P)
        out = []
        for k in range(n_frames):
            ok, T = vo.stereo_callback_batch([seqs[s].left[k] for s in order], [seqs[s].right[k] for s in order])
            out.append((ok.copy(), T.copy(), [st.as_dict() for st in vo.stats]))
        vo.close()
        return out

    a = run([0, 1, 2]); b = run([0, 1, 2])
    for (ok1, T1, s1), (ok2, T2, s2) in zip(a, b):
        assert np.array_equal(ok1, ok2) and np.array_equal(T1, T2) and s1 == s2                     # bit-identical, run to run
    perm = [2, 0, 1, 2, 1]
    c = run(perm)
    for k in range(4):
        for slot, s in enumerate(perm):
            assert c[k][0][slot] == a[k][0][s] and np.array_equal(c[k][1][slot], a[k][1][s]) and c[k][2][slot] == a[k][2][s], (k, slot)
    single = run([1])
    for k in range(4):
        assert np.array_equal(single[k][1][0], a[k][1][1]) and single[k][2][0] == a[k][2][1]
    assert all(x[0].all() for x in a[1:]) and a[1][2][0]["n_into_lk"] > 1500
    vo = api.BatchVisualOdometry(W, H, 1, api.default_config(**over)); vo.initalize_projection_matricies(*P)
    for k in (0, 1, 1):
        ok, T = vo.stereo_callback_batch([seqs[0].left[k]], [seqs[0].right[k]])
    assert ok[0] and np.abs(T[0] - np.eye(4)).max() < 1e-3


FUZZ_CASES = int(os.environ.get("SVO_FUZZ_CASES", "16"))          # the suite runs 16; SVO_FUZZ_CASES=400 for a one-off sweep
FUZZ_BATCH_CASES = int(os.environ.get("SVO_FUZZ_BATCH_CASES", "4"))  # many-sequence contexts; SVO_FUZZ_BATCH_CASES=100 for a sweep


@pytest.mark.parametrize("case", range(FUZZ_BATCH_CASES))
def test_fuzz_many_sequence_contexts(api, case):
    """Seeded random configurations of the MANY-SEQUENCE path (contexts of 9-14 sequences: pyramids of the next frame built ahead
    on a second stream into a fourth slot, strided second detection pass, 256-thread compaction): any LK window, 2-5 levels, 1-3
    frames in flight, two frame streams per context — one of them with black frames spliced in at random times (empty feature
    sets, second passes, stale pyramids, recoveries) — every sequence against the oracle, frame by frame."""
    from stereo_visual_odometry_amd import synthetic as syn
    import torch
    rng = np.random.default_rng(31000 + case)
    w, h = int(rng.choice([320, 352, 417])), int(rng.choice([160, 176, 203]))
    cal = dict(syn.KITTI00, width=w, height=h, cx=w / 2.0, cy=h / 2.0)
    NF = 6
    win = int(rng.choice([10, 15, 21, 21])) if case < 4 else int(rng.integers(5, 32))
    over = dict(win_w=win, win_h=win, max_level=int(rng.integers(1, 5)), fast_threshold=int(rng.choice([12, 20, 35])),
                ransac_iterations=int(rng.choice([50, 100])), lk_max_count=int(rng.choice([10, 30])), max_translation_norm=2.0)
    Pl, Pr = syn.projection_matrices(cal)
    streams = []
    for j in range(2):
        sq = syn.StereoSequence(cal=cal, n_frames=NF, seed=7000 + 2 * case + j, step=float(rng.uniform(0.1, 0.4)),
                                movers=float(rng.choice([0.0, 0.3])), cell_px=float(rng.uniform(10.0, 20.0)))
        L, R = list(sq.left), list(sq.right)
        if j == 1:
            black = np.zeros_like(L[0])
            for b in rng.choice(NF, size=int(rng.integers(1, 3)), replace=False):
                L[int(b)] = black; R[int(b)] = black
        streams.append((L, R))
    want = []
    for L, R in streams:
        o = orc.VisualOdometry(orc.default_config(**over)); o.initalize_projection_matricies(Pl, Pr)
        per = []
        for k in range(NF):
            ok, T = o.stereo_callback(L[k], R[k])
            per.append((ok, T.copy(), {f[0]: getattr(o.stats, f[0]) for f in o.stats._fields_}, [a.copy() for a in o.features()]))
        want.append(per)
    B, depth = int(rng.integers(9, 15)), int(rng.integers(1, 4))
    vo = api.BatchVisualOdometry(w, h, B, api.default_config(**over)); vo.initalize_projection_matricies(Pl, Pr)
    which = lambda i: (i * 7 + case) % 2
    dev = [[(torch.from_numpy(np.ascontiguousarray(L[k])).cuda(), torch.from_numpy(np.ascontiguousarray(R[k])).cuda()) for k in range(NF)] for L, R in streams]
    torch.cuda.synchronize()
    sub = 0
    for k in range(NF):
        while sub < NF and sub - k < depth:
            vo.submit_device([dev[which(i)][sub][0].data_ptr() for i in range(B)], [dev[which(i)][sub][1].data_ptr() for i in range(B)], w)
            sub += 1
        ok, T = vo.collect()
        for i in range(B):
            wnt = want[which(i)][k]
            sg = vo.stats[i].as_dict()
            assert bool(ok[i]) == wnt[0] and sg == wnt[2], (case, over, B, depth, k, i, sg, wnt[2])
            assert np.abs(T[i][:3, 3] - wnt[1][:3, 3]).max() < POSE_TOL_T and rot_angle(T[i][:3, :3], wnt[1][:3, :3]) < POSE_TOL_R
    for i in (0, 1, B - 1):
        f = vo.features(i); wnt = want[which(i)][NF - 1][3]
        assert np.array_equal(bits(f[0]), bits(wnt[0])) and np.array_equal(f[1], wnt[1]) and np.array_equal(f[2], wnt[2])
    vo.close()


@pytest.mark.parametrize("case", range(FUZZ_CASES))
def test_fuzz_scenes_and_configs(api, case):
    """Seeded random scenes x image degradations x configurations: high contrast (the wide LK reductions), low contrast
    (minimum-eigenvalue rejections), noise, black bars (windows over flat areas and borders), every window / level count,
    loose and strict thresholds.  Everything a frame produces must match the oracle on every frame."""
    from stereo_visual_odometry_amd import synthetic as syn
    rng = np.random.default_rng(9000 + case)
    w, h = int(rng.choice([320, 352, 417])), int(rng.choice([160, 176, 203]))
    cal = dict(syn.KITTI00, width=w, height=h, cx=w / 2.0, cy=h / 2.0)
    seq = syn.StereoSequence(cal=cal, n_frames=4, seed=500 + case, step=float(rng.uniform(0.1, 0.7)),
                             yaw_amp_deg=float(rng.uniform(0.0, 1.2)), cell_px=float(rng.uniform(9.0, 22.0)))
    gain, bias, sigma = float(rng.choice([0.35, 1.0, 1.0, 2.5])), float(rng.uniform(-20, 20)), float(rng.choice([0.0, 0.0, 2.0, 6.0]))
    bar = int(rng.choice([0, 0, 12, 30]))

    def degrade(img, k, cam):
        f = (img.astype(np.float64) - 128.0) * gain + 128.0 + bias
        if sigma > 0:
            f = f + np.random.default_rng(77 * case + 2 * k + cam).normal(0.0, sigma, img.shape)
        out = np.clip(np.rint(f), 0, 255).astype(np.uint8)
        if bar:
            out[:, :bar] = 0; out[-bar // 2:, :] = 255
        return out

    fr = _Frames(seq, [degrade(seq.left[k], k, 0) for k in range(4)], [degrade(seq.right[k], k, 1) for k in range(4)])
    win = int(rng.choice([7, 10, 15, 21, 31])) if case < 16 else int(rng.integers(5, 32))     # later cases: any window 5..31
    movers = 0.0 if case < 16 else float(rng.choice([0.0, 0.2, 0.4]))
    if movers:
        seq = syn.StereoSequence(cal=cal, n_frames=4, seed=500 + case, step=float(rng.uniform(0.1, 0.7)), movers=movers, mover_step=(0.3, 0.1),
                                 yaw_amp_deg=float(rng.uniform(0.0, 1.2)), cell_px=float(rng.uniform(9.0, 22.0)))
        fr = _Frames(seq, [degrade(seq.left[k], k, 0) for k in range(4)], [degrade(seq.right[k], k, 1) for k in range(4)])
    over = dict(win_w=win, win_h=win, max_level=int(rng.integers(1, 5)), fast_threshold=int(rng.choice([8, 20, 35])),
                ransac_iterations=int(rng.choice([20, 100, 250])), ransac_reprojection_error=float(rng.choice([1.0, 8.0])),
                optical_flow_min_eig_threshold=float(rng.choice([1e-4, 1e-3, 3e-2])),
                circular_matching_success_threshold=float(rng.choice([0.05, 0.15, 0.6])),
                lk_max_count=int(rng.choice([5, 30])), max_translation_norm=2.0)
    if case >= 8 and case % 4 == 3:                                  # a quarter of the cases: the float-sums LK (OpenCV's summation order)
        over["lk_float_sums"] = 1
    run_both(api, fr, over, 4)
