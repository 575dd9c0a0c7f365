"""The detection front on the GPU (FAST-9/16 scores, strict 3x3 NMS, the bucket grid; svo_kernels_img.hip) held to
tests/fast_ref.py — the detector written from its definition — at the edges a rewrite of the kernel goes wrong at: saturated
pixels with thresholds up to 255, threshold 0 and the clamped ends, images around the smallest one with an interior tile
(132x36), equal scores straddling a tile seam, 7-pixel images, padded rows, negative track coordinates, and every launch shape
the frame pipeline has for detection.  Where the CPU oracle computes the same thing its bytes are compared too.
test_fast_ref.py asserts on the reference alone that these fixtures hold the corners, ties and edge points they are for."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import fast_ref as fr
import oracle_lib as orc
import scenes
from gpu_kit import api, f32_bits as bits  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

NAMES = fr.case_names()


def same_features(got, want):
    return (len(got[1]) == len(want[1]) and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2], want[2]))


# ---------------------------------------------------------------- stage entry points
@pytest.mark.parametrize("name", NAMES)
def test_score_map_equals_the_definition(api, name):
    img = fr.case_image(name)
    for th in fr.THRESHOLDS:
        got = api.fastScoreMap(img, th)
        assert np.array_equal(got, fr.case_scores(name, th)[0]), th
        assert np.array_equal(got, orc.fast_score_map(img, th)), th


@pytest.mark.parametrize("name", NAMES)
def test_fast_detect_equals_the_definition(api, name):
    img = fr.case_image(name)
    for th in fr.THRESHOLDS:
        xy, resp = api.featureDetectionFast(img, th)
        wxy, wresp = fr.fast_keypoints(img, th)
        assert np.array_equal(bits(xy), bits(wxy)) and np.array_equal(bits(resp), bits(wresp)), th
        oxy, oresp = orc.fast_detect(img, th)
        assert np.array_equal(bits(xy), bits(oxy)) and np.array_equal(bits(resp), bits(oresp)), th


def _detect(api, buf, w, h, stride, th, cap, sentinel=-7.0):
    """svo_fast_detect into arrays eight entries longer than cap, pre-filled with a sentinel -> (n_out, xy, resp)"""
    xy = np.full((cap + 8, 2), sentinel, np.float32)
    resp = np.full(cap + 8, sentinel, np.float32)
    n = C.c_int(-1)
    api.check(api.lib.svo_fast_detect(0, api.ptr(buf), w, h, stride, int(th), cap, api.ptr(xy), api.ptr(resp), C.byref(n)))
    return n.value, xy, resp


@pytest.mark.parametrize("name", ["rand36x132", "rand40x200"])
def test_padded_rows_with_poisoned_padding(api, name):
    """stride = w + 5: the padding bytes (the complement of the pixel beside them, a corner-maker) must never be read as pixels"""
    img = fr.case_image(name)
    h, w = img.shape
    buf = np.empty((h, w + 5), np.uint8)
    buf[:, :w] = img
    buf[:, w:] = 255 - img[:, w - 5:]
    for th in (0, 5, 20, 128):
        want = fr.case_scores(name, th)[0]
        got = np.full((h, w), 0xCC, np.uint8)
        api.check(api.lib.svo_fast_score_map(0, api.ptr(buf), w, h, w + 5, th, api.ptr(got)))
        assert np.array_equal(got, want), th
        wxy, wresp = fr.fast_keypoints(img, th)
        n, xy, resp = _detect(api, buf, w, h, w + 5, th, len(wxy))
        assert n == len(wxy) and np.array_equal(bits(xy[:n]), bits(wxy)) and np.array_equal(bits(resp[:n]), bits(wresp)), th


@pytest.mark.parametrize("name", ["rand37x133", "seam"])
def test_fast_detect_capacity_below_the_count(api, name):
    """n_out is the true count whatever cap is; exactly min(n, cap) entries are written, in raster order"""
    img = fr.case_image(name)
    h, w = img.shape
    wxy, wresp = fr.fast_keypoints(img, 20)
    total = len(wxy)
    assert total >= 10
    for cap in (0, 1, total // 2, total - 1, total, total + 3):
        n, xy, resp = _detect(api, img, w, h, w, 20, cap)
        m = min(cap, total)
        assert n == total, cap
        assert np.array_equal(bits(xy[:m]), bits(wxy[:m])) and np.array_equal(bits(resp[:m]), bits(wresp[:m])), cap
        assert (xy[m:] == -7.0).all() and (resp[m:] == -7.0).all(), cap
    n = C.c_int(-1)                                   # cap 0 needs no arrays at all
    api.check(api.lib.svo_fast_detect(0, api.ptr(img), w, h, w, 20, 0, None, None, C.byref(n)))
    assert n.value == total


@pytest.mark.parametrize("shape", [(6, 64), (64, 6)])
def test_images_below_seven_pixels_are_an_argument_error(api, shape):
    img = np.zeros(shape, np.uint8)
    h, w = shape
    out = np.zeros(shape, np.uint8)
    assert api.lib.svo_fast_score_map(0, api.ptr(img), w, h, w, 20, api.ptr(out)) == api._lib.SVO_ERR_ARG
    n = C.c_int(-1)
    xy = np.zeros((8, 2), np.float32); resp = np.zeros(8, np.float32)
    assert api.lib.svo_fast_detect(0, api.ptr(img), w, h, w, 20, 8, api.ptr(xy), api.ptr(resp), C.byref(n)) == api._lib.SVO_ERR_ARG
    assert n.value == -1 and not xy.any()


# ---------------------------------------------------------------- svo_append_features_from_image
def _append(api, cfg, img, th, xy, ages, st):
    h, w = img.shape
    n0 = len(ages)
    cap = n0 + cfg.buckets_along_height * cfg.buckets_along_width * cfg.features_per_bucket + 64
    oxy = np.zeros((cap, 2), np.float32); oag = np.zeros(cap, np.int32); ost = np.zeros(cap, np.int32)
    oxy[:n0], oag[:n0], ost[:n0] = xy, ages, st
    n = C.c_int(n0)
    api.check(api.lib.svo_append_features_from_image(0, C.byref(cfg), api.ptr(np.ascontiguousarray(img)), w, h, w, int(th), cap,
                                                     C.byref(n), api.ptr(oxy), api.ptr(oag), api.ptr(ost)))
    assert 0 <= n.value <= cap
    return oxy[:n.value].copy(), oag[:n.value].copy(), ost[:n.value].copy()


def _append_ref(cfg, img, th, xy, ages, st):
    return fr.append_features(img, th, xy, ages, st, cfg.buckets_along_height, cfg.buckets_along_width, cfg.bucket_start_row,
                              cfg.features_per_bucket, cfg.age_threshold, cfg.fast_threshold)


# default: capacity 1, the atomicMax path.  features_per_bucket 3: the general walk.  4x8 from row 0: many candidates per bucket,
# ties on (score, input order) decide.
GRIDS = {"default": dict(), "per3": dict(features_per_bucket=3),
         "coarse": dict(buckets_along_height=4, buckets_along_width=8, bucket_start_row=0),
         "coarse_per3": dict(buckets_along_height=4, buckets_along_width=8, bucket_start_row=0, features_per_bucket=3)}


def _append_image(name):
    if name == "black":
        return np.zeros((32, 64), np.uint8)
    return fr.case_image(name)                        # 40x200 and 40x136: at least 32x136, larger than the LK window


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("name", ["rand40x200", "sat40x200", "blk40x200", "seam"])
def test_append_features_equals_the_definition(api, name, grid):
    """existing tracks on bucket edges, at negative and out-of-grid coordinates, of every age and strength, then the image's
    keypoints; at thresholds below cfg.fast_threshold the new keypoints' bucket scores are negative (truncation, not floor)"""
    img = _append_image(name)
    h, w = img.shape
    cfg = api.default_config(**GRIDS[grid])
    xy, ages, st = fr.track_fixture(w, h, cfg.buckets_along_height, cfg.buckets_along_width, seed=5)
    none = np.zeros(0, np.int32)
    for th in (0, 5, 20, 254):
        want = _append_ref(cfg, img, th, xy, ages, st)
        got = _append(api, cfg, img, th, xy, ages, st)
        assert len(want[1]) > 0 and same_features(got, want), (th, len(got[1]), len(want[1]))
        want = _append_ref(cfg, img, th, np.zeros((0, 2), np.float32), none, none)       # and from an empty set
        assert same_features(_append(api, cfg, img, th, np.zeros((0, 2), np.float32), none, none), want), th


@pytest.mark.parametrize("grid,kept", [("coarse", [(-0.5, 3.0)]), ("coarse_per3", [(-0.5, 3.0), (5.0, -0.25), (2.0, 2.0)])])
def test_append_features_truncates_negative_coordinates_toward_zero(api, grid, kept):
    """Image 64x32, grid 4x8 from row 0, tracks (-0.5, 3), (5, -0.25), (-8, 3), (2, 2), age 0, strength 40.  The bucket index is
    (int)(coordinate / bucket size): a coordinate in (-bucket, 0) truncates to 0 and the track is kept (bucket (0, 0), first
    come), one at -bucket or below is outside the grid.  Found failing on the capacity-1 path, whose offer_tracks() tested the
    float's sign and returned (2, 2); fixed to the integer test of the general walk."""
    cfg = api.default_config(**GRIDS[grid])
    img = _append_image("black")
    xy = np.array(fr.NEGATIVE_TRACKS, np.float32)
    ages, st = np.zeros(4, np.int32), np.full(4, 40, np.int32)
    want = _append_ref(cfg, img, 20, xy, ages, st)
    assert [tuple(p) for p in want[0].tolist()] == kept
    got = _append(api, cfg, img, 20, xy, ages, st)
    assert same_features(got, want), got[0].tolist()
    assert same_features(got, orc.bucket_filter(64, 32, xy, ages, st, 4, 8, 0, cfg.features_per_bucket))


@pytest.mark.parametrize("grid", ["default", "coarse"])
def test_append_features_bucket_score_truncates_toward_zero(api, grid, monkeypatch):
    """Capacity 1, where the score is computed in offer_tracks() (tracks) and in the FAST kernel (keypoints).  (strength - 20) / 20
    is 0 for strengths 1..19 under C's truncation and -1 under floor, so a weak newcomer beats a track of strength 0 (score -1)
    only when the division truncates.  Tracks against tracks on a black image, then threshold-5 keypoints against tracks."""
    cfg = api.default_config(**GRIDS[grid])
    bah, baw = cfg.buckets_along_height, cfg.buckets_along_width
    cases = []
    img = _append_image("black")
    bh, bw = -(-32 // bah), -(-64 // baw)
    centres = [(bw * c + 0.5 * bw, bh * r + 0.5 * bh) for r in range(cfg.bucket_start_row, bah, max(1, bah // 8)) for c in range(0, baw, max(1, baw // 8))]
    xy = np.repeat(np.array(centres, np.float32), 2, 0)              # per bucket: strength 0 first, then 1..19
    st = np.zeros(len(xy), np.int32); st[1::2] = 1 + np.arange(len(centres)) % 19
    cases.append((img, 20, xy, np.zeros(len(xy), np.int32), st))
    img = _append_image("rand40x200")
    kxy, resp = fr.fast_keypoints(img, 5)
    weak = kxy[resp < 20]                                            # a track of strength 0 on every weak keypoint
    assert len(weak) >= 10
    cases.append((img, 5, weak, np.zeros(len(weak), np.int32), np.zeros(len(weak), np.int32)))
    told_apart = []
    for img, th, xy, ages, st in cases:
        want = _append_ref(cfg, img, th, xy, ages, st)
        with monkeypatch.context() as m:
            m.setattr(fr, "_cdiv", lambda a, b: a // b)
            told_apart.append(not same_features(_append_ref(cfg, img, th, xy, ages, st), want))
        assert same_features(_append(api, cfg, img, th, xy, ages, st), want), th
    # the fixtures tell the two divisions apart (in the coarse grid a strong keypoint wins every bucket of the noise image)
    assert told_apart[0] and (told_apart[1] or grid == "coarse")


# ---------------------------------------------------------------- frame pipeline
FW, FH = 320, 160


def _frame(kind, seed):
    rng = np.random.default_rng([77, seed])
    if kind == "texture":
        return scenes.random_texture(FH, FW, 100 + seed, smooth=1)
    if kind == "sat":
        return fr.saturated(rng, FH, FW)
    img = scenes.make_empty_image(FH, FW)             # sparse: six triangles, fewer than 100 features -> second pass at 20 / 4,
    faint = scenes.make_empty_image(FH, FW)           # which alone sees the six faint ones (contrast 12, negative bucket scores)
    for k in range(6):
        scenes.add_triangle(img, 25 + 3 * seed + 45 * k, 28 + seed + 19 * k, 8)
        scenes.add_triangle(faint, 40 + 3 * seed + 45 * k, 120 + seed - 19 * k, 8)
    return np.maximum(img, faint // 10)


def _bgr(gray, seed):
    """three different planes; cv::FAST scans the first W BYTES of every interleaved row, which is what detection must see"""
    return np.stack([gray, np.roll(gray, 5 + seed, 1), 255 - gray], 2).copy()


def _detect_ref(cfg, img):
    view = SimpleNamespace(**{k: getattr(cfg, k) for k in ("buckets_along_height", "buckets_along_width", "bucket_start_row",
                                                           "features_per_bucket", "age_threshold", "fast_threshold",
                                                           "pre_matching_feature_threshold")})
    return fr.detect_for_frame(img, view)


def _check_frame(stats, tracks, ref, tag):
    xy, ages, st, second = ref
    assert stats.n_after_detect == len(xy) and stats.second_pass == int(second), (tag, stats.n_after_detect, len(xy), second)
    assert stats.n_into_lk == len(xy), tag
    known = set(bits(xy).view(np.uint64).ravel().tolist())
    pl0 = bits(tracks["pl0"]).view(np.uint64).ravel().tolist()
    assert len(pl0) == stats.n_after_bounds and set(pl0) <= known, tag          # (capacities above 1 can hold a keypoint twice)
    return len(pl0)


def _projection():
    from stereo_visual_odometry_amd import synthetic as syn
    return syn.projection_matrices(dict(syn.KITTI00, width=FW, height=FH, cx=FW / 2.0, cy=FH / 2.0))


LONE = {"four_levels": dict(), "three_levels": dict(max_level=2), "bgr": dict(), "per2": dict(features_per_bucket=2)}


@pytest.mark.parametrize("kind", ["texture", "sat", "sparse"])
@pytest.mark.parametrize("ctx", list(LONE))
def test_frame_detection_equals_the_definition(api, ctx, kind):
    """Two identical stereo frames: the second detects on the first's left image, from an empty feature set.  four_levels takes
    the fused front (k_front_a / k_front_b), three_levels the separate launches, bgr detects on the byte image, per2 the general
    walk over the score map."""
    cfg = api.default_config(max_translation_norm=5.0, **LONE[ctx])
    gray = _frame(kind, 1)
    left = _bgr(gray, 1) if ctx == "bgr" else gray
    right = scenes.shift_image(gray, -3, 0)
    right = _bgr(right, 1) if ctx == "bgr" else right
    vo = api.VisualOdometry(cfg=cfg); vo.initalize_projection_matricies(*_projection())
    vo.stereo_callback(left, right)
    assert vo.stats.fail_reason == 1
    vo.stereo_callback(left, right)
    fused = bool(vo.last_frame_path() & api._lib.PATH_FRONT_FUSED)
    assert fused == (ctx == "four_levels") and vo.pyramid_levels() == (3 if ctx == "three_levels" else 4)
    seen = np.ascontiguousarray(left.reshape(FH, -1)[:, :FW])
    ref = _detect_ref(vo.cfg, seen)
    assert ref[3] == (kind == "sparse") and len(ref[0]) > 0
    if kind == "sparse":
        assert (ref[2] < vo.cfg.fast_threshold).any() or ctx == "bgr"          # the second pass added keypoints of its own
    n = _check_frame(vo.stats, vo.last_tracks(), ref, (ctx, kind))
    if kind == "texture":
        assert n >= 50                                # the subset check is not vacuous
    vo.close()


def test_frame_detection_nine_sequences_with_different_images(api):
    """More than eight sequences: k_fast<0> with a block per tile and sequence and, for the sparse ones, the strided second-pass
    kernels.  Every sequence has another image, so a tile or grid row that lands in the wrong sequence shows."""
    B = 9
    kinds = ["texture", "sparse", "sat", "sparse", "texture", "sat", "sparse", "texture", "sparse"]
    lefts = [_frame(k, i) for i, k in enumerate(kinds)]
    rights = [scenes.shift_image(im, -3, 0) for im in lefts]
    cfg = api.default_config(max_translation_norm=5.0)
    vo = api.BatchVisualOdometry(FW, FH, B, cfg); vo.initalize_projection_matricies(*_projection())
    vo.stereo_callback_batch(lefts, rights)
    vo.stereo_callback_batch(lefts, rights)
    refs = [_detect_ref(cfg, im) for im in lefts]
    assert len({len(r[0]) for r in refs}) >= 6        # the sequences really differ
    for i in range(B):
        assert refs[i][3] == (kinds[i] == "sparse")
        n = _check_frame(vo.stats[i], vo.last_tracks(i), refs[i], (i, kinds[i]))
        assert n >= 50 or kinds[i] != "texture"
    vo.close()


# ---------------------------------------------------------------- more than eight sequences at features_per_bucket = 2
NINE_KINDS = ["texture", "sparse", "sat", "sparse", "texture", "sat", "sparse", "texture", "sparse"]
IDLE = (1, 4)


@pytest.fixture(scope="module")
def nine_per2(api):
    """Nine sequences with different images (the kinds of test_frame_detection_nine_sequences_with_different_images) at capacity
    2, the same stereo pair every frame: frame 2 detects from the empty set; frame 3 runs with sequences 1 and 4 idle; frame 4
    with all nine again.  Everything the tests look at is recorded here, with the references (computed once)."""
    B = len(NINE_KINDS)
    lefts = [_frame(k, i) for i, k in enumerate(NINE_KINDS)]
    rights = [scenes.shift_image(im, -3, 0) for im in lefts]
    cfg = api.default_config(max_translation_norm=5.0, features_per_bucket=2)
    refs = [_detect_ref(cfg, im) for im in lefts]
    cfg1 = api.default_config(max_translation_norm=5.0)
    sparse1 = [_detect_ref(cfg1, lefts[i]) for i in range(B) if NINE_KINDS[i] == "sparse"]
    vo = api.BatchVisualOdometry(FW, FH, B, cfg); vo.initalize_projection_matricies(*_projection())

    def snapshot():
        return dict(stats=list(vo.stats), tracks=[vo.last_tracks(i) for i in range(B)], feats=[vo.features(i) for i in range(B)])

    vo.stereo_callback_batch(lefts, rights)
    vo.stereo_callback_batch(lefts, rights)
    f2 = snapshot()
    active = [i not in IDLE for i in range(B)]
    vo.stereo_callback_batch(lefts, rights, active=active)
    f3 = snapshot()
    vo.stereo_callback_batch(lefts, rights)
    f4 = snapshot()
    vo.close()
    return SimpleNamespace(B=B, cfg=cfg, lefts=lefts, refs=refs, sparse1=sparse1, f2=f2, f3=f3, f4=f4)


def test_frame_detection_nine_sequences_two_per_bucket(nine_per2):
    """The general walk, the keypoint list and the block emit behind seq_of() at more than eight sequences; the four sparse
    sequences take the second pass.  The fixture tells capacity 2 from capacity 1: the reference gives 18 features with a second
    pass for every sparse sequence at capacity 2 (12 at capacity 1), 3994-4061 for the textures, 627-649 for the saturated."""
    t = nine_per2
    for i, k in enumerate(NINE_KINDS):
        n, second = len(t.refs[i][0]), t.refs[i][3]
        if k == "sparse":
            assert n == 18 and second, (i, n, second)
        elif k == "texture":
            assert 3994 <= n <= 4061 and not second, (i, n)
        else:
            assert 627 <= n <= 649 and not second, (i, n)
    assert [(len(r[0]), bool(r[3])) for r in t.sparse1] == [(12, True)] * 4
    for i, k in enumerate(NINE_KINDS):
        n = _check_frame(t.f2["stats"][i], t.f2["tracks"][i], t.refs[i], (i, k))
        assert n >= 50 or k != "texture"


def test_idle_sequences_keep_their_feature_set_and_grid(nine_per2):
    """Frame 3 with sequences 1 and 4 idle: the seven active ones detect what the reference detects from the feature set frame 2
    left them; the idle ones report fail_reason 5 and keep their set; their next active frame detects what the reference detects
    from that set — an idle frame leaves feature set and grid state alone."""
    t = nine_per2
    for i, k in enumerate(NINE_KINDS):
        if i in IDLE:
            assert t.f3["stats"][i].fail_reason == 5, i
            assert same_features(t.f3["feats"][i], t.f2["feats"][i]), i
            ref = fr.detect_for_frame(t.lefts[i], t.cfg, existing=t.f2["feats"][i])
            assert len(ref[0]) > 0
            _check_frame(t.f4["stats"][i], t.f4["tracks"][i], ref, (i, k, "after idle"))
        else:
            assert t.f3["stats"][i].fail_reason != 5, i
            ref = fr.detect_for_frame(t.lefts[i], t.cfg, existing=t.f2["feats"][i])
            assert len(ref[0]) > 0
            _check_frame(t.f3["stats"][i], t.f3["tracks"][i], ref, (i, k, "beside idle"))


# ---------------------------------------------------------------- svo_bucket_filter: the stage call's wrappers
def _stage_filter(api, w, h, xy, ages, st, bah, baw, start_row, per, age_thr, fast_thr):
    oxy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2).copy(); oag = np.ascontiguousarray(ages, np.int32).copy()
    ost = np.ascontiguousarray(st, np.int32).copy()
    n = C.c_int(len(oag))
    api.check(api.lib.svo_bucket_filter(0, w, h, C.byref(n), api.ptr(oxy), api.ptr(oag), api.ptr(ost), bah, baw, start_row, per, age_thr, fast_thr))
    assert 0 <= n.value <= len(oag)
    return oxy[:n.value].copy(), oag[:n.value].copy(), ost[:n.value].copy()


def test_bucket_filter_stage_call_equals_the_pipeline(api):
    """The stage call and the frame pipeline run one walk and one emit through two sets of wrappers: on the coarse_per3 grid with
    track_fixture they give the same set — the pipeline's taken through svo_append_features_from_image on a black image, so that
    the tracks are its whole input — and that set is the oracle's and the definition's."""
    cfg = api.default_config(**GRIDS["coarse_per3"])
    img = _append_image("black")
    h, w = img.shape
    bah, baw, row0, per = cfg.buckets_along_height, cfg.buckets_along_width, cfg.bucket_start_row, cfg.features_per_bucket
    xy, ages, st = fr.track_fixture(w, h, bah, baw, seed=5)
    want = fr.bucket_filter(w, h, xy, ages, st, bah, baw, row0, per, cfg.age_threshold, cfg.fast_threshold)
    assert per < len(want[1]) < len(ages)
    pipeline = _append(api, cfg, img, 20, xy, ages, st)
    stage = _stage_filter(api, w, h, xy, ages, st, bah, baw, row0, per, cfg.age_threshold, cfg.fast_threshold)
    assert same_features(stage, pipeline)
    assert same_features(stage, orc.bucket_filter(w, h, xy, ages, st, bah, baw, row0, per, cfg.age_threshold, cfg.fast_threshold))
    assert same_features(stage, want)


@pytest.mark.parametrize("start_row,n_out", [(0, 96), (1, 72)])
def test_bucket_filter_every_bucket_full(api, start_row, n_out):
    """64x32, grid 4x8 of 8x8 buckets, five candidates in every bucket at capacity 3: 96 outputs in one call — more than a wave,
    fewer than the emit's block — and, with start_row = 1, an empty grid row 0 in front of the rest."""
    rng = np.random.default_rng(9)
    w, h, bah, baw, per = 64, 32, 4, 8, 3
    cells = np.array([(8 * c, 8 * r) for r in range(bah) for c in range(baw)], np.float32)
    xy = (np.repeat(cells, 5, 0) + rng.uniform(0, 7.99, (5 * len(cells), 2))).astype(np.float32)
    ages = rng.integers(0, 4, len(xy)).astype(np.int32)
    st = rng.integers(0, 256, len(xy)).astype(np.int32)
    order = rng.permutation(len(xy))
    xy, ages, st = xy[order], ages[order], st[order]
    want = orc.bucket_filter(w, h, xy, ages, st, bah, baw, start_row, per, 20, 20)
    assert len(want[1]) == n_out
    got = _stage_filter(api, w, h, xy, ages, st, bah, baw, start_row, per, 20, 20)
    assert same_features(got, want), (len(got[1]), n_out)
    assert same_features(got, fr.bucket_filter(w, h, xy, ages, st, bah, baw, start_row, per, 20, 20))
