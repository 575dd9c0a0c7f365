"""The CPU oracle's detector (oracle/orc_fast.c, orc_bucket.c) held to tests/fast_ref.py, which is written from what FAST-9/16,
strict 3x3 non-max suppression and the bucket grid mean rather than from cv::FAST's arithmetic — and the conditions that keep
these comparisons (and the GPU ones of test_gpu_detect_edges.py, which use the same fixtures) from passing vacuously."""
import numpy as np
import pytest

import fast_ref as fr
import oracle_lib as orc
from gpu_kit import f32_bits as bits

NAMES = fr.case_names()
BIG = [n for n in NAMES if n != "seam" and fr.case_image(n).shape[0] >= 19]          # 19x67 and larger


def test_fixture_images_are_what_they_claim():
    assert len(NAMES) == 28 and len(set(NAMES)) == 28
    assert [fr.case_image(n).shape for n in NAMES[:9]] == fr.SIZES
    for n in NAMES:
        img = fr.case_image(n)
        assert img.dtype == np.uint8 and np.array_equal(img, dict(fr.cases())[n]), n          # seeded: the same on every call
        if n.startswith("sat"):
            assert set(np.unique(img)) <= {0, 1, 254, 255}
        if n.startswith("blk"):
            h, w = img.shape
            assert np.array_equal(img[0:h - h % 2:2], img[1:h:2]) and np.array_equal(img[:, 0:w - w % 2:2], img[:, 1:w:2])
    s = fr.case_image("seam")
    assert s.shape == fr.SEAM_SHAPE
    assert np.array_equal(s[:, 64:128], s[:, 63::-1]) and np.array_equal(s[16:32], s[15::-1])


@pytest.mark.parametrize("name", [n for n in NAMES if fr.case_image(n).size <= 7 * 64])
def test_reference_formulations_agree_on_small_images(name):
    """best arc's minimum |diff| - 1 against the literal scan over t'"""
    img = fr.case_image(name)
    max_t = fr.literal_max_threshold(img)
    for th in fr.THRESHOLDS:
        for nonmax in (True, False):
            a, b = fr.case_scores(name, th, nonmax), fr.fast_scores_literal(img, th, nonmax, max_t)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (th, nonmax)


def test_reference_on_images_below_seven_pixels_is_empty():
    for shape in ((6, 64), (64, 6), (3, 3)):
        score, kept = fr.fast_scores(np.full(shape, 7, np.uint8), 0)
        assert score.shape == shape and not score.any() and not kept.any()
        assert fr.fast_keypoints(np.zeros(shape, np.uint8), 5)[0].shape == (0, 2)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_score_maps_equal_the_definition(name):
    img = fr.case_image(name)
    for th in fr.THRESHOLDS:
        for nonmax in (True, False):
            assert np.array_equal(orc.fast_score_map(img, th, nonmax), fr.case_scores(name, th, nonmax)[0]), (th, nonmax)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_keypoints_equal_the_definition(name):
    img = fr.case_image(name)
    cap = img.size // 4 + 16                          # what orc.fast_detect allocates: without nonmax noise can exceed it
    for th in fr.THRESHOLDS:
        for nonmax in (True, False):                  # without nonmax a corner that scores 0 (th = 0) is still a keypoint
            xy, resp = orc.fast_detect(img, th, nonmax)
            wxy, wresp = fr.fast_keypoints(img, th, nonmax)
            assert nonmax is False or len(wxy) <= cap
            wxy, wresp = wxy[:cap], wresp[:cap]
            assert np.array_equal(bits(xy), bits(wxy)) and np.array_equal(bits(resp), bits(wresp)), (th, nonmax)


# ---------------------------------------------------------------- the fixtures really exercise what they are for
@pytest.mark.parametrize("name", [n for n in BIG if n.startswith(("rand", "blk"))])
def test_noise_and_block_images_keep_corners(name):
    for th in (-3, 0, 1, 5, 20):
        assert int(fr.case_scores(name, th)[1].sum()) >= 10, th


@pytest.mark.parametrize("name", [n for n in BIG if n.startswith("sat")])
def test_saturated_images_keep_a_corner_at_254_and_none_at_255(name):
    assert int(fr.case_scores(name, 254)[1].sum()) >= 1
    for th in (255, 300):
        assert not fr.case_scores(name, th)[1].any() and not fr.case_scores(name, th, False)[1].any()


def test_block_images_hold_plateaus_of_equal_score():
    for name in (n for n in BIG if n.startswith("blk")):
        raw = fr.case_scores(name, 5, False)[0].astype(int)
        assert int(((raw[:, :-1] == raw[:, 1:]) & (raw[:, :-1] > 0)).sum()) >= 5, name


@pytest.mark.parametrize("th", [5, 20])
def test_seam_image_ties_across_both_tile_seams(th):
    raw = fr.case_scores("seam", th, False)[0]
    kept = fr.case_scores("seam", th)[1]
    assert int(((raw[:, 63] == raw[:, 64]) & (raw[:, 63] > 0)).sum()) >= 5             # columns 63|64
    assert int(((raw[15] == raw[16]) & (raw[15] > 0)).sum()) >= 5                       # rows 15|16
    assert not kept[:, 63:65].any() and not kept[15:17].any()
    assert int(kept.sum()) >= 10


def test_a_corner_can_score_zero_at_threshold_zero():
    hit = 0
    for name in BIG:
        score, corner = fr.case_scores(name, 0, False)
        hit += int((corner & (score == 0)).sum())
    assert hit >= 1


# ---------------------------------------------------------------- bucket filter
# (per_bucket, (bah, baw, start_row), (w, h)): the grids of test_bucket_filter_parity, 1x1 at capacity 1, and a grid larger than
# the image (bucket size 1)
BUCKET_CASES = [(1, (92, 160, 4), (640, 360)), (3, (10, 12, 1), (640, 360)), (7, (1, 1, 0), (640, 360)), (2, (5, 9, 2), (640, 360)),
                (1, (1, 1, 0), (640, 360)), (1, (4, 8, 0), (64, 32)), (2, (20, 30, 1), (24, 16))]


def _filter_both(per, grid, size, trace=None):
    w, h = size
    xy, ages, st = fr.track_fixture(w, h, grid[0], grid[1], seed=3)
    got = orc.bucket_filter(w, h, xy, ages, st, grid[0], grid[1], grid[2], per, 20, 20)
    want = fr.bucket_filter(w, h, xy, ages, st, grid[0], grid[1], grid[2], per, 20, 20, trace=trace)
    return (xy, ages, st), got, want


@pytest.mark.parametrize("per,grid,size", BUCKET_CASES)
def test_oracle_bucket_filter_equals_the_sequential_restatement(per, grid, size):
    _, got, want = _filter_both(per, grid, size)
    assert len(want[1]) > 0
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_bucket_filter_on_the_negative_coordinate_inputs():
    """image 64x32, grid 4x8, capacity 1: (-0.5, 3) truncates to bucket (0, 0), comes first and is never strictly beaten"""
    xy = np.array(fr.NEGATIVE_TRACKS, np.float32)
    args = (64, 32, xy, np.zeros(4, np.int32), np.full(4, 40, np.int32), 4, 8, 0, 1, 20, 20)
    want = fr.bucket_filter(*args)
    assert want[0].tolist() == [[-0.5, 3.0]]
    got = orc.bucket_filter(*args)
    assert np.array_equal(bits(got[0]), bits(want[0]))


def test_bucket_fixture_has_inputs_where_truncation_and_floor_differ(monkeypatch):
    (xy, ages, st), _, want = _filter_both(3, (10, 12, 1), (640, 360))
    differ = [(s - 20) // 20 != fr._cdiv(s - 20, 20) for s in st.tolist()]
    assert sum(differ) >= 10 and (np.asarray(ages)[differ] < 20).any()
    monkeypatch.setattr(fr, "_cdiv", lambda a, b: a // b)            # and a flooring filter ends with another set
    floored = fr.bucket_filter(640, 360, xy, ages, st, 10, 12, 1, 3, 20, 20)
    assert not (np.array_equal(floored[0], want[0]) and np.array_equal(floored[2], want[2]))


def test_bucket_fixture_has_replacements_decided_by_ties():
    for per, grid, size in BUCKET_CASES[1:4]:
        trace = {}
        _filter_both(per, grid, size, trace)
        assert trace["tie_kept"] >= 1, (per, grid, trace)
    trace = {}
    _filter_both(3, (10, 12, 1), (640, 360), trace)
    assert trace["tie_first_min"] >= 1, trace


def test_bucket_fixture_holds_every_kind_of_edge_point():
    w, h, bah, baw = 640, 360, 10, 12
    xy, ages, st = fr.track_fixture(w, h, bah, baw, seed=3)
    bh, bw = -(-h // bah), -(-w // baw)
    x, y = xy[:, 0], xy[:, 1]
    assert ((x > -bw) & (x < 0)).any() and ((y > -bh) & (y < 0)).any() and (x <= -bw).any() and (y <= -bh).any()
    assert (np.signbit(x) & (x == 0)).any() and (np.signbit(y) & (y == 0)).any()
    assert (x >= baw * bw).any() and (y >= bah * bh).any() and (x == w - 1).any() and (y == h - 1).any()
    assert ((x > 0) & (x % bw == 0)).any() and ((y > 0) & (y % bh == 0)).any()
    assert (ages == 20).any() and (ages > 20).any() and (st < 20).any() and st.min() >= 0 and st.max() <= 255


def test_detect_for_frame_runs_the_second_pass_on_a_sparse_image():
    from types import SimpleNamespace
    import scenes
    cfg = SimpleNamespace(buckets_along_height=92, buckets_along_width=160, bucket_start_row=4, features_per_bucket=1,
                          age_threshold=20, fast_threshold=20, pre_matching_feature_threshold=100)
    img = scenes.make_empty_image(160, 320)
    for k in range(6):
        scenes.add_triangle(img, 30 + 45 * k, 30 + 20 * k, 8)
    xy, ages, st, second = fr.detect_for_frame(img, cfg)
    assert second and 0 < len(xy) < 100 and (ages == 0).all()
    # the oracle's chain (append at 20, then at 20 / 4 over the survivors)
    oxy, oresp = orc.fast_detect(img, 20)
    a = orc.bucket_filter(320, 160, oxy, np.zeros(len(oxy), np.int32), oresp.astype(np.int32))
    oxy, oresp = orc.fast_detect(img, 5)
    b = orc.bucket_filter(320, 160, np.concatenate([a[0], oxy]), np.concatenate([a[1], np.zeros(len(oxy), np.int32)]),
                          np.concatenate([a[2], oresp.astype(np.int32)]))
    assert np.array_equal(bits(b[0]), bits(xy)) and np.array_equal(b[2], st)
    dense = fr.detect_for_frame(scenes.random_texture(160, 320, 4, smooth=1), cfg)
    assert not dense[3] and len(dense[0]) >= 100
