"""tests/input_format_ref.py (the numpy side of the input-format tests) against the committed fixtures: its BGR formula gives
the grey frames of run1_frames_0_7.npz from the colour fixture byte for byte — the same restatement of cv::cvtColor BGR2GRAY as
tests/golden/make_run1_fixture.py and tools/svo_cli.cpp --gray 1 — and every other format is tied to that one."""
import os

import numpy as np
import pytest

import golden_run1
import input_format_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def bgr():
    return golden_run1.bgr_frames(8)


def test_bgr8_equals_the_committed_grey_fixture(bgr):
    d = np.load(os.path.join(GOLD, "run1_frames_0_7.npz"))
    for cam, frames in zip(("left", "right"), bgr):
        for k in range(8):
            assert np.array_equal(ref.to_grey(frames[k], "bgr8"), d[cam][k]), (cam, k)


def test_formula_on_the_extremes():
    px = lambda b, g, r: ref.to_grey(np.array([[[b, g, r]]], np.uint8), "bgr8")[0, 0]
    assert px(0, 0, 0) == 0 and px(255, 255, 255) == 255                # the weights sum to 2^14
    assert px(255, 0, 0) == (255 * 1868 + 8192) >> 14 and px(0, 255, 0) == (255 * 9617 + 8192) >> 14 and px(0, 0, 255) == (255 * 4899 + 8192) >> 14
    assert ref.WB + ref.WG + ref.WR == 1 << ref.SHIFT


def test_rgb_is_bgr_with_the_channels_swapped(bgr):
    a = bgr[0][3]
    assert np.array_equal(ref.to_grey(np.ascontiguousarray(a[:, :, ::-1]), "rgb8"), ref.to_grey(a, "bgr8"))
    assert not np.array_equal(ref.to_grey(a, "rgb8"), ref.to_grey(a, "bgr8"))        # the frames are not grey: the order matters


def test_alpha_is_ignored(bgr):
    a = bgr[1][5]
    rng = np.random.default_rng(4)
    for alpha in (np.zeros(a.shape[:2], np.uint8), rng.integers(0, 256, a.shape[:2]).astype(np.uint8)):
        bgra = np.concatenate([a, alpha[..., None]], -1)
        rgba = np.concatenate([a[:, :, ::-1], alpha[..., None]], -1)
        assert np.array_equal(ref.to_grey(bgra, "bgra8"), ref.to_grey(a, "bgr8"))
        assert np.array_equal(ref.to_grey(rgba, "rgba8"), ref.to_grey(a, "bgr8"))


def test_yuv422_picks_the_stated_byte():
    rng = np.random.default_rng(5)
    row = rng.integers(0, 256, (7, 2 * 13)).astype(np.uint8)          # 13 pixels of 2 bytes per row
    f = row.reshape(7, 13, 2)
    assert np.array_equal(ref.to_grey(f, "yuv422"), row[:, 1::2])     # UYVY: byte 2x + 1
    assert np.array_equal(ref.to_grey(f, "yuv422_yuy2"), row[:, 0::2])   # YUY2: byte 2x


def test_mono8_is_the_byte_and_shapes_are_checked():
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(ref.to_grey(a, "mono8"), a)
    with pytest.raises(AssertionError):
        ref.to_grey(a, "bgr8")
    with pytest.raises(AssertionError):
        ref.to_grey(np.zeros((3, 4, 3), np.uint8), "bgra8")


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_colour_of_round_trips(fmt):
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, (19, 23)).astype(np.uint8)
    f, g = ref.colour_of(a, fmt, rng)
    assert f.shape == (19, 23) + ((ref.BPP[fmt],) if fmt != "mono8" else ()) and np.array_equal(ref.to_grey(f, fmt), g)
    assert np.array_equal(g, ref.colour_of(a, "bgr8", rng)[1])
