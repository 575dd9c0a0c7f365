"""svo_describe_points on a real GPU against the numpy reference (tests/descriptor_ref.py, written from include/svo.h's "Binary
descriptors"): descriptors and orientation bins bit for bit — random, flat and ramp images at 64 x 48 and 67 x 19 (odd, barely above
the 16-pixel minimum), points on every corner and edge, at the centre rule's rounding seams, within 15 of two borders at once and
outside the image, a strided image, the counts at the kernel's four-points-per-block and 64-lane seams, and the refusals."""
import numpy as np
import pytest

import descriptor_ref as ref
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (67, 19)]


def edge_points(w, h):
    """the corners, points along every edge, the rounding seams, points near two borders at once, points outside the image"""
    p = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    p += [(x, 0) for x in range(1, w - 1, 7)] + [(x, h - 1) for x in range(2, w - 1, 7)]
    p += [(0, y) for y in range(1, h - 1, 3)] + [(w - 1, y) for y in range(2, h - 1, 3)]
    p += [(10.5, 7.5), (10.49999997, 7.49999997), (0.49999997, 0.49999997), (0.5, 0.5), (w - 1.5, h - 1.5), (w - 0.50000003, h - 0.6)]
    p += [(3, 2), (14, 14), (w - 3, 4), (5, h - 2), (w - 15, h - 15), (w - 4.25, h - 3.75)]
    p += [(-0.4, 5), (-7, -9), (w + 20, 3), (5, h + 0.2), (1e6, -1e6), (w - 0.5, h - 0.5)]
    return np.array(p, np.float32)


def check(api, img, xy):
    d, b = api.describe_points(img, xy)
    wd, wb = ref.describe(np.ascontiguousarray(img), xy)
    assert d.shape == (len(xy), 32) and d.dtype == np.uint8 and b.shape == (len(xy),)
    assert np.array_equal(b, wb), "bins differ at %s" % np.nonzero(b != wb)[0][:8]
    assert np.array_equal(d, wd), "descriptors differ at rows %s" % np.nonzero((d != wd).any(1))[0][:8]
    return d, b


@pytest.mark.parametrize("w,h", SIZES)
def test_random_image_at_every_kind_of_point(api, w, h):
    rng = np.random.default_rng(w)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    xy = np.concatenate([edge_points(w, h), rng.uniform(-2, [w + 2, h + 2], (60, 2)).astype(np.float32)])
    d, b = check(api, img, xy)
    assert len(np.unique(b)) > 10 and len(np.unique(d, axis=0)) > 50, "vacuous"
    assert api.last_stage_path() & api._lib.PATH_DESCRIPTORS


@pytest.mark.parametrize("w,h", SIZES)
def test_flat_image_and_the_tie_ramps(api, w, h):
    flat = np.full((h, w), 200, np.uint8)
    d, b = check(api, flat, edge_points(w, h))
    assert not b.any() and not d.any(), "a flat patch: bin 0 and no test is a strict less-than"
    rows = np.arange(h, dtype=np.uint8)[:, None]
    mid = np.array([[w // 2, h // 2]], np.float32) if h >= 31 else np.zeros((0, 2), np.float32)
    for img, want in ((np.repeat(60 + rows, w, 1), 7), (np.repeat(190 - rows, w, 1), 22)):
        _, b = check(api, img, np.concatenate([edge_points(w, h), mid]))
        if len(mid):
            assert b[-1] == want                                     # the whole patch inside the image: m10 = 0 exactly


def test_a_ramp_per_bin_centre_gives_every_bin(api):
    got = [int(check(api, ref.ramp(64, 48, k), np.array([[32, 24], [3, 40], [60.5, 2.5]], np.float32))[1][0]) for k in range(30)]
    assert got == list(range(30)), got


def test_strided_image(api):
    rng = np.random.default_rng(9)
    big = rng.integers(0, 256, (48, 96), dtype=np.uint8)
    img = big[:, 5:72]                                               # 67 wide, rows 96 bytes apart, an odd first byte
    assert img.strides[0] == 96 and not img.flags["C_CONTIGUOUS"]
    check(api, img, edge_points(67, 48))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257])
def test_counts_at_the_block_and_wave_seams(api, n):
    rng = np.random.default_rng(100 + n)
    img = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    xy = rng.uniform(0, [64, 48], (n, 2)).astype(np.float32)
    d, b = check(api, img, xy)
    assert len(d) == n


def test_refusals(api):
    L = api._lib
    img = np.zeros((48, 64), np.uint8)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(L.SvoError, match="status %d" % L.SVO_ERR_ARG):
            api.describe_points(img, np.array([[3, 3], [bad, 4]], np.float32))
    for shape in ((48, 15), (15, 48)):
        with pytest.raises(L.SvoError, match="status %d" % L.SVO_ERR_ARG):
            api.describe_points(np.zeros(shape, np.uint8), np.array([[3, 3]], np.float32))
    d, b = api.describe_points(np.zeros((16, 16), np.uint8), np.array([[0, 0], [15, 15]], np.float32))   # the minimum is legal
    assert d.shape == (2, 32) and not d.any()
