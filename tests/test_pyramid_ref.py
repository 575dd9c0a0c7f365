"""The numpy pyramid reference (tests/pyramid_ref.py) against the CPU oracle's buildOpticalFlowPyramid, and its border rule
against a scalar restatement of cv::borderInterpolate.  No GPU needed: the GPU pyramid tests lean on this reference."""
import numpy as np
import pytest

import oracle_lib as orc
import pyramid_ref as ref


def border_interpolate(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), the scalar loop as OpenCV writes it (delta = 1)."""
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while True:
        p = -p if p < 0 else 2 * n - 2 - p
        if 0 <= p < n:
            return p


def texture(w, h, seed):
    """Noise over a smooth ramp: every tap of the 5x5 kernel matters, and the sums cover the whole range."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0)
    return np.clip(base + rng.integers(-60, 61, (h, w)), 0, 255).astype(np.uint8)


def test_border_rule_is_border_interpolate():
    for n in range(1, 49):
        for pad in (12, 24, 40):
            i = np.arange(-pad, n + pad)
            got = ref.reflect101(i, n)
            want = [border_interpolate(int(k), n) for k in i]
            assert got.tolist() == want, (n, pad)


def test_padded_level_is_the_indexed_level():
    rng = np.random.default_rng(5)
    for w, h in ((6, 12), (12, 6), (1, 3), (17, 2), (40, 33)):
        lv = rng.integers(0, 256, (h, w)).astype(np.uint8)
        pad = 28
        p = ref.padded(lv, pad)
        assert p.shape == (h + 2 * pad, w + 2 * pad)
        assert np.array_equal(p[pad:pad + h, pad:pad + w], lv)
        for y in range(-pad, h + pad, 5):
            for x in range(-pad, w + pad, 3):
                assert p[y + pad, x + pad] == lv[border_interpolate(y, h), border_interpolate(x, w)], (w, h, x, y)


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_reference_equals_oracle_pyramid(shape):
    w, h = shape
    img = texture(w, h, w + h)
    for win in ref.WINDOWS:
        if w <= win or h <= win:
            continue
        full = ref.pyramid(img, win, 5)
        for max_level in range(6):
            o = orc.Pyramid(img, (win, win), max_level)
            n = len(ref.level_sizes(w, h, win, max_level))
            assert o.nlevels == n, (shape, win, max_level)
            for lv in range(n):
                assert np.array_equal(full[lv], o.level(lv)), (shape, win, max_level, lv)


def test_bgr_and_raw_frames():
    import rectify_ref
    bgr = np.stack([texture(90, 46, s) for s in (1, 2, 3)], -1)
    p = ref.pyramids(bgr, 5, 3)
    assert len(p) == 3 and all(len(x) == 4 for x in p)
    for c in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(p[c], ref.pyramid(bgr[:, :, c].copy(), 5, 3)))
    raw = texture(100, 60, 9)
    K = [[80.0, 0, 50.0], [0, 80.0, 30.0], [0, 0, 1]]
    maps = rectify_ref.init_rectify_map(K, [-0.1, 0.01, 0, 0, 0], None, None, 90, 46)
    got = ref.pyramids(raw, 5, 3, maps)[0]
    want = ref.pyramid(rectify_ref.remap(raw, *maps), 5, 3)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
