"""The numpy derivative-plane reference (tests/deriv_ref.py) against the CPU oracle's calcScharrDeriv (orc_scharr), bit for bit, and
the guard of the case matrix the GPU test runs.  No GPU needed: tests/test_gpu_deriv_planes.py leans on this reference."""
import ctypes as C

import numpy as np
import pytest

import deriv_ref as ref
import oracle_lib as orc
import pyramid_ref
import test_gpu_pyramids as tp
from test_pyramid_ref import texture


def oracle_scharr(level):
    """(dx, dy) of orc_scharr on one packed level, int64 (h, w)."""
    level = np.ascontiguousarray(level, np.uint8)
    h, w = level.shape
    out = np.full((h, w, 2), 0x5555, np.int16)
    orc.lib().orc_scharr(level.ctypes.data_as(C.c_void_p), w, h, w, out.ctypes.data_as(C.c_void_p), 2 * w)
    return out[:, :, 0].astype(np.int64), out[:, :, 1].astype(np.int64)


def assert_four_times_the_oracle(level, what):
    ix, iy = ref.scharr4(level)
    ox, oy = oracle_scharr(level)
    assert np.array_equal(ix, 4 * ox) and np.array_equal(iy, 4 * oy), what
    return ix, iy


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_reference_is_four_times_the_oracle_scharr(case):
    (w, h), win, ml, B, inp, ex, chain = case
    levels = pyramid_ref.pyramid(texture(w, h, w + h), win, ml)
    assert len(levels) >= 2
    for lv in range(1, len(levels)):
        assert_four_times_the_oracle(levels[lv], (case, lv))


def checkerboard(w, h, square):
    y, x = np.mgrid[0:h, 0:w]
    return (255 * ((x // square + y // square) & 1)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(67, 35), (64, 16), (17, 9), (33, 13), (3, 3)])
def test_synthetic_images(shape):
    """All 0 and all 255 differentiate to zero; a 0/255 checkerboard of 3 x 3 squares reaches both ends of the range (a board of single
    pixels has equal columns x - 1 and x + 1: its derivatives vanish, which is checked too)."""
    w, h = shape
    for v in (0, 255):
        ix, iy = assert_four_times_the_oracle(np.full((h, w), v, np.uint8), (shape, v))
        assert not ix.any() and not iy.any()
    ix, iy = assert_four_times_the_oracle(checkerboard(w, h, 1), (shape, "pixels"))
    assert not ix.any() and not iy.any()
    ix, iy = assert_four_times_the_oracle(checkerboard(w, h, 3), (shape, "squares"))
    if w >= 9 and h >= 9:
        assert ix.max() == ref.BOUND and ix.min() == -ref.BOUND and iy.max() == ref.BOUND and iy.min() == -ref.BOUND


def test_planes_embed_the_derivatives_in_zeros():
    lv = texture(21, 10, 3)
    ix, iy = ref.scharr4(lv)
    for pad in (12, 40):
        px, py = ref.planes(lv, pad)
        assert px.dtype == np.int16 and px.shape == py.shape == (10 + 2 * pad, 21 + 2 * pad)
        for p, d in ((px, ix), (py, iy)):
            assert np.array_equal(p[pad:pad + 10, pad:pad + 21], d)
            q = p.copy(); q[pad:pad + 10, pad:pad + 21] = 0
            assert not q.any()
    # the edge samples differentiate the REFLECT_101 border: column -1 is column 1, so Ix vanishes in the first and last column
    assert not ix[:, 0].any() and not ix[:, -1].any() and not iy[0, :].any() and not iy[-1, :].any()
    assert ix[:, 1:-1].any() and iy[1:-1, :].any()


def test_case_matrix_covers_the_edges():
    """The level chains are the ones the stop rule builds, and between them they hold what k_deriv_levels can get wrong: every width
    residue mod 4 (the tail stores), a level narrower than a 64-wide tile, widths of exactly 64, 65 and 129 (a last tile column of one
    sample), a level wider than 256, heights of exactly 16 and 17 and one below 16, pyramids of 2 and of 5 levels (the tile-to-level
    walk), every pad; and the variants: inputs, frames in flight, a masked frame, a reset, the three other ingest kernels, the bench
    shape.  A later edit cannot make the matrix vacuous."""
    widths, heights, nlevels, pads = set(), set(), set(), set()
    for (w, h), win, ml, B, inp, ex, chain in ref.CASES:
        assert 9 <= B <= 12
        sizes = pyramid_ref.level_sizes(w, h, win, ml)
        assert sizes[1:] == chain and len(chain) >= 1, ((w, h), win, ml, sizes)
        nlevels.add(len(sizes))
        pads.add(tp.lk_pad_for(win))
        widths |= {lw for lw, lh in chain}
        heights |= {lh for lw, lh in chain}
        assert 2 <= ex["frames"] <= 5 and (ex["frames"] >= 3 or (w, h) == (1241, 376))
    assert {lw % 4 for lw in widths} == {0, 1, 2, 3}
    assert min(widths) < 64 and {64, 65, 129} <= widths and max(widths) > 256
    assert {16, 17} <= heights and min(heights) < 16
    assert {2, 5} <= nlevels
    assert pads >= {12, 16, 24, 28, 40}
    inputs = {c[4] for c in ref.CASES}
    assert {"host", "pinned"} <= inputs and any(i.startswith("dev") for i in inputs)
    assert {c[5].get("depth", 1) for c in ref.CASES if c[4].startswith("dev")} == {1, 2, 3}
    for key in ("mask", "reset", "rect", "fmt", "clahe"):
        assert any(key in c[5] for c in ref.CASES), key
    assert any(c[5].get("fmt") == "bgr8" for c in ref.CASES)
    assert any("mask" in c[5] and c[4].startswith("dev") for c in ref.CASES) and any("mask" in c[5] and not c[4].startswith("dev") for c in ref.CASES)
    bench = [c for c in ref.CASES if c[0] == (1241, 376)]
    assert len(bench) == 1 and bench[0][1:4] == (21, 4, 9) and bench[0][5]["frames"] == 2
    assert bench[0][6] == [(621, 188), (311, 94), (156, 47), (78, 24)]
