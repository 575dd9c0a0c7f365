"""The guard of the case matrix tests/test_gpu_front_batch.py runs (tests/front_batch_cases.py): the tile constants of the
many-sequence front, restated, and the sizes they make special, so that a later edit cannot empty the matrix.  No GPU needed."""
import re
import os

import numpy as np

import front_batch_cases as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "stereo_visual_odometry_amd", "csrc", "svo_kernels_img.hip")


def test_the_restated_tile_constants_are_the_kernels():
    text = open(SRC).read()
    define = lambda name: int(re.search(r"^#define %s (\d+)\s*$" % name, text, re.M).group(1))
    assert (define("FB_W"), define("FB_H")) == (fb.FAST_TW, fb.FAST_TH)
    assert (define("DV_VEC"), define("DV_ROWS")) == (fb.PLANE_V, fb.PLANE_ROWS)
    assert re.search(r"__launch_bounds__\(256\) void k_fast_batch\(", text) and fb.FAST_THREADS == 256
    assert int(re.search(r"^#define SVO_LONE_MAX_SEQ (\d+)", open(os.path.join(os.path.dirname(SRC), "svo_internal.hpp")).read(), re.M).group(1)) == 8


def test_the_contexts_are_the_smallest_many_sequence_ones():
    assert all(9 <= c[3] <= 12 for c in fb.CASES) and {c[3] for c in fb.CASES} >= {9, 10, 11, 12}
    assert all(len(fb.levels_of(c)) >= 2 for c in fb.CASES), "a case without a level >= 1 keeps no planes"


def test_level_0_hits_the_fast_tile_edges():
    """Widths and heights of k T - 1, k T and k T + 1 of the FAST tile."""
    assert {c[0][0] % fb.FAST_TW for c in fb.CASES} >= {fb.FAST_TW - 1, 0, 1}
    assert {c[0][1] % fb.FAST_TH for c in fb.CASES} >= {fb.FAST_TH - 1, 0, 1}
    assert any(c[0][0] > 2 * fb.FAST_TW and c[0][1] > 2 * fb.FAST_TH for c in fb.CASES), "no image with an interior tile"
    assert any(c[0][1] <= 2 * fb.FAST_TH for c in fb.CASES) and any(c[0][0] < 2 * fb.FAST_TW for c in fb.CASES)


def test_the_levels_hit_the_plane_vector_edges():
    """Levels >= 1: vector counts of k V - 1, k V, k V + 1 samples from the vectors' origin (x = -(pad & 7)) and from x = 0, row
    counts of k R - 1, k R, k R + 1, every width residue mod 4 and mod V, a level narrower than one vector, one shorter than the rows
    a thread walks, one narrower than the pad, and both vector origins (pad = 0 and 4 mod 8)."""
    V, R = fb.PLANE_V, fb.PLANE_ROWS
    from_origin, from_zero, rows, mod4, origins = set(), set(), set(), set(), set()
    narrow = short = below_pad = False
    for c in fb.CASES:
        pad = fb.lk_pad_for(c[1])
        assert pad >= 8 and pad % 4 == 0
        origins.add(pad & 7)
        for w, h in fb.levels_of(c)[1:]:
            from_origin.add((w + (pad & 7)) % V); from_zero.add(w % V); rows.add(h % R); mod4.add(w % 4)
            narrow |= w < V
            short |= h < R
            below_pad |= w < pad
    assert from_origin == set(range(V)) and from_zero == set(range(V)) and mod4 == {0, 1, 2, 3}
    assert rows >= {R - 1, 0, 1}
    assert narrow and short and below_pad and origins == {0, 4}


def test_the_streams_hold_what_they_are_for():
    kinds = {k for c in fb.CASES for k in c[4]}
    assert kinds == {"scene", "dots", "dense", "black"}
    for c in fb.CASES:
        (w, h), win, ml, B, ks = c
        for j, kind in enumerate(ks):
            if kind == "scene":
                continue
            L, R = fb.stream(kind, w, h, 1000 * win + 31 * j + w)
            assert len(L) == len(R) == fb.N_FRAMES and all(a.shape == (h, w) and a.dtype == np.uint8 for a in L + R)
            if kind == "black":
                assert not L[0].any() and not R[0].any()
            if kind == "dense":                                       # a tile queues more candidates than its block has threads
                assert fb.screen_count_max(L[0]) > fb.FAST_THREADS, fb.case_id(c)
            if kind == "dots":                                        # bright pixels on both sides of the margin and of every seam, on both axes
                bright = L[0] >= 150
                for x in fb.special_columns(w, fb.FAST_TW):
                    assert bright[:, x].any(), (fb.case_id(c), "column", x)
                for y in fb.special_columns(h, fb.FAST_TH):
                    assert bright[y, :].any(), (fb.case_id(c), "row", y)
                assert {2, 3, w - 4, w - 3} <= set(fb.special_columns(w, fb.FAST_TW))
    assert any(c[0][0] > fb.FAST_TW and "dots" in c[4] for c in fb.CASES) and any(c[0][1] > fb.FAST_TH and "dots" in c[4] for c in fb.CASES)
