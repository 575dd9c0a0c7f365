"""svo_desc_index_read_rows (include/svo.h, "Landmark consolidation") on the GPU: the rows read back equal, byte for byte, the arrays
that went in — after add, add_points, truncate, retire and transform_points; over spans of 4 095, 4 096, 4 097 and 8 193 rows, the
seams of the 4096-row staging; with each output left out in turn; on an index without points; and the refusals."""
import numpy as np
import pytest

import consolidate_ref as cr
import desc_retire_ref as rr
from gpu_kit import api  # noqa: F401  (the fixture is found by name)
from test_gpu_desc_retire import make_index, refused

pytestmark = pytest.mark.gpu


def test_after_add_add_points_truncate_retire_and_transform(api):
    case = rr.index_case(600, seed=1)                 # every 11th row has no point: fill goes through add and add_points in turn
    ix = make_index(api, case)
    try:
        assert not cr.same_rows(ix.read_rows(), cr.as_read(case))
        assert not cr.same_rows(ix.read_rows((130, 131)), tuple(a[130:131] for a in cr.as_read(case)))
        assert all(len(a) == 0 for a in ix.read_rows((77, 77)))
        ix.truncate(500)
        now = {k: v[:500] for k, v in case.items()}
        assert not cr.same_rows(ix.read_rows(), cr.as_read(now))
        keep, kept_before = rr.retire(now["ids"], now["tags"], (20, 480), tag_window=(1, 5), latest_per_id=True)
        assert ix.retire(rows=(20, 480), tags=(1, 5), latest_per_id=True).tolist() == kept_before.tolist()
        now = {k: v[keep] for k, v in now.items()}
        assert 100 < len(now["ids"]) < 450 and not cr.same_rows(ix.read_rows(), cr.as_read(now))
        T = np.eye(4); T[:3, 3] = (1.5, -2.25, 3.0); T[0, 1] = 0.125
        now["xyz"], moved, _ = rr.transform(now["xyz"], now["tags"], T, (10, 120), (0, 3))
        assert ix.transform_points(T, rows=(10, 120), tags=(0, 3))[0] == moved > 0
        assert not cr.same_rows(ix.read_rows(), cr.as_read(now))
        assert not cr.same_rows(ix.read_rows((33, 140)), tuple(a[33:140] for a in cr.as_read(now)))
    finally:
        ix.close()


def test_the_stagings_seams_and_each_output_left_out(api):
    n = 8193 + 5
    case = cr.index_case(n, views=3, seed=2, none_every=0)
    case["tags"][4000:4100] = np.arange(100)
    ix = make_index(api, case)
    want = cr.as_read(case)
    try:
        for lo, m in ((0, 4095), (1, 4096), (2, 4097), (5, 8193), (0, n)):
            assert not cr.same_rows(ix.read_rows((lo, lo + m)), tuple(a[lo:lo + m] for a in want)), (lo, m)
        names = ("desc", "ids", "xyz", "tags")
        for left_out in names:
            got = ix.read_rows((3, 4200), want=[k for k in names if k != left_out])
            for k, g, w in zip(names, got, want):
                assert (g is None) if k == left_out else np.array_equal(g.view(np.uint8), w[3:4200].view(np.uint8)), (left_out, k)
        assert api._lib.lib.svo_desc_index_read_rows(ix._h, 0, -1, None, None, None, None) == api._lib.SVO_OK
    finally:
        ix.close()


def test_an_index_without_points_and_the_refusals(api):
    L = api._lib
    case = rr.index_case(300, seed=3, points=False)
    ix = make_index(api, case, points=False)
    try:
        d, i, x, t = ix.read_rows(want=("desc", "ids"))
        assert x is None and t is None and np.array_equal(d, case["desc"]) and np.array_equal(i, case["ids"])
        refused(api, L.SVO_ERR_STATE, ix.read_rows)
        refused(api, L.SVO_ERR_STATE, ix.read_rows, (0, -1), ("tags",))
        refused(api, L.SVO_ERR_STATE, ix.read_rows, (0, -1), ("desc", "xyz"))
        for lo, hi in ((-1, 5), (5, 3), (0, 301), (301, -1), (0, -2)):
            guard = np.full((8, 32), 0xAB, np.uint8)
            assert L.lib.svo_desc_index_read_rows(ix._h, lo, hi, L.ptr(guard), None, None, None) == L.SVO_ERR_ARG and (guard == 0xAB).all()
        assert L.lib.svo_desc_index_read_rows(None, 0, -1, None, None, None, None) == L.SVO_ERR_ARG
    finally:
        ix.close()
