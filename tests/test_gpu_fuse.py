"""The descriptor index's landmark fusion (include/svo.h, "Landmark fusion": svo_desc_index_match_near, svo_desc_index_pair_near,
svo_desc_index_relabel, svo_desc_index_fuse) on a real GPU against the numpy reference (tests/fuse_ref.py) on the synthetic rows of
tests/fuse_cases.py.  Every rule is integers and f32 compares on points that sit on a 0.25 lattice, so every comparison is equality,
bit for bit.  An index has no call that returns its ids: where every row's descriptor is its own, a search for the descriptors over
the whole index returns each row with its id, which is how the ids are read; the points are read through two projections."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import fuse_cases as fc
import fuse_ref as fr
import reloc_ref as rref
from stereo_visual_odometry_amd import _lib, api

pytestmark = pytest.mark.gpu


def ids_of(index, desc):
    """the ids of an index whose rows' descriptors are all different, with the check that rows and descriptors are where they were"""
    rows = index.match(desc)
    assert np.array_equal(rows["row"], np.arange(len(desc))) and not rows["dist"].any()
    return rows["id"].copy()


def points_of(index):
    """the rows' points as two projections show them (x / z, y / z and z / x, y / x after a shift that puts every point in front);
    a row without a point is (+inf, +inf)"""
    K = np.eye(3, dtype=np.float32)
    swap = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float64)
    return index.project(K, np.eye(3), [0, 0, 5.0]).tobytes() + index.project(K, swap, [0, 0, 5.0]).tobytes()


# ---- 1. match_near
@pytest.mark.parametrize("n, d", fc.NEAR_SIZES)
def test_match_near_equals_the_reference(n, d):
    c = fc.near_scene(n, d)
    index = ac.build_index(api, c)
    for radius in fc.RADII:
        want = fr.match_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], radius)
        for chunk in (64, 0):
            index.chunk_rows = chunk
            got = index.match_near(c["src"], c["dst"], radius)
            assert len(got) == n and got.tobytes() == want.tobytes(), (radius, chunk)
    if n >= 1 and d >= 4:                              # the planted rows: at the radius, one ulp beyond, at it on z, coincident
        d0 = c["dst"][0]
        assert index.match_near(c["src"], (d0, d0 + 2), 0.5)[0]["row"] == d0 and index.match_near(c["src"], (d0 + 1, d0 + 2), 0.5)[0]["row"] == -1
        assert index.match_near(c["src"], (d0 + 2, d0 + 3), 0.5)[0]["row"] == d0 + 2 and index.match_near(c["src"], (d0, d0 + 4), 0.0)[0]["row"] == d0 + 3


def test_match_near_with_everything_admitted_is_match_rows():
    c = fc.near_scene(200, 1000, all_points=True)
    index = ac.build_index(api, c)
    for chunk in (64, 0):
        index.chunk_rows = chunk
        assert index.match_near(c["src"], c["dst"], 100.0).tobytes() == index.match_rows(c["src"], c["dst"]).tobytes()
    m = len(c["desc"])                                 # the source span in front of the destination, spans that touch, row_hi = -1
    got = index.match_near((0, fc.PAD), (fc.PAD, -1), 100.0)
    assert got.tobytes() == index.match_rows((0, fc.PAD), (fc.PAD, m)).tobytes()


def test_match_near_above_the_scratch_budget():
    """n x pieces above 1 << 22 partial states: the search goes in launches of fewer source rows, by the unguided plan"""
    c = fc.near_scene(4096, 1000)
    index = ac.build_index(api, c)
    index.chunk_rows = 1                               # 1000 pieces x 4096 rows = 4.1 M states
    want = fr.match_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], 0.5)
    assert index.match_near(c["src"], c["dst"], 0.5).tobytes() == want.tobytes()


# ---- 2. pair_near
def test_pair_near_of_landmarks_with_three_rows_on_each_side():
    c = fc.pair_scene()
    index = ac.build_index(api, c)
    want = fr.pair_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    assert len(want[0]) == 40
    for chunk in (64, 0):
        index.chunk_rows = chunk
        ps, pd = index.pair_near(c["src"], c["dst"], c["radius"])
        assert np.array_equal(ps, want[0]) and np.array_equal(pd, want[1])
    tight = dict(max_dist=2, ratio_num=1, ratio_den=2)                              # another rule 3
    ps, pd = index.pair_near(c["src"], c["dst"], c["radius"], **tight)
    want = fr.pair_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"], 2, 1, 2)
    assert np.array_equal(ps, want[0]) and np.array_equal(pd, want[1]) and 0 < len(ps) < 40


@pytest.mark.parametrize("n, d", ((65, 1000), (4096, 1000)))
def test_pair_near_where_descriptors_and_ids_repeat(n, d):
    c = fc.near_scene(n, d)
    index = ac.build_index(api, c)
    ps, pd = index.pair_near(c["src"], c["dst"], 0.5, max_dist=256, ratio_num=1, ratio_den=1)
    want = fr.pair_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], 0.5, 256, 1, 1)
    print(len(ps), "pairs")
    assert np.array_equal(ps, want[0]) and np.array_equal(pd, want[1]) and len(ps) > 0


# ---- 3. relabel
@pytest.fixture(scope="module")
def big_index():
    """200 000 rows without points, and their ids as a search reads them: built once, relabelled test after test"""
    ri = fc.relabel_index()
    index = api.DescriptorIndex(fc.RELABEL_ROWS)
    index.add(ri["desc"], ri["ids"])
    return index, ri["desc"], {"ids": ri["ids"].copy()}


@pytest.mark.parametrize("rows", ((70_001, 130_003), (0, -1)))          # per list the span first: the whole index still has rows to change
@pytest.mark.parametrize("n", fc.RELABEL_N)
def test_relabel_equals_the_reference(big_index, n, rows):
    index, desc, state = big_index
    frm, to = fc.relabel_lists(n)
    want, changed = fr.relabel(state["ids"], frm, to, rows)
    assert index.relabel(frm, to, rows) == changed    # in this file's order every step with n > 0 changes rows (tests/test_fuse_ref.py)
    got = ids_of(index, desc)                          # descriptors and rows unchanged; the ids the reference's
    state["ids"] = got
    assert np.array_equal(got, want) and index.size == fc.RELABEL_ROWS


def test_relabel_chain_repeat_and_from_equals_to():
    desc = np.random.default_rng(5).integers(0, 256, (8, 32), dtype=np.uint8)
    ids = np.array([1, 2, 3, 1, 2, 3, 4, (1 << 63) + 5], np.uint64)
    for frm, to, rows in (([1, 2], [2, 3], (0, -1)), ([1, 1], [7, 8], (0, -1)), ([1, 1, 4], [1, 9, 4], (0, -1)),
                          ([(1 << 63) + 5, 3], [0, 1 << 63], (3, 8)), ([9, 9], [9, 9], (0, -1)), ([1], [2], (4, 4))):
        index = api.DescriptorIndex(8)
        index.add(desc, ids)
        want, changed = fr.relabel(ids, frm, to, rows)
        assert index.relabel(np.array(frm, np.uint64), np.array(to, np.uint64), rows) == changed
        assert np.array_equal(ids_of(index, desc), want), (frm, to)


# ---- 4. fuse
@pytest.mark.parametrize("n, d", ((200, 1000), (1500, 3000)))
def test_fuse_equals_the_reference_and_a_second_call_changes_nothing(n, d):
    c = fc.merge_scene(n, d)
    index = ac.build_index(api, c)
    pts = points_of(index)
    want = fr.fuse(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    assert want["n_fused"] > 0 and want["n_same"] > 0 and want["n_rows_relabelled"] > want["n_fused"]       # the scene's condition
    ps, pd = index.pair_near(c["src"], c["dst"], c["radius"])                                               # the dry run changes nothing
    assert np.array_equal(ps, want["pair_src"]) and np.array_equal(pd, want["pair_dst"]) and np.array_equal(ids_of(index, c["desc"]), c["ids"])
    res, pairs = index.fuse(c["src"], c["dst"], c["radius"])
    print(res)
    assert res == (want["n_pairs"], want["n_same"], want["n_fused"], want["n_rows_relabelled"])
    assert np.array_equal(pairs["src"], want["pair_src"]) and np.array_equal(pairs["dst"], want["pair_dst"])
    assert np.array_equal(ids_of(index, c["desc"]), want["ids"]) and points_of(index) == pts and index.size == len(c["desc"])
    again, pairs2 = index.fuse(c["src"], c["dst"], c["radius"])
    second = fr.fuse(c["desc"], want["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    assert again == (second["n_pairs"], second["n_pairs"], 0, 0) and again.n_fused == 0 and again.n_same == again.n_pairs > 0
    assert np.array_equal(pairs2["src"], second["pair_src"]) and np.array_equal(ids_of(index, c["desc"]), want["ids"])


def test_fuse_in_a_relabel_span_and_at_a_small_chunk():
    c = fc.merge_scene(200, 1000)
    index = ac.build_index(api, c, chunk_rows=64)
    span = (1050, 1130)
    want = fr.fuse(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"], relabel_rows=span)
    res, _ = index.fuse(c["src"], c["dst"], c["radius"], relabel=span)
    assert res == (want["n_pairs"], want["n_same"], want["n_fused"], want["n_rows_relabelled"]) and 0 < res.n_rows_relabelled
    got = ids_of(index, c["desc"])
    assert np.array_equal(got, want["ids"]) and np.array_equal(got[:span[0]], c["ids"][:span[0]]) and np.array_equal(got[span[1]:], c["ids"][span[1]:])


def test_zero_pairs_is_a_success():
    c = fc.merge_scene(200, 1000)
    index = ac.build_index(api, c)
    for kw in (dict(src=(300, 300)), dict(dst=(40, 40)), dict(max_dist=0, ratio_num=1, ratio_den=1 << 20)):
        src, dst = kw.pop("src", c["src"]), kw.pop("dst", c["dst"])
        res, pairs = index.fuse(src, dst, c["radius"], **kw)
        assert res == (0, 0, 0, 0) and len(pairs["src"]) == 0 and len(pairs["dst"]) == 0
    far = api.DescriptorIndex(16, points=True)        # two rows that look alike, a metre apart: the gate admits nothing
    far.add_points(np.zeros((2, 32), np.uint8), [1, 2], np.array([[0, 0, 0], [1, 0, 0]], np.float32))
    assert far.fuse((1, 2), (0, 1), 0.5)[0] == (0, 0, 0, 0) and far.fuse((1, 2), (0, 1), 1.0)[0] == (1, 0, 1, 1)
    assert np.array_equal(ids_of(index, c["desc"]), c["ids"])


def test_refusals_leave_ids_and_outputs_untouched():
    c = fc.merge_scene(200, 1000)
    index = ac.build_index(api, c)
    size = index.size
    bad = [dict(src_lo=-1), dict(src_hi=size + 1), dict(src_lo=1100, src_hi=1099), dict(dst_lo=-1), dict(dst_hi=size + 1), dict(dst_lo=60, dst_hi=59),
           dict(dst_hi=1001), dict(dst_hi=-1), dict(src_lo=999), dict(src_lo=0, src_hi=-1),
           dict(relabel_lo=-1), dict(relabel_hi=size + 1), dict(relabel_lo=10, relabel_hi=9),
           dict(radius=-0.5), dict(radius=float("inf")), dict(radius=float("nan")),
           dict(max_dist=-1), dict(max_dist=257), dict(ratio_num=0), dict(ratio_den=0), dict(ratio_num=(1 << 20) + 1), dict(ratio_den=(1 << 20) + 1)]
    for over in bad:
        p = api.DescriptorIndex.fuse_params((1000, 1200), (0, 1000), 0.5)
        for k, v in over.items():
            setattr(p, k, v)
        r = _lib.SvoFuseResult()
        C.memset(C.byref(r), 0x5A, C.sizeof(r))
        before = bytes(r)
        ps, pd = np.full(200, 77, np.int32), np.full(200, 77, np.int32)
        k = C.c_int(-7)
        assert _lib.lib.svo_desc_index_fuse(index._h, C.byref(p), C.byref(r), _lib.ptr(ps), _lib.ptr(pd)) == _lib.SVO_ERR_ARG, over
        assert _lib.lib.svo_desc_index_pair_near(index._h, C.byref(p), C.byref(k), _lib.ptr(ps), _lib.ptr(pd)) == _lib.SVO_ERR_ARG, over
        assert bytes(r) == before and (ps == 77).all() and (pd == 77).all() and k.value == -7, over
    rows = np.zeros(10, _lib.DESC_MATCH_DTYPE); rows["row"] = 99
    for src, dst, radius in (((-1, 5), (10, 20), 0.5), ((0, size + 1), (0, 0), 0.5), ((5, 4), (10, 20), 0.5), ((0, 5), (-1, 20), 0.5),
                             ((0, 5), (10, size + 1), 0.5), ((0, 5), (4, 20), 0.5), ((0, 10), (0, -1), 0.5), ((0, 5), (10, 20), -1.0),
                             ((0, 5), (10, 20), float("nan")), ((0, 5), (10, 20), float("inf"))):
        assert _lib.lib.svo_desc_index_match_near(index._h, src[0], src[1], dst[0], dst[1], radius, _lib.ptr(rows)) == _lib.SVO_ERR_ARG, (src, dst, radius)
        assert (rows["row"] == 99).all()
    assert _lib.lib.svo_desc_index_match_near(index._h, 0, 5, 10, 20, 0.5, None) == _lib.SVO_ERR_ARG
    one = np.array([1], np.uint64)
    k = C.c_int(-7)
    for n, f, t, lo, hi in ((-1, one, one, 0, -1), ((1 << 20) + 1, one, one, 0, -1), (1, None, one, 0, -1), (1, one, None, 0, -1), (1, one, one, -1, 5),
                            (1, one, one, 0, size + 1), (1, one, one, 6, 5)):
        assert _lib.lib.svo_desc_index_relabel(index._h, n, _lib.ptr(f), _lib.ptr(t), lo, hi, C.byref(k)) == _lib.SVO_ERR_ARG and k.value == -7
    assert _lib.lib.svo_desc_index_fuse(index._h, None, None, None, None) == _lib.SVO_ERR_ARG
    assert np.array_equal(ids_of(index, c["desc"]), c["ids"])                       # nothing of all that touched an id
    # more than 4096 source rows
    big = api.DescriptorIndex(4200, points=True)
    big.add_points(np.zeros((4200, 32), np.uint8), np.arange(4200), np.zeros((4200, 3), np.float32))
    with pytest.raises(_lib.SvoError, match="4096 source rows"):
        big.fuse((0, 4097), (4097, 4200), 0.5)
    with pytest.raises(_lib.SvoError, match="4096 source rows"):
        big.match_near((0, 4097), (4097, 4200), 0.5)
    assert len(big.match_near((0, 4096), (4096, 4200), 0.5)) == 4096
    # an index without points: SVO_ERR_STATE for everything but relabel
    plain = api.DescriptorIndex(16)
    plain.add(np.zeros((8, 32), np.uint8), np.arange(8))
    p = api.DescriptorIndex.fuse_params((0, 4), (4, 8), 0.5)
    r = _lib.SvoFuseResult()
    assert _lib.lib.svo_desc_index_fuse(plain._h, C.byref(p), C.byref(r), None, None) == _lib.SVO_ERR_STATE
    assert _lib.lib.svo_desc_index_pair_near(plain._h, C.byref(p), None, None, None) == _lib.SVO_ERR_STATE
    assert _lib.lib.svo_desc_index_match_near(plain._h, 0, 4, 4, 8, 0.5, _lib.ptr(rows)) == _lib.SVO_ERR_STATE
    assert plain.relabel([3], [30]) == 1 and plain.match(np.zeros((1, 32), np.uint8), 3, 4)[0]["id"] == 30


def test_null_outputs_and_timing():
    c = fc.merge_scene(200, 1000)
    index = ac.build_index(api, c)
    p = api.DescriptorIndex.fuse_params(c["src"], c["dst"], c["radius"])
    assert _lib.lib.svo_desc_index_pair_near(index._h, C.byref(p), None, None, None) == 0
    assert index.stats()["last_kernels_ms"] == 0.0
    index.set_timing(True)
    for call in (lambda: index.match_near(c["src"], c["dst"], 0.5), lambda: index.pair_near(c["src"], c["dst"], 0.5),
                 lambda: index.relabel([11 + (1 << 63)], [11]), lambda: _lib.lib.svo_desc_index_fuse(index._h, C.byref(p), None, None, None)):
        assert call() is not None and 0.0 < index.stats()["last_kernels_ms"] < 1000.0
    want = fr.fuse(c["desc"], fr.relabel(c["ids"], [11 + (1 << 63)], [11])[0], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    assert np.array_equal(ids_of(index, c["desc"]), want["ids"])


# ---- 5. the reason for the feature, end to end
def test_a_merged_map_relocalises_only_after_its_landmarks_are_fused():
    c = fc.duplicate_scene()
    L = fc.DUP_L
    index = ac.build_index(api, c)
    K = fc.DUP_K.reshape(3, 3)
    res, cand = index.localize(K, c["query"], c["xy"], np.eye(3), np.zeros(3))
    assert res.n_candidates == 0 and not res.success                               # before: every landmark has a twin of another id
    want = fr.fuse(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    fused, pairs = index.fuse(c["src"], c["dst"], c["radius"])
    assert fused.n_fused == L and fused.n_rows_relabelled == L and fused == (L, 0, L, L)
    assert np.array_equal(pairs["src"], want["pair_src"]) and np.array_equal(pairs["dst"], want["pair_dst"])
    assert np.array_equal(ids_of(index, c["desc"]), want["ids"])
    res, cand = index.localize(K, c["query"], c["xy"], np.eye(3), np.zeros(3))
    print(res.n_candidates, res.n_inliers)
    assert res.n_candidates == L and res.success
    sel = rref.select_index(c["query"], c["xy"], c["desc"], want["ids"], c["xyz"], c["tags"])
    assert np.array_equal(cand["query"], sel["query"]) and np.array_equal(cand["row"], sel["row"])
    assert index.retire(latest_per_id=True, want_map=False) == L                    # what the fusion makes useful: one row per landmark
