"""The descriptor index's maintenance calls on a real GPU (include/svo.h, "Index maintenance": svo_desc_index_retire,
svo_desc_index_transform_points) against tests/desc_retire_ref.py, on the index's behaviour only — there is no "dump the index" call:

 - size and kept_before equal the reference's;
 - a match of every descriptor the index held before the call, plus random queries, equals desc_match_ref.match on the reference's
   compacted arrays in every field (at 300 000 rows: a sample of the old descriptors, the reference's distance matrix sets the limit);
 - project under an identity guide equals guide_ref.project on the reference's compacted points bit for bit, and two projections
   that hand coordinates through unchanged (Zc = 1, fx = fy = 1) return the points themselves bit for bit, +inf for a row without one;
 - the tags, where a test says so, through the counts of transform_points with the identity over one tag at a time.

The slab is forced to 64 rows unless a test says otherwise, so that 65 rows are two slabs.  The 300 000-row run is at the default slab
of 262 144 rows: two slabs in the scope, and 1 172 block counts, a scan over more than one block (five) of block counts."""
import ctypes as C

import numpy as np
import pytest

import desc_match_ref as mref
import desc_retire_ref as ref
import guide_cases as cases
import guide_ref as gref
from gpu_kit import api, projections, same, snap, streams  # noqa: F401  (the fixture is found by name)
from test_desc_retire_ref import some_ids

pytestmark = pytest.mark.gpu

K_ONE = np.eye(3, dtype=np.float32)
# x_cam = R X + t with Zc = 1: (u, v) = (x, y) and (z, z) exactly
READ_XY = (np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64), np.array([0, 0, 1.0]))
READ_Z = (np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0]], np.float64), np.array([0, 0, 1.0]))


def make_index(api, case, points=True, capacity=None, slab=64):
    ix = api.DescriptorIndex(capacity or max(len(case["ids"]), 1), points=points)
    ix.retire_slab_rows = slab
    fill(ix, case, points)
    return ix


def fill(ix, case, points=True):
    ix.truncate(0)
    if points:
        rows = case["tags"] >= 0                                         # add_points takes tags >= 0: the rows without a point go through add
        r = 0
        while r < len(rows):                                            # runs of rows with / without a point, in row order
            e = r
            while e < len(rows) and rows[e] == rows[r]:
                e += 1
            if rows[r]:
                ix.add_points(case["desc"][r:e], case["ids"][r:e], case["xyz"][r:e], case["tags"][r:e])
            else:
                ix.add(case["desc"][r:e], case["ids"][r:e])
            r = e
    else:
        ix.add(case["desc"], case["ids"])
    assert ix.size == len(case["ids"])


def read_points(ix):
    """the index's points bit for bit: (n, 3) float32, +inf for a row without a point"""
    xy, z = ix.project(K_ONE, *READ_XY), ix.project(K_ONE, *READ_Z)
    assert xy.shape == z.shape and z[:, 0].tobytes() == z[:, 1].tobytes()
    return np.concatenate([xy, z[:, :1]], 1)


def want_points(xyz, tags):
    p = np.array(xyz, np.float32).reshape(-1, 3)
    p[np.asarray(tags) == ref.POINT_NONE] = np.inf
    return p


def queries(case, seed, n_random=8, sample=None):
    rng = np.random.default_rng(seed)
    old = case["desc"] if sample is None or sample >= len(case["desc"]) else case["desc"][rng.choice(len(case["desc"]), sample, replace=False)]
    return np.concatenate([old, rng.integers(0, 256, (n_random, 32), dtype=np.uint8)])


def check_index(ix, case, keep, points=True, tags=False, sample=None, seed=1):
    """the index now against the reference's compacted arrays"""
    d, i, x, t = case["desc"][keep], case["ids"][keep], case["xyz"][keep], case["tags"][keep]
    assert ix.size == len(d)
    q = queries(case, seed, sample=sample)
    got, want = ix.match(q), mref.match(q, d, i)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    if not points:
        return
    assert ix.project(cases.K_SCENE, np.eye(3), np.zeros(3)).tobytes() == gref.project(cases.K_SCENE, np.eye(3), np.zeros(3), x, t).tobytes()
    assert read_points(ix).tobytes() == want_points(x, t).tobytes()
    if tags:
        for tag in np.unique(t[t >= 0]):
            assert ix.transform_points(np.eye(4), tags=(tag, tag)) == (int((t == tag).sum()), 0), tag


def retire_and_check(ix, case, points=True, tags=False, sample=None, **rule):
    """one retire call on ix, which holds `case`, against the reference -> (keep, kept_before)"""
    rows = rule.pop("rows", (0, -1))
    keep, kept_before = ref.retire(case["ids"], case["tags"] if points else None, rows, **rule)
    got = ix.retire(rows=rows, tags=rule.get("tag_window"), drop_ids=rule.get("drop_ids"),
                    latest_per_id=rule.get("latest_per_id", False), scope=rule.get("scope", False))
    assert got.dtype == np.int32 and got.tolist() == kept_before.tolist(), rule
    check_index(ix, case, keep, points, tags, sample)
    return keep, kept_before


def refused(api, code, fn, *a, **kw):
    with pytest.raises(api._lib.SvoError) as e:
        fn(*a, **kw)
    assert "status %d:" % code in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ the seams
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300])
def test_wave_block_and_slab_seams(api, n):
    """keep all, drop all, alternate rows, only the first row, only the last row, at every size around 64, 128 and 256"""
    case = ref.index_case(n, seed=n)
    case["ids"] = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)      # one row per id: a list names rows
    ix = make_index(api, case)
    try:
        rules = [dict(), dict(drop_ids=[]), dict(scope=True), dict(drop_ids=case["ids"][1::2]), dict(drop_ids=case["ids"][:1]),
                 dict(drop_ids=case["ids"][-1:]), dict(drop_ids=case["ids"][0::2], latest_per_id=True)]
        for k, rule in enumerate(rules):
            if k:
                fill(ix, case)
            keep, _ = retire_and_check(ix, case, tags=n in (65, 300), **rule)
            if k < 2:
                assert keep.all()
        assert not keep[0::2].any() and keep[1::2].all()
    finally:
        ix.close()


def test_every_scope_of_a_27_row_index(api):
    """LATEST_PER_ID over every scope [lo, hi): the ids' rows lie scattered, so runs straddle both scope edges (the CPU test of the
    generator asserts it); every third scope with the tag rule and a list as well"""
    case = ref.index_case(27, seed=27)
    drop = some_ids(case)
    ix = make_index(api, case, slab=8)
    try:
        k = 0
        for lo in range(28):
            for hi in range(lo, 28):
                rule = dict(rows=(lo, hi), latest_per_id=True)
                if k % 3 == 2:
                    rule.update(tag_window=(1, 6), drop_ids=drop)
                if k:
                    fill(ix, case)
                keep, _ = retire_and_check(ix, case, **rule)
                assert keep[:lo].all() and keep[hi:].all()
                k += 1
        assert k == 406
    finally:
        ix.close()


RULES = [dict(tag_window=(2, 5)), dict(tag_window=(5, 2)), dict(tag_window=(-1, 3)), dict(drop_ids="some"), dict(drop_ids=[]),
         dict(drop_ids=np.array([5, 6, 2 ** 64 - 2], np.uint64)), dict(latest_per_id=True), dict(scope=True),
         dict(tag_window=(1, 6), drop_ids="some", latest_per_id=True), dict(tag_window=(1, 6), drop_ids="some", latest_per_id=True, scope=True)]


@pytest.mark.parametrize("rows", [(0, -1), (40, 260)], ids=["all", "40-260"])
def test_each_flag_alone_and_all_combined(api, rows):
    """300 rows; the list is unsorted, has duplicates and names ids the index lacks ("some"), is empty, or names only absent ids"""
    case = ref.index_case(300, seed=300)
    ix = make_index(api, case)
    try:
        for k, rule in enumerate(RULES):
            rule = dict(rule, rows=rows)
            if isinstance(rule.get("drop_ids"), str):
                rule["drop_ids"] = some_ids(case)
            if k:
                fill(ix, case)
            keep, _ = retire_and_check(ix, case, tags=True, **rule)
            lo, hi = rows[0], 300 if rows[1] == -1 else rows[1]
            if k in (4, 5):
                assert keep.all()
            if k in (1, 7, 9):
                assert not keep[lo:hi].any()
            if k in (0, 3, 6, 8):
                assert 0 < keep[lo:hi].sum() < hi - lo
    finally:
        ix.close()


def test_ids_zero_and_all_ones(api):
    case = ref.index_case(120, seed=5)
    zero, ones = case["ids"] == 0, case["ids"] == ref.U64_MAX
    assert zero.sum() == 1 and ones.sum() == 2
    case["ids"][7::10] = 0; case["ids"][3::10] = ref.U64_MAX                 # more rows of both
    ix = make_index(api, case)
    try:
        keep, _ = retire_and_check(ix, case, latest_per_id=True)
        zero, ones = np.flatnonzero(case["ids"] == 0), np.flatnonzero(case["ids"] == ref.U64_MAX)
        assert keep[zero].tolist() == [False] * (len(zero) - 1) + [True] and keep[ones].tolist() == [False] * (len(ones) - 1) + [True]
        fill(ix, case)
        keep, _ = retire_and_check(ix, case, drop_ids=[0])
        assert not keep[zero].any() and keep[ones].all()
        fill(ix, case)
        keep, _ = retire_and_check(ix, case, drop_ids=np.array([ref.U64_MAX], np.uint64), latest_per_id=True)
        assert not keep[ones].any() and keep[zero].sum() == 1
    finally:
        ix.close()


def test_one_id_on_every_row(api):
    """5 000 rows of one id: every lane of the insert meets one slot, and exactly the last row survives"""
    case = ref.index_case(5000, seed=11)
    case["ids"][:] = 42
    ix = make_index(api, case)
    try:
        keep, kept_before = retire_and_check(ix, case, latest_per_id=True)
        assert np.flatnonzero(keep).tolist() == [4999] and kept_before[-1] == 1
    finally:
        ix.close()


def test_the_table_at_its_design_load(api):
    """2 000 distinct ids in 4 000 rows: the 8 192-slot table holds 2 000 rows at the end and met 4 000 inserts"""
    case = ref.index_case(4000, seed=12)
    rng = np.random.default_rng(12)
    case["ids"] = np.repeat(rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * np.uint64(2), 2)[rng.permutation(4000)]
    assert len(np.unique(case["ids"])) == 2000
    ix = make_index(api, case)
    try:
        keep, _ = retire_and_check(ix, case, latest_per_id=True)
        assert keep.sum() == 2000
    finally:
        ix.close()


def test_300000_rows_at_the_default_slab(api):
    """every flag at once over 300 000 rows at the default slab (262 144 rows: the scope is two slabs); 1 172 blocks of keep flags, so
    the scan of the block counts runs over five blocks.  The match is checked on 24 of the old descriptors and 8 random queries."""
    n = 300000
    rng = np.random.default_rng(13)
    case = dict(desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), ids=(rng.permutation(n) // 8).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15),
                xyz=rng.uniform(-20, 20, (n, 3)).astype(np.float32), tags=(np.arange(n) * 8 // n).astype(np.int32))
    ix = make_index(api, case, slab=0)
    try:
        assert ix.retire_slab_rows == 262144 < n
        drop = np.unique(case["ids"])[::5][rng.permutation(7500)]
        keep, kept_before = retire_and_check(ix, case, sample=24, rows=(1000, 299500), tag_window=(1, 6), drop_ids=drop, latest_per_id=True)
        assert 20000 < kept_before[-1] < 100000 and keep[:1000].all() and keep[299500:].all()
        st = ix.retire_stats()
        assert st["scratch_bytes"] <= scratch_bound(298500, len(drop), 262144, n - 1000, latest=True, by_ids=True), st
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ bookkeeping
def test_add_truncate_and_retire_again(api):
    case = ref.index_case(200, seed=21)
    more = ref.index_case(30, seed=22, points=False)
    ix = make_index(api, case, capacity=400)
    try:
        keep, kept_before = retire_and_check(ix, case, tag_window=(2, 6), latest_per_id=True)
        n_kept = int(kept_before[-1])
        assert 0 < n_kept < 200
        assert ix.retire(want_map=False) == n_kept                       # without the map: the new size alone
        again = ix.retire(tags=(2, 6), latest_per_id=True)             # the same rule again: nothing left to drop
        assert again.tolist() == list(range(n_kept + 1))
        after = {k: v[keep] for k, v in case.items()}
        assert ix.add_points(more["desc"], more["ids"], more["xyz"], more["tags"]) == n_kept
        both = {k: np.concatenate([after[k], more[k]]) for k in case}
        check_index(ix, both, np.ones(len(both["ids"]), bool), tags=True)
        ix.truncate(n_kept - 5)
        check_index(ix, after, np.arange(n_kept) < n_kept - 5)
        assert ix.retire(rows=(0, -1), scope=True).tolist() == [0] * (n_kept - 4) and ix.size == 0
        assert ix.retire().tolist() == [0]                              # an empty index
    finally:
        ix.close()


def test_localize_is_the_same_after_retiring_rows_it_never_chose(api):
    """the 160 landmarks of tests/test_gpu_guide_localize.py's scene behind 50 rows of something else: localize with row_lo = 50
    before, and over the whole index after a retire that drops exactly those 50 rows, returns the same pose bits"""
    s = cases.repeated_scene()
    junk = ref.index_case(50, seed=31)
    junk["tags"][:] = 3
    desc, ids = np.concatenate([junk["desc"], s["desc"][:160]]), np.concatenate([junk["ids"], s["ids"][:160]])
    xyz, tags = np.concatenate([junk["xyz"], s["xyz"][:160]]), np.concatenate([junk["tags"], s["tags"][:160] + 9])
    ix = api.DescriptorIndex(256, points=True)
    ix.retire_slab_rows = 64
    try:
        ix.add_points(desc, ids, xyz, tags)
        before, cand0 = ix.localize(s["K"], s["query"], s["xy"], s["R0"], s["t0"], row_lo=50, reproj_error=2.0)
        kept_before = ix.retire(tags=(9, 9))
        assert kept_before.tolist() == [0] * 51 + list(range(1, 161)) and ix.size == 160
        after, cand1 = ix.localize(s["K"], s["query"], s["xy"], s["R0"], s["t0"], reproj_error=2.0)
        assert before.success and before.n_candidates == 160 and before.n_inliers >= 150
        assert (after.success, after.n_candidates, after.n_inliers, after.iters_run) == (before.success, before.n_candidates, before.n_inliers, before.iters_run)
        assert after.R.tobytes() == before.R.tobytes() and after.t.tobytes() == before.t.tobytes() and after.T.tobytes() == before.T.tobytes()
        assert cand1["query"].tolist() == cand0["query"].tolist() and cand1["row"].tolist() == kept_before[cand0["row"]].tolist()
        assert cand1["inlier"].tolist() == cand0["inlier"].tolist()
    finally:
        ix.close()


def test_an_index_without_points(api):
    case = ref.index_case(150, seed=41, points=False)
    ix = make_index(api, case, points=False)
    try:
        refused(api, api._lib.SVO_ERR_STATE, ix.retire, tags=(0, 3))
        refused(api, api._lib.SVO_ERR_STATE, ix.retire, tags=(0, 3), latest_per_id=True)
        refused(api, api._lib.SVO_ERR_STATE, ix.transform_points, np.eye(4))
        check_index(ix, case, np.ones(150, bool), points=False)
        retire_and_check(ix, case, points=False, rows=(10, 140), drop_ids=some_ids(case), latest_per_id=True)
        fill(ix, case, points=False)
        retire_and_check(ix, case, points=False, latest_per_id=True)
        fill(ix, case, points=False)
        retire_and_check(ix, case, points=False, rows=(20, 30), scope=True)
    finally:
        ix.close()


def test_every_refusal_changes_nothing(api):
    L = api._lib
    case = ref.index_case(100, seed=51)
    ix = make_index(api, case)
    ids = np.array([1, 2, 3], np.uint64)

    def raw(**f):
        rule = L.SvoRetireRule()
        rule.row_hi = -1
        for k, v in f.items():
            setattr(rule, k, v)
        kept_before, n_kept = np.full(101, -7, np.int32), C.c_int(-7)
        rc = L.lib.svo_desc_index_retire(ix._h, C.byref(rule), L.ptr(kept_before), C.byref(n_kept))
        assert (kept_before == -7).all() and n_kept.value == -7
        return rc

    try:
        assert raw(flags=16) == L.SVO_ERR_ARG and raw(flags=0x80000001, tag_hi=9) == L.SVO_ERR_ARG
        for lo, hi in ((-1, 5), (5, 3), (0, 101), (101, -1), (0, -2)):
            assert raw(flags=L.RETIRE_SCOPE, row_lo=lo, row_hi=hi) == L.SVO_ERR_ARG, (lo, hi)
            refused(api, L.SVO_ERR_ARG, ix.transform_points, np.eye(4), rows=(lo, hi))
        assert raw(flags=L.RETIRE_SCOPE, n_ids=-1) == L.SVO_ERR_ARG and raw(flags=0, n_ids=(1 << 24) + 1, ids=ids.ctypes.data) == L.SVO_ERR_ARG
        assert raw(flags=L.RETIRE_BY_IDS, n_ids=3) == L.SVO_ERR_ARG         # a list without an address
        assert L.lib.svo_desc_index_retire(ix._h, None, None, None) == L.SVO_ERR_ARG and L.lib.svo_desc_index_retire(None, None, None, None) == L.SVO_ERR_ARG
        for bad in (np.nan, np.inf, -np.inf):
            T = np.eye(4); T[1, 2] = bad
            refused(api, L.SVO_ERR_ARG, ix.transform_points, T)
        refused(api, L.SVO_ERR_ARG, setattr, ix, "retire_slab_rows", -1)
        refused(api, L.SVO_ERR_ARG, setattr, ix, "retire_slab_rows", (1 << 24) + 1)
        assert ix.retire_slab_rows == 64
        check_index(ix, case, np.ones(100, bool), tags=True)
        # and what is legal at the edges: an empty scope, a null list of no entries, no outputs
        assert ix.retire(rows=(100, -1), scope=True).tolist() == list(range(101)) and ix.retire(rows=(40, 40), scope=True).tolist() == list(range(101))
        rule = L.SvoRetireRule(); rule.flags = L.RETIRE_BY_IDS; rule.row_hi = -1
        assert L.lib.svo_desc_index_retire(ix._h, C.byref(rule), None, None) == L.SVO_OK and ix.size == 100
        check_index(ix, case, np.ones(100, bool))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ scratch
def scratch_bound(m, n_ids, slab, moving, latest, by_ids):
    """include/svo.h, "Index maintenance", Memory: max(65 536, 2 need - 1)"""
    R = lambda b: (b + 255) // 256 * 256
    slots = 2
    while slots < 2 * m:
        slots *= 2
    need = R(m) + R(4 * (m + 1)) + R(4 * ((m + 255) // 256 + 257)) + (R(4 * slots) if latest else 0) + (R(8 * n_ids) if by_ids else 0) + R(56 * min(slab, moving))
    return max(65536, 2 * need - 1)


def test_the_scratch_stays_within_the_stated_bound(api):
    for n, slab, rule in ((300, 64, dict(latest_per_id=True)), (5000, 64, dict(tag_window=(1, 6))), (5000, 0, dict(drop_ids="some", latest_per_id=True)),
                          (40000, 0, dict(tag_window=(1, 6), drop_ids="some", latest_per_id=True))):
        case = ref.index_case(n, seed=n, spread=False)
        if rule.get("drop_ids") == "some":
            rule["drop_ids"] = some_ids(case)
        ix = make_index(api, case, slab=slab)
        try:
            assert ix.retire_stats() == dict(last_kernels_ms=0.0, scratch_allocations=0, scratch_bytes=0, scratch_bytes_outgrown=0)
            ix.retire(rows=(10, n - 10), tags=rule.get("tag_window"), drop_ids=rule.get("drop_ids"), latest_per_id=rule.get("latest_per_id", False))
            st = ix.retire_stats()
            bound = scratch_bound(n - 20, len(rule.get("drop_ids", [])), slab or 262144, n - 10, "latest_per_id" in rule, "drop_ids" in rule)
            print(n, slab, st, bound)
            assert 0 < st["scratch_bytes"] <= bound and st["scratch_allocations"] == 1 and st["scratch_bytes_outgrown"] == 0
        finally:
            ix.close()


def test_growing_and_retiring_40_times_allocates_log_times(api):
    step = 700
    case = ref.index_case(40 * step, seed=61, spread=False)
    ix = api.DescriptorIndex(40 * step, points=True)
    ix.set_timing(True)
    try:
        ids, tags = np.zeros(0, np.uint64), np.zeros(0, np.int32)
        for k in range(40):
            s = slice(k * step, (k + 1) * step)
            ix.add_points(case["desc"][s], case["ids"][s], case["xyz"][s], np.maximum(case["tags"][s], 0))
            ids, tags = np.concatenate([ids, case["ids"][s]]), np.concatenate([tags, np.maximum(case["tags"][s], 0)])
            keep, kept_before = ref.retire(ids, tags, drop_ids=case["ids"][s][:3], latest_per_id=True)
            assert ix.retire(drop_ids=case["ids"][s][:3], latest_per_id=True).tolist() == kept_before.tolist(), k
            ids, tags = ids[keep], tags[keep]
            assert ix.retire_stats()["last_kernels_ms"] > 0
        st = ix.retire_stats()
        bound = scratch_bound(len(keep), 3, 262144, len(keep), True, True)
        print(st, len(keep), bound)
        assert st["scratch_bytes"] <= bound
        assert st["scratch_allocations"] <= int(np.ceil(np.log2(bound / 65536))) + 1 <= 8
        assert st["scratch_bytes_outgrown"] < st["scratch_bytes"]
        ix.set_timing(False)
        ix.retire()
        assert ix.retire_stats()["last_kernels_ms"] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ transform_points
def rigid(seed):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = cases.rot(*rng.uniform(-0.5, 0.5, 3))
    T[:3, 3] = rng.uniform(-3, 3, 3)
    return T


def transform_and_check(ix, state, T, rows=(0, -1), tags=None):
    """one transform_points call against the reference; state: the index's xyz, updated"""
    after, moved, skipped = ref.transform(state["xyz"], state["tags"], T, rows, tags)
    assert ix.transform_points(T, rows=rows, tags=tags) == (moved, skipped)
    assert read_points(ix).tobytes() == want_points(after, state["tags"]).tobytes()
    changed = (after.view(np.uint32) != state["xyz"].view(np.uint32)).any(1)
    state["xyz"] = after
    return moved, skipped, changed


def test_transform_points_equals_the_reference(api):
    case = ref.index_case(300, seed=71)
    ix = make_index(api, case)
    state = dict(xyz=case["xyz"].copy(), tags=case["tags"])
    has = case["tags"] != ref.POINT_NONE
    try:
        moved, skipped, changed = transform_and_check(ix, state, np.eye(4))
        assert (moved, skipped) == (int(has.sum()), 0) and not changed.any()           # the identity changes no bit
        moved, _, changed = transform_and_check(ix, state, rigid(1))
        assert moved == has.sum() and changed[has].all() and not changed[~has].any()
        scale = rigid(2); scale[:3, :3] *= 1.0371
        transform_and_check(ix, state, scale)
        # the filters at their edges: rows 64 and 192 are the first in and the first out, tags 2 and 5 the window's ends
        moved, _, changed = transform_and_check(ix, state, rigid(3), rows=(64, 192))
        assert changed[64] == has[64] and changed[191] == has[191] and not changed[:64].any() and not changed[192:].any() and moved == has[64:192].sum()
        moved, _, changed = transform_and_check(ix, state, rigid(4), tags=(2, 5))
        t = case["tags"]
        assert changed.tolist() == ((t >= 2) & (t <= 5)).tolist() and changed[t == 2].any() and changed[t == 5].any() and moved == changed.sum()
        moved, _, changed = transform_and_check(ix, state, rigid(5), rows=(100, 250), tags=(-1, 3))     # -1 in the window selects no row without a point
        assert changed.tolist() == ((t >= 0) & (t <= 3) & (np.arange(300) >= 100) & (np.arange(300) < 250)).tolist()
        assert transform_and_check(ix, state, rigid(6), tags=(5, 2))[:2] == (0, 0) and transform_and_check(ix, state, rigid(6), rows=(7, 7))[:2] == (0, 0)
        # a scale that overflows f32 for the rows far from x = 0: they stay as they are and are counted
        big = np.eye(4); big[0, 0] = 3e37
        moved, skipped, changed = transform_and_check(ix, state, big)
        assert skipped > 20 and moved > 20 and moved + skipped == has.sum() and np.isfinite(state["xyz"]).all()
        # the ids and descriptors are where they were
        check_index(ix, dict(case, xyz=state["xyz"]), np.ones(300, bool))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ frames in flight
def test_retire_and_transform_beside_frames_in_flight_change_nothing(api):
    """a 9-sequence context with two frames submitted, retire and transform_points on an index, then the frames collected: equal in
    every bit to a run without the calls"""
    import torch
    w, h, B = 320, 160, 9
    S = streams(B, 3, 4100, w, h)
    Pl, Pr = projections(w, h)
    dev = [[(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in zip(*s)] for s in S]
    torch.cuda.synchronize()
    case = ref.index_case(3000, seed=81)
    runs = {}
    for beside in (False, True):
        vo = api.BatchVisualOdometry(w, h, B, api.default_config(win_w=21, win_h=21, max_level=3, max_translation_norm=2.0))
        vo.initalize_projection_matricies(Pl, Pr)
        ix = make_index(api, case) if beside else None
        out = []
        try:
            vo.stereo_callback_batch([s[0][0] for s in S], [s[1][0] for s in S])
            for k in (1, 2):
                vo.submit_device([dev[i][k][0].data_ptr() for i in range(B)], [dev[i][k][1].data_ptr() for i in range(B)], w)
            if ix:
                keep, kept_before = ref.retire(case["ids"], case["tags"], (100, 2900), tag_window=(1, 6), latest_per_id=True)
                assert ix.retire(rows=(100, 2900), tags=(1, 6), latest_per_id=True).tolist() == kept_before.tolist()
                _, moved, skipped = ref.transform(case["xyz"][keep], case["tags"][keep], rigid(9))
                assert ix.transform_points(rigid(9)) == (moved, skipped)
            for k in (1, 2):
                ok, T = vo.collect()
                out.append((ok.tobytes(), T.tobytes(), [snap(vo, i) for i in range(B)]))
        finally:
            vo.close()
            if ix:
                ix.close()
        runs[beside] = out
    del dev
    for k, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert a[0] == b[0] and a[1] == b[1], "frame %d: ok / pose" % (k + 1)
        assert all(same(p, q) for p, q in zip(a[2], b[2])), "frame %d: features / tracks" % (k + 1)
    assert any(np.frombuffer(a[0], np.uint8).any() for a in runs[False])
