"""The batched relocalisation on a real GPU (include/svo.h, "Batched relocalisation": svo_desc_index_localize_batch,
svo_desc_index_get_batch_order).

The oracle is the contract: the single calls on the same index, camera by camera — the result record in every bit, cand_query,
cand_row, cand_inlier — and for the candidates tests/reloc_batch_ref.py's numpy loop as well.  The index is
tests/reloc_batch_cases.py's 2624 rows (guide_cases.planned_case() and repeated_scene()); the cameras have different camera matrices
and priors.  One call takes slices of 0, 1, 63, 64, 65, 1024, 1025 and 4096 queries with a camera whose prior sees nothing, one at
min_candidates - 1 and one at min_candidates, one whose PnP fails, a query with a NaN pixel and the repeated-structure camera, at
chunk_rows 64 and the default, over the whole index and over a row range that starts inside a tile and whose length is no multiple of
8, with the sort on and off, and without guides.  Camera counts 1, 2, 8, 9 (where the PnP kernels change their build) and 65; the
lane order; two workloads of identical shape back to back, so that a query no lane served shows the previous call's partial states;
every refusal with `results` unchanged.  The single calls' results are computed once per (camera, search, row range) and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import reloc_batch_cases as bc
import reloc_batch_ref as bref
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kit(api):
    rows = bc.index_rows()
    ix = api.DescriptorIndex(len(rows["desc"]) + 8, points=True)
    bc.fill(ix, rows)
    assert ix.size == len(rows["desc"])
    single = {}

    def one(cam, K, guided, rng):
        """the single call for this camera, cached: (RelocResult, candidates)"""
        key = (id(cam), K.tobytes(), guided, rng)
        if key not in single:
            if guided:
                single[key] = ix.localize_guided(K, cam["R"], cam["t"], cam["radius"], cam["query"], cam["xy"], row_lo=rng[0], row_hi=rng[1])
            else:
                single[key] = ix.localize(K, cam["query"], cam["xy"], cam["R"], cam["t"], row_lo=rng[0], row_hi=rng[1])
        return single[key]

    yield dict(ix=ix, rows=rows, one=one)
    ix.close()


@functools.lru_cache(maxsize=None)
def numpy_reference(guided):
    """the numpy loop over MIX's cameras, once per kind of search"""
    return bref.select_batch(bc.index_rows(), [bc.cameras()[n] for n in bc.MIX], guided)


def same_record(a, b):
    return (a.success, a.n_candidates, a.n_inliers, a.iters_run) == (b.success, b.n_candidates, b.n_inliers, b.iters_run) and \
        a.R.tobytes() == b.R.tobytes() and a.t.tobytes() == b.t.tobytes() and a.T.tobytes() == b.T.tobytes()


def check_against_single(kit, names, K, guides, queries, xys, guided, rng=(0, -1)):
    """one batch call of the named cameras against their single calls -> the batch's results"""
    cams = bc.cameras()
    got = kit["ix"].localize_batch(K, queries, xys, guides if guided else None, rotations=[g[0] for g in guides], translations=[g[1] for g in guides],
                                   row_lo=rng[0], row_hi=rng[1])
    assert len(got) == len(names)
    for b, name in enumerate(names):
        want = kit["one"](cams[name], K[b], guided, rng)
        assert same_record(got[b][0], want[0]), (b, name, got[b][0], want[0])
        for f in ("query", "row", "inlier"):
            assert got[b][1][f].tobytes() == want[1][f].tobytes(), (b, name, f)
    return got


@pytest.mark.parametrize("rng", bc.ROW_RANGES, ids=["all_rows", "inside_a_tile"])
@pytest.mark.parametrize("chunk", [64, 0], ids=["chunk64", "chunk_default"])
@pytest.mark.parametrize("search", ["guided", "guided_unsorted", "unguided"])
def test_every_slice_size_in_one_call_equals_the_single_calls(kit, search, chunk, rng):
    ix = kit["ix"]
    K, guides, queries, xys = bc.workload(bc.MIX)
    ix.chunk_rows = chunk
    ix.set_guided_sort(search != "guided_unsorted")
    try:
        got = check_against_single(kit, bc.MIX, K, guides, queries, xys, search != "unguided", rng)
    finally:
        ix.chunk_rows = 0
        ix.set_guided_sort(True)
    if rng != (0, -1):
        return
    by = dict(zip(bc.MIX, got))
    want = numpy_reference(search != "unguided")
    for (rec, cand), w, name in zip(got, want, bc.MIX):                  # the candidates against the numpy loop as well
        assert cand["query"].tolist() == w["query"].tolist() and cand["row"].tolist() == w["row"].tolist(), name
    assert by["n0"][0].n_candidates == 0 and not by["n0"][0].success
    if search == "unguided":
        assert by["repeated"][0].n_candidates == 0
        return
    assert by["repeated"][0].n_candidates == 160 and by["repeated"][0].success
    assert by["nothing"][0].n_candidates == 0 and not by["nothing"][0].success and by["nothing"][0].iters_run == 0
    assert by["five"][0].n_candidates == bc.MIN_CANDIDATES - 1 and not by["five"][0].success and by["five"][0].iters_run == 0
    assert by["six"][0].n_candidates == bc.MIN_CANDIDATES and by["six"][0].success
    r = by["random"][0]                                                  # the PnP fails: R and t are the guess, untouched
    c = bc.cameras()["random"]
    assert r.n_candidates == 40 and not r.success and r.R.tobytes() == c["R"].tobytes() and r.t.reshape(3).tobytes() == c["t"].tobytes()
    assert not (by["n1024"][1]["query"] == 7).any()                     # the NaN pixel admits nothing


@pytest.mark.parametrize("count", bc.COUNTS)
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
def test_camera_counts_equal_the_single_calls(kit, guided, count):
    names, K, guides, queries, xys = bc.small(count)
    check_against_single(kit, names, K, guides, queries, xys, guided)


def test_the_lane_order_is_a_permutation_sorted_by_cell(kit):
    ix = kit["ix"]
    K, guides, queries, xys = bc.workload(bc.MIX)
    begin = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    ix.localize_batch(K, queries, xys, guides)
    order = ix.batch_order()
    assert len(order) == begin[-1]
    for b, name in enumerate(bc.MIX):
        lo, hi = begin[b], begin[b + 1]
        assert sorted(order[lo:hi].tolist()) == list(range(lo, hi)), name
        keys = bc.cell_keys(xys[b][order[lo:hi] - lo], guides[b][2])
        pairs = [tuple(k) for k in keys.tolist()]
        assert pairs == sorted(pairs), name
    assert (order != np.arange(len(order))).any()
    ix.set_guided_sort(False)
    try:
        ix.localize_batch(K, queries, xys, guides)
        assert ix.batch_order().tolist() == list(range(begin[-1]))
    finally:
        ix.set_guided_sort(True)
    ix.localize_batch(K, queries, xys)                                   # unguided: the identity
    assert ix.batch_order().tolist() == list(range(begin[-1]))


def test_two_workloads_of_one_shape_back_to_back(kit):
    for search in (True, False):
        for names in (bc.STALE_A, bc.STALE_B, bc.STALE_A):
            K, guides, queries, xys = bc.workload(names)
            check_against_single(kit, names, K, guides, queries, xys, search)


def test_no_cameras_is_legal(kit):
    assert kit["ix"].localize_batch(np.zeros((0, 3, 3), np.float32), [], [], []) == []


def test_timing_spans_the_calls_kernels(kit):
    ix = kit["ix"]
    K, guides, queries, xys = bc.workload(bc.STALE_A)
    ix.set_timing(True)
    try:
        ix.localize_batch(K, queries, xys, guides)
        assert 0 < ix.stats()["last_kernels_ms"] < 1000
    finally:
        ix.set_timing(False)


def test_every_refusal_leaves_the_results_unchanged(api, kit):
    lib, _lib = api._lib.lib, api._lib
    ix = kit["ix"]
    K, guides, queries, xys = bc.workload(["six", "five"])
    Kf = np.ascontiguousarray(K.reshape(2, 9), np.float32)
    q, p = np.concatenate(queries), np.concatenate(xys)
    begin = np.array([0, 6, 11], np.int32)
    g = (_lib.SvoRelocGuide * 2)(*[ix.guide(*x) for x in guides])
    prm = ix.reloc_params()
    res = (_lib.SvoRelocResult * 2)()
    for r in res:
        r.success, r.n_candidates, r.n_inliers, r.iters_run = 77, 78, 79, 80
        r.R[:] = [1.5] * 9; r.t[:] = [2.5] * 3; r.T[:] = [3.5] * 16
    before = bytes(res)
    ptr = api.ptr

    def call(index=ix._h, n=2, K=Kf, guides=g, begin=begin, query=q, xy=p, params=prm, results=res):
        return lib.svo_desc_index_localize_batch(index, n, ptr(K), guides, ptr(begin), ptr(query), ptr(xy), None if params is None else C.byref(params),
                                                 results, None, None, None)

    ARG, STATE = _lib.SVO_ERR_ARG, _lib.SVO_ERR_STATE
    bad_g = (_lib.SvoRelocGuide * 2)(*[ix.guide(*x) for x in guides]); bad_g[1].radius = -1.0
    nan_g = (_lib.SvoRelocGuide * 2)(*[ix.guide(*x) for x in guides]); nan_g[1].t[2] = float("nan")
    nan_K = Kf.copy(); nan_K[1, 4] = np.inf
    big = np.array([0, 4097, 4098], np.int32)
    cases = [(dict(index=None), ARG), (dict(params=None), ARG), (dict(n=-1), ARG), (dict(n=1025), ARG), (dict(begin=None), ARG),
             (dict(begin=np.array([1, 6, 11], np.int32)), ARG), (dict(begin=np.array([0, 6, 5], np.int32)), ARG), (dict(begin=big), ARG),
             (dict(K=None), ARG), (dict(results=None), ARG), (dict(query=None), ARG), (dict(xy=None), ARG),
             (dict(guides=bad_g), ARG), (dict(guides=nan_g), ARG), (dict(K=nan_K), ARG),
             (dict(params=ix.reloc_params(row_lo=5, row_hi=4)), ARG), (dict(params=ix.reloc_params(row_hi=ix.size + 1)), ARG),
             (dict(params=ix.reloc_params(max_dist=257)), ARG), (dict(params=ix.reloc_params(ratio_num=0)), ARG),
             (dict(params=ix.reloc_params(ratio_den=(1 << 20) + 1)), ARG), (dict(params=ix.reloc_params(min_candidates=5)), ARG)]
    for kw, status in cases:
        assert call(**kw) == status, kw
        assert bytes(res) == before, kw
    # a total above 1 << 20: 257 slices of 4096 and one more query
    many = np.minimum(np.arange(259, dtype=np.int64) * 4096, (1 << 20) + 1).astype(np.int32)
    assert lib.svo_desc_index_localize_batch(ix._h, 258, ptr(np.zeros((258, 9), np.float32)), None, ptr(many), ptr(q), ptr(p), C.byref(prm),
                                             (_lib.SvoRelocResult * 258)(), None, None, None) == ARG
    plain = api.DescriptorIndex(64)                                      # an index without points
    try:
        assert call(index=plain._h) == STATE and bytes(res) == before
    finally:
        plain.close()
    assert call() == _lib.SVO_OK and bytes(res) != before               # and the call itself is sound
    n = C.c_int(0)
    assert lib.svo_desc_index_get_batch_order(ix._h, 0, None, None) == ARG
    fresh = api.DescriptorIndex(64, points=True)
    try:
        assert lib.svo_desc_index_get_batch_order(fresh._h, 0, None, C.byref(n)) == STATE
    finally:
        fresh.close()
