"""svo_desc_index_consolidate (include/svo.h, "Landmark consolidation") on the GPU against tests/consolidate_ref.py: after every
call read_rows of the whole index equals the reference's four arrays byte for byte, kept_before and the result record equal the
reference's.  The slab of the compaction is forced to 64 rows except where noted.  The cases: the sizes around a wave, a block and
a slab; groups of 1 .. 200 views interleaved row by row (the wave's 64 views, the cap, the bisection for the last 64); one id a row;
ids 0 and 2^64 - 1 and ids that collide in the table; rows without a point and rows outside the tag window inside a partial scope;
identical descriptors; radius 0, one that cuts a view off, one above every distance; 70 000 rows at the default slab (274 blocks:
the scan's second level); the call repeated; every refusal; the scratch's bound; a call beside frames in flight."""
import ctypes as C

import numpy as np
import pytest

import align_ref as aref
import consolidate_ref as cr
from gpu_kit import api, projections, same, snap, streams  # noqa: F401  (the fixture is found by name)
from test_gpu_desc_retire import make_index, refused

pytestmark = pytest.mark.gpu


def check_call(ix, case, radius, rows=(0, -1), tags=None):
    """one consolidate call on ix, which holds `case`, against the reference -> the reference's output"""
    want = cr.consolidate(case["desc"], case["ids"], case["xyz"], case["tags"], radius, rows, tags)
    res, kept_before = ix.consolidate(radius, rows=rows, tags=tags)
    assert kept_before.dtype == np.int32 and kept_before.tolist() == want["kept_before"].tolist()
    assert tuple(res) == tuple(want["result"]), (res, want["result"])
    assert ix.size == want["result"].n_kept
    assert not cr.same_rows(ix.read_rows(), cr.as_read(want))
    return want


def run_case(api, case, radius, rows=(0, -1), tags=None, slab=64, again=True):
    ix = make_index(api, case, slab=slab)
    try:
        want = check_call(ix, case, radius, rows, tags)
        if again:                                     # the same call on the result changes nothing
            n = len(want["ids"])
            hi = rows[1] if rows[1] == -1 else int(want["kept_before"][rows[1]])
            second = check_call(ix, want, radius, (rows[0], hi), tags)
            assert second["result"].n_dropped == 0 and second["kept_before"].tolist() == list(range(n + 1))
            assert not cr.same_rows(cr.as_read(second), cr.as_read(want))
        return want
    finally:
        ix.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 300])
def test_wave_block_and_slab_seams(api, n):
    want = run_case(api, cr.index_case(n, views=3, seed=n), 0.2)
    assert n < 63 or want["result"].n_dropped > n // 3


def test_groups_of_1_to_200_views_interleaved(api):
    sizes = [1, 2, 3, 63, 64, 65, 129, 200, 1, 2, 5, 8, 30]
    case = cr.group_sizes_case(sizes, seed=1)
    want = run_case(api, case, 0.2)
    r = want["result"]
    assert (r.n_members, r.n_groups, r.n_capped_groups) == (sum(sizes), len(sizes), 3) and r.n_far_views > 20
    assert run_case(api, case, 0.2, slab=0)["result"] == r


def test_one_id_on_each_of_1000_rows(api):
    case = cr.index_case(1000, views=1, seed=2, none_every=0)
    case["ids"] = np.random.default_rng(2).permutation(1000).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    want = run_case(api, case, 0.2)
    assert want["result"] == cr.Result(1000, 1000, 0, 0, 0, 1000)


def test_ids_zero_all_ones_and_colliding(api):
    """ids 0 and 2^64 - 1, and 40 ids whose probes start at one slot of the 1024-slot table of a 512-row scope"""
    n, slots = 512, 1024
    case = cr.index_case(n, views=4, seed=3)
    start = lambda v: aref.mix64(int(v)) & (slots - 1)
    hit, v = [], 1
    while len(hit) < 40:
        if start(v) == start(1):
            hit.append(v)
        v += 1
    rng = np.random.default_rng(3)
    case["ids"][:200] = np.array(hit, np.uint64)[rng.integers(0, 40, 200)]
    case["ids"][200:230] = np.uint64(0)
    case["ids"][230:260] = cr.U64_MAX
    perm = rng.permutation(n)
    for k in ("desc", "ids", "xyz"):
        case[k] = case[k][perm]
    want = run_case(api, case, 0.2)
    assert {0, int(cr.U64_MAX)} <= set(int(v) for v in want["ids"]) and set(hit) <= set(int(v) for v in want["ids"])


def test_non_members_inside_a_partial_scope(api):
    case = cr.index_case(700, views=6, seed=4)
    t = case["tags"]
    for rows, tags in (((37, 651), (2, 5)), ((64, 128), None), ((0, 700), (3, 3)), ((300, 300), None), ((10, 690), (5, 2))):
        lo, hi = rows
        inside = (np.arange(700) >= lo) & (np.arange(700) < hi)
        want = run_case(api, case, 0.3, rows=rows, tags=tags)
        if rows == (37, 651):
            assert (t[inside] == -1).any() and ((t[inside] >= 0) & ((t[inside] < 2) | (t[inside] > 5))).any() and want["result"].n_dropped > 100
        if tags == (5, 2) or lo == hi:
            assert want["result"] == cr.Result(0, 0, 0, 0, 0, 700)


def test_identical_descriptors_the_latest_view_wins(api):
    case = cr.group_sizes_case([7, 2, 64, 70], seed=5)
    for v in np.unique(case["ids"]):
        rows = np.flatnonzero(case["ids"] == v)
        case["desc"][rows] = case["desc"][rows[0]]
    want = run_case(api, case, 0.0)
    for v in np.unique(case["ids"]):                  # radius 0 and the latest view the medoid: the latest row as it was
        last = np.flatnonzero(case["ids"] == v)[-1]
        at = int(np.flatnonzero(want["ids"] == v)[0])
        assert want["xyz"][at].tobytes() == case["xyz"][last].tobytes()


@pytest.mark.parametrize("radius", [0.0, 0.5, 1e6], ids=["zero", "cuts-one-off", "above-all"])
def test_the_gate(api, radius):
    case = cr.group_sizes_case([8] * 40, seed=6)
    for v in np.unique(case["ids"]):                  # per group: seven views within 0.05 of the centre, one 0.6 .. 1 off on one axis
        rows = np.flatnonzero(case["ids"] == v)
        centre = case["xyz"][rows[0]].copy()
        rng = np.random.default_rng(int(v) & 0xFFFF)
        case["xyz"][rows] = centre + rng.uniform(-0.05, 0.05, (8, 3)).astype(np.float32)
        case["xyz"][rows[rng.integers(0, 8)], rng.integers(0, 3)] += np.float32(rng.uniform(0.7, 1.0))
    far = run_case(api, case, radius)["result"].n_far_views
    assert (radius == 0.0 and far >= 7 * 38) or (radius == 0.5 and 30 <= far < 200) or (radius == 1e6 and far == 0), far


def test_70000_rows_at_the_default_slab(api):
    want = run_case(api, cr.index_case(70000, views=8, seed=7, none_every=0), 0.2, slab=0, again=False)
    assert 8000 < want["result"].n_groups < 9000 and want["result"].n_far_views > 5000


def test_every_refusal_changes_nothing(api):
    L = api._lib
    case = cr.index_case(100, views=4, seed=8)
    ix = make_index(api, case)

    def raw(**f):
        p = L.SvoConsolidateParams()
        L.lib.svo_consolidate_params_default(C.byref(p), 0.1)
        assert (p.row_lo, p.row_hi, p.tag_lo, p.tag_hi, p.reserved) == (0, -1, 0, 2 ** 31 - 1, 0) and p.radius == np.float32(0.1)
        for k, v in f.items():
            setattr(p, k, v)
        kept_before, res = np.full(101, -7, np.int32), L.SvoConsolidateResult()
        res.n_kept = -7
        rc = L.lib.svo_desc_index_consolidate(ix._h, C.byref(p), C.byref(res), L.ptr(kept_before))
        assert (kept_before == -7).all() and res.n_kept == -7
        return rc

    try:
        for lo, hi in ((-1, 5), (5, 3), (0, 101), (101, -1), (0, -2)):
            assert raw(row_lo=lo, row_hi=hi) == L.SVO_ERR_ARG, (lo, hi)
            refused(api, L.SVO_ERR_ARG, ix.read_rows, (lo, hi))
        for bad in (np.nan, np.inf, -np.inf, -1e-30):
            assert raw(radius=bad) == L.SVO_ERR_ARG, bad
        assert L.lib.svo_desc_index_consolidate(ix._h, None, None, None) == L.SVO_ERR_ARG
        assert L.lib.svo_desc_index_consolidate(None, None, None, None) == L.SVO_ERR_ARG
        assert not cr.same_rows(ix.read_rows(), cr.as_read(case)) and ix.size == 100
        plain = api.DescriptorIndex(16)
        try:
            plain.add(case["desc"][:8], case["ids"][:8])
            refused(api, L.SVO_ERR_STATE, plain.consolidate, 0.1)
            assert plain.size == 8
        finally:
            plain.close()
        # what is legal at the edges: an empty scope, no outputs
        assert ix.consolidate(0.1, rows=(100, -1))[1].tolist() == list(range(101)) and ix.consolidate(0.1, rows=(40, 40))[0].n_kept == 100
        p = ix.consolidate_params(0.0)
        assert L.lib.svo_desc_index_consolidate(ix._h, C.byref(p), None, None) == L.SVO_OK
        assert not cr.same_rows(ix.read_rows(), cr.as_read(cr.consolidate(case["desc"], case["ids"], case["xyz"], case["tags"], 0.0)))
    finally:
        ix.close()


def scratch_bound(m, slab, moving):
    """include/svo.h, "Landmark consolidation", Memory, under the growth rule of "Index maintenance": max(65 536, 2 need - 1)"""
    R = lambda b: (b + 255) // 256 * 256
    slots = 2
    while slots < 2 * m:
        slots *= 2
    need = R(m) + R(4 * (m + 1)) + R(4 * ((m + 255) // 256 + 257)) + 2 * R(4 * slots) + R(4 * m) + R(56 * min(slab, moving))
    return max(65536, 2 * need - 1)


def test_the_scratch_stays_within_the_stated_bound(api):
    for n, slab in ((300, 64), (5000, 64), (40000, 0)):
        case = cr.index_case(n, views=5, seed=n)
        ix = make_index(api, case, slab=slab)
        try:
            assert ix.retire_stats()["scratch_bytes"] == 0
            ix.consolidate(0.2, rows=(10, n - 10))
            st, bound = ix.retire_stats(), scratch_bound(n - 20, slab or 262144, n - 10)
            print(n, slab, st, bound)
            assert 0 < st["scratch_bytes"] <= bound and st["scratch_allocations"] == 1 and st["scratch_bytes_outgrown"] == 0
        finally:
            ix.close()


def test_consolidate_beside_frames_in_flight_changes_nothing(api):
    """a 9-sequence context with two frames submitted, consolidate and read_rows on an index, then the frames collected: equal in every
    bit to a run without the calls"""
    import torch
    w, h, B = 320, 160, 9
    S = streams(B, 3, 4100, w, h)
    Pl, Pr = projections(w, h)
    dev = [[(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in zip(*s)] for s in S]
    torch.cuda.synchronize()
    case = cr.index_case(3000, views=6, seed=9)
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
                check_call(ix, case, 0.2, (100, 2900), (1, 6))
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
