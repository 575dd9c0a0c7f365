"""The batched place candidates (include/svo.h, "Batched place candidates": svo_desc_index_tag_votes_batch, places_from_ids_batch,
places_batch) on a real GPU.  The oracle is the contract: the single calls on the same index, camera by camera and field by field,
and the numpy reference (tests/place_batch_ref.py) as well; every camera of every call is compared.  Every rule is integers, so
every comparison is equality, bit for bit.  The rows are tests/place_cases.py's vote scenes, the lists tests/place_batch_cases.py's.
The Python facade is what the tests call."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import desc_match_ref as mref
import place_batch_cases as pbc
import place_batch_ref as pbr
import place_cases as pc
import place_ref as pr
from stereo_visual_odometry_amd import _lib, api

pytestmark = pytest.mark.gpu

SPAN = dict(runs=(0, 1023), one_tag=(0, 15), own_tag=(0, pc.VOTE_ROWS["own_tag"] - 1), interleaved=(0, 49))
_INDEX = {}


def index_of(kind):
    """one index per vote scene for the whole module: no call of this file changes an index"""
    if kind not in _INDEX:
        _INDEX[kind] = ac.build_index(api, pc.vote_scene(kind))
    return _INDEX[kind]


def check_votes(kind, lists, rows=(0, -1), span=None, reference=True):
    """tag_votes_batch against the single call for every camera and against the reference -> the batch's four arrays"""
    span = SPAN[kind] if span is None else span
    index, c = index_of(kind), pc.vote_scene(kind)
    nb = span[1] - span[0] + 1
    got = index.tag_votes_batch(lists, rows, span)
    assert got[0].shape == (len(lists), nb) and all(a.dtype == np.int32 for a in got) and all(len(a) == nb for a in got[1:])
    for b, m in enumerate(lists):
        one = index.tag_votes(m, rows, span)
        assert got[0][b].tobytes() == one[0].tobytes(), (kind, b, len(m), rows, span)
        for name, g, w in zip(("rows", "row_first", "row_end"), got[1:], one[1:]):
            assert g.tobytes() == w.tobytes(), (kind, b, name, rows, span)
    if reference:
        want = pbr.tag_votes_batch(c["ids"], c["tags"], lists, rows, span)
        for name, g, w in zip(("votes", "rows", "row_first", "row_end"), got, want):
            assert g.tobytes() == w.tobytes(), (kind, name, rows, span)
    return got


def check_places_from_ids(kind, lists, reference=True, **kw):
    """places_from_ids_batch against the single call for every camera and against the reference -> the batch's list"""
    index, c = index_of(kind), pc.vote_scene(kind)
    kw.setdefault("tags", SPAN[kind])
    got = index.places_from_ids_batch(lists, **kw)
    assert len(got) == len(lists)
    ref_kw = dict(kw)
    span = ref_kw.pop("tags")
    for b, m in enumerate(lists):
        res, places = index.places_from_ids(m, **kw)
        assert got[b][0] == res and got[b][1].dtype == _lib.PLACE_DTYPE and got[b][1].tobytes() == places.tobytes(), (kind, b, kw)
        if reference:
            w = pr.places_from_ids(c["ids"], c["tags"], m, tag_span=span, **ref_kw)
            assert res == (w["n_landmarks"], w["n_tags_voted"], w["n_places"]) and places.tobytes() == w["places"].tobytes(), (kind, b, kw)
    return got


# ---- 1. the number of cameras
@pytest.mark.parametrize("cameras", (1, 2, 9, 65))
def test_camera_counts(cameras):
    lists = pbc.small_lists("interleaved", cameras)
    votes = check_votes("interleaved", lists)[0]
    assert (votes.sum(1) > 0).all()
    check_places_from_ids("interleaved", lists, max_places=5, separation=1)


def test_1024_cameras_of_4_ids():
    lists = pbc.small_lists("own_tag", 1024)
    rows = (5, 1_001)                                  # the reference walks these rows once a camera
    votes = check_votes("own_tag", lists, rows)[0]
    assert (votes.sum(1) > 0).sum() > 512
    got = check_places_from_ids("own_tag", lists, rows=rows, max_places=3)
    assert sum(g[0].n_places > 0 for g in got) > 512
    # the cameras' order changes nothing but the order of the results
    rev = index_of("own_tag").places_from_ids_batch(lists[::-1], rows=rows, tags=SPAN["own_tag"], max_places=3)[::-1]
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, rev))


# ---- 2. the lists
@pytest.mark.parametrize("kind", pc.VOTE_KINDS)
def test_slices_of_0_1_63_64_65_and_4096_entries_in_one_call(kind):
    """runs: tag runs of 1, 63, 64, 65 and 700 rows; own_tag: a tag per row; one_tag: one tag for all.  The lists hold duplicates,
    absent ids, ids 0 and 2^64 - 1 and ids several cameras share; rows without a point and rows of other tags lie in the range"""
    lists = pbc.mixed_lists(kind)
    assert tuple(len(m) for m in lists) == pbc.SLICES
    votes = check_votes(kind, lists)[0]
    assert not votes[0].any() and votes[1].sum() > 0 and votes[5].sum() > votes[4].sum() > 0
    got = check_places_from_ids(kind, lists, max_places=64)
    assert [g[0].n_landmarks for g in got] == [len(np.unique(m)) for m in lists]
    check_places_from_ids(kind, lists, max_places=8, separation=3, min_votes=2)


def test_a_call_whose_cameras_all_have_empty_slices():
    empty = [np.zeros(0, np.uint64)] * 5
    got = check_votes("interleaved", empty)
    assert not got[0].any() and got[1].sum() > 0
    assert all(g[0] == (0, 0, 0) and len(g[1]) == 0 for g in check_places_from_ids("interleaved", empty))
    out = index_of("interleaved").places_batch([np.zeros((0, 32), np.uint8)] * 3, tags=(0, 49))
    assert all(r == (0, 0, 0) and len(p) == 0 and len(c["query"]) == 0 for r, p, c in out)
    assert index_of("interleaved").places_from_ids_batch([]) == [] and index_of("interleaved").places_batch([]) == []
    assert index_of("interleaved").tag_votes_batch([], tags=(0, 3))[0].shape == (0, 4)


def test_an_id_held_by_1_2_64_65_and_all_cameras():
    lists = pbc.shared_lists("interleaved")
    u = pc.vote_scene("interleaved")["universe"]
    assert [sum(u[10 + i] in m for m in lists) for i in range(5)] == list(pbc.HELD_BY)
    check_votes("interleaved", lists)
    check_places_from_ids("interleaved", lists, max_places=4)


def test_ids_that_collide_under_the_tables_hash():
    lists = pbc.colliding_lists("interleaved")
    votes = check_votes("interleaved", lists)[0]
    assert (votes.sum(1) > 0).all()
    got = check_places_from_ids("interleaved", lists)
    assert all(g[0].n_landmarks == len(np.unique(m)) < len(m) for g, m in zip(got, lists))


# ---- 3. the rows and the window
@pytest.mark.parametrize("rows", ((37, 69_001), (255, 257), (100, 163), (63, 64), (1000, 1000), (69_999, -1)))
def test_row_ranges_that_start_and_end_inside_waves(rows):
    check_votes("runs", pbc.mixed_lists("runs")[2:], rows)


@pytest.mark.parametrize("kind, span", (("runs", (301, 301)), ("one_tag", (7, 7)), ("one_tag", (8, 8)), ("interleaved", (10, 39)),
                                        ("interleaved", (pc.BIG_TAG, pc.BIG_TAG)), ("own_tag", (1000, 1064))))
def test_tag_windows_of_one_bin_and_tags_outside_the_window(kind, span):
    check_votes(kind, pbc.mixed_lists(kind), (0, -1), span)
    check_places_from_ids(kind, pbc.mixed_lists(kind)[3:], tags=span, rows=(129, pc.VOTE_ROWS[kind] - 77), max_places=2)


def test_one_call_on_exactly_2_to_the_24_bins():
    """16 cameras x 2^20 tags"""
    lists = pbc.small_lists("own_tag", 16, 64)
    votes = check_votes("own_tag", lists, (0, -1), (0, pr.MAX_TAGS - 1))[0]
    assert votes.shape == (16, 1 << 20) and (votes.sum(1) > 0).all() and not votes[:, pc.VOTE_ROWS["own_tag"]:].any()


def test_calls_of_different_shapes_back_to_back_start_from_a_clean_table_and_clean_votes():
    wide, narrow = pbc.mixed_lists("runs"), pbc.small_lists("interleaved", 9)
    few = [np.array(m[:3]) for m in wide[2:5]]
    for lists, span in ((wide, (0, 1023)), (few, (50, 60)), (wide, (0, 1023)), (few[:1], (0, 1023)), (wide, (55, 700))):
        check_votes("runs", lists, (0, -1), span, reference=False)
        check_places_from_ids("runs", lists, reference=False, tags=span, max_places=6)
    check_votes("interleaved", narrow)                 # another index, its own scratch


# ---- 4. places_batch
NEAR = (3_001, 6_002)                                 # the rows the queries are searched in: the reference's search stays short
CAMERA_QUERIES = ((0, 0), (0, 1), (1, 64), (64, 128), (128, 193), (0, 4096))


@pytest.fixture(scope="module")
def query_scene():
    """test_gpu_place.py's: interleaved's rows and 4096 queries, every second one a row of NEAR with 0 .. 3 bits flipped, the others
    random, with the reference's search of them in NEAR; the cameras take slices of 0, 1, 63, 64, 65 and 4096 of them"""
    c = pc.vote_scene("interleaved")
    rng = np.random.default_rng(11)
    src = rng.integers(NEAR[0], NEAR[1], 4096)
    q = ac.flip_bits(rng, c["desc"][src], rng.integers(0, 4, 4096))
    q[1::2] = rng.integers(0, 256, (2048, 32), dtype=np.uint8)
    m = mref.match(q, c["desc"], c["ids"], *NEAR)
    return c, [q[a:b] for a, b in CAMERA_QUERIES], [m[a:b] for a, b in CAMERA_QUERIES]


def check_places(index, c, queries, matches, **kw):
    got = index.places_batch(queries, **kw)
    assert len(got) == len(queries)
    ref_kw = dict(kw)
    span = ref_kw.pop("tags", (0, pr.MAX_TAGS - 1))
    want = pbr.places_batch(queries, c["desc"], c["ids"], c["tags"], matches=matches, tag_span=span, **ref_kw)
    for b, q in enumerate(queries):
        res, places, cand = index.places(q, **kw)
        g, w = got[b], want[b]
        assert g[0] == res == (w["n_landmarks"], w["n_tags_voted"], w["n_places"]), (b, kw)
        assert g[1].tobytes() == places.tobytes() == w["places"].tobytes(), (b, kw)
        assert g[2]["query"].tobytes() == cand["query"].tobytes() and g[2]["row"].tobytes() == cand["row"].tobytes(), (b, kw)
        assert np.array_equal(cand["query"], w["cand_query"]) and np.array_equal(cand["row"], w["cand_row"]), (b, kw)
    return got


def test_places_batch_equals_the_single_calls_and_the_reference(query_scene):
    c, queries, matches = query_scene
    index = index_of("interleaved")
    got = check_places(index, c, queries, matches, rows=NEAR, tags=(0, 49), max_places=64)
    assert [g[0].n_landmarks > 0 for g in got] == [False, True, True, True, True, True] and got[5][0].n_places == 50
    check_places(index, c, queries, matches, rows=NEAR, tags=(5, 30), max_places=3, max_dist=1, ratio_num=1, ratio_den=2)
    try:
        for chunk in (64, 0):                          # the search's plan changes nothing
            index.chunk_rows = chunk
            check_places(index, c, queries, matches, rows=NEAR, tags=(0, 49), max_places=8, separation=1, min_votes=30)
    finally:
        index.chunk_rows = 0
    again = index.places_batch(queries[::-1], rows=NEAR, tags=(0, 49), max_places=64)[::-1]        # the cameras' order
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2]["row"].tobytes() == b[2]["row"].tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("case", pc.PICK_CASES, ids=lambda c: c[0])
def test_rule_3_per_camera(case):
    """ties, separation, min_votes and max_places: every camera asks for its own part of the histogram's landmarks"""
    name, votes, tag_lo, min_votes, separation, max_places, want_tags = case
    c = pc.histogram_scene(votes, tag_lo)
    index = ac.build_index(api, c)
    try:
        q = c["query"]
        queries = [q, q[::2], q[1::2], q[:0], q[:len(q) // 3], q[::-1]]
        kw = dict(tags=(tag_lo, tag_lo + len(votes) - 1), min_votes=min_votes, separation=separation, max_places=max_places)
        got = check_places(index, c, queries, None, **kw)
        if want_tags is not None:
            assert got[0][1]["tag"].tolist() == list(want_tags) == got[5][1]["tag"].tolist()
        lists = [c["ids"][g[2]["row"]] for g in got]   # the same landmarks, known by id
        by_id = index.places_from_ids_batch(lists, **kw)
        assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(by_id, got))
    finally:
        index.close()


# ---- 5. refusals
def test_refusals_change_nothing():
    index = index_of("interleaved")
    lists = pbc.small_lists("interleaved", 9)
    begin, ids = pbc.offsets(lists), np.concatenate(lists)
    size = index.size
    ARG, STATE = _lib.SVO_ERR_ARG, _lib.SVO_ERR_STATE
    lib, ptr = _lib.lib, _lib.ptr
    votes, out = np.full(64, 77, np.int32), [np.full(8, 77, np.int32) for _ in range(3)]
    res = (_lib.SvoPlaceResult * 9)(*[_lib.SvoPlaceResult(-7, -7, -7) for _ in range(9)])
    places = np.full(9 * 64, -5, _lib.PLACE_DTYPE)
    cq, cr = np.full(64, 77, np.int32), np.full(64, 77, np.int32)
    q = pc.vote_scene("interleaved")["desc"][:36].copy()
    good = api.DescriptorIndex.place_params(tags=(0, 3))

    def untouched():
        return (votes == 77).all() and all((a == 77).all() for a in out) and all((r.n_landmarks, r.n_tags_voted, r.n_places) == (-7, -7, -7) for r in res) and \
            (places["tag"] == -5).all() and (cq == 77).all() and (cr == 77).all()

    def all_three(n, bg, expect=ARG):
        """a call's offsets, refused alike by the three entries"""
        assert lib.svo_desc_index_tag_votes_batch(index._h, n, ptr(bg), ptr(ids), 0, -1, 0, 3, ptr(votes), *(ptr(a) for a in out)) == expect, (n, bg)
        assert lib.svo_desc_index_places_from_ids_batch(index._h, n, ptr(bg), ptr(ids), C.byref(good), res, ptr(places)) == expect, (n, bg)
        assert lib.svo_desc_index_places_batch(index._h, n, ptr(bg), ptr(q), C.byref(good), res, ptr(places), ptr(cq), ptr(cr)) == expect, (n, bg)
        assert untouched()

    all_three(-1, begin); all_three(1025, begin); all_three(9, None)
    all_three(2, np.array([1, 2, 3], np.int32)); all_three(2, np.array([0, 5, 4], np.int32)); all_three(1, np.array([0, 4097], np.int32))
    all_three(257, (np.arange(258) * 4096).astype(np.int32))                # 257 x 4096 > 1 << 20 in all
    for rows, span in (((-1, 5), (0, 3)), ((0, size + 1), (0, 3)), ((5, 4), (0, 3)), ((0, -1), (-1, 2)), ((0, -1), (3, 2)), ((0, -1), (0, pr.MAX_TAGS)),
                       ((0, -1), (0, 2 ** 31 - 1))):
        assert lib.svo_desc_index_tag_votes_batch(index._h, 9, ptr(begin), ptr(ids), rows[0], rows[1], span[0], span[1], ptr(votes), *(ptr(a) for a in out)) == ARG, (rows, span)
        assert untouched()
    b17 = np.zeros(18, np.int32)                       # 17 x 2^20 bins; and 1024 x 16 385
    assert lib.svo_desc_index_tag_votes_batch(index._h, 17, ptr(b17), None, 0, -1, 0, pr.MAX_TAGS - 1, ptr(votes), *(ptr(a) for a in out)) == ARG
    assert b"narrow the tag window" in lib.svo_last_error()
    b1024 = np.zeros(1025, np.int32)
    assert lib.svo_desc_index_tag_votes_batch(index._h, 1024, ptr(b1024), None, 0, -1, 5, 5 + 16384, ptr(votes), *(ptr(a) for a in out)) == ARG
    wide = api.DescriptorIndex.place_params(tags=(0, pr.MAX_TAGS - 1))
    assert lib.svo_desc_index_places_from_ids_batch(index._h, 17, ptr(b17), None, C.byref(wide), res, ptr(places)) == ARG
    assert lib.svo_desc_index_places_batch(index._h, 17, ptr(b17), None, C.byref(wide), res, ptr(places), ptr(cq), ptr(cr)) == ARG
    assert lib.svo_desc_index_tag_votes_batch(index._h, 9, ptr(begin), None, 0, -1, 0, 3, ptr(votes), *(ptr(a) for a in out)) == ARG      # null ids
    assert lib.svo_desc_index_places_batch(index._h, 9, ptr(begin), None, C.byref(good), res, ptr(places), ptr(cq), ptr(cr)) == ARG       # null queries
    assert untouched()
    for over in (dict(min_votes=0), dict(separation=-1), dict(max_places=0), dict(max_places=65), dict(max_dist=-1), dict(max_dist=257), dict(ratio_num=0),
                 dict(ratio_den=(1 << 20) + 1), dict(tag_lo=-1), dict(tag_lo=9, tag_hi=8), dict(tag_lo=0, tag_hi=pr.MAX_TAGS), dict(row_lo=-1), dict(row_hi=size + 1)):
        p = api.DescriptorIndex.place_params(tags=(0, 49), **over)
        assert lib.svo_desc_index_places_batch(index._h, 9, ptr(begin), ptr(q), C.byref(p), res, ptr(places), ptr(cq), ptr(cr)) == ARG, over
        if not {"max_dist", "ratio_num", "ratio_den"} & set(over):
            assert lib.svo_desc_index_places_from_ids_batch(index._h, 9, ptr(begin), ptr(ids), C.byref(p), res, ptr(places)) == ARG, over
        assert untouched()
    assert lib.svo_desc_index_places_batch(index._h, 9, ptr(begin), ptr(q), None, res, ptr(places), None, None) == ARG
    assert lib.svo_desc_index_places_from_ids_batch(index._h, 9, ptr(begin), ptr(ids), None, res, ptr(places)) == ARG
    assert lib.svo_desc_index_places_from_ids_batch(None, 9, ptr(begin), ptr(ids), C.byref(good), res, ptr(places)) == ARG
    plain = api.DescriptorIndex(16)                    # an index without points has no tags
    try:
        plain.add(np.zeros((8, 32), np.uint8), np.arange(8))
        assert lib.svo_desc_index_tag_votes_batch(plain._h, 9, ptr(begin), ptr(ids), 0, -1, 0, 3, ptr(votes), *(ptr(a) for a in out)) == STATE
        assert lib.svo_desc_index_places_from_ids_batch(plain._h, 9, ptr(begin), ptr(ids), C.byref(good), res, ptr(places)) == STATE
        assert lib.svo_desc_index_places_batch(plain._h, 9, ptr(begin), ptr(q), C.byref(good), res, ptr(places), ptr(cq), ptr(cr)) == STATE
    finally:
        plain.close()
    assert untouched()
    # every output may be null, and zero cameras writes nothing
    assert lib.svo_desc_index_tag_votes_batch(index._h, 9, ptr(begin), ptr(ids), 0, -1, 0, 3, None, None, None, None) == 0
    assert lib.svo_desc_index_places_from_ids_batch(index._h, 9, ptr(begin), ptr(ids), C.byref(good), None, None) == 0
    assert lib.svo_desc_index_places_batch(index._h, 9, ptr(begin), ptr(q), C.byref(good), None, None, None, None) == 0
    assert lib.svo_desc_index_tag_votes_batch(index._h, 0, None, None, 0, -1, 0, 3, ptr(votes), *(ptr(a) for a in out)) == 0 and untouched()
    keep = np.full(4, -9, np.int32)                    # one output alone
    assert lib.svo_desc_index_tag_votes_batch(index._h, 9, ptr(begin), ptr(ids), 0, -1, 0, 3, None, None, ptr(keep), None) == 0
    assert np.array_equal(keep, index.tag_votes(lists[0], (0, -1), (0, 3))[2])
    check_votes("interleaved", lists)                  # and the index answers as before


def test_nothing_beyond_a_cameras_entries_is_written():
    index = index_of("interleaved")
    lists = pbc.mixed_lists("interleaved")
    begin, ids = pbc.offsets(lists), np.concatenate(lists)
    B = len(lists)
    p = api.DescriptorIndex.place_params(tags=(0, 49), max_places=64, min_votes=3)
    res = (_lib.SvoPlaceResult * B)()
    places = np.full((B, 64), -5, _lib.PLACE_DTYPE)
    assert _lib.lib.svo_desc_index_places_from_ids_batch(index._h, B, _lib.ptr(begin), _lib.ptr(ids), C.byref(p), res, _lib.ptr(places)) == 0
    for b in range(B):
        assert (places[b, :res[b].n_places]["tag"] >= 0).all() and (places[b, res[b].n_places:]["tag"] == -5).all() and res[b].n_places < 64


# ---- 6. beside frames in flight
def run_in_flight(with_index):
    """test_gpu_reloc_frames' six frames as device frames, three in flight -> per frame (ok, pose, observation rows, descriptor rows) as bytes"""
    import torch
    from test_gpu_reloc_frames import N_FRAMES, W, context, frames
    L, R = frames()
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in zip(L, R)]
    torch.cuda.synchronize()
    vo = context(api)
    c = pc.planted_scene()
    ix = ac.build_index(api, c) if with_index else None
    q, qi = c["query"], c["query_ids"]
    out, found = [], 0
    try:
        for k0 in range(0, N_FRAMES, 3):
            for k in range(k0, k0 + 3):
                vo.submit_device([dev[k][0].data_ptr()], [dev[k][1].data_ptr()], W)
                if ix:                                 # frames in flight: the call waits for its own stream only
                    got = ix.places_batch([q, q[:10], q[:0]], tags=(0, 11))
                    found += [g[1]["tag"].tolist() for g in got] == [[5, 6, 7], [5, 6, 7], []]
            for k in range(k0, k0 + 3):
                if ix:
                    got = ix.places_from_ids_batch([qi, qi[:1]], tags=(0, 11), separation=2)
                    found += [g[1]["tag"].tolist() for g in got] == [[5], [5]]
                    found += ix.tag_votes_batch([qi, qi[:7]], (0, -1), (0, 11))[0].sum(1).tolist() == [120, 21]
                ok, T = vo.collect()
                out.append((ok.tobytes(), T.tobytes(), vo.last_track_obs(0).tobytes(), vo.last_track_descriptors(0).tobytes()))
        if ix:
            assert found == 3 * N_FRAMES
    finally:
        vo.close()
        if ix:
            ix.close()
        del dev
    return out


def test_batch_calls_between_submit_and_collect_change_nothing():
    plain, beside = run_in_flight(False), run_in_flight(True)
    assert len(plain) == len(beside) > 0
    for k, (a, b) in enumerate(zip(plain, beside)):
        assert a == b, "frame %d" % k
