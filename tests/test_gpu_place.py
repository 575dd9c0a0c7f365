"""The descriptor index's place candidates (include/svo.h, "Place candidates": svo_desc_index_tag_votes, svo_desc_index_places,
svo_desc_index_places_from_ids) on a real GPU against the numpy reference (tests/place_ref.py) on the synthetic rows of
tests/place_cases.py.  Every rule is integers, so every comparison is equality, bit for bit: all four arrays of tag_votes, every
field of the result, every place's 32 bytes, and the recognised landmarks' lists.  The Python facade is what the tests call."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import place_cases as pc
import desc_match_ref as mref
import place_ref as pr
from stereo_visual_odometry_amd import _lib, api

pytestmark = pytest.mark.gpu

# the tags a vote scene's rows lie in (BIG_TAG and -1 apart): runs grow to about 900
SPAN = dict(runs=(0, 1023), one_tag=(0, 15), own_tag=(0, pc.VOTE_ROWS["own_tag"] - 1), interleaved=(0, 49))
_INDEX = {}


def index_of(kind):
    """one index per vote scene for the whole module: no call of this file changes an index"""
    if kind not in _INDEX:
        _INDEX[kind] = ac.build_index(api, pc.vote_scene(kind))
    return _INDEX[kind]


def check_votes(kind, lst, rows, span):
    c = pc.vote_scene(kind)
    want = pr.tag_votes(c["ids"], c["tags"], lst, rows, span)
    got = index_of(kind).tag_votes(lst, rows, span)
    for name, g, w in zip(("votes", "rows", "row_first", "row_end"), got, want):
        assert g.dtype == np.int32 and len(g) == span[1] - span[0] + 1 and g.tobytes() == w.tobytes(), (kind, len(lst), rows, span, name)
    return want


# ---- 1. tag_votes
@pytest.mark.parametrize("n", pc.ID_COUNTS)
@pytest.mark.parametrize("kind", pc.VOTE_KINDS)
def test_tag_votes_equals_the_reference(kind, n):
    """the whole index; the lists hold duplicated ids, ids absent from the index, ids 0 and 2^64 - 1, and ids whose probes collide"""
    votes, rows, _, _ = check_votes(kind, pc.id_list(kind, n), (0, -1), SPAN[kind])
    assert rows.sum() > 0 and (votes.sum() > 0) == (n > 0)


@pytest.mark.parametrize("rows", ((37, 69_001), (255, 257), (256, 512), (100, 163), (63, 64), (1000, 1000), (70_000, 70_000), (69_999, -1)))
def test_tag_votes_in_row_ranges_that_start_and_end_inside_waves_and_blocks(rows):
    check_votes("runs", pc.id_list("runs", 4096), rows, SPAN["runs"])


@pytest.mark.parametrize("kind, span", (("runs", (100, 300)), ("runs", (301, 301)), ("one_tag", (7, 7)), ("one_tag", (8, 20)), ("interleaved", (10, 39)),
                                        ("own_tag", (1000, 1064)), ("interleaved", (pc.BIG_TAG, pc.BIG_TAG)), ("one_tag", (6, 8))))
def test_tag_votes_with_tags_below_and_above_the_span(kind, span):
    """rows whose tag lies outside [tag_lo, tag_hi], rows without a point and rows tagged BIG_TAG sit inside the row range"""
    check_votes(kind, pc.id_list(kind, 4096), (0, -1), span)
    check_votes(kind, pc.id_list(kind, 65), (129, pc.VOTE_ROWS[kind] - 77), span)


def test_tag_votes_over_the_largest_span():
    """SVO_PLACE_MAX_TAGS bins: from 0, where every row of own_tag has its bin, and around BIG_TAG, where a twentieth of the rows meet in one"""
    votes, rows, _, _ = check_votes("own_tag", pc.id_list("own_tag", 4096), (0, -1), (0, pr.MAX_TAGS - 1))
    assert rows.sum() == pc.VOTE_ROWS["own_tag"] and votes.sum() > 0
    lo = pc.BIG_TAG - 5
    votes, rows, _, _ = check_votes("interleaved", pc.id_list("interleaved", 4096), (0, -1), (lo, lo + pr.MAX_TAGS - 1))
    assert rows[5] == rows.sum() > 500
    top = 2 ** 31 - 1
    check_votes("runs", pc.id_list("runs", 64), (0, -1), (top - pr.MAX_TAGS + 1, top))


def test_tag_votes_twice_with_different_spans_starts_from_cleared_bins():
    lst = pc.id_list("runs", 4096)
    for span in ((0, 1023), (50, 60), (0, 1023), (55, 700), (50, 60)):
        check_votes("runs", lst, (0, -1), span)
    for span in ((0, 49), (0, 3)):                     # another index, its own scratch
        check_votes("interleaved", pc.id_list("interleaved", 64), (0, -1), span)


@pytest.mark.parametrize("kind", pc.VOTE_KINDS)
def test_tag_votes_without_the_wave_combined_atomics_is_the_same(kind):
    index = index_of(kind)
    index.set_place_combine(False)
    try:
        check_votes(kind, pc.id_list(kind, 4096), (0, -1), SPAN[kind])
        check_votes(kind, pc.id_list(kind, 65), (33, pc.VOTE_ROWS[kind] - 1), SPAN[kind])
    finally:
        index.set_place_combine(True)


def test_tag_votes_outputs_may_be_null_and_an_empty_index_votes_nothing():
    index = index_of("interleaved")
    c = pc.vote_scene("interleaved")
    lst = pc.id_list("interleaved", 64)
    want = pr.tag_votes(c["ids"], c["tags"], lst, (0, -1), (0, 49))
    for keep in range(4):
        out = [np.full(50, -9, np.int32) if i == keep else None for i in range(4)]
        assert _lib.lib.svo_desc_index_tag_votes(index._h, len(lst), _lib.ptr(lst), 0, -1, 0, 49, *(_lib.ptr(a) for a in out)) == 0
        assert np.array_equal(out[keep], want[keep])
    empty = api.DescriptorIndex(8, points=True)
    try:
        assert all(not a.any() and len(a) == 3 for a in empty.tag_votes(lst, (0, -1), (0, 2)))
        res, places = empty.places_from_ids(lst, tags=(0, 2))
        assert res == (len(np.unique(lst)), 0, 0) and len(places) == 0
        res, places, cand = empty.places(c["desc"][:5], tags=(0, 2))
        assert res == (0, 0, 0) and len(places) == 0 and len(cand["query"]) == 0
    finally:
        empty.close()


# ---- 2. places
def check_places(index, c, query, matches=None, **kw):
    """places against the reference, every field; twice, for identical bytes -> the reference's dict.  matches: the reference's
    search of these queries in these rows, where a test computes it once for several calls"""
    ref_kw = dict(kw)
    span = ref_kw.pop("tags", (0, pr.MAX_TAGS - 1))
    want = pr.places(query, c["desc"], c["ids"], c["tags"], tag_span=span, matches=matches, **ref_kw)
    res, places, cand = index.places(query, **kw)
    assert res == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]), (res, kw)
    assert places.dtype == _lib.PLACE_DTYPE and places.tobytes() == want["places"].tobytes(), kw
    assert np.array_equal(cand["query"], want["cand_query"]) and np.array_equal(cand["row"], want["cand_row"]), kw
    again = index.places(query, **kw)
    assert again[0] == res and again[1].tobytes() == places.tobytes() and again[2]["row"].tobytes() == cand["row"].tobytes()
    return want


@pytest.fixture(scope="module")
def query_scene():
    """interleaved's rows and 4096 queries: every second one the descriptor of one of the rows NEAR with 0 .. 3 bits flipped (rows of
    one landmark have unrelated descriptors here, so a recognised row is a recognised landmark), the others random; and the
    reference's search of them in NEAR, which the reference needs about a second for"""
    c = pc.vote_scene("interleaved")
    rng = np.random.default_rng(11)
    src = rng.integers(NEAR[0], NEAR[1], 4096)
    q = ac.flip_bits(rng, c["desc"][src], rng.integers(0, 4, 4096))
    q[1::2] = rng.integers(0, 256, (2048, 32), dtype=np.uint8)
    return c, q, mref.match(q, c["desc"], c["ids"], *NEAR)


NEAR = (3_001, 6_002)                                 # the rows the 4096 queries are searched in: the reference's search stays short


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 4096))
def test_places_equals_the_reference(query_scene, n):
    c, q, m = query_scene
    index = index_of("interleaved")
    want = check_places(index, c, q[:n], m[:n], rows=NEAR, tags=(0, 49), max_places=64)
    assert want["n_landmarks"] <= (n + 1) // 2 and (n < 63 or want["n_landmarks"] > n // 4)          # the random queries recognise nothing
    sel = index.select(q[:n], np.zeros((n, 2), np.float32), row_lo=NEAR[0], row_hi=NEAR[1])          # the recognised landmarks are select's own
    cand = index.places(q[:n], rows=NEAR, tags=(0, 49))[2]
    assert cand["query"].tobytes() == sel["query"].tobytes() and cand["row"].tobytes() == sel["row"].tobytes() and len(sel["row"]) == want["n_landmarks"]
    if n == 4096:
        assert want["n_places"] == 50                  # every tag voted
        check_places(index, c, q, m, rows=NEAR, tags=(0, 49), max_places=64, separation=2, min_votes=30)
        check_places(index, c, q, m, rows=NEAR, tags=(5, 30), max_places=3, max_dist=1, ratio_num=1, ratio_den=2)
        for chunk in (64, 0):                          # the search's plan changes nothing
            index.chunk_rows = chunk
            check_places(index, c, q, m, rows=NEAR, tags=(0, 49), max_places=8, separation=1)
    if n == 65:                                        # the whole index, and a range that ends at its last row
        check_places(index, c, q[:n], tags=(0, 49))
        check_places(index, c, q[:n], rows=(NEAR[0], -1), tags=(0, 49), max_places=3)


@pytest.mark.parametrize("case", pc.PICK_CASES, ids=lambda c: c[0])
def test_rule_3_cases_through_real_descriptors(case):
    name, votes, tag_lo, min_votes, separation, max_places, want_tags = case
    c = pc.histogram_scene(votes, tag_lo)
    index = ac.build_index(api, c)
    try:
        span = (tag_lo, tag_lo + len(votes) - 1)
        kw = dict(tags=span, min_votes=min_votes, separation=separation, max_places=max_places)
        want = check_places(index, c, c["query"], **kw)
        assert want["n_landmarks"] == sum(votes)
        got_votes = index.tag_votes(c["ids"][want["cand_row"]], (0, -1), span)
        assert got_votes[0].tolist() == list(votes) and got_votes[1].tolist() == [v + 1 for v in votes]
        if want_tags is not None:
            assert want["places"]["tag"].tolist() == list(want_tags)
        else:
            assert want["n_places"] == 64
        res, places = index.places_from_ids(c["ids"][want["cand_row"]], **kw)       # the same landmarks, known by id
        assert res == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]) and places.tobytes() == want["places"].tobytes()
    finally:
        index.close()


@pytest.mark.parametrize("kind", ("runs", "own_tag"))
def test_places_from_ids_equals_the_reference(kind):
    c = pc.vote_scene(kind)
    index = index_of(kind)
    for n, kw in ((4096, dict(max_places=64)), (4096, dict(max_places=8, separation=3, min_votes=2)), (65, dict(rows=(500, 2_900), max_places=5)),
                  (0, dict()), (1, dict(tags=(0, pr.MAX_TAGS - 1)))):
        lst = pc.id_list(kind, n)
        ref_kw = dict(kw)
        span = ref_kw.pop("tags", SPAN[kind])
        want = pr.places_from_ids(c["ids"], c["tags"], lst, tag_span=span, **ref_kw)
        res, places = index.places_from_ids(lst, **dict(kw, tags=span))
        assert res == (want["n_landmarks"], want["n_tags_voted"], want["n_places"]), (kind, n, kw)
        assert places.tobytes() == want["places"].tobytes(), (kind, n, kw)
        assert want["n_places"] == 0 if n == 0 else (want["n_places"] > 0 or kw.get("min_votes", 1) > 1)     # one row a tag never has two votes


# ---- 3. the planted scene, end to end
def test_the_planted_scene_finds_the_keyframe_and_localizes_in_its_rows():
    c = pc.planted_scene()
    index = ac.build_index(api, c)
    try:
        span = (0, pc.KEYFRAMES - 1)
        want = check_places(index, c, c["query"], tags=span)
        assert want["places"]["tag"].tolist() == [5, 6, 7] and want["places"]["votes"].tolist() == [40, 40, 40]
        votes = index.tag_votes(c["query_ids"], (0, -1), span)[0]
        assert votes.tolist() == [0] * 5 + [40] * 3 + [0] * 4
        split = pr.best_row_votes(c["query"], c["desc"], c["ids"], c["tags"], tag_span=span)         # the vote by match's best row
        best = index.match(c["query"])
        assert np.bincount(c["tags"][best["row"]], minlength=pc.KEYFRAMES).tolist() == split.tolist() != votes.tolist()
        res, places, _ = index.places(c["query"], tags=span, separation=2)
        assert res == (40, 3, 1) and places["tag"].tolist() == [pc.QUERIED]
        top = places[0]
        lo, hi = int(top["row_first"]), int(top["row_end"])
        assert (c["tags"][lo:hi] == pc.QUERIED).all() and hi - lo == int(top["rows"]) == 120
        loc, cand = index.localize(pc.PLANTED_K.reshape(3, 3), c["query"], c["xy"], row_lo=lo, row_hi=hi)
        assert loc.success and loc.n_candidates == 40 and (cand["row"] >= lo).all() and (cand["row"] < hi).all()
    finally:
        index.close()


# ---- 4. refusals
def test_refusals_change_nothing():
    index = index_of("interleaved")
    lst = pc.id_list("interleaved", 64)
    size = index.size
    out = [np.full(4, 77, np.int32) for _ in range(4)]
    ARG, STATE = _lib.SVO_ERR_ARG, _lib.SVO_ERR_STATE
    for n, ids, rows, span in ((64, lst, (-1, 5), (0, 3)), (64, lst, (0, size + 1), (0, 3)), (64, lst, (5, 4), (0, 3)), (64, lst, (0, -1), (-1, 2)),
                               (64, lst, (0, -1), (3, 2)), (64, lst, (0, -1), (0, pr.MAX_TAGS)), (64, lst, (0, -1), (0, 2 ** 31 - 1)), (-1, lst, (0, -1), (0, 3)),
                               (4097, lst, (0, -1), (0, 3)), (64, None, (0, -1), (0, 3))):
        assert _lib.lib.svo_desc_index_tag_votes(index._h, n, _lib.ptr(ids), rows[0], rows[1], span[0], span[1], *(_lib.ptr(a) for a in out)) == ARG, (n, rows, span)
        assert all((a == 77).all() for a in out)
    q = pc.vote_scene("interleaved")["desc"][:8].copy()
    res, places = _lib.SvoPlaceResult(-7, -7, -7), np.full(64, -5, _lib.PLACE_DTYPE)
    cq, cr = np.full(8, 77, np.int32), np.full(8, 77, np.int32)
    for over in (dict(min_votes=0), dict(separation=-1), dict(max_places=0), dict(max_places=65), dict(max_dist=-1), dict(max_dist=257), dict(ratio_num=0),
                 dict(ratio_den=(1 << 20) + 1), dict(tag_lo=-1), dict(tag_lo=9, tag_hi=8), dict(tag_lo=0, tag_hi=pr.MAX_TAGS), dict(row_lo=-1), dict(row_hi=size + 1)):
        p = api.DescriptorIndex.place_params(tags=(0, 49), **over)
        assert _lib.lib.svo_desc_index_places(index._h, 8, _lib.ptr(q), C.byref(p), C.byref(res), _lib.ptr(places), _lib.ptr(cq), _lib.ptr(cr)) == ARG, over
        if not {"max_dist", "ratio_num", "ratio_den"} & set(over):
            assert _lib.lib.svo_desc_index_places_from_ids(index._h, 64, _lib.ptr(lst), C.byref(p), C.byref(res), _lib.ptr(places)) == ARG, over
        assert (res.n_landmarks, res.n_tags_voted, res.n_places) == (-7, -7, -7) and (places["tag"] == -5).all() and (cq == 77).all() and (cr == 77).all()
    p = api.DescriptorIndex.place_params(tags=(0, 49))
    assert _lib.lib.svo_desc_index_places(index._h, 4097, _lib.ptr(q), C.byref(p), C.byref(res), _lib.ptr(places), None, None) == ARG
    assert _lib.lib.svo_desc_index_places(index._h, 8, None, C.byref(p), C.byref(res), _lib.ptr(places), None, None) == ARG
    assert _lib.lib.svo_desc_index_places(index._h, 8, _lib.ptr(q), None, C.byref(res), _lib.ptr(places), None, None) == ARG
    assert _lib.lib.svo_desc_index_places_from_ids(index._h, 4097, _lib.ptr(lst), C.byref(p), C.byref(res), _lib.ptr(places)) == ARG
    plain = api.DescriptorIndex(16)                    # an index without points has no tags
    try:
        plain.add(np.zeros((8, 32), np.uint8), np.arange(8))
        assert _lib.lib.svo_desc_index_tag_votes(plain._h, 64, _lib.ptr(lst), 0, -1, 0, 3, *(_lib.ptr(a) for a in out)) == STATE
        assert _lib.lib.svo_desc_index_places(plain._h, 8, _lib.ptr(q), C.byref(p), C.byref(res), _lib.ptr(places), None, None) == STATE
        assert _lib.lib.svo_desc_index_places_from_ids(plain._h, 64, _lib.ptr(lst), C.byref(p), C.byref(res), _lib.ptr(places)) == STATE
    finally:
        plain.close()
    check_votes("interleaved", lst, (0, -1), (0, 49))   # and the index answers as before


# ---- 5. beside frames in flight
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
    out, found = [], 0
    try:
        for k0 in range(0, N_FRAMES, 3):
            for k in range(k0, k0 + 3):
                vo.submit_device([dev[k][0].data_ptr()], [dev[k][1].data_ptr()], W)
                if ix:                                 # frames in flight: the call waits for its own stream only
                    found += ix.places(c["query"], tags=(0, 11))[1]["tag"].tolist() == [5, 6, 7]
            for k in range(k0, k0 + 3):
                if ix:
                    found += ix.places_from_ids(c["query_ids"], tags=(0, 11), separation=2)[1]["tag"].tolist() == [5]
                    found += int(ix.tag_votes(c["query_ids"], (0, -1), (0, 11))[0].sum()) == 120
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


def test_place_calls_beside_frames_in_flight_change_nothing():
    plain, beside = run_in_flight(False), run_in_flight(True)
    assert len(plain) == len(beside) > 0
    for k, (a, b) in enumerate(zip(plain, beside)):
        assert a == b, "frame %d" % k
    assert sum(len(a[3]) for a in plain) > 32 * 500
