"""The relocaliser's selection on a real GPU (include/svo.h, "Relocalisation": svo_desc_index_select, svo_desc_index_localize) against
tests/reloc_ref.py on the host's copies of the same arrays — every field of every candidate: query, row, pixel and point bits.

The inputs are tests/reloc_cases.py's: 4096 queries whose planned distances put a query on each side of every clause of rule 1
(dist == max_dist and max_dist + 1, dist * den == dist2 * num, a best row without a point), ids shared between the queries (0, 4095),
(j, j + 64), (j, j + 1024) at equal and unequal distances, three queries of one id, and a loser that was the only query between two
survivors.  The reference search over the 4096 x 4608 case runs once (a few seconds of numpy); every test slices it.  Sizes 1, 63,
64, 65, 1023, 1025, 4096 are prefixes of that list; 4097 queries are refused.  Then: nothing and everything accepted, a lone candidate
(dist2 = 257), a search that takes two k_desc_match launches, the gate at min_candidates - 1 and min_candidates, localize against
api.cameraToWorld on select's arrays byte for byte, and the refusals."""
import numpy as np
import pytest

import desc_match_ref as mref
import reloc_cases as cases
import reloc_ref as rref
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

RULE = dict(max_dist=40, ratio_num=7, ratio_den=10)


@pytest.fixture(scope="module")
def big(api):
    """the clause case in an index, and the reference's search rows for all of its queries over the whole index"""
    c = cases.clause_case()
    ix = api.DescriptorIndex(len(c["desc"]) + 8, points=True)
    cases.fill(ix, c)
    assert ix.size == len(c["desc"])
    c["rows"] = mref.match(c["query"], c["desc"], c["ids"])
    c["ix"] = ix
    yield c
    ix.close()


def expect(c, which, **rule):
    """the reference's candidates for the queries `which` (indices into the case's list) from the search rows computed once"""
    q, r = rref.select(c["rows"][which], c["tags"], **dict(RULE, **rule))
    return dict(query=q, row=r, xy=c["xy"][which][q], xyz=c["xyz"][r])


def same(got, want):
    assert got["query"].tolist() == want["query"].tolist()
    assert got["row"].tolist() == want["row"].tolist()
    assert got["xy"].tobytes() == want["xy"].tobytes() and got["xyz"].tobytes() == want["xyz"].tobytes()


def test_the_case_is_what_it_plans(big):
    """the search returns the planned distances where a clause is named, so that each clause does decide somewhere"""
    rows, d1, d2 = big["rows"], big["d1"], big["d2"]
    assert (rows["row"] == big["row_a"]).all() and (rows["dist"] == d1).all()
    planned = d2 > 0
    assert (rows["dist2"][planned] == d2[planned]).all() and (rows["dist2"][~planned] > 70).all()
    want = expect(big, np.arange(cases.N))
    kept = set(want["query"].tolist())
    first = [j for j in range(16) if j in kept]
    assert first == [0, 1, 4, 7, 8, 9, 12, 15], first                   # kinds 2, 3, 5, 6 rejected; 1 (dist == max_dist) kept
    for loser, winner in ((4095, 0), (72, 8), (16, 80), (1028, 4), (24, 1048), (1500, 100), (3000, 100)):
        assert loser not in kept and winner in kept, (loser, winner)
    assert 15 in kept and 17 in kept                                    # 16 was the only accepted query between them
    # kinds 0, 1, 4, 7 below N_B; above it kinds 3 and 6 have no planned second row and pass too; seven shared ids
    assert len(kept) == cases.N_B // 2 + (cases.N - cases.N_B) * 6 // 8 - 7


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 4096])
def test_select_equals_the_reference_at_every_size(big, n):
    which = np.arange(n)
    same(big["ix"].select(big["query"][:n], big["xy"][:n], **RULE), expect(big, which))


def test_select_from_the_middle_of_the_list(big):
    which = np.arange(700, 700 + 1500)                                  # other wave and pass boundaries than a prefix has
    same(big["ix"].select(big["query"][which], big["xy"][which], **RULE), expect(big, which))


def test_4097_queries_are_refused(api, big):
    q = np.zeros((4097, 32), np.uint8)
    with pytest.raises(api._lib.SvoError, match="status %d" % api._lib.SVO_ERR_ARG):
        big["ix"].select(q, np.zeros((4097, 2), np.float32))


def test_nothing_and_everything_accepted(big):
    allq = np.arange(cases.N)
    none = big["ix"].select(big["query"], big["xy"], max_dist=0, ratio_num=7, ratio_den=10)
    assert len(none["query"]) == 0 and len(expect(big, allq, max_dist=0)["query"]) == 0
    # every query whose row has a point, under the widest rule: all of them pass rule 1, so only the shared ids drop anything
    which = np.flatnonzero(big["tags"][big["row_a"]] >= 0)
    wide = dict(max_dist=256, ratio_num=1 << 20, ratio_den=1)
    got = big["ix"].select(big["query"][which], big["xy"][which], **wide)
    same(got, expect(big, which, **wide))
    assert len(got["query"]) == len(np.unique(big["rows"]["id"][which])) == len(which) - 7


def test_a_lone_candidate_passes_with_dist2_257(big):
    j = 1                                                               # kind 1: dist 40 == max_dist
    row = int(big["row_a"][j])
    rows = mref.match(big["query"][:64], big["desc"], big["ids"], row, row + 1)
    assert rows["dist2"][j] == mref.NO_DIST and rows["dist"][j] == 40 and (np.delete(rows["dist"], j) > 40).all()
    q, r = rref.select(rows, big["tags"], **RULE)
    got = big["ix"].select(big["query"][:64], big["xy"][:64], row_lo=row, row_hi=row + 1, **RULE)
    assert got["query"].tolist() == q.tolist() == [j] and got["row"].tolist() == r.tolist() == [row]
    empty = big["ix"].select(big["query"][:64], big["xy"][:64], row_lo=row, row_hi=row, **RULE)    # an empty range: rows of SVO_MATCH_NONE
    assert len(empty["query"]) == 0


def test_a_search_of_two_launches(big):
    """chunk_rows = 1 over 1100 rows: 1100 partial states per query, 4096 x 1100 is beyond the budget of one launch (1 << 22), so the
    search is two k_desc_match launches back to back, the second one's queries and result rows at an offset"""
    ix, n_rows = big["ix"], 1100
    first = (1 << 22) // n_rows // 64 * 64                              # the queries of the first launch
    assert 4096 * n_rows > 1 << 22 and 2048 <= first < 4096
    hi = big["n_with"]                                                  # the last 1100 rows with points: those of the last ~1260 queries
    lo = hi - n_rows
    rows = mref.match(big["query"], big["desc"], big["ids"], lo, hi)
    q, r = rref.select(rows, big["tags"], **RULE)
    ix.chunk_rows = 1
    try:
        got = ix.select(big["query"], big["xy"], row_lo=lo, row_hi=hi, **RULE)
    finally:
        ix.chunk_rows = 0
    assert got["query"].tolist() == q.tolist() and got["row"].tolist() == r.tolist()
    assert got["xy"].tobytes() == big["xy"][q].tobytes() and got["xyz"].tobytes() == big["xyz"][r].tobytes()
    assert (q < first).sum() > 100 and (q >= first).sum() > 100         # candidates from both launches' queries


@pytest.fixture(scope="module")
def world(api):
    s = cases.scene(40, 5, outliers=6)
    ix = api.DescriptorIndex(64, points=True)
    ix.add_points(s["desc"], s["ids"], s["xyz"], s["tags"])
    s["ix"] = ix
    yield s
    ix.close()


def test_the_gate(world):
    s, ix = world, world["ix"]
    want = rref.select_index(s["query"], s["xy"], s["desc"], s["ids"], s["xyz"], s["tags"])
    assert len(want["query"]) == 40
    res, cand = ix.localize(s["K"], s["query"], s["xy"], min_candidates=41)
    assert not rref.gate(40, 41)
    assert (res.success, res.n_candidates, res.n_inliers, res.iters_run) == (False, 40, 0, 0)
    assert np.array_equal(res.R, np.eye(3)) and not res.t.any() and not res.T.any() and not cand["inlier"].any()
    assert cand["query"].tolist() == want["query"].tolist() and cand["row"].tolist() == want["row"].tolist()
    res, cand = ix.localize(s["K"], s["query"], s["xy"], min_candidates=40)
    assert rref.gate(40, 40)
    assert res.success and res.n_candidates == 40 and res.iters_run > 0 and res.n_inliers == cand["inlier"].sum() == 34
    assert not cand["inlier"][:6].any()                                  # the six moved pixels
    assert np.abs(res.R - s["R"]).max() < 1e-3 and np.abs(res.t.ravel() - s["t"]).max() < 1e-2
    M = np.eye(4); M[:3, :3] = res.R; M[:3, 3] = res.t.ravel()
    assert np.abs(res.T @ M - np.eye(4)).max() < 1e-12


def test_localize_is_camera_to_world_on_selects_arrays(api, world):
    s, ix = world, world["ix"]
    sel = ix.select(s["query"], s["xy"])
    same(sel, rref.select_index(s["query"], s["xy"], s["desc"], s["ids"], s["xyz"], s["tags"]))
    R0 = np.eye(3); t0 = np.array([0.1, 0.0, 0.2])
    for over in (dict(), dict(ransac_iterations=30, reproj_error=2.0, confidence=0.9)):
        prm = ix.reloc_params(**over)
        (inl, ok), R, t, iters = api.cameraToWorld(s["K"], sel["xy"], sel["xyz"], R0, t0, prm.ransac_iterations, prm.reproj_error, prm.confidence)
        res, cand = ix.localize(s["K"], s["query"], s["xy"], R0, t0, params=prm)
        assert ok and res.success and res.iters_run == iters and res.n_inliers == len(inl)
        assert res.R.tobytes() == R.tobytes() and res.t.tobytes() == t.tobytes()
        assert np.flatnonzero(cand["inlier"]).tolist() == inl.tolist()
        assert res.T.tobytes() == api.getInverseTransform(R, t).tobytes()


def test_refusals(api, world):
    ARG, STATE = "status %d" % api._lib.SVO_ERR_ARG, "status %d" % api._lib.SVO_ERR_STATE
    s = world
    plain = api.DescriptorIndex(64)
    try:
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.add_points(s["desc"], s["ids"], s["xyz"])              # no points
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.select(s["query"], s["xy"])
        plain.add(s["desc"][:3], s["ids"][:3])
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.enable_points()                                        # not empty
        plain.truncate(0)
        plain.enable_points()
        plain.enable_points()                                            # twice is legal
        bad = s["xyz"][:4].copy(); bad[2, 1] = np.inf
        with pytest.raises(api._lib.SvoError, match=ARG):
            plain.add_points(s["desc"][:4], s["ids"][:4], bad)
        with pytest.raises(api._lib.SvoError, match=ARG):
            plain.add_points(s["desc"][:4], s["ids"][:4], s["xyz"][:4], [0, 1, -1, 2])
        assert plain.size == 0                                           # all or none
        assert plain.add_points(s["desc"][:4], s["ids"][:4], s["xyz"][:4]) == 0 and plain.add(s["desc"][4:6], s["ids"][4:6]) == 4
        got = plain.select(s["query"][:6], s["xy"][:6])                  # the plain rows carry SVO_POINT_NONE
        assert got["query"].tolist() == [0, 1, 2, 3]
        plain.truncate(2)                                                # the points go with their rows ...
        plain.add(s["desc"][2:4], s["ids"][2:4])                         # ... and rows added in their place have none
        assert plain.select(s["query"][:6], s["xy"][:6])["query"].tolist() == [0, 1]
    finally:
        plain.close()
    ix = s["ix"]
    for over in (dict(min_candidates=5), dict(ratio_num=0), dict(ratio_den=0), dict(ratio_num=-7), dict(ratio_den=(1 << 20) + 1),
                 dict(max_dist=-1), dict(max_dist=257), dict(row_lo=3, row_hi=2), dict(row_hi=41)):
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.select(s["query"], s["xy"], **over)
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.localize(s["K"], s["query"], s["xy"], **over)
