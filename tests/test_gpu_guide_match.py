"""The guided search on a real GPU (include/svo.h, "Guided search": svo_desc_index_project, svo_desc_index_match_guided) against
tests/guide_ref.py on the host's copies of the same arrays — every field of every result row, every bit of every projection.

The inputs are tests/guide_cases.py's planned case: an index of 2304 rows and 4096 queries with, each on its own query and rows, a
query that admits nothing, a query admissible only in the last row of a chunk and the first of the next (at 64 and at 1024), a whole
wave that admits nothing in thirty chunks, a wave in which exactly one lane admits a row, a best admissible row whose nearest
inadmissible neighbour has the same id, a second found only in another chunk, and the clause rows of rules 1 and 2.  The reference
search over the 4096 x 2304 case runs once (about two seconds of numpy); every test slices it.  Sizes 1, 63, 64, 65, 1025 and 4096
are prefixes of the list, each at chunk_rows 64, 1024 and 4096 (one chunk); 4097 queries are refused.  Then: a row sub-range,
project on the whole index, on a sub-range that starts inside a block and under both clause priors, the gate's clauses at radius
12, 0 and 0.25, shuffled queries and the sort switched off, radius 3e38 against the unguided search, the kernel time, the refusals."""
import numpy as np
import pytest

import guide_cases as cases
import guide_ref as gref
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu


def fill(ix, c, keep=None):
    """the rows of a case into an index with points, run by run: add_points where the rows have a point, plain add where not"""
    rows = np.arange(len(c["desc"])) if keep is None else np.flatnonzero(keep)
    has = c["tags"][rows] >= 0
    cut = np.flatnonzero(np.diff(has.astype(np.int8))) + 1
    for seg in np.split(rows, cut):
        if c["tags"][seg[0]] < 0:
            ix.add(c["desc"][seg], c["ids"][seg])
        else:
            ix.add_points(c["desc"][seg], c["ids"][seg], c["xyz"][seg], c["tags"][seg])


@pytest.fixture(scope="module")
def big(api):
    c = cases.planned_case()
    ix = api.DescriptorIndex(cases.N_ROWS + 8, points=True)
    fill(ix, c)
    assert ix.size == cases.N_ROWS
    c["uv"] = gref.project(c["K"], c["R"], c["t"], c["xyz"], c["tags"])
    c["rows"] = gref.match(c["query"], c["xy"], c["desc"], c["ids"], c["uv"], c["radius"])
    c["ix"] = ix
    c["guide"] = (c["K"], c["R"], c["t"], c["radius"])
    yield c
    ix.close()


def test_the_case_is_what_it_plans(big):
    rows, uv = big["rows"], big["uv"]
    adm = gref.admissible(uv, big["xy"][:192], big["radius"])
    assert rows["row"][0] == -1 and not adm[0].any()                                   # A
    assert np.flatnonzero(adm[1]).tolist() == [63, 64, 1023, 1024] and rows["row"][1] == 1024 and rows["row2"][1] in (63, 64, 1023)   # B
    assert (adm[64:128].sum(1) == 1).all() and (adm[64:128].argmax(1) >= 30 * 64).all() and not adm[64:128, :30 * 64].any()           # C
    assert np.flatnonzero(adm[128:192].any(1)).tolist() == [2] and np.flatnonzero(adm[130]).tolist() == [700]                         # D
    assert np.flatnonzero(adm[2]).tolist() == [200] and rows["row"][2] == 200 and rows["row2"][2] == -1 and rows["dist"][2] == 20      # E
    assert big["ids"][201] == big["ids"][200] and bin(int.from_bytes(bytes(big["desc"][201] ^ big["query"][2]), "little")).count("1") == 2
    assert rows["row"][3] == 10 and rows["row2"][3] == 2203 and 10 // 64 != 2203 // 64 and 10 // 1024 != 2203 // 1024               # F
    assert 3000 < (rows["row"] >= 0).sum() < 4000 and 3000 < (rows["row2"] >= 0).sum()
    assert (~np.isfinite(uv).all(1)).sum() > 40                                        # rows without a point, and the clause rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4096])
def test_match_guided_equals_the_reference_at_every_size_and_chunk(big, n):
    ix = big["ix"]
    try:
        for chunk in (64, 1024, 4096):
            ix.chunk_rows = chunk
            got = ix.match_guided(*big["guide"], big["query"][:n], big["xy"][:n])
            assert got.tobytes() == big["rows"][:n].tobytes(), chunk
    finally:
        ix.chunk_rows = 0


def test_4097_queries_are_refused(api, big):
    with pytest.raises(api._lib.SvoError, match="status %d" % api._lib.SVO_ERR_ARG):
        big["ix"].match_guided(*big["guide"], np.zeros((4097, 32), np.uint8), np.zeros((4097, 2), np.float32))
    with pytest.raises(api._lib.SvoError, match="status %d" % api._lib.SVO_ERR_ARG):
        big["ix"].select_guided(*big["guide"], np.zeros((4097, 32), np.uint8), np.zeros((4097, 2), np.float32))


def test_a_row_sub_range(big):
    which = np.arange(0, 700)
    for lo, hi, chunk in ((100, 2100, 64), (65, 1023, 1024), (700, 701, 0), (500, 500, 0)):
        want = gref.match(big["query"][which], big["xy"][which], big["desc"], big["ids"], big["uv"], big["radius"], lo, hi)
        big["ix"].chunk_rows = chunk
        try:
            got = big["ix"].match_guided(*big["guide"], big["query"][which], big["xy"][which], lo, hi)
        finally:
            big["ix"].chunk_rows = 0
        assert got.tobytes() == want.tobytes(), (lo, hi)
    assert (want["row"] == -1).all() and (want["dist"] == 257).all()                   # the empty range


def test_project_equals_the_reference(big):
    ix = big["ix"]
    assert ix.project(big["K"], big["R"], big["t"]).tobytes() == big["uv"].tobytes()
    assert ix.project(big["K"], big["R"], big["t"], 259, 2001).tobytes() == big["uv"][259:2001].tobytes()   # starts and ends inside a block
    assert ix.project(big["K"], big["R"], big["t"], 7, 7).shape == (0, 2)
    rng = np.random.default_rng(8)
    R, t = np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(size=3) * 3           # a pose that puts rows behind the camera too
    want = gref.project(big["K"], R, t, big["xyz"], big["tags"])
    assert 200 < np.isfinite(want).all(1).sum() < 2200
    assert ix.project(big["K"], R, t).tobytes() == want.tobytes()
    lo = cases.N_ROWS - 8                                                              # the clause rows under both clause priors
    for (K, R, t), vis in zip(cases.CLAUSE_GUIDES, cases.CLAUSE_VISIBLE):
        got = ix.project(K, R, t, lo, cases.N_ROWS)
        assert got.tobytes() == gref.project(K, R, t, big["xyz"][lo:], big["tags"][lo:]).tobytes()
        assert np.isfinite(got).all(1).tolist() == vis


def test_the_gates_clauses(big):
    lo = cases.N_ROWS - 8                                                              # row lo is the plain clause row: (445, 180) here
    assert big["uv"][lo].tolist() == [445.0, 180.0]
    rng = np.random.default_rng(9)
    for radius in (12.0, 0.0, 0.25):
        xy, plan = cases.clause_pixels(445, 180, radius)
        query = rng.integers(0, 256, (len(xy), 32), dtype=np.uint8)
        want = gref.match(query, xy, big["desc"], big["ids"], big["uv"], radius, lo, cases.N_ROWS)
        got = big["ix"].match_guided(big["K"], big["R"], big["t"], radius, query, xy, lo, cases.N_ROWS)
        assert got.tobytes() == want.tobytes(), radius
        assert ((want["row"] == lo) | (want["row2"] == lo)).tolist() == plan.tolist(), radius


def test_results_do_not_depend_on_the_query_order(big):
    ix = big["ix"]
    perm = np.random.default_rng(10).permutation(cases.N_QUERIES)
    got = ix.match_guided(*big["guide"], big["query"][perm], big["xy"][perm])
    assert got.tobytes() == big["rows"][perm].tobytes()
    ix.set_guided_sort(False)
    try:
        for chunk in (64, 0):
            ix.chunk_rows = chunk
            assert ix.match_guided(*big["guide"], big["query"], big["xy"]).tobytes() == big["rows"].tobytes()
            assert ix.match_guided(*big["guide"], big["query"][perm][:1000], big["xy"][perm][:1000]).tobytes() == big["rows"][perm][:1000].tobytes()
    finally:
        ix.set_guided_sort(True); ix.chunk_rows = 0


def test_radius_3e38_is_the_unguided_search(api, big):
    keep = np.isfinite(big["uv"]).all(1)                                               # every row kept has a point in front of the camera
    assert 2100 < keep.sum() < cases.N_ROWS
    ix = api.DescriptorIndex(int(keep.sum()), points=True)
    try:
        fill(ix, big, keep)
        q, xy = big["query"][:1025], big["xy"][:1025]
        plain = ix.match(q)
        for chunk in (64, 0):
            ix.chunk_rows = chunk
            assert ix.match_guided(big["K"], big["R"], big["t"], 3e38, q, xy).tobytes() == plain.tobytes()
        assert ix.match_guided(big["K"], big["R"], big["t"], 3e38, q, xy, 70, 1500).tobytes() == ix.match(q, 70, 1500).tobytes()
    finally:
        ix.close()


def test_kernel_time_of_a_guided_call(big):
    ix = big["ix"]
    ix.set_timing(True)
    try:
        ix.match_guided(*big["guide"], big["query"], big["xy"])
        assert 0 < ix.stats()["last_kernels_ms"] < 1000
        ix.select_guided(*big["guide"], big["query"], big["xy"])
        assert 0 < ix.stats()["last_kernels_ms"] < 1000
    finally:
        ix.set_timing(False)


def test_refusals(api, big):
    ARG, STATE = "status %d" % api._lib.SVO_ERR_ARG, "status %d" % api._lib.SVO_ERR_STATE
    ix, K, R, t = big["ix"], big["K"], big["R"], big["t"]
    q, xy = big["query"][:8], big["xy"][:8]
    bad_R = R.copy(); bad_R[1, 2] = np.nan
    bad_t = t.copy(); bad_t[0] = np.inf
    bad_K = K.copy(); bad_K[2, 2] = np.nan                                             # an entry the projection does not even use
    for args in ((K, R, t, -1.0), (K, R, t, np.nan), (K, R, t, np.inf), (K, bad_R, t, 5.0), (K, R, bad_t, 5.0), (bad_K, R, t, 5.0)):
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.match_guided(*args, q, xy)
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.select_guided(*args, q, xy)
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.localize_guided(*args, q, xy)
    for args in ((K, bad_R, t), (K, R, bad_t), (bad_K, R, t)):
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.project(*args)
    for lo, hi in ((-1, 5), (5, 4), (0, cases.N_ROWS + 1)):
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.match_guided(K, R, t, 5.0, q, xy, lo, hi)
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.project(K, R, t, lo, hi)
    for over in (dict(min_candidates=5), dict(ratio_num=0), dict(max_dist=257), dict(row_lo=3, row_hi=2)):
        with pytest.raises(api._lib.SvoError, match=ARG):
            ix.select_guided(K, R, t, 5.0, q, xy, **over)
    plain = api.DescriptorIndex(16)
    try:
        plain.add(big["desc"][:4], big["ids"][:4])
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.project(K, R, t)
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.match_guided(K, R, t, 5.0, q, xy)
        with pytest.raises(api._lib.SvoError, match=STATE):
            plain.select_guided(K, R, t, 5.0, q, xy)
    finally:
        plain.close()
    assert ix.match_guided(K, R, t, 0.0, q, xy).tobytes() == gref.match(q, xy, big["desc"], big["ids"], big["uv"], 0.0).tobytes()   # radius 0 is legal
