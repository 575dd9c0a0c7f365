"""tests/desc_match_ref.py, the definitional reference of the descriptor index's search (include/svo.h, "Descriptor index"), on hand
cases with written-out answers; and the input generators tests/test_gpu_desc_match.py uses, checked here, on the reference, for not
being vacuous: enough queries whose best distance is shared by several rows (the tie rule decides), and enough whose plain
second-nearest row carries the best row's id (the id rule decides).  No GPU."""
import numpy as np

import desc_match_ref as mref

SEED = 2369                                           # the generators' seed: tie_set(SEED, 130, 27) meets both conditions on every slice below


def bits(*positions):
    """a 32-byte descriptor with exactly these bits set (bit i is bit i % 8 of byte i // 8)"""
    d = np.zeros(32, np.uint8)
    for p in positions:
        d[p // 8] |= 1 << (p % 8)
    return d


def tie_set(seed, n, m, n_bases=5, max_flips=2, flip_bits=6):
    """n queries and m index rows drawn as 0 .. max_flips bit flips, among the first flip_bits bits, off a pool of n_bases random
    bases: rows off one base lie 0 .. 2 max_flips apart, with many equal distances.  ids are shared by runs of 1 .. 4 consecutive
    rows, all rows of a run off one base, as a landmark seen in several frames is -> (query (n, 32), desc (m, 32), ids (m,) uint64)"""
    rng = np.random.default_rng(seed)
    bases = rng.integers(0, 256, (n_bases, 32), dtype=np.uint8)

    def flipped(b):
        d = bases[b].copy()
        for p in rng.choice(flip_bits, rng.integers(0, max_flips + 1), replace=False):
            d[p // 8] ^= 1 << (p % 8)
        return d

    desc, ids = [], []
    next_id = 1000
    while len(desc) < m:
        b = rng.integers(n_bases)
        for _ in range(min(rng.integers(1, 5), m - len(desc))):
            desc.append(flipped(b)); ids.append(next_id)
        next_id += rng.integers(1, 4)                 # ids increase, not densely
    query = [flipped(rng.integers(n_bases)) for _ in range(n)]
    return (np.array(query, np.uint8).reshape(n, 32), np.array(desc, np.uint8).reshape(m, 32), np.array(ids, np.uint64))


def random_set(seed, n, m, run=4):
    """uniformly random descriptors, ids in runs of `run` rows"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (m, 32), dtype=np.uint8),
            (7 + np.arange(m) // run).astype(np.uint64))


def tie_fraction(query, desc, lo=0, hi=-1):
    """the fraction of queries with two or more rows at the best distance"""
    hi = len(desc) if hi == -1 else hi
    D = mref.ref.hamming(query, desc[lo:hi])
    return float(((D == D.min(1, keepdims=True)).sum(1) >= 2).mean())


def same_id_second_fraction(query, desc, ids, lo=0, hi=-1):
    """the fraction of queries whose plain second-nearest row carries the best row's id"""
    best = mref.match(query, desc, ids, lo, hi)
    second = mref.plain_second(query, desc, lo, hi)
    ok = second >= 0
    return float((ids[second[ok]] == best["id"][ok]).sum() / max(len(query), 1))


def row(m):
    return tuple(int(m[f]) for f in ("row", "dist", "id", "row2", "dist2", "id2"))


# ------------------------------------------------------------------------------------------------ hand cases
def test_a_tie_for_best_goes_to_the_lower_row():
    desc = np.stack([bits(0, 1, 2), bits(5), bits(9), bits(0, 1)])       # distances to the zero query: 3 1 1 2
    m = mref.match(np.zeros((1, 32), np.uint8), desc, [10, 11, 12, 13])
    assert row(m[0]) == (1, 1, 11, 2, 1, 12)
    m = mref.match(np.zeros((1, 32), np.uint8), desc, [10, 11, 12, 13], 2, 4)   # without row 1 the other tied row is the best
    assert row(m[0]) == (2, 1, 12, 3, 2, 13)


def test_the_second_skips_rows_of_the_best_id():
    desc = np.stack([bits(0), bits(0, 1), bits(0, 1, 2), bits(0, 1, 2, 3)])   # distances 1 2 3 4
    m = mref.match(np.zeros((1, 32), np.uint8), desc, [5, 5, 9, 5])      # best and the plain runner-up share id 5: row2 is the third-nearest
    assert row(m[0]) == (0, 1, 5, 2, 3, 9)
    assert mref.plain_second(np.zeros((1, 32), np.uint8), desc)[0] == 1


def test_one_id_everywhere_leaves_no_second():
    desc = np.stack([bits(0, 1), bits(0), bits(3, 4, 5)])
    m = mref.match(np.zeros((1, 32), np.uint8), desc, [4, 4, 4])
    assert row(m[0]) == (1, 1, 4, mref.NONE, mref.NO_DIST, 0)
    assert int(m["dist"][0]) * 10 < int(m["dist2"][0]) * 7             # a lone candidate passes the ratio test


def test_an_empty_range():
    desc = np.stack([bits(0), bits(1)])
    for lo, hi in ((0, 0), (1, 1), (2, 2)):
        m = mref.match(np.zeros((3, 32), np.uint8), desc, [1, 2], lo, hi)
        assert all(row(r) == (mref.NONE, mref.NO_DIST, 0, mref.NONE, mref.NO_DIST, 0) for r in m)
    assert len(mref.match(np.zeros((0, 32), np.uint8), desc, [1, 2])) == 0
    assert m.dtype.itemsize == 32 and (m["reserved"] == 0).all()


def test_a_row_itself_and_its_complement():
    rng = np.random.default_rng(1)
    desc = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    q = np.stack([desc[1], ~desc[1]])
    m = mref.match(q, desc, [1, 2, 3])
    assert (int(m["row"][0]), int(m["dist"][0])) == (1, 0)
    assert int(m["row"][1]) != 1 and int(m["row2"][1]) != 1            # the complement is the farthest row of all
    m = mref.match(q, desc, [1, 2, 3], 1, 2)
    assert row(m[0]) == (1, 0, 2, mref.NONE, mref.NO_DIST, 0) and row(m[1]) == (1, 256, 2, mref.NONE, mref.NO_DIST, 0)


# ------------------------------------------------------------------------------------------------ the generators are not vacuous
def shared_case():
    """the one tie set the GPU tests slice: 130 queries, 27 rows"""
    return tie_set(SEED, 130, 27)


def test_the_tie_set_has_ties_and_same_id_runner_ups():
    Q, D, I = shared_case()
    assert Q.shape == (130, 32) and D.shape == (27, 32) and I.shape == (27,)
    runs = np.diff(np.flatnonzero(np.r_[True, I[1:] != I[:-1], True]))
    assert runs.min() >= 1 and runs.max() <= 4 and len(runs) >= 8
    for n, m in ((65, 27), (130, 27), (64, 9), (63, 16), (65, 8)):     # the slices the GPU tests take
        q, d, ids = Q[:n], D[:m], I[:m]
        t, s = tie_fraction(q, d), same_id_second_fraction(q, d, ids)
        print("tie_set n = %d m = %d: %.2f of the queries tie for best, %.2f have a runner-up with the best's id" % (n, m, t, s))
        assert t >= 0.1 and s >= 0.1, (n, m, t, s)


def test_the_id_rule_changes_answers_on_the_tie_set():
    q, d, ids = shared_case()
    m = mref.match(q, d, ids)
    assert (m["row2"] != mref.plain_second(q, d)).mean() >= 0.1
    assert (m["id2"][m["row2"] >= 0] != m["id"][m["row2"] >= 0]).all()


def test_the_random_set_has_runs_of_four():
    q, d, ids = random_set(3, 5, 10)
    assert ids.tolist() == [7, 7, 7, 7, 8, 8, 8, 8, 9, 9] and len(np.unique(d, axis=0)) == 10
