"""tests/reloc_ref.py on hand-made cases, one per clause of the selection rules of include/svo.h ("Relocalisation"), and the
transform of svo_desc_index_add_frame_points against exact rational arithmetic."""
from fractions import Fraction

import numpy as np

import desc_match_ref as mref
import reloc_ref as rref


def rows(spec):
    """[(id, row, dist, dist2), ...] -> result rows; row = -1 gives the empty row"""
    m = np.zeros(len(spec), mref.DTYPE)
    for j, (i, row, dist, dist2) in enumerate(spec):
        m[j] = (i, 0, row, -1 if dist2 == mref.NO_DIST else 0, dist, dist2, 0)
    return m


TAGS = np.array([0, 3, rref.POINT_NONE, 7, 0, 0, 0, 0])        # row 2 has no point
RULE = dict(max_dist=40, ratio_num=7, ratio_den=10)


def sel(spec, **over):
    q, r = rref.select(rows(spec), TAGS, **dict(RULE, **over))
    return q.tolist(), r.tolist()


def test_rule_1_every_clause():
    assert sel([(5, 0, 10, 20)]) == ([0], [0])
    assert sel([(5, -1, 257, 257)]) == ([], [])                 # no best row
    assert sel([(5, 2, 10, 20)]) == ([], [])                    # the best row has no point
    assert sel([(5, 1, 40, 200)]) == ([0], [1])                 # dist == max_dist
    assert sel([(5, 1, 41, 200)]) == ([], [])                   # max_dist + 1
    assert sel([(5, 1, 7, 10)]) == ([], [])                     # 7 * 10 == 10 * 7: strict, rejected
    assert sel([(5, 1, 7, 11)]) == ([0], [1])
    assert sel([(5, 1, 40, mref.NO_DIST)]) == ([0], [1])        # a lone candidate: 257 passes
    assert sel([(5, 1, 0, 0)]) == ([], [])                      # 0 < 0 is false
    assert sel([(5, 1, 0, 1)]) == ([0], [1])
    assert sel([(5, 3, 256, 257)], max_dist=256, ratio_num=1 << 20, ratio_den=1 << 20) == ([0], [3])   # the largest terms stay exact


def test_rule_2_one_pixel_per_landmark():
    assert sel([(5, 0, 10, 30), (5, 1, 9, 30)]) == ([1], [1])                       # the smaller distance
    assert sel([(5, 0, 9, 30), (5, 1, 9, 30)]) == ([0], [0])                        # equal distances: the smaller j
    assert sel([(5, 0, 12, 30), (5, 1, 9, 30), (5, 3, 11, 30)]) == ([1], [1])       # three of one id
    assert sel([(5, 0, 9, 30), (6, 1, 12, 30), (5, 3, 8, 30)]) == ([1, 2], [1, 3])
    # a rejected query does not compete: the loser of rule 1 cannot beat an accepted one of its id
    assert sel([(5, 2, 1, 30), (5, 1, 9, 30)]) == ([1], [1])
    assert sel([(5, 0, 41, 200), (5, 1, 30, 200)]) == ([1], [1])
    # ids are 64 bits wide: both halves tell landmarks apart
    assert sel([(1 << 32, 0, 9, 30), (1, 1, 9, 30), ((1 << 32) + 1, 3, 9, 30)]) == ([0, 1, 2], [0, 1, 3])


def test_rule_3_order_is_increasing_query():
    # the loser (j = 1) was the only thing between two survivors; its winner comes last
    assert sel([(1, 0, 9, 30), (2, 1, 9, 30), (3, 3, 9, 30), (2, 4, 8, 30)]) == ([0, 2, 3], [0, 3, 4])
    assert sel([]) == ([], [])


def test_rule_4_gate():
    assert not rref.gate(5, 6) and rref.gate(6, 6) and rref.gate(7, 6)


def test_select_index_runs_the_search_first():
    rng = np.random.default_rng(1)
    desc = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    ids = np.array([1, 2, 3, 4, 1, 2, 3, 4], np.uint64)
    xyz = rng.normal(size=(8, 3)).astype(np.float32)
    query = desc[[4, 2, 0, 7]].copy()
    query[2, 0] ^= 1                                            # row 0 at distance 1; row 4 (id 1 too) is query 0's, at distance 0
    xy = np.arange(8, dtype=np.float32).reshape(4, 2)
    got = rref.select_index(query, xy, desc, ids, xyz, TAGS)
    # query 0 -> row 4 (id 1, dist 0), query 1 -> row 2 (no point), query 2 -> row 0 (id 1, dist 1: loses), query 3 -> row 7
    assert got["query"].tolist() == [0, 3] and got["row"].tolist() == [4, 7]
    assert np.array_equal(got["xy"], xy[[0, 3]]) and np.array_equal(got["xyz"], xyz[[4, 7]])
    # rows 0 .. 3 only: random rows are ~128 bits from queries 0 and 3 (beyond max_dist), query 2 alone keeps a match
    old = rref.select_index(query, xy, desc, ids, xyz, TAGS, 0, 4)
    assert old["query"].tolist() == [2] and old["row"].tolist() == [0]


def test_map_points_is_the_rounded_chain():
    rng = np.random.default_rng(2)
    T = np.eye(4)
    T[:3, :] = rng.normal(size=(3, 4)) * [1, 1, 1, 50]
    p = (rng.normal(size=(40, 3)) * 30).astype(np.float32)
    got = rref.map_points(T, p)
    assert got.dtype == np.float32 and np.array_equal(rref.map_points(np.eye(4), p), p)
    for i in range(len(p)):
        for r in range(3):
            # each step rounded to f64 (float(Fraction) rounds to nearest even, as the hardware does), left to right
            v = float(Fraction(T[r, 0]) * Fraction(float(p[i, 0])))
            v = float(Fraction(v) + Fraction(float(Fraction(T[r, 1]) * Fraction(float(p[i, 1])))))
            v = float(Fraction(v) + Fraction(float(Fraction(T[r, 2]) * Fraction(float(p[i, 2])))))
            v = float(Fraction(v) + Fraction(T[r, 3]))
            assert np.float32(v) == got[i, r], (i, r)
