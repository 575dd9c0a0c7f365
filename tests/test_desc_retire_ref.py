"""tests/desc_retire_ref.py against a second, deliberately naive O(n^2) statement of the retire rule (include/svo.h, "Index
maintenance") on the generator the GPU tests use, the transform against Python's exact rational arithmetic where one rounding decides,
and the generator against what it claims: ids with 1 .. 9 rows, rows of an id on both sides of a scope edge, SVO_POINT_NONE rows,
tags on both window edges, ids 0 and 2^64 - 1.  No GPU."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import desc_retire_ref as ref

RULES = [dict(), dict(scope=True), dict(tag_window=(2, 5)), dict(tag_window=(5, 2)), dict(drop_ids="some"), dict(latest_per_id=True),
         dict(tag_window=(1, 6), drop_ids="some", latest_per_id=True), dict(tag_window=(-1, 3), latest_per_id=True),
         dict(tag_window=(2, 5), drop_ids="some", latest_per_id=True, scope=True)]


def some_ids(case, seed=3):
    """an id list as a caller writes it: every third id of the index, unsorted, with duplicates and with ids the index lacks"""
    rng = np.random.default_rng(seed)
    u = np.unique(case["ids"])[::3]
    extra = np.array([12345, 2 ** 64 - 2], np.uint64)
    lst = np.concatenate([u, u[:3], extra])
    return lst[rng.permutation(len(lst))]


def rule_args(case, rule):
    r = dict(rule)
    if r.get("drop_ids") == "some":
        r["drop_ids"] = some_ids(case)
    return r


@pytest.mark.parametrize("n", [0, 1, 27, 64, 130])
def test_the_reference_equals_the_naive_statement(n):
    case = ref.index_case(n, seed=n)
    scopes = [(0, -1), (0, 0), (n // 3, n - n // 4), (n, n), (n // 2, n // 2 + 1 if n else 0)]
    for rows, rule in itertools.product(scopes, RULES):
        a = rule_args(case, rule)
        keep, kb = ref.retire(case["ids"], case["tags"], rows, **a)
        keep2, kb2 = ref.naive_retire(case["ids"], case["tags"], rows, **a)
        assert keep.tolist() == keep2.tolist() and kb.tolist() == kb2.tolist(), (n, rows, rule)
        assert kb[0] == 0 and kb[-1] == keep.sum() and ((kb[1:] - kb[:-1]) == keep).all()


def test_every_scope_of_the_27_row_index():
    case = ref.index_case(27, seed=27)
    for lo in range(28):
        for hi in range(lo, 28):
            for rule in (dict(latest_per_id=True), dict(tag_window=(1, 6), latest_per_id=True)):
                a, b = ref.retire(case["ids"], case["tags"], (lo, hi), **rule), ref.naive_retire(case["ids"], case["tags"], (lo, hi), **rule)
                assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


def test_the_generator_hits_what_it_claims():
    for n in (27, 300):
        case = ref.index_case(n, seed=n)
        ids, tags = case["ids"], case["tags"]
        assert (ids == 0).any() and (ids == ref.U64_MAX).any()
        assert (tags == ref.POINT_NONE).any() and (case["xyz"][tags == ref.POINT_NONE] == 0).all()
        lo, hi = n // 3, n - n // 4
        inside = set(ids[lo:hi].tolist())
        assert inside & set(ids[:lo].tolist()) and inside & set(ids[hi:].tolist())       # ids with rows on both sides of both scope edges
        for w_lo, w_hi in ((2, 5), (1, 6)):                                               # tags on the edges and just outside them
            assert all((tags == t).any() for t in (w_lo - 1, w_lo, w_hi, w_hi + 1))
    assert ref.run_lengths(ref.index_case(300, seed=300)["ids"]) == list(range(1, 10))
    assert ref.run_lengths(ref.index_case(300, points=False, spread=False)["ids"]) == list(range(1, 10))
    plain = ref.index_case(64, points=False)
    assert (plain["tags"] >= 0).all()


def test_latest_keeps_the_last_row_of_each_id_among_the_survivors():
    ids = np.array([7, 7, 8, 7, 8, 9, 7], np.uint64)
    tags = np.array([0, 1, 1, 2, 2, 3, 4], np.int32)
    keep, kb = ref.retire(ids, tags, latest_per_id=True)
    assert keep.tolist() == [False, False, False, False, True, True, True] and kb.tolist() == [0, 0, 0, 0, 0, 1, 2, 3]
    # the scope ends before the last 7: inside it row 3 is the latest 7, and the 7 behind the scope stays
    keep, _ = ref.retire(ids, tags, rows=(0, 5), latest_per_id=True)
    assert keep.tolist() == [False, False, False, True, True, True, True]
    # the tag rule first: the latest is decided among its survivors
    keep, _ = ref.retire(ids, tags, tag_window=(0, 1), latest_per_id=True)
    assert keep.tolist() == [False, True, True, False, False, False, False]


def exact(T, p, c):
    """coordinate c of the rule's result with each operation rounded to f64 by exact rational arithmetic, then to f32"""
    def rnd(q):
        return Fraction(float(q))                                     # float(Fraction) rounds to nearest even, as IEEE does
    v = rnd(Fraction(float(T[4 * c])) * Fraction(float(p[0])))
    for k in (1, 2):
        v = rnd(v + rnd(Fraction(float(T[4 * c + k])) * Fraction(float(p[k]))))
    v = rnd(v + Fraction(float(T[4 * c + 3])))
    return np.float32(float(v))


def test_the_transform_rounds_every_operation_on_its_own():
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-50, 50, (40, 3)).astype(np.float32)
    tags = np.arange(40, dtype=np.int32) % 5
    tags[::7] = ref.POINT_NONE
    T = np.eye(4)
    T[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0] * 1.0000001
    T[:3, 3] = [0.1, -3.3, 1e-3]
    after, moved, skipped = ref.transform(xyz, tags, T, rows=(3, 37), tag_window=(1, 3))
    sel = (np.arange(40) >= 3) & (np.arange(40) < 37) & (tags >= 1) & (tags <= 3)
    assert moved == sel.sum() and skipped == 0
    assert after[~sel].tobytes() == xyz[~sel].tobytes()
    for r in np.flatnonzero(sel):
        assert [exact(T.reshape(16), xyz[r], c) for c in range(3)] == after[r].tolist()
    # overflow: the row stays and is counted
    big = np.eye(4); big[0, 0] = 1e38
    after, moved, skipped = ref.transform(xyz, tags, big)
    over = (tags != ref.POINT_NONE) & (np.abs(xyz[:, 0].astype(np.float64) * 1e38) > np.finfo(np.float32).max)
    assert skipped == over.sum() > 0 and moved == (tags != ref.POINT_NONE).sum() - skipped
    assert after[over].tobytes() == xyz[over].tobytes() and np.isfinite(after).all()
