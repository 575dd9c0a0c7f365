"""The landmark fusion's numpy reference (tests/fuse_ref.py) against answers known by construction: the gate at, below and one ulp
beyond the radius and on rows without points; the search against a loop over the admissible rows one by one; with everything admitted,
desc_match_ref.match itself; the pairs of a landmark with three rows on each side; the relabel's chain, repeat and from == to; and the
duplicate-landmark scene that is the reason for the feature — no query of the merged map passes the ratio test before the fusion,
every one after it.  No GPU."""
import numpy as np
import pytest

import desc_match_ref as mref
import descriptor_ref as ref
import fuse_cases as fc
import fuse_ref as fr
import reloc_ref as rref


def test_gate_limits_are_inclusive_and_f32():
    c = fc.near_scene(65, 1000)
    s0, d0 = c["src"][0], c["dst"][0]
    planted = list(range(d0, d0 + 4))                 # p + 0.5 on x, one ulp beyond, p - 0.5 on z, p itself
    assert fr.gate(c["xyz"], c["tags"], [s0], planted, 0.5).tolist() == [[True, False, True, True]]
    assert fr.gate(c["xyz"], c["tags"], [s0], planted, 0.0).tolist() == [[False, False, False, True]]
    assert fr.gate(c["xyz"], c["tags"], [s0], planted, 100.0).all()
    assert float(c["xyz"][d0 + 1, 0]) - float(c["xyz"][s0, 0]) == 0.5 + 2.0 ** -23          # exact in f32, above 0.5
    tags = c["tags"].copy()
    tags[s0] = -1
    assert not fr.gate(c["xyz"], tags, [s0], planted, 100.0).any()                          # a source row without a point admits nothing
    tags = c["tags"].copy()
    tags[d0 + 3] = -1
    assert fr.gate(c["xyz"], tags, [s0], planted, 100.0).tolist() == [[True, True, True, False]]


def by_loop(c, radius):
    """rules 1 - 2 row by row on Python integers"""
    (s0, s1), (d0, d1) = c["src"], c["dst"]
    out = []
    for s in range(s0, s1):
        adm = [r for r in range(d0, d1) if c["tags"][s] != -1 and c["tags"][r] != -1 and
               all(abs(np.float32(c["xyz"][r, a]) - np.float32(c["xyz"][s, a])) <= np.float32(radius) for a in range(3))]
        keys = sorted((int(ref.hamming(c["desc"][s:s + 1], c["desc"][r:r + 1])[0, 0]), r) for r in adm)
        best = keys[0] if keys else (mref.NO_DIST, mref.NONE)
        other = [k for k in keys if c["ids"][k[1]] != c["ids"][best[1]]] if keys else []
        second = other[0] if other else (mref.NO_DIST, mref.NONE)
        out.append((best[1], second[1], best[0], second[0], int(c["ids"][best[1]]) if keys else 0, int(c["ids"][second[1]]) if other else 0))
    return out


@pytest.mark.parametrize("n, d", ((63, 7), (65, 9), (20, 300)))
@pytest.mark.parametrize("radius", fc.RADII)
def test_match_near_equals_a_loop_over_the_admissible_rows(n, d, radius):
    c = fc.near_scene(n, d)
    m = fr.match_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], radius)
    got = [(int(r["row"]), int(r["row2"]), int(r["dist"]), int(r["dist2"]), int(r["id"]), int(r["id2"])) for r in m]
    assert got == by_loop(c, radius)


def test_everything_admitted_is_the_plain_search():
    c = fc.near_scene(200, 1000, all_points=True)
    m = fr.match_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], 100.0)
    want = mref.match(c["desc"][c["src"][0]:c["src"][1]], c["desc"], c["ids"], *c["dst"])
    assert m.tobytes() == want.tobytes()
    empty = fr.match_near(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], (5, 5), 100.0)
    assert (empty["row"] == mref.NONE).all() and (empty["dist2"] == mref.NO_DIST).all() and not empty["id"].any()


def test_pairs_of_a_landmark_with_three_rows_on_each_side():
    c = fc.pair_scene()
    out = fr.fuse(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    # one pair per landmark: 40; every second landmark has one id on both sides
    assert (out["n_pairs"], out["n_same"], out["n_fused"], out["n_rows_relabelled"]) == (40, 20, 20, 60)
    assert len(set(c["ids"][out["pair_src"]].tolist())) == 40 and len(set(c["ids"][out["pair_dst"]].tolist())) == 40
    assert np.array_equal(out["ids"][out["pair_src"]], c["ids"][out["pair_dst"]])           # the source landmark has its partner's id
    assert np.array_equal(out["ids"][:120], c["ids"][:120])                                  # the destination keeps its ids
    again = fr.fuse(c["desc"], out["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    assert (again["n_pairs"], again["n_same"], again["n_fused"], again["n_rows_relabelled"]) == (40, 40, 0, 0)
    assert np.array_equal(again["ids"], out["ids"])
    only_src = fr.fuse(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"], relabel_rows=(130, 150))
    assert np.array_equal(only_src["ids"][:130], c["ids"][:130]) and np.array_equal(only_src["ids"][150:], c["ids"][150:])
    assert np.array_equal(only_src["ids"][130:150], out["ids"][130:150])


def test_relabel_is_one_simultaneous_step():
    ids = np.array([1, 2, 3, 1, 2, 3, 4, (1 << 63) + 5], np.uint64)
    new, k = fr.relabel(ids, [1, 2], [2, 3])                                                 # a chain: no row of id 1 becomes 3
    assert new.tolist() == [2, 3, 3, 2, 3, 3, 4, (1 << 63) + 5] and k == 4
    new, k = fr.relabel(ids, [1, 1], [7, 8])                                                 # a repeated `from`: the first wins
    assert new.tolist() == [7, 2, 3, 7, 2, 3, 4, (1 << 63) + 5] and k == 2
    new, k = fr.relabel(ids, [1, 1, 4], [1, 9, 4])                                           # from == to is ignored, as if absent
    assert new.tolist() == [9, 2, 3, 9, 2, 3, 4, (1 << 63) + 5] and k == 2
    new, k = fr.relabel(ids, [(1 << 63) + 5, 3], [0, 1 << 63], rows=(3, 8))                  # a span; ids >= 2^63; 0 is an id like any other
    assert new.tolist() == [1, 2, 3, 1, 2, 1 << 63, 4, 0] and k == 2
    new, k = fr.relabel(ids, [], [])
    assert np.array_equal(new, ids) and k == 0


def test_the_planted_list_entries_are_what_the_docstring_says():
    f, t = fc.relabel_lists(4096)
    u = fc.relabel_index()["universe"]
    assert (f[0], t[0], f[1]) == (u[10], u[11], u[11]) and f[2] == f[3] and t[2] != t[3] and f[4] == t[4] == f[5]
    mask = fc.table_slots(4096) - 1
    import align_ref as aref
    assert len({aref.mix64(int(v)) & mask for v in f[6:9]}) == 1 and len(set(f[6:9].tolist())) == 3
    assert (fc.relabel_index()["ids"] >= np.uint64(1 << 63)).any()


def test_the_gpu_tests_relabel_sequence_changes_rows_at_every_step():
    """tests/test_gpu_fuse.py applies each list to a span and then to the whole index, list after list on one index"""
    ids = fc.relabel_index()["ids"]
    for n in fc.RELABEL_N:
        for rows in ((70_001, 130_003), (0, -1)):
            ids, changed = fr.relabel(ids, *fc.relabel_lists(n), rows)
            assert (changed > 0) == (n > 0), (n, rows)


def test_duplicate_landmarks_fail_the_ratio_test_until_they_are_fused():
    c = fc.duplicate_scene()
    L = fc.DUP_L
    D = ref.hamming(c["base"], c["base"])
    np.fill_diagonal(D, 256)
    assert D.min() >= 64                                                                     # the scene's condition, on its own input
    m = mref.match(c["query"], c["desc"], c["ids"])
    assert (m["dist"] == 16).all() and (m["dist2"] == 16).all() and (m["row"] == np.arange(L)).all() and (m["row2"] == L + np.arange(L)).all()
    before = rref.select_index(c["query"], c["xy"], c["desc"], c["ids"], c["xyz"], c["tags"])
    assert len(before["query"]) == 0                                                         # 16 * 10 < 16 * 7 is false for every query
    out = fr.fuse(c["desc"], c["ids"], c["xyz"], c["tags"], c["src"], c["dst"], c["radius"])
    assert (out["n_pairs"], out["n_same"], out["n_fused"], out["n_rows_relabelled"]) == (L, 0, L, L)
    assert np.array_equal(out["ids"][L:], c["ids"][:L]) and np.array_equal(out["pair_dst"], np.arange(L))
    after = rref.select_index(c["query"], c["xy"], c["desc"], out["ids"], c["xyz"], c["tags"])
    assert np.array_equal(after["query"], np.arange(L)) and np.array_equal(after["row"], np.arange(L))
