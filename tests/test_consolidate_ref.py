"""tests/consolidate_ref.py, the numpy statement of the five rules of "Landmark consolidation" (include/svo.h), against the
properties the rules promise: a group of one row is unchanged in every bit, a second call changes nothing, a tie of the sums goes to
the later row, a group of more than 64 keeps its last 64 views, radius 0 admits only points equal to the medoid's, non-members are
carried, kept_before is retire's — and a constructed case in which the order of the float64 sum changes the float32 result, so the
order rule is shown to bind."""
import numpy as np

import consolidate_ref as cr
import desc_retire_ref as rr


def one_group(desc, xyz, radius, ids=None, tags=None):
    n = len(desc)
    return cr.consolidate(desc, np.full(n, 7, np.uint64) if ids is None else ids, xyz, np.zeros(n, np.int32) if tags is None else tags, radius)


def test_a_group_of_one_row_is_unchanged_in_every_bit():
    c = cr.index_case(200, views=1, seed=1)
    c["ids"] = np.arange(200, dtype=np.uint64) * np.uint64(3)
    c["xyz"][3] = (-0.0, 0.0, -0.0)                   # 0.0 + -0.0 would lose the sign: a group of one is not summed
    out = cr.consolidate(c["desc"], c["ids"], c["xyz"], c["tags"], 0.5)
    assert not cr.same_rows(cr.as_read(out), cr.as_read(c))
    assert out["result"].n_dropped == 0 and out["result"].n_groups == out["result"].n_members == int((c["tags"] != -1).sum())
    assert out["kept_before"].tolist() == list(range(201))


def test_a_second_call_changes_nothing():
    c = cr.index_case(600, views=5, seed=2)
    a = cr.consolidate(c["desc"], c["ids"], c["xyz"], c["tags"], 0.2)
    assert a["result"].n_dropped > 300 and a["result"].n_far_views > 0
    b = cr.consolidate(a["desc"], a["ids"], a["xyz"], a["tags"], 0.2)
    assert not cr.same_rows(cr.as_read(b), cr.as_read(a)) and b["result"].n_dropped == 0
    assert b["result"].n_groups == a["result"].n_groups == b["result"].n_members


def test_the_tie_goes_to_the_later_row():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 256, (2, 32), dtype=np.uint8)             # two views: both sums are d(0, 1)
    xyz = np.array([[0, 0, 0], [5, 5, 5]], np.float32)
    out = one_group(d, xyz, 0.1)
    assert np.array_equal(out["desc"][0], d[1]) and out["xyz"][0].tolist() == [5, 5, 5] and out["result"].n_far_views == 1
    same = np.repeat(d[:1], 5, 0)                                  # identical descriptors: every sum is 0, the latest view wins
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    assert one_group(same, pts, 0.0)["xyz"][0].tolist() == pts[4].tolist()
    three = np.zeros((3, 32), np.uint8)                            # views 0 and 1 are equal, view 2 differs in one bit: sums 1, 1, 2
    three[2, 0] = 1
    assert one_group(three, np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32), 0.0)["xyz"][0].tolist() == [2, 0, 0]


def test_the_cap_keeps_the_last_64_views():
    rng = np.random.default_rng(4)
    k = 80
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d = np.repeat(base[None], k, 0)
    d[16:] ^= rng.integers(0, 256, 32, dtype=np.uint8)             # the first 16 views are one descriptor, the last 64 another
    d[40, 0] ^= 1                                                  # and one of those is off by a bit: never the medoid
    xyz = np.zeros((k, 3), np.float32)
    xyz[:16] = 100.0                                               # would pull the mean if they contributed
    xyz[16:, 0] = np.arange(64)
    out = one_group(d, xyz, 1000.0)
    assert len(out["ids"]) == 1 and out["result"] == cr.Result(80, 1, 79, 0, 1, 1)
    assert np.array_equal(out["desc"][0], d[79]) and out["xyz"][0].tolist() == [31.5, 0, 0]
    sixty_four = one_group(d[16:], xyz[16:], 1000.0)
    assert sixty_four["result"].n_capped_groups == 0 and sixty_four["xyz"][0].tolist() == [31.5, 0, 0]


def test_radius_zero_admits_only_the_medoids_own_point():
    d = np.zeros((4, 32), np.uint8)
    d[0, 0] = 0xFF                                                 # views 1 .. 3 agree: the medoid is view 3
    xyz = np.array([[1, 1, 1], [2, 2, 2], [1, 1, 1], [2, 2, 2]], np.float32)
    out = one_group(d, xyz, 0.0)
    assert out["xyz"][0].tolist() == [2, 2, 2] and out["result"].n_far_views == 2
    assert one_group(d, xyz, 1.0)["xyz"][0].tolist() == [1.5, 1.5, 1.5]
    cut = xyz.copy(); cut[0] = (2, 2, 3.5)                         # a radius that cuts one view off, on one axis
    out = one_group(d, cut, 1.0)
    assert out["result"].n_far_views == 1 and out["xyz"][0].tolist() == [np.float32(5 / 3)] * 3


def test_non_members_are_carried_and_kept_before_is_retires():
    c = cr.index_case(500, views=6, seed=5)
    rows, window = (37, 451), (2, 5)
    out = cr.consolidate(c["desc"], c["ids"], c["xyz"], c["tags"], 0.3, rows=rows, tag_window=window)
    member = np.zeros(500, bool)
    member[rows[0]:rows[1]] = True
    member &= (c["tags"] >= window[0]) & (c["tags"] <= window[1])
    assert (~member).sum() > 100 and (c["tags"][rows[0]:rows[1]] == -1).any()
    keep, kept_before = rr.retire(c["ids"], np.where(member, 0, -1), rows=(0, -1), tag_window=(0, 0), latest_per_id=True)
    keep |= ~member                                                # retire drops the non-members of its window; consolidation keeps them
    kb = np.zeros(501, np.int32); kb[1:] = np.cumsum(keep)
    assert np.array_equal(out["kept_before"], kb) and out["result"].n_kept == kb[-1] == len(out["ids"])
    stay = np.flatnonzero(~member)
    for name in ("desc", "ids", "xyz", "tags"):
        assert np.array_equal(out[name][kb[stay]], c[name][stay]), name
    assert np.array_equal(out["ids"], c["ids"][keep]) and np.array_equal(out["tags"], c["tags"][keep])


def test_the_order_of_the_sum_binds():
    """One group of four views with x = 4, 2^-22, 2^-51, 2^-51 in ascending rows, all near.  Ascending: 0 + 4 and + 2^-22 are exact;
    2^-51 is half an ulp of a float64 in [4, 8) (ulp 2^-50), a tie that rounds to the even neighbour, which is the sum as it stood:
    both small views are lost, the sum is 4 + 2^-22, the quotient by 4 is 1 + 2^-24 exactly, a float32 tie between 1 and 1 + 2^-23
    that rounds to even: 1.0.  Descending: 2^-51 + 2^-51 = 2^-50, + 2^-22, + 4 are all exact (53 bits); the quotient is
    1 + 2^-24 + 2^-52, above the tie: 1 + 2^-23.  The two orders give different float32 results, so the rule's order binds."""
    xyz = np.zeros((4, 3), np.float32)
    xyz[:, 0] = [4.0, 2.0 ** -22, 2.0 ** -51, 2.0 ** -51]
    assert xyz[:, 0].astype(np.float64).tolist() == [4.0, 2.0 ** -22, 2.0 ** -51, 2.0 ** -51]     # each is a float32
    d, ids, tags = np.zeros((4, 32), np.uint8), np.full(4, 7, np.uint64), np.zeros(4, np.int32)
    a = cr.consolidate(d, ids, xyz, tags, 8.0)
    b = cr.consolidate(d, ids, xyz, tags, 8.0, order="descending")
    assert a["result"].n_far_views == b["result"].n_far_views == 0
    assert a["xyz"][0, 0] == np.float32(1.0) and b["xyz"][0, 0] == np.float32(1.0 + 2.0 ** -23)
    assert a["xyz"][0, 0] != b["xyz"][0, 0]
