"""The place candidates' numpy reference (tests/place_ref.py) against answers known by construction: rule 2 against a loop over the
rows one by one on tiny inputs; the planted scene of 12 keyframes whose landmarks are each seen from three — the queried group's
votes fall whole on the three keyframes that saw it, which the per-best-row vote does not give; and rule 3 on hand-made histograms
against the tags written next to them and against a brute-force loop.  No GPU."""
import numpy as np
import pytest

import place_cases as pc
import place_ref as pr


def votes_by_loop(ids, tags, m_ids, rows, tag_span):
    nb = tag_span[1] - tag_span[0] + 1
    out = [[0] * nb for _ in range(4)]
    seen = [False] * nb
    M = [int(v) for v in m_ids]
    for r in range(rows[0], rows[1]):
        t = int(tags[r])
        if t < tag_span[0] or t > tag_span[1]:
            continue
        b = t - tag_span[0]
        out[1][b] += 1
        out[0][b] += 1 if int(ids[r]) in M else 0
        out[2][b] = r if not seen[b] else min(out[2][b], r)
        out[3][b] = max(out[3][b], r + 1)
        seen[b] = True
    return out


@pytest.mark.parametrize("seed", range(6))
def test_rule_2_against_a_loop(seed):
    rng = np.random.default_rng(seed)
    m = 60
    ids = rng.integers(0, 12, m).astype(np.uint64)
    ids[rng.random(m) < 0.2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    tags = rng.integers(-1, 9, m).astype(np.int32)
    m_ids = rng.integers(0, 14, int(rng.integers(0, 8))).astype(np.uint64)
    if seed % 2:
        m_ids = np.concatenate([m_ids, m_ids[:2], np.array([0xFFFFFFFFFFFFFFFF], np.uint64)])       # duplicates, the largest id
    for rows in ((0, m), (7, 41), (13, 13)):
        for span in ((0, 8), (2, 5), (3, 3), (0, 20)):
            got = pr.tag_votes(ids, tags, m_ids, rows, span)
            want = votes_by_loop(ids, tags, m_ids, rows, span)
            for g, w in zip(got, want):
                assert g.dtype == np.int32 and g.tolist() == w, (rows, span)


def test_a_landmark_with_two_rows_under_one_tag_counts_twice_and_rows_without_points_never():
    ids = np.array([5, 5, 6, 5, 7], np.uint64)
    tags = np.array([2, 2, 2, -1, 3], np.int32)
    votes, rows, first, end = pr.tag_votes(ids, tags, [5], (0, -1), (0, 3))
    assert votes.tolist() == [0, 0, 2, 0] and rows.tolist() == [0, 0, 3, 1] and first.tolist() == [0, 0, 0, 4] and end.tolist() == [0, 0, 3, 5]


def test_the_planted_scene_votes_whole_where_best_row_voting_splits():
    c = pc.planted_scene()
    span = (0, pc.KEYFRAMES - 1)
    out = pr.places(c["query"], c["desc"], c["ids"], c["tags"], tag_span=span)
    assert out["n_landmarks"] == pc.PER_GROUP and sorted(int(v) for v in c["ids"][out["cand_row"]]) == sorted(int(v) for v in c["query_ids"])
    votes, rows, first, end = pr.tag_votes(c["ids"], c["tags"], c["ids"][out["cand_row"]], (0, -1), span)
    want = [0] * pc.KEYFRAMES
    for k in range(pc.QUERIED, pc.QUERIED + pc.SEEN_IN):
        want[k] = pc.PER_GROUP                        # the three keyframes that saw all forty
    assert votes.tolist() == want
    assert rows.tolist() == [pc.PER_GROUP * min(k + 1, pc.SEEN_IN) for k in range(pc.KEYFRAMES)]
    assert (end - first == rows).all()                # a keyframe's rows are contiguous here
    # the vote by match's best row: forty votes in all, smeared over the three keyframes
    split = pr.best_row_votes(c["query"], c["desc"], c["ids"], c["tags"], tag_span=span)
    print("covisibility", votes.tolist(), "best row", split.tolist())
    assert int(split.sum()) == pc.PER_GROUP and split.tolist() != votes.tolist() and int(split.max()) < pc.PER_GROUP
    # the places: the tie of the three goes to the oldest, which is the keyframe queried; separation 1 leaves it alone
    assert out["places"]["tag"].tolist() == [5, 6, 7] and out["places"]["votes"].tolist() == [40, 40, 40] and out["n_tags_voted"] == 3
    top = out["places"][0]
    assert (int(top["row_first"]), int(top["row_end"]), int(top["rows"])) == (int(first[5]), int(end[5]), 120)
    one = pr.places(c["query"], c["desc"], c["ids"], c["tags"], tag_span=span, separation=2)
    assert one["places"]["tag"].tolist() == [5]
    # row_hi keeps the recent keyframes out: without keyframes 6 .. 11 only keyframe 5 saw the group
    early = pr.places(c["query"], c["desc"], c["ids"], c["tags"], rows=(0, int(first[6])), tag_span=span)
    assert early["places"]["tag"].tolist() == [5] and early["n_tags_voted"] == 1


def pick_by_loop(votes, tag_lo, min_votes, separation, max_places):
    alive = {b for b, v in enumerate(votes) if v >= min_votes}
    out = []
    while alive and len(out) < max_places:
        top = max(votes[b] for b in alive)
        best = min(b for b in alive if votes[b] == top)
        out.append(tag_lo + best)
        alive = {b for b in alive if not (best - separation <= b <= best + separation)}
    return out


@pytest.mark.parametrize("case", pc.PICK_CASES, ids=lambda c: c[0])
def test_rule_3_on_hand_made_histograms(case):
    name, votes, tag_lo, min_votes, separation, max_places, want = case
    v = np.array(votes, np.int32)
    rows, first, end = v + 1, np.arange(len(v), dtype=np.int32) * 10, np.arange(len(v), dtype=np.int32) * 10 + 7
    voted, pl = pr.pick(v, rows, first, end, tag_lo, min_votes, separation, max_places)
    loop = pick_by_loop(list(votes), tag_lo, min_votes, separation, max_places)
    assert pl["tag"].tolist() == loop and voted == sum(1 for x in votes if x >= 1)
    if want is None:
        assert len(pl) == 64 and (np.diff(pl["votes"]) <= 0).all()
    else:
        assert pl["tag"].tolist() == list(want)
    for p in pl:                                       # a place carries its own bin's counts
        b = int(p["tag"]) - tag_lo
        assert (int(p["votes"]), int(p["rows"]), int(p["row_first"]), int(p["row_end"])) == (votes[b], votes[b] + 1, 10 * b, 10 * b + 7)
        assert not p["reserved"].any()


def test_rule_3_on_random_histograms_against_the_loop():
    rng = np.random.default_rng(3)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        votes = rng.integers(0, 6, n).astype(np.int32)
        mv, sep, mp = int(rng.integers(1, 5)), int(rng.integers(0, 6)), int(rng.integers(1, 12))
        _, pl = pr.pick(votes, votes, votes, votes, 100, mv, sep, mp)
        assert pl["tag"].tolist() == pick_by_loop(votes.tolist(), 100, mv, sep, mp)


def test_the_vote_scenes_are_what_their_names_say():
    runs = pc.vote_scene("runs")["tags"]
    lens = np.diff(np.flatnonzero(np.diff(np.where(runs < 0, -2, runs)) != 0))
    assert (pc.vote_scene("one_tag")["tags"].max() == pc.BIG_TAG) and set(np.unique(pc.vote_scene("one_tag")["tags"])) == {-1, 7, pc.BIG_TAG}
    assert np.array_equal(pc.vote_scene("own_tag")["tags"], np.arange(pc.VOTE_ROWS["own_tag"]))
    assert len(lens) > 100
    for kind in pc.VOTE_KINDS:
        c = pc.vote_scene(kind)
        assert 0 in c["ids"] and 0xFFFFFFFFFFFFFFFF in c["ids"]
        lst = pc.id_list(kind, 4096)
        assert len(np.unique(lst)) < len(lst) and (~np.isin(lst, c["ids"])).any() and np.isin(lst, c["ids"]).any()
