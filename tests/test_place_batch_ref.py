"""tests/place_batch_ref.py, the batched place candidates' reference, held to a brute-force count — plain Python loops over rows,
cameras and lists, no numpy — on small hand-made cases."""
import numpy as np

import place_batch_ref as pbr

TOP = 2 ** 64 - 1
#        row: 0  1  2    3  4  5  6    7  8   9
IDS = [7, 7, 9, TOP, 0, 9, 7, 11, 0, 13]
TAGS = [0, 0, 1, 1, -1, 2, 2, 2, 5, 1]


def brute(ids, tags, lists, rows, span):
    nb = span[1] - span[0] + 1
    votes = [[0] * nb for _ in lists]
    n_rows, first, end = [0] * nb, [0] * nb, [0] * nb
    for r in range(rows[0], rows[1]):
        if not span[0] <= tags[r] <= span[1]:
            continue
        t = tags[r] - span[0]
        first[t] = r if n_rows[t] == 0 else first[t]
        n_rows[t] += 1
        end[t] = r + 1
        for b, m in enumerate(lists):
            votes[b][t] += 1 if any(v == ids[r] for v in m) else 0       # a set: a repeated id votes once a row
    return votes, n_rows, first, end


def check(lists, rows=(0, len(IDS)), span=(0, 5)):
    got = pbr.tag_votes_batch(np.array(IDS, np.uint64), np.array(TAGS, np.int32), [np.array(m, np.uint64) for m in lists], rows, span)
    want = brute(IDS, TAGS, lists, rows, span)
    assert got[0].shape == (len(lists), span[1] - span[0] + 1) and got[0].dtype == np.int32
    for g, w in zip(got, want):
        assert np.asarray(g).tolist() == w
    return got


def test_one_id_in_three_cameras_and_twice_in_one():
    votes = check([[7], [9, 7, 7], [7, 11], [13]])[0]
    assert votes[0].tolist() == [2, 0, 1, 0, 0, 0] and votes[1].tolist() == [2, 1, 2, 0, 0, 0]       # 7 twice in camera 1: no extra vote
    assert votes[2].tolist() == [2, 0, 2, 0, 0, 0] and votes[3].tolist() == [0, 1, 0, 0, 0, 0]


def test_ids_0_and_the_largest_empty_lists_and_absent_ids():
    votes = check([[0], [TOP], [], [12345], [0, TOP]])[0]
    assert votes[0].tolist() == [0, 0, 0, 0, 0, 1]      # row 4 holds id 0 too, but has no point
    assert votes[1].tolist() == [0, 1, 0, 0, 0, 0] and not votes[2].any() and not votes[3].any()
    assert votes[4].tolist() == (votes[0] + votes[1]).tolist()


def test_row_ranges_windows_and_no_cameras():
    check([[7], [9]], rows=(1, 7), span=(1, 2))
    check([[7], [9]], rows=(3, 3))
    check([[7, 9, 0]], span=(5, 5))
    got = check([])
    assert got[0].shape == (0, 6) and got[1].tolist() == [2, 3, 3, 0, 0, 1]


def test_places_per_camera_are_the_single_reference():
    ids, tags = np.array(IDS, np.uint64), np.array(TAGS, np.int32)
    lists = [np.array(m, np.uint64) for m in ([7, 9], [7, 7], [], [9, 11, 13])]
    got = pbr.places_from_ids_batch(ids, tags, lists, tag_span=(0, 5), max_places=2)
    assert [g["n_landmarks"] for g in got] == [2, 1, 0, 3] and [g["n_places"] for g in got] == [2, 2, 0, 2]
    assert got[0]["places"]["tag"].tolist() == [0, 2] and got[0]["places"]["votes"].tolist() == [2, 2]      # ties: the smaller tag
    assert got[3]["places"]["tag"].tolist() == [1, 2] and got[3]["places"]["votes"].tolist() == [2, 2]
    assert got[0]["places"]["row_first"].tolist() == [0, 5] and got[0]["places"]["row_end"].tolist() == [2, 8]
