"""tests/insert_ref.py held to a second statement of the rules of include/svo.h, "Batched insertion": a loop over entries and rows
that appends one row at a time with Python integers for the ids and one f64 expression per coordinate.  No GPU.  Also here: the
four new symbols are in the header and in the binding table."""
import os
import re

import numpy as np
import pytest

import insert_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row_by_row(entries, need_flags, id_base, with_points, cam_to_map, tags, size):
    need = need_flags | (ir.OBS_HAS_XYZ if with_points else 0)
    desc, ids, xyz, tg, first, added = [], [], [], [], [], []
    at = size
    for b, (obs, d) in enumerate(entries):
        first.append(at); added.append(0)
        for i in range(len(obs)):
            if (int(obs["flags"][i]) & need) != need:
                continue
            desc.append(bytes(d[i])); ids.append((int(obs["id"][i]) + (int(id_base[b]) if id_base is not None else 0)) % (1 << 64))
            if with_points:
                x, y, z = (np.float64(v) for v in obs["xyz"][i])
                if cam_to_map is None:
                    p = [obs["xyz"][i][r] for r in range(3)]
                else:
                    T = np.asarray(cam_to_map[b], np.float64).reshape(4, 4)
                    with np.errstate(over="ignore", invalid="ignore"):
                        p = [np.float32(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]) for r in range(3)]
                xyz.append(p); tg.append(int(tags[b]) if tags is not None else 0)
            at += 1; added[-1] += 1
    return desc, ids, xyz, tg, first, added


def agree(entries, need_flags, id_base=None, with_points=False, cam_to_map=None, tags=None, size=0):
    got = ir.insert(entries, need_flags, id_base, with_points, cam_to_map, tags, size)
    desc, ids, xyz, tg, first, added = row_by_row(entries, need_flags, id_base, with_points, cam_to_map, tags, size)
    assert [bytes(r) for r in got["desc"]] == desc
    assert [int(v) for v in got["ids"]] == ids and got["ids"].dtype == np.uint64
    assert list(got["first_row"]) == first and list(got["n_added"]) == added
    if with_points:
        assert got["xyz"].dtype == np.float32 and got["xyz"].tobytes() == np.array(xyz, np.float32).reshape(-1, 3).tobytes()
        assert list(got["tags"]) == tg
    else:
        assert got["xyz"] is None and got["tags"] is None
    return got


def entries_of(rows, pattern="random", seed=5):
    return [ir.make_entry(r, ir.flag_pattern(pattern, r, seed + b), seed + 100 * b) for b, r in enumerate(rows)]


@pytest.mark.parametrize("with_points", [False, True])
@pytest.mark.parametrize("pattern", ["none", "all", "alternate", "tile_last", "lanes_63_64", "random"])
def test_patterns(pattern, with_points):
    e = entries_of([0, 1, 63, 64, 65, 255, 256, 257, 513], pattern)
    T = [ir.pose(b) for b in range(len(e))] if with_points else None
    agree(e, ir.OBS_INLIER, None, with_points, T, list(range(len(e))) if with_points else None, size=7)


def test_need_flags_zero_keeps_every_row_and_points_need_xyz():
    e = entries_of([40, 3], "alternate")
    e[0][0]["flags"][5] = 0                                                   # no bit at all: kept by the plain call, not with points
    assert agree(e, 0)["n_added"].tolist() == [40, 3]
    assert agree(e, 0, with_points=True)["n_added"].tolist() == [39, 3]


def test_id_wraps_at_two_to_the_64():
    e = entries_of([4, 4], "all")
    e[1][0]["id"][:] = [0, 1, 2, -1]                                          # int64 -1 is 2^64 - 1 as uint64
    base = np.array([(1 << 64) - 2, (1 << 64) - 1], np.uint64)
    got = agree(e, ir.OBS_INLIER, base)
    assert got["ids"].tolist() == [(1 << 64) - 2, (1 << 64) - 1, 0, 1, (1 << 64) - 1, 0, 1, (1 << 64) - 2]


def test_an_entry_without_rows_and_duplicates():
    a, b = entries_of([10, 7], "random", 9)
    empty = ir.make_entry(0, 0, 1)
    got = agree([a, empty, b, a, empty], ir.OBS_INLIER, np.array([0, 5, 1 << 48, 0, 9], np.uint64), True, [ir.pose(i) for i in range(5)], [0, 1, 2, 3, 4], size=100)
    assert got["n_added"][1] == 0 and got["n_added"][4] == 0 and got["n_added"][0] == got["n_added"][3]
    assert got["first_row"][1] == got["first_row"][2]


def test_cam_to_map_none_stores_xyz_as_it_is():
    e = entries_of([30], "all")
    got = agree(e, ir.OBS_INLIER, None, True, None, [3])
    assert got["xyz"].tobytes() == e[0][0]["xyz"].tobytes()


def test_plain_call_on_an_index_with_points():
    got = ir.insert(entries_of([5], "all"), ir.OBS_INLIER, index_has_points=True)
    assert np.isinf(got["xyz"]).all() and (got["tags"] == ir.POINT_NONE).all()


def test_refusals():
    e = entries_of([20], "all")
    with pytest.raises(ir.Refused):
        ir.insert(e, ir.OBS_INLIER, size=5, capacity=24)
    assert ir.insert(e, ir.OBS_INLIER, size=5, capacity=25)["n_added"].tolist() == [20]
    with pytest.raises(ir.Refused):
        ir.insert(e, ir.OBS_INLIER, with_points=True, tags=[-1])
    bad = np.eye(4); bad[1, 2] = np.nan
    with pytest.raises(ir.Refused):
        ir.insert(e, ir.OBS_INLIER, with_points=True, cam_to_map=[bad])
    with pytest.raises(ir.Refused):
        ir.insert(e, ir.OBS_INLIER, with_points=True, cam_to_map=[ir.pose(1, 1e38)])
    e[0][0]["flags"][:] = ir.OBS_HAS_XYZ                                       # nothing kept: nothing to refuse
    assert ir.insert(e, ir.OBS_INLIER, with_points=True, cam_to_map=[ir.pose(1, 1e38)])["n_added"].tolist() == [0]


NEW = ("svo_desc_index_add_frames", "svo_desc_index_add_frames_points", "svo_desc_index_add_obs", "svo_desc_index_get_insert_stats")


def test_the_new_symbols_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "svo.h")).read()
    from stereo_visual_odometry_amd import _lib
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), s
        assert s in _lib.PROTOTYPES and hasattr(_lib.lib, s), s
    assert "#define SVO_INSERT_MAX_ENTRIES 1024" in txt
