"""tests/reloc_batch_cases.py is what tests/test_gpu_reloc_batch.py needs, asserted without a GPU — the GPU tests' conditions are
conditions, not measurements — with tests/reloc_batch_ref.py, the numpy loop over the slices, and the CPU oracle's PnP:
the slice sizes, the camera that sees nothing, the cameras at min_candidates - 1 and min_candidates, the camera whose PnP fails,
the NaN pixel, the repeated-structure camera's 160 candidates guided and none unguided, different camera matrices and priors, the two
workloads of one shape, the camera counts across the build switch, and the row range that starts inside a tile."""
import numpy as np

import guide_ref as gref
import oracle_lib as orc
import reloc_batch_cases as bc
import reloc_batch_ref as bref


def select(name, guided=True, **kw):
    return bref.select_batch(bc.index_rows(), [bc.cameras()[name]], guided, **kw)[0]


def test_the_index_and_the_slices():
    rows, cams = bc.index_rows(), bc.cameras()
    assert len(rows["desc"]) == len(rows["ids"]) == len(rows["xyz"]) == len(rows["tags"]) == 2624 and bc.SCENE_LO == 2304
    assert [len(cams[n]["query"]) for n in bc.MIX[:8]] == [0, 1, 63, 64, 65, 1024, 1025, 4096]
    assert len({cams[n]["K"].tobytes() for n in bc.MIX}) >= 7 and len({cams[n]["R"].tobytes() + cams[n]["t"].tobytes() for n in bc.MIX}) >= 9
    assert [len(cams[a]["query"]) for a in bc.STALE_A] == [len(cams[b]["query"]) for b in bc.STALE_B]
    assert all(cams[a]["query"].tobytes() != cams[b]["query"].tobytes() for a, b in zip(bc.STALE_A, bc.STALE_B))
    assert sum(len(cams[n]["query"]) for n in bc.MIX) > 4096              # one call holds more than a single call may
    assert any(len(cams[n]["query"]) > 1024 for n in bc.MIX)              # and a camera that spans several tile groups
    assert min(bc.COUNTS) == 1 and 8 in bc.COUNTS and 9 in bc.COUNTS and max(bc.COUNTS) > 64
    lo, hi = bc.ROW_RANGES[1]
    assert lo % 1024 != 0 and lo % 64 != 0 and (hi - lo) % 8 != 0 and hi <= 2624 and hi - lo > 1024


def test_the_planned_cameras():
    assert len(select("nothing")["query"]) == 0
    uv = gref.project(bc.cameras()["nothing"]["K"], bc.cameras()["nothing"]["R"], bc.cameras()["nothing"]["t"], bc.index_rows()["xyz"][bc.SCENE_LO:],
                      bc.index_rows()["tags"][bc.SCENE_LO:])
    assert not np.isfinite(uv).any()                                      # the scene is behind this prior
    assert len(select("repeated")["query"]) == 160 and len(select("repeated", guided=False)["query"]) == 0
    assert len(select("five")["query"]) == bc.MIN_CANDIDATES - 1 and len(select("six")["query"]) == bc.MIN_CANDIDATES == len(select("sixb")["query"])
    for name in ("n63", "n64", "n65", "n63b", "n64b", "n65b"):
        assert len(select(name)["query"]) >= 10 and len(select(name, guided=False)["query"]) >= 10, name
    c = bc.cameras()["n1024"]
    assert np.isnan(c["xy"][7, 0]) and 7 not in select("n1024")["query"].tolist() and len(select("n1024")["query"]) > 100
    lo, hi = bc.ROW_RANGES[1]
    assert len(select("n1025", row_lo=lo, row_hi=hi)["query"]) > 50 and len(select("repeated", row_lo=lo, row_hi=hi)["query"]) > 100


def test_the_pnp_of_the_planned_cameras():
    """the CPU oracle's RANSAC-PnP on the reference's candidates: which cameras find a pose"""
    for name, succeeds in (("repeated", True), ("six", True), ("n64", True), ("random", False)):
        c, s = bc.cameras()[name], select(name)
        ok, R, t, inl, _ = orc.camera_to_world(c["K"], s["xy"], s["xyz"], c["R"], c["t"])
        assert bool(ok) == succeeds, name
    assert len(select("random")["query"]) == 40


def test_the_small_cycle_has_its_own_camera_matrices():
    names, K, guides, queries, xys = bc.small(65)
    assert len(names) == 65 and set(names) == set(bc.SMALL)
    assert K[0].tobytes() != K[len(bc.SMALL)].tobytes() and names[0] == names[len(bc.SMALL)]


def test_cell_keys_order_pixels_by_cell():
    k = bc.cell_keys(np.array([[5, 5], [30, 5], [5, 30], [np.nan, 1], [-1, -1]], np.float32), 12.0)
    assert k.tolist() == [[0, 0], [0, 1], [1, 0], [np.inf, np.inf], [-1, -1]]
    assert bc.cell_keys(np.array([[2.5, 0.2]], np.float32), 0.0).tolist() == [[0, 2]]   # a side of 1 px at least
