"""Guided relocalisation on a real GPU (include/svo.h, "Guided search": svo_desc_index_select_guided,
svo_desc_index_localize_guided) on the repeated-structure scene of tests/guide_cases.py: 160 landmarks, each stored twice 4 m apart
with the same descriptor.

 - the unguided calls fail as the reference says they must: select gives 0 candidates, localize success = 0;
 - select_guided equals tests/guide_ref.py's candidates: query, row, pixel bits, point bits — 160, all on the first copy;
 - localize_guided equals api.cameraToWorld on those arrays byte for byte: pose, inlier set, iterations; its pose is the true one;
 - the gate at min_candidates - 1 and at min_candidates, by cutting the query list;
 - the results with the sort off, and at chunk_rows 64, are the same."""
import numpy as np
import pytest

import guide_cases as cases
import guide_ref as gref
import reloc_ref as rref
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(api):
    s = cases.repeated_scene()
    ix = api.DescriptorIndex(len(s["desc"]), points=True)
    ix.add_points(s["desc"], s["ids"], s["xyz"], s["tags"])
    s["ix"] = ix
    s["guide"] = (s["K"], s["R0"], s["t0"], s["radius"])
    s["want"] = gref.select_index(*s["guide"], s["query"], s["xy"], s["desc"], s["ids"], s["xyz"], s["tags"])
    yield s
    ix.close()


def same(got, want):
    assert got["query"].tolist() == want["query"].tolist() and got["row"].tolist() == want["row"].tolist()
    assert got["xy"].tobytes() == want["xy"].tobytes() and got["xyz"].tobytes() == want["xyz"].tobytes()


def test_unguided_the_ratio_test_rejects_every_query(world):
    s, ix = world, world["ix"]
    assert len(rref.select_index(s["query"], s["xy"], s["desc"], s["ids"], s["xyz"], s["tags"])["query"]) == 0
    assert len(ix.select(s["query"], s["xy"])["query"]) == 0
    res, cand = ix.localize(s["K"], s["query"], s["xy"], s["R0"], s["t0"])
    assert (res.success, res.n_candidates, res.n_inliers, res.iters_run) == (False, 0, 0, 0) and len(cand["query"]) == 0


def test_select_guided_equals_the_reference(world):
    s, ix = world, world["ix"]
    assert len(s["want"]["query"]) == 160 and (s["want"]["row"] == np.arange(160)).all()
    same(ix.select_guided(*s["guide"], s["query"], s["xy"]), s["want"])
    ix.set_guided_sort(False); ix.chunk_rows = 64
    try:
        same(ix.select_guided(*s["guide"], s["query"], s["xy"]), s["want"])
    finally:
        ix.set_guided_sort(True); ix.chunk_rows = 0
    # a tighter radius than the prior's error loses queries, as the reference says
    tight = gref.select_index(s["K"], s["R0"], s["t0"], 6.0, s["query"], s["xy"], s["desc"], s["ids"], s["xyz"], s["tags"])
    assert 6 <= len(tight["query"]) < 160
    same(ix.select_guided(s["K"], s["R0"], s["t0"], 6.0, s["query"], s["xy"]), tight)


def test_localize_guided_is_camera_to_world_on_select_guideds_arrays(api, world):
    s, ix = world, world["ix"]
    sel = ix.select_guided(*s["guide"], s["query"], s["xy"])
    same(sel, s["want"])
    for guess, over in (((s["R0"], s["t0"]), dict(reproj_error=2.0)), ((np.eye(3), np.zeros(3)), dict(ransac_iterations=30, reproj_error=2.0, confidence=0.9))):
        prm = ix.reloc_params(**over)
        (inl, ok), R, t, iters = api.cameraToWorld(s["K"], sel["xy"], sel["xyz"], guess[0], guess[1], prm.ransac_iterations, prm.reproj_error, prm.confidence)
        res, cand = ix.localize_guided(*s["guide"], s["query"], s["xy"], guess[0], guess[1], params=prm)
        assert ok and res.success and res.n_candidates == 160 and res.iters_run == iters and res.n_inliers == len(inl) >= 150
        assert cand["query"].tolist() == sel["query"].tolist() and cand["row"].tolist() == sel["row"].tolist()
        assert res.R.tobytes() == R.tobytes() and res.t.tobytes() == t.tobytes()
        assert np.flatnonzero(cand["inlier"]).tolist() == inl.tolist()
        assert res.T.tobytes() == api.getInverseTransform(R, t).tobytes()
        assert np.abs(res.R - s["R"]).max() < 1e-3 and np.abs(res.t.ravel() - s["t"]).max() < 1e-2
    # the guess defaults to the guide's pose
    a, _ = ix.localize_guided(*s["guide"], s["query"], s["xy"], reproj_error=2.0)
    b, _ = ix.localize_guided(*s["guide"], s["query"], s["xy"], s["R0"], s["t0"], reproj_error=2.0)
    assert a.success and a.R.tobytes() == b.R.tobytes() and a.t.tobytes() == b.t.tobytes()


def test_the_gate_by_cutting_the_query_list(world):
    s, ix = world, world["ix"]
    q, xy = s["query"][:40], s["xy"][:40]
    want = gref.select_index(*s["guide"], q, xy, s["desc"], s["ids"], s["xyz"], s["tags"])
    assert len(want["query"]) == 40
    res, cand = ix.localize_guided(*s["guide"], q, xy, min_candidates=41, reproj_error=2.0)
    assert not rref.gate(40, 41)
    assert (res.success, res.n_candidates, res.n_inliers, res.iters_run) == (False, 40, 0, 0)
    assert res.R.tobytes() == s["R0"].tobytes() and res.t.ravel().tobytes() == s["t0"].tobytes() and not res.T.any() and not cand["inlier"].any()
    assert cand["query"].tolist() == want["query"].tolist() and cand["row"].tolist() == want["row"].tolist()
    res, cand = ix.localize_guided(*s["guide"], q, xy, min_candidates=40, reproj_error=2.0)
    assert rref.gate(40, 40)
    assert res.success and res.n_candidates == 40 and res.iters_run > 0 and res.n_inliers == cand["inlier"].sum() >= 36
