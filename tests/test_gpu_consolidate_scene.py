"""Why the consolidation exists (include/svo.h, "Landmark consolidation"), on 160 planted landmarks of 8 views each, against
svo_desc_index_retire's SVO_RETIRE_LATEST_PER_ID, the only other way to thin the index.

The descriptor part.  Views 0 .. 6 of a landmark are its base descriptor with 12 bits flipped, the latest view (7: the one taken just
before the track was lost) has 70 flipped; the queries are the base with 6 flipped; max_dist is 40.  By the triangle inequality two
normal views are at most 24 apart and a normal view and the latest at most 82, at least 58: a normal view's sum is <= 6 x 24 + 82 =
226 and the latest's >= 7 x 58 = 406, so the medoid is a normal view, at most 18 from its query, while the latest view is at least 64
from it.  retire(latest_per_id) and select give 0 candidates, consolidate and select 160.

The point part.  The latest view's point is 0.3 m off (+x in the map, for every landmark: a bias, which moves the pose instead of
being voted out); views 0 .. 5 are off by +-0.02 m at most in sign-alternating pairs, view 6 is exact.  radius is 0.1, so the latest
view is far and the mean of the seven others is the true point up to float32 rounding.  With max_dist 100 the queries also accept
the latest views; on the queries both indexes accept, localize after consolidate must return a pose nearer the truth than localize
after latest_per_id.  On the host (the first test: reloc_ref's selection, pnp_ref's least-squares pose on the candidates) the two
translation errors are 0.30 m and below 1e-5 m, more than the 10 x the case was built for; the GPU test asserts the plain inequality.
Measured on an MI355X: 123 queries both accept; 0.3000 m after latest_per_id, 6.6e-8 m after consolidate."""
import numpy as np
import pytest

import consolidate_ref as cr
import desc_retire_ref as rr
import pnp_ref
import reloc_cases as rc
import reloc_ref
from gpu_kit import api  # noqa: F401  (the fixture is found by name)

N, VIEWS, RADIUS, OFF = 160, 8, 0.1, 0.3


def planted():
    s = rc.scene(N, 3301, noise_bits=0)
    rng = np.random.default_rng(3302)
    desc, xyz = np.zeros((VIEWS, N, 32), np.uint8), np.zeros((VIEWS, N, 3), np.float32)
    for j in range(N):
        for v in range(VIEWS):
            desc[v, j] = rc.flip(rng, s["desc"][j], 70 if v == VIEWS - 1 else 12)
        for v in (0, 2, 4):
            d = rng.uniform(-0.02, 0.02, 3).astype(np.float32)
            xyz[v, j], xyz[v + 1, j] = s["xyz"][j] + d, s["xyz"][j] - d
        xyz[6, j] = s["xyz"][j]
        xyz[7, j] = s["xyz"][j] + np.array([OFF, 0, 0], np.float32)
    query = np.stack([rc.flip(rng, d, 6) for d in s["desc"]])
    case = dict(desc=desc.reshape(-1, 32), ids=np.tile(s["ids"], VIEWS), xyz=xyz.reshape(-1, 3), tags=np.repeat(np.arange(VIEWS), N).astype(np.int32))
    return s, case, query


def pose_error(R, t, s):
    """(translation error of the camera centre in m, rotation error in rad)"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return float(np.linalg.norm(-R.T @ t + s["R"].T @ s["t"])), pnp_ref.rot_angle(R, s["R"])


def thinned(case):
    keep, _ = rr.retire(case["ids"], case["tags"], latest_per_id=True)
    latest = {k: case[k][keep] for k in ("desc", "ids", "xyz", "tags")}
    return latest, cr.consolidate(case["desc"], case["ids"], case["xyz"], case["tags"], RADIUS)


def test_the_scene_on_the_host():
    s, case, query = planted()
    latest, cons = thinned(case)
    assert cons["result"] == cr.Result(N * VIEWS, N, N * (VIEWS - 1), N, 0, N) and len(latest["ids"]) == N
    sel = {name: reloc_ref.select_index(query, s["xy"], m["desc"], m["ids"], m["xyz"], m["tags"], max_dist=40) for name, m in (("latest", latest), ("cons", cons))}
    assert len(sel["latest"]["query"]) == 0 and len(sel["cons"]["query"]) == N
    wide = {name: reloc_ref.select_index(query, s["xy"], m["desc"], m["ids"], m["xyz"], m["tags"], max_dist=100) for name, m in (("latest", latest), ("cons", cons))}
    both = np.intersect1d(wide["latest"]["query"], wide["cons"]["query"])
    assert len(both) >= 100
    err = {}
    for name, w in wide.items():
        pick = np.isin(w["query"], both)
        R, t = pnp_ref.minimise(s["K"], s["R"], s["t"], w["xyz"][pick], w["xy"][pick])[:2]
        err[name] = pose_error(R, t, s)
    print("host: %d queries both accept; pose error (m, rad) after latest_per_id %s, after consolidate %s" % (len(both), err["latest"], err["cons"]))
    assert err["latest"][0] > 10 * err["cons"][0] and err["latest"][0] > 0.2


@pytest.mark.gpu
def test_select_and_localize_after_consolidate_and_after_latest_per_id(api):
    s, case, query = planted()
    latest, cons = thinned(case)
    got = {}
    for name in ("latest", "cons"):
        ix = api.DescriptorIndex(N * VIEWS, points=True)
        try:
            ix.add_points(case["desc"], case["ids"], case["xyz"], case["tags"])
            if name == "latest":
                assert ix.retire(latest_per_id=True)[-1] == N
            else:
                assert tuple(ix.consolidate(RADIUS)[0]) == tuple(cons["result"])
            assert not cr.same_rows(ix.read_rows(), cr.as_read(latest if name == "latest" else cons))
            narrow = ix.select(query, s["xy"], max_dist=40)
            wide = ix.select(query, s["xy"], max_dist=100)
            got[name] = (ix, len(narrow["query"]), wide["query"])
        except Exception:
            ix.close()
            raise
    try:
        assert got["latest"][1] == 0 and got["cons"][1] == N
        both = np.intersect1d(got["latest"][2], got["cons"][2])
        assert len(both) >= 100
        err = {}
        for name in ("latest", "cons"):
            rec, cand = got[name][0].localize(s["K"], query[both], s["xy"][both], max_dist=100)
            assert rec.success and rec.n_candidates == len(both), (name, rec)
            err[name] = pose_error(rec.R, rec.t, s)
        print("GPU: %d queries both accept; pose error (m, rad) after latest_per_id %s, after consolidate %s" % (len(both), err["latest"], err["cons"]))
        assert err["cons"][0] < err["latest"][0]
    finally:
        for ix, _, _ in got.values():
            ix.close()
