"""Inputs of the batched relocalisation's tests (include/svo.h, "Batched relocalisation").

index_rows(): guide_cases.planned_case()'s 2304 rows followed by guide_cases.repeated_scene()'s 320 — one index of 2624 rows.

cameras(): the named cameras, each a dict of K, the prior R, t, radius, query, xy:
  n0, n1, n63, n64, n65, n1024, n1025   slices of the planned case's queries under slightly different camera matrices and priors;
                          n1024's query 7 has a NaN pixel;
  n4096                   the planned case whole, under its own prior and K, so that its situations A - G occur in a batch;
  repeated                the repeated-structure scene: 160 candidates guided, none unguided;
  nothing                 the scene's queries under a prior that looks the other way: no row is visible;
  five, six               the scene's first 5 and 6 queries: min_candidates - 1 and min_candidates candidates at the default 6;
  random                  40 of the planned case's rows, found again by their own descriptors behind a gate that admits everything, at
                          random pixels: 40 candidates whose PnP fails.
MIX is the order in which one call takes them all; small(count) cycles through the small ones with a camera matrix of its own per
camera, for the camera counts 1, 2, 8, 9 and 65; STALE_A and STALE_B are two workloads of identical shape."""
import functools

import numpy as np

import guide_cases as gc

MIN_CANDIDATES = 6
SCENE_LO = gc.N_ROWS                                                     # the scene's rows follow the planned case's
MIX = ["n0", "n1", "n63", "n64", "n65", "n1024", "n1025", "n4096", "repeated", "nothing", "five", "six", "random"]
SMALL = ["repeated", "n63", "six", "n64", "five", "random", "n65", "nothing", "n1"]
STALE_A, STALE_B = ["n63", "n64", "n65", "six"], ["n63b", "n64b", "n65b", "sixb"]
COUNTS = [1, 2, 8, 9, 65]
ROW_RANGES = [(0, -1), (1030, gc.N_ROWS + 317)]                          # the second starts inside a tile; its length, 1591, is no multiple of 8


@functools.lru_cache(maxsize=None)
def index_rows():
    p, s = gc.planned_case(), gc.repeated_scene()
    return dict(desc=np.concatenate([p["desc"], s["desc"]]), ids=np.concatenate([p["ids"], s["ids"] + np.uint64(1 << 40)]),
                xyz=np.concatenate([p["xyz"], s["xyz"]]), tags=np.concatenate([p["tags"], s["tags"]]))


def fill(ix, rows):
    """the rows into an api.DescriptorIndex(points=True), run by run: add_points where the rows have a point, plain add where not"""
    has = rows["tags"] >= 0
    for seg in np.split(np.arange(len(has)), np.flatnonzero(np.diff(has.astype(np.int8))) + 1):
        if has[seg[0]]:
            ix.add_points(rows["desc"][seg], rows["ids"][seg], rows["xyz"][seg], rows["tags"][seg])
        else:
            ix.add(rows["desc"][seg], rows["ids"][seg])


def _cam(K, R, t, radius, query, xy):
    return dict(K=np.asarray(K, np.float32).reshape(3, 3), R=np.asarray(R, np.float64).reshape(3, 3), t=np.asarray(t, np.float64).reshape(3),
                radius=float(radius), query=np.ascontiguousarray(query, np.uint8).reshape(-1, 32), xy=np.ascontiguousarray(xy, np.float32).reshape(-1, 2))


@functools.lru_cache(maxsize=None)
def cameras():
    p, s = gc.planned_case(), gc.repeated_scene()
    cams = {}
    slices = dict(n0=(0, 0), n1=(5, 6), n63=(200, 263), n64=(300, 364), n65=(400, 465), n1024=(0, 1024), n1025=(1000, 2025),
                  n63b=(500, 563), n64b=(600, 664), n65b=(700, 765))
    for i, (name, (lo, hi)) in enumerate(slices.items()):
        K = p["K"].copy()
        K[0, 0] += 3 * i; K[1, 1] += 2 * i; K[0, 2] += 0.5 * i
        cams[name] = _cam(K, gc.rot(0.001 * i, -0.002 * i, 0.0), [0.01 * i, -0.005 * i, 0.02 * i], p["radius"], p["query"][lo:hi], p["xy"][lo:hi])
    cams["n1024"]["xy"][7] = (np.nan, 100.0)
    cams["n4096"] = _cam(p["K"], p["R"], p["t"], p["radius"], p["query"], p["xy"])
    cams["repeated"] = _cam(s["K"], s["R0"], s["t0"], s["radius"], s["query"], s["xy"])
    cams["nothing"] = _cam(s["K"], gc.rot(0, np.pi, 0) @ s["R0"], s["t0"], s["radius"], s["query"], s["xy"])
    cams["five"] = _cam(s["K"], s["R0"], s["t0"], s["radius"], s["query"][:5], s["xy"][:5])
    cams["six"] = _cam(s["K"], s["R0"], s["t0"], s["radius"], s["query"][:6], s["xy"][:6])
    cams["sixb"] = _cam(s["K"], s["R0"], s["t0"], s["radius"], s["query"][20:26], s["xy"][20:26])
    rng = np.random.default_rng(4)
    # behind a gate that admits every visible row each query finds the row it copies, at distance 0; the pixels are random
    rows = np.flatnonzero(p["tags"][:2000] >= 0)
    rows = rows[np.unique(p["ids"][rows], return_index=True)[1]][:40]
    cams["random"] = _cam(p["K"], p["R"], p["t"], 3e38, p["desc"][rows], np.stack([rng.uniform(0, 640, 40), rng.uniform(0, 360, 40)], 1))
    return cams


def workload(names):
    """-> (K (B, 3, 3), guides [(R, t, radius)], queries, xys) of the named cameras, for api.DescriptorIndex.localize_batch"""
    c = [cameras()[n] for n in names]
    return np.stack([x["K"] for x in c]), [(x["R"], x["t"], x["radius"]) for x in c], [x["query"] for x in c], [x["xy"] for x in c]


def small(count):
    """`count` cameras cycling through SMALL, camera b with a camera matrix of its own -> (names, K, guides, queries, xys)"""
    names = [SMALL[b % len(SMALL)] for b in range(count)]
    K, guides, queries, xys = workload(names)
    K = K.copy()
    for b in range(count):
        K[b, 0, 0] += 0.25 * (b // len(SMALL)); K[b, 1, 2] += 0.125 * (b // len(SMALL))
    return names, K, guides, queries, xys


def cell_keys(xy, radius):
    """the order kernel's key of each pixel as a sortable pair -> (n, 2) float64 (cy, cx), a non-finite pixel (inf, inf)"""
    side = max(2.0 * float(radius), 1.0)
    with np.errstate(all="ignore"):
        c = np.floor(np.asarray(xy, np.float32).astype(np.float64) / side)
    c[~np.isfinite(c).all(1)] = np.inf
    return c[:, ::-1]
