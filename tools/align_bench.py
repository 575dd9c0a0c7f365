#!/usr/bin/env python3
"""What aligning two row spans of a descriptor index costs on the device (include/svo.h, "Map alignment"), and what the host loop it
replaces costs:

    python tools/align_bench.py [--out FILE] [--sizes 65536,1048576] [--source 2048] [--repeats 7]

One process.  Per destination size: an index of `size` destination rows (random descriptors, ids in runs of 4) followed by `source`
source rows, each a destination row's descriptor with up to 8 bits flipped, its point moved by a rigid motion, 5 mm of noise and 30 %
outliers.  The legs run alternately, each once as a warm-up and then --repeats times, and are reported as the median, the smallest and
the largest wall time of the synchronous call(s) in milliseconds:

  align        svo_desc_index_align: nothing is uploaded; beside it the device span from its first kernel to its last (HIP events:
               svo_desc_index_set_timing)
  match_rows   svo_desc_index_match_rows alone: the search's share of the call
  host_1, host_16
               the path the call replaces: svo_desc_index_match with the caller's own copy of the source descriptors, then rules 2 - 9
               in numpy on the host with 1 and with 16 threads over the hypotheses (batched eigh for Horn's quaternion), then nothing
               more — transform_points is the same call after either.  The host path's pairs and inliers equal the device's (checked,
               untimed).

Figures, not pass marks.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M64 = (1 << 64) - 1
INLIER_DIST, HYPOTHESES, OUTLIERS, SIGMA = 0.05, 256, 0.3, 0.005


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample(h, n):
    out, k = [], 0
    while k < 64 and len(out) < 3:
        d = (mix64((h << 32) | k) >> 32) % n
        k += 1
        if d not in out:
            out.append(d)
    c = 0
    while len(out) < 3:
        if c not in out:
            out.append(c)
        c += 1
    return out


def scene(size, n_src, seed=5):
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (size + n_src, 32), dtype=np.uint8)
    pick = rng.choice(size // 4, n_src, replace=False) * 4                 # one row of n_src different landmarks
    flips = rng.integers(0, 256, (n_src, 8))
    src = desc[pick].copy()
    for b in range(8):
        on = rng.random(n_src) < 0.5
        src[np.flatnonzero(on), flips[on, b] >> 3] ^= (1 << (flips[on, b] & 7)).astype(np.uint8)
    desc[size:] = src
    ids = np.concatenate([np.arange(size) // 4, 10 ** 9 + np.arange(n_src)]).astype(np.uint64)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    xyz = rng.uniform(-30, 30, (size + n_src, 3)).astype(np.float32)
    P = xyz[size:].astype(np.float64)
    Q = P @ R.T + np.array([12.0, -3.0, 40.0]) + rng.normal(0, SIGMA, P.shape)
    out = rng.random(n_src) < OUTLIERS
    Q[out] += rng.uniform(1, 5, (int(out.sum()), 3)) * rng.choice([-1.0, 1.0], (int(out.sum()), 3))
    xyz[pick] = Q.astype(np.float32)
    return dict(desc=desc, ids=ids, xyz=xyz, tags=np.zeros(size + n_src, np.int32))


def host_pairs(m, ids_src, tags, tags_src, max_dist=40, num=7, den=10):
    """rules 2 - 5 in numpy on the result rows m of the source rows"""
    row = m["row"].astype(np.int64)
    dist, dist2 = m["dist"].astype(np.int64), m["dist2"].astype(np.int64)
    acc = (row >= 0) & (tags_src != -1) & (dist <= max_dist) & (dist * den < dist2 * num)
    acc[acc] &= tags[row[acc]] != -1
    j = np.flatnonzero(acc)
    for key in (m["id"], ids_src):                                        # rule 3, then rule 4: the first of (key, dist, j)
        o = j[np.lexsort((j, dist[j], key[j]))]
        first = np.ones(len(o), bool)
        first[1:] = key[o][1:] != key[o][:-1]
        j = np.sort(o[first])
    return j, row[j]


def horn_batch(P, Q):
    """Horn's closed form for a batch of point sets (B, k, 3) -> R (B, 3, 3), t (B, 3)"""
    cp, cq = P.mean(1), Q.mean(1)
    S = np.einsum("bki,bkj->bij", P - cp[:, None], Q - cq[:, None])
    N = np.empty((len(P), 4, 4))
    N[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]; N[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    N[:, 2, 2] = S[:, 1, 1] - S[:, 2, 2] - S[:, 0, 0]; N[:, 3, 3] = S[:, 2, 2] - S[:, 0, 0] - S[:, 1, 1]
    N[:, 0, 1] = N[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]; N[:, 0, 2] = N[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]; N[:, 0, 3] = N[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]; N[:, 1, 3] = N[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]; N[:, 2, 3] = N[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    q = np.linalg.eigh(N)[1][:, :, 3]
    q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)], -1),
                  np.stack([2 * (q1 * q2 + q0 * q3), q0 * q0 + q2 * q2 - q1 * q1 - q3 * q3, 2 * (q2 * q3 - q0 * q1)], -1),
                  np.stack([2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 + q3 * q3 - q1 * q1 - q2 * q2], -1)], 1)
    return R, cq - np.einsum("bij,bj->bi", R, cp)


def host_fit(P, Q, picks, pool, threads, min_pairs=6, rounds=4):
    """rules 6 - 10 in numpy; the hypotheses in `threads` slices"""
    d2 = float(np.float32(INLIER_DIST)) ** 2

    def score(sl):
        R, t = horn_batch(P[picks[sl]], Q[picks[sl]])
        r = np.einsum("bij,nj->bni", R, P) + t[:, None] - Q[None]
        return ((r * r).sum(2) <= d2).sum(1)

    cuts = np.linspace(0, len(picks), threads + 1).astype(int)
    slices = [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    counts = np.concatenate(list(pool.map(score, slices)) if threads > 1 else [score(s) for s in slices])
    best = int(np.argmax(counts))                                         # the first of the largest
    R, t = horn_batch(P[picks[best]][None], Q[picks[best]][None])
    inl = (((P @ R[0].T + t[0] - Q) ** 2).sum(1)) <= d2
    for _ in range(rounds):
        if inl.sum() < 3:
            break
        R, t = horn_batch(P[inl][None], Q[inl][None])
        new = (((P @ R[0].T + t[0] - Q) ** 2).sum(1)) <= d2
        same = np.array_equal(new, inl)
        inl = new
        if same:
            break
    return inl.sum() >= min_pairs, R[0], t[0], inl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--source", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from stereo_visual_odometry_amd import api
    res = {"tool": "align_bench", "source_rows": a.source, "hypotheses": HYPOTHESES, "inlier_dist": INLIER_DIST, "repeats": a.repeats, "sizes": {}}
    pool = ThreadPoolExecutor(16)
    for size in (int(s) for s in a.sizes.split(",")):
        s = scene(size, a.source)
        ix = api.DescriptorIndex(size + a.source, points=True)
        ix.add_points(s["desc"], s["ids"], s["xyz"], s["tags"])
        ix.set_timing(True)
        src, dst = (size, size + a.source), (0, size)
        copy = s["desc"][size:].copy()                                    # the caller's private copy of the source descriptors
        got = {}

        def leg_align():
            got["align"] = ix.align(src, dst, INLIER_DIST, hypotheses=HYPOTHESES)
            return ix.stats()["last_kernels_ms"]

        def leg_rows():
            ix.match_rows(src, dst)
            return ix.stats()["last_kernels_ms"]

        def leg_host(threads):
            m = ix.match(copy, dst[0], dst[1])
            j, rows = host_pairs(m, s["ids"][size:], s["tags"], s["tags"][size:])
            P, Q = s["xyz"][size + j].astype(np.float64), s["xyz"][rows].astype(np.float64)
            picks = np.array([sample(h, len(j)) for h in range(HYPOTHESES)])
            got["host"] = (j, rows) + host_fit(P, Q, picks, pool, threads)
            return 0.0

        legs = {"align": leg_align, "match_rows": leg_rows, "host_1": lambda: leg_host(1), "host_16": lambda: leg_host(16)}
        walls, kern = {k: [] for k in legs}, {k: [] for k in legs}
        for rep in range(a.repeats + 1):                                  # alternating; the first round is the warm-up
            for k, f in legs.items():
                t0 = time.perf_counter()
                ms = f()
                if rep:
                    walls[k].append((time.perf_counter() - t0) * 1e3); kern[k].append(ms)
        r, pairs = got["align"]
        j, rows, ok, R, t, inl = got["host"]
        same = bool(np.array_equal(pairs["src"], size + j) and np.array_equal(pairs["dst"], rows) and np.array_equal(pairs["inlier"].astype(bool), inl)
                    and ok == r.success and np.abs(R - r.R).max() < 1e-9 and np.abs(t - r.t).max() < 1e-6)
        out = {k: {"wall_ms_median": float(np.median(v)), "wall_ms_min": float(min(v)), "wall_ms_max": float(max(v))} for k, v in walls.items()}
        for k in ("align", "match_rows"):
            out[k]["kernels_ms_median"] = float(np.median(kern[k]))
        out.update(n_pairs=int(r.n_pairs), n_inliers=int(r.n_inliers), success=bool(r.success), host_equals_device=same)
        res["sizes"][str(size)] = out
        ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
