#!/usr/bin/env python3
"""What fusing the landmarks of two row spans of a descriptor index costs on the device (include/svo.h, "Landmark fusion"), and what
the host path it replaces costs:

    python tools/fuse_bench.py [--out FILE] [--sizes 65536,1048576] [--source 2048] [--repeats 7] [--host-repeats 2]

One process.  Per destination size: an index of `size` destination rows (random descriptors, ids in runs of 4, points uniform in a
cube of side SIDE) followed by `source` source rows, each a destination row's descriptor with up to 8 bits flipped, under an id of its
own, its point within RADIUS / 2 of that row's on every axis.  The gate's cube of side 2 RADIUS admits (2 RADIUS / SIDE)^3 = 1 / 1000
of the destination rows for a source row away from the walls; the share the scene really has is counted on the host and reported.  The
legs run alternately, each once as a warm-up and then --repeats times (the host legs --host-repeats times), and are reported as the
median, the smallest and the largest wall time of the synchronous call(s) in milliseconds:

  fuse         svo_desc_index_fuse over the whole index: nothing is uploaded; beside it the device span from its first kernel to its
               last (HIP events: svo_desc_index_set_timing).  Untimed, a relabel of the source span puts the old ids back before the
               next round, so every round fuses the same landmarks.
  match_near   svo_desc_index_match_near alone: the search's share of the call
  host_1, host_16
               the path the call replaces, on the caller's own copies of the descriptors, points and ids: the gate and the search in
               numpy (x first, then y and z on the survivors; popcounts of the admitted rows only) on 1 and on 16 threads over the
               source rows, rules 2 - 5 of "Map alignment", the map and the relabel in numpy, then a new index built from the copies
               with the new ids.  The host path's pairs and ids equal the device's (checked, untimed).
  relabel_4096, relabel_1048576
               svo_desc_index_relabel alone over the 1 048 576-row index with lists of that many entries (`from` values drawn with
               repeats from the ids in use); rounds alternate between the list and its inverse, so every round changes rows.  The wall
               time includes the lists' upload; the kernels' span is beside it.

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
from align_bench import host_pairs  # noqa: E402  (rules 2 - 5 in numpy: the alignment's tool has them)

RADIUS, SIDE = 0.5, 10.0
POP = np.array([bin(i).count("1") for i in range(256)], np.int64)
NONE, NO_DIST = -1, 257
DTYPE = np.dtype([("id", "<u8"), ("id2", "<u8"), ("row", "<i4"), ("row2", "<i4"), ("dist", "<u2"), ("dist2", "<u2"), ("reserved", "<u4")])


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
    xyz = rng.uniform(0, SIDE, (size + n_src, 3)).astype(np.float32)
    xyz[size:] = xyz[pick] + rng.uniform(-RADIUS / 2, RADIUS / 2, (n_src, 3)).astype(np.float32)
    return dict(desc=desc, ids=ids, xyz=xyz, tags=np.zeros(size + n_src, np.int32))


def host_match_near(s, size, rows, radius):
    """rules 1 - 2 for the source rows `rows` against the destination rows [0, size) -> (result rows, the admitted rows' count)"""
    desc, ids, xyz = s["desc"], s["ids"], s["xyz"]
    r = np.float32(radius)
    out = np.zeros(len(rows), DTYPE)
    out["row"] = out["row2"] = NONE
    out["dist"] = out["dist2"] = NO_DIST
    n_adm = 0
    for k, q in enumerate(rows):
        c = np.flatnonzero(np.abs(xyz[:size, 0] - xyz[q, 0]) <= r)
        c = c[(np.abs(xyz[c, 1] - xyz[q, 1]) <= r) & (np.abs(xyz[c, 2] - xyz[q, 2]) <= r)]
        n_adm += len(c)
        if not len(c):
            continue
        key = POP[desc[c] ^ desc[q]].sum(1) * (1 << 32) + c
        b = int(key.argmin())
        o = out[k]
        o["row"], o["dist"], o["id"] = c[b], key[b] >> 32, ids[c[b]]
        other = ids[c] != ids[c[b]]
        if other.any():
            key2 = np.where(other, key, np.iinfo(np.int64).max)
            b2 = int(key2.argmin())
            o["row2"], o["dist2"], o["id2"] = c[b2], key2[b2] >> 32, ids[c[b2]]
    return out, n_adm


def host_relabel(ids, frm, to):
    """rule 5 in numpy for distinct `from` values"""
    o = np.argsort(frm)
    f, t = frm[o], to[o]
    at = np.minimum(np.searchsorted(f, ids), len(f) - 1) if len(f) else np.zeros(len(ids), np.int64)
    hit = (f[at] == ids) if len(f) else np.zeros(len(ids), bool)
    new = ids.copy()
    new[hit] = t[at[hit]]
    return new


def stats(v):
    return {"wall_ms_median": float(np.median(v)), "wall_ms_min": float(min(v)), "wall_ms_max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--source", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=2)
    a = ap.parse_args()
    from stereo_visual_odometry_amd import api
    res = {"tool": "fuse_bench", "source_rows": a.source, "radius": RADIUS, "side": SIDE, "repeats": a.repeats, "host_repeats": a.host_repeats, "sizes": {}}
    pool = ThreadPoolExecutor(16)
    for size in (int(s) for s in a.sizes.split(",")):
        s = scene(size, a.source)
        m_all = size + a.source
        ix = api.DescriptorIndex(m_all, points=True)
        ix.add_points(s["desc"], s["ids"], s["xyz"], s["tags"])
        ix.set_timing(True)
        src, dst = (size, m_all), (0, size)
        got, admitted = {}, [0]

        def leg_fuse():
            got["fuse"] = ix.fuse(src, dst, RADIUS)
            return ix.stats()["last_kernels_ms"]

        def leg_near():
            ix.match_near(src, dst, RADIUS)
            return ix.stats()["last_kernels_ms"]

        def leg_host(threads):
            cuts = np.linspace(size, m_all, 4 * threads + 1).astype(int)
            parts = [np.arange(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
            work = lambda rows: host_match_near(s, size, rows, RADIUS)    # noqa: E731
            done = list(pool.map(work, parts)) if threads > 1 else [work(p) for p in parts]
            m, admitted[0] = np.concatenate([d[0] for d in done]), sum(d[1] for d in done)
            j, rows = host_pairs(m, s["ids"][size:], s["tags"], s["tags"][size:])
            frm, to = s["ids"][size + j], s["ids"][rows]
            keep = frm != to
            new = host_relabel(s["ids"], frm[keep], to[keep])
            fresh = api.DescriptorIndex(m_all, points=True)
            fresh.add_points(s["desc"], new, s["xyz"], s["tags"])
            fresh.close()
            got["host"] = (size + j, rows, new)
            return 0.0

        def undo():                                                       # untimed: the source span back under its own ids
            r, pairs = got["fuse"]
            ix.relabel(s["ids"][pairs["dst"]], s["ids"][pairs["src"]], rows=src)

        legs = {"fuse": (leg_fuse, a.repeats), "match_near": (leg_near, a.repeats), "host_1": (lambda: leg_host(1), a.host_repeats),
                "host_16": (lambda: leg_host(16), a.host_repeats)}
        walls, kern = {k: [] for k in legs}, {k: [] for k in legs}
        for rep in range(max(a.repeats, a.host_repeats) + 1):             # alternating; the first round is the warm-up
            for k, (f, reps) in legs.items():
                if rep > reps:
                    continue
                t0 = time.perf_counter()
                ms = f()
                if rep:
                    walls[k].append((time.perf_counter() - t0) * 1e3); kern[k].append(ms)
                if k == "fuse":
                    undo()
        r, pairs = got["fuse"]
        hs, hd, new = got["host"]
        out = {k: stats(v) for k, v in walls.items()}
        for k in ("fuse", "match_near"):
            out[k]["kernels_ms_median"] = float(np.median(kern[k]))
        ix.fuse(src, dst, RADIUS)                                         # once more, and the ids as a search of each source row alone reads them
        now = np.array([ix.match(s["desc"][q:q + 1], q, q + 1)[0]["id"] for q in range(size, m_all)], np.uint64)
        same = bool(np.array_equal(pairs["src"], hs) and np.array_equal(pairs["dst"], hd) and np.array_equal(now, new[size:]))
        out.update(n_pairs=int(r.n_pairs), n_fused=int(r.n_fused), n_rows_relabelled=int(r.n_rows_relabelled), host_equals_device=same,
                   admitted_share_of_destination=admitted[0] / (a.source * float(size)))
        if size == 1 << 20:
            rng = np.random.default_rng(9)
            for n in (4096, 1 << 20):
                frm = rng.integers(0, size // 4, n).astype(np.uint64)
                to = frm + np.uint64(1 << 40)
                w, kms, changed = [], [], []
                for rep in range(a.repeats + 1):
                    f, t = (frm, to) if rep % 2 == 0 else (to, frm)
                    t0 = time.perf_counter()
                    c = ix.relabel(f, t, rows=dst)
                    if rep:
                        w.append((time.perf_counter() - t0) * 1e3); kms.append(ix.stats()["last_kernels_ms"]); changed.append(c)
                if a.repeats % 2 == 0:                                    # leave the ids as they were
                    ix.relabel(to, frm, rows=dst)
                out["relabel_%d" % n] = dict(stats(w), kernels_ms_median=float(np.median(kms)), rows_changed=int(np.median(changed)))
        res["sizes"][str(size)] = out
        ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
