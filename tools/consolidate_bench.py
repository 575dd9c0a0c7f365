#!/usr/bin/env python3
"""What consolidating a descriptor index on the device costs (include/svo.h, "Landmark consolidation"), beside its floor and beside
the host path it replaces:

    python tools/consolidate_bench.py [--out FILE] [--sizes 65536,1048576] [--repeats 7]

One process.  Per index size, rows with points, 8 views per landmark scattered over the index (tools/desc_retire_bench.py's rows),
the views of a landmark within 0.05 of its centre and every seventh 0.5 off; every leg is run once as a warm-up and then --repeats
times, the index re-filled (untimed) before each run, and reported as the median wall time of the synchronous call beside the
device time of its kernels (HIP events: svo_desc_index_set_timing, svo_desc_index_get_retire_stats):

  consolidate  consolidate(radius=0.2) over the whole index; kept_before is returned
  latest       retire(latest_per_id=True) on the same index: the floor, since consolidation does that work — the table, the ranks, the
               compaction — plus the member list and the group kernel.  How far above it consolidation lands is reported, not asserted.
  host         the path the call replaces: read_rows, tests/consolidate_ref.py's numpy reference, truncate(0) and add_points (one
               run without a warm-up above 100 000 rows: it takes seconds).  The index after it equals the device leg's (checked).

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
VIEWS, RADIUS = 8, 0.2


def rows_of(size, seed=7):
    rng = np.random.default_rng(seed)
    which = rng.permutation(size) // VIEWS
    ids = (which.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    n_ids = size // VIEWS + 1
    base = rng.integers(0, 256, (n_ids, 32), dtype=np.uint8)
    noise = np.full((size, 32), 0xFF, np.uint8)
    for _ in range(4):                                # a bit survives four ANDs with probability 1 / 16: about 16 bits flipped a view
        noise &= rng.integers(0, 256, (size, 32), dtype=np.uint8)
    centre = rng.uniform(-50, 50, (n_ids, 3))
    xyz = centre[which] + rng.uniform(-0.05, 0.05, (size, 3)) + (np.arange(size) % 7 == 3)[:, None] * 0.5
    return dict(desc=base[which] ^ noise, ids=ids, xyz=xyz.astype(np.float32), tags=(np.arange(size, dtype=np.int64) * 8 // size).astype(np.int32))


def fill(ix, rows):
    ix.truncate(0)
    ix.add_points(rows["desc"], rows["ids"], rows["xyz"], rows["tags"])


def timed(call, before, repeats, warm=True):
    walls, out = [], None
    for k in range(repeats + (1 if warm else 0)):
        before()
        t0 = time.perf_counter()
        out = call()
        if k or not warm:
            walls.append((time.perf_counter() - t0) * 1e3)
    return walls, out


def one_size(api, size, repeats):
    import consolidate_ref as cr
    rows = rows_of(size)
    ix = api.DescriptorIndex(size, points=True)
    ix.set_timing(True)
    legs = {}

    def device_leg(name, call):
        kern = []

        def run():
            out = call()
            kern.append(ix.retire_stats()["last_kernels_ms"])
            return out
        walls, out = timed(run, lambda: fill(ix, rows), repeats)
        legs[name] = dict(wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)), kernels_ms_median=float(np.median(kern[1:])), rows_kept=ix.size)
        return out

    device_leg("latest", lambda: ix.retire(latest_per_id=True))
    res, _ = device_leg("consolidate", lambda: ix.consolidate(RADIUS))
    after = ix.read_rows()

    def host():
        d, i, x, t = ix.read_rows()
        out = cr.consolidate(d, i, x, t, RADIUS)
        ix.truncate(0)
        ix.add_points(out["desc"], out["ids"], out["xyz"], out["tags"])
        return out
    few = size > 100000
    walls, out = timed(host, lambda: fill(ix, rows), 1 if few else min(repeats, 3), warm=not few)
    assert tuple(out["result"]) == tuple(res) and not cr.same_rows(ix.read_rows(), after), "the host path does not give the device's index"
    legs["host"] = dict(wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)), runs=len(walls), rows_kept=ix.size)
    st = ix.retire_stats()
    ix.close()
    c, l = legs["consolidate"], legs["latest"]
    return dict(size=size, repeats=repeats, views=VIEWS, radius=RADIUS, slab_rows=262144, result=res._asdict(), legs=legs,
                consolidate_over_latest=dict(wall=c["wall_ms_median"] / l["wall_ms_median"], kernels=c["kernels_ms_median"] / l["kernels_ms_median"]),
                host_over_consolidate_wall=legs["host"]["wall_ms_median"] / c["wall_ms_median"],
                scratch_bytes=st["scratch_bytes"], scratch_allocations=st["scratch_allocations"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from stereo_visual_odometry_amd import api
    out = dict(shape="rows with points, 8 views per landmark scattered over the index, every seventh row's point 0.5 off",
               sizes=[one_size(api, int(s), args.repeats) for s in args.sizes.split(",")])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
