#!/usr/bin/env python3
"""What maintaining a descriptor index on the device costs (include/svo.h, "Index maintenance"), and what the host round trip it
replaces costs:

    python tools/desc_retire_bench.py [--out FILE] [--sizes 65536,1048576] [--repeats 7]

One process, like tools/desc_match_bench.py's children.  Per index size, rows with points, tags r * 8 // size and ids in runs of 8
scattered over the index; every leg is run once as a warm-up and then --repeats times, the index re-filled (untimed) before each
run that changes it, and reported as the median wall time of the synchronous call beside the device time of its kernels (HIP events:
svo_desc_index_set_timing, svo_desc_index_get_retire_stats):

  window     retire(tags=(4, 7)): the tags drop the older half; kept_before is returned
  latest     retire(tags=(1, 7), drop_ids=every 16th id, latest_per_id=True): every flag; kept_before is returned
  transform  transform_points(T) over every row
  rebuild_window, rebuild_latest
             the same result without the feature: the caller holds a host copy of every row, filters it in numpy, calls truncate(0)
             and add_points.  The index after it answers a sample of queries exactly as after the device leg (checked, untimed).

Bytes moved: 56 B read per row of the scope plus 56 B written per kept row, 32 B per moved point row; divided by the kernel time and
by the wall time, beside the 8 TB/s HBM peak and the 4 TB/s a copy reaches that DESIGN.md quotes.  A figure, not a pass mark.  The
one comparison with a verdict: window and latest take less wall time than their rebuild at every size ("faster_than_rebuild").
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TBS, COPY_TBS = 8.0, 4.0


def rows_of(size, seed=7):
    rng = np.random.default_rng(seed)
    ids = ((rng.permutation(size) // 8).astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return dict(desc=rng.integers(0, 256, (size, 32), dtype=np.uint8), ids=ids, xyz=rng.uniform(-50, 50, (size, 3)).astype(np.float32),
                tags=(np.arange(size, dtype=np.int64) * 8 // size).astype(np.int32))


def host_keep(rows, window, drop=None, latest=False):
    """the caller's numpy filter on the parent commit: the rows a rebuild adds again"""
    alive = (rows["tags"] >= window[0]) & (rows["tags"] <= window[1])
    if drop is not None:
        alive &= ~np.isin(rows["ids"], drop)
    if latest:
        r = np.flatnonzero(alive)
        _, first_of_reversed = np.unique(rows["ids"][r][::-1], return_index=True)
        alive = np.zeros(len(alive), bool)
        alive[r[len(r) - 1 - first_of_reversed]] = True
    return alive


def fill(ix, rows, keep=None):
    ix.truncate(0)
    if keep is None:
        ix.add_points(rows["desc"], rows["ids"], rows["xyz"], rows["tags"])
    else:
        ix.add_points(rows["desc"][keep], rows["ids"][keep], rows["xyz"][keep], rows["tags"][keep])


def timed(call, before, repeats):
    """warm-up + repeats of call(), before() untimed in front of each -> (walls ms, what the last call returned)"""
    walls, out = [], None
    for k in range(repeats + 1):
        before()
        t0 = time.perf_counter()
        out = call()
        if k:
            walls.append((time.perf_counter() - t0) * 1e3)
    return walls, out


def rate(n_bytes, ms):
    return n_bytes / (ms * 1e-3) / 1e12 if ms > 0 else None


def one_size(api, size, repeats):
    rows = rows_of(size)
    drop = np.unique(rows["ids"])[::16]
    probe = np.concatenate([rows["desc"][:: max(size // 48, 1)][:48], np.random.default_rng(1).integers(0, 256, (16, 32), dtype=np.uint8)])
    ix = api.DescriptorIndex(size, points=True)
    ix.set_timing(True)
    legs = {}
    answers = {}

    def device_leg(name, **rule):
        kern = []

        def call():
            kb = ix.retire(**rule)
            kern.append(ix.retire_stats()["last_kernels_ms"])
            return kb
        walls, kb = timed(call, lambda: fill(ix, rows), repeats)
        kept = int(kb[-1])
        moved = 56 * size + 56 * kept
        k = float(np.median(kern[1:]))
        answers[name] = ix.match(probe).tobytes()
        legs[name] = dict(wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)), kernels_ms_median=k, rows_kept=kept, bytes_moved=moved,
                          tb_per_s_kernels=rate(moved, k), tb_per_s_wall=rate(moved, float(np.median(walls))))

    def rebuild_leg(name, of, **rule):
        def call():
            keep = host_keep(rows, **rule)
            fill(ix, rows, keep)
            return keep
        walls, keep = timed(call, lambda: fill(ix, rows), repeats)
        assert int(keep.sum()) == legs[of]["rows_kept"] and ix.match(probe).tobytes() == answers[of], "%s does not give %s's index" % (name, of)
        legs[name] = dict(wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)), rows_kept=int(keep.sum()))

    device_leg("window", tags=(4, 7))
    rebuild_leg("rebuild_window", "window", window=(4, 7))
    device_leg("latest", tags=(1, 7), drop_ids=drop, latest_per_id=True)
    rebuild_leg("rebuild_latest", "latest", window=(1, 7), drop=drop, latest=True)
    fill(ix, rows)
    th = 0.01
    T = np.array([[np.cos(th), -np.sin(th), 0, 0.05], [np.sin(th), np.cos(th), 0, -0.02], [0, 0, 1, 0.01], [0, 0, 0, 1]])
    kern = []

    def move():
        r = ix.transform_points(T)
        kern.append(ix.retire_stats()["last_kernels_ms"])
        return r
    walls, (moved, skipped) = timed(move, lambda: None, repeats)
    k = float(np.median(kern[1:]))
    legs["transform"] = dict(wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)), kernels_ms_median=k, rows_moved=moved, rows_skipped=skipped,
                             bytes_moved=32 * moved, tb_per_s_kernels=rate(32 * moved, k), tb_per_s_wall=rate(32 * moved, float(np.median(walls))))
    st = ix.retire_stats()
    ix.close()
    faster = {leg: legs[leg]["wall_ms_median"] < legs["rebuild_" + leg]["wall_ms_median"] for leg in ("window", "latest")}
    return dict(size=size, repeats=repeats, slab_rows=262144, legs=legs, faster_than_rebuild=faster,
                rebuild_over_device_wall={leg: legs["rebuild_" + leg]["wall_ms_median"] / legs[leg]["wall_ms_median"] for leg in ("window", "latest")},
                scratch_bytes=st["scratch_bytes"], scratch_allocations=st["scratch_allocations"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from stereo_visual_odometry_amd import api
    out = dict(shape="rows with points, tags r * 8 // size, ids in runs of 8 scattered over the index", hbm_peak_tb_per_s=HBM_PEAK_TBS, copy_tb_per_s=COPY_TBS,
               sizes=[one_size(api, int(s), args.repeats) for s in args.sizes.split(",")])
    out["acceptance"] = all(all(s["faster_than_rebuild"].values()) for s in out["sizes"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
