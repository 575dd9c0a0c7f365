#!/usr/bin/env python3
"""What a descriptor-index search costs (include/svo.h, "Descriptor index"), and what the host loop it replaces costs:

    python tools/desc_match_bench.py [--out FILE] [--sizes 65536,1048576] [--queries 2048] [--calls 20] [--chunk-rows 0]

Per index size, n queries on random descriptors with ids in runs of 4: the wall time of the synchronous svo_desc_index_match call
(upload of the queries and download of the rows included) and the device time of its two kernels (HIP events:
svo_desc_index_set_timing, svo_desc_index_get_stats), as medians of --calls calls after 5 warm-up calls; pairs per second from the
kernel time; and
tools/desc_match_host.cpp — INTEGRATION.md's former popcountll loop with the index's best / second-by-id rule, -O3 -march=native,
16 threads — on the same shape on this machine, after that program has reproduced tests/desc_match_ref.py on a small case, as the
GPU rows of a 65 x 1025 case have.  Every step runs under its own time limit: the host program and one child python per index size
(--child), one after the other, so one process has the GPU open at a time; the first failure ends the run.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HOST_THREADS = 16


def random_rows(seed, n, m):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (m, 32), dtype=np.uint8), (7 + np.arange(m) // 4).astype(np.uint64))


def child(size, n, calls, chunk_rows):
    """one index size on the GPU -> a JSON line"""
    import desc_match_ref as mref
    from stereo_visual_odometry_amd import api
    q, d, ids = random_rows(size, n, size)
    ix = api.DescriptorIndex(size)
    if chunk_rows:
        ix.chunk_rows = chunk_rows
    t0 = time.perf_counter()
    ix.add(d, ids)
    add_ms = (time.perf_counter() - t0) * 1e3
    got = ix.match(q[:65], 0, 1025 if size >= 1025 else size)         # the rows are right before they are timed
    assert got.tobytes() == mref.match(q[:65], d, ids, 0, 1025 if size >= 1025 else size).tobytes(), "the GPU rows differ from the reference"
    ix.set_timing(True)
    for _ in range(5):
        ix.match(q)
    wall, kern = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = ix.match(q)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(ix.stats()["last_kernels_ms"])
    k = float(np.median(kern))
    r = dict(size=size, queries=n, calls=calls, chunk_rows=ix.chunk_rows, add_ms=add_ms, wall_ms_median=float(np.median(wall)), wall_ms_min=float(min(wall)),
             kernels_ms_median=k, kernels_ms_min=float(min(kern)), pairs_per_s=n * size / (k * 1e-3), checksum=int(out["row"].sum() + out["dist"].sum()))
    ix.close()
    print(json.dumps(r))


def step(cmd, limit, what):
    """one step under its own time limit -> its last output line; anything else ends the run"""
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("%s failed (exit status %s):\n%s\n%s" % (what, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    lines = r.stdout.strip().splitlines()
    return lines[-1] if lines else ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--chunk-rows", type=int, default=0, help="svo_desc_index_set_chunk_rows (0: the default)")
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.queries, args.calls, args.chunk_rows)
    sizes = [int(s) for s in args.sizes.split(",")]
    out = dict(shape="%d queries, random descriptors, ids in runs of 4" % args.queries, gpu=[], host=[])
    if not args.no_host:
        import desc_match_ref as mref
        exe = os.path.join(ROOT, "tools", "desc_match_host")
        step(["g++", "-O3", "-march=native", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "desc_match_host.cpp"), "-o", exe], 120, "building the host baseline")
        from test_desc_match_ref import shared_case
        q, d, ids = shared_case()
        with tempfile.TemporaryDirectory() as tmp:
            case = os.path.join(tmp, "case.bin")
            with open(case, "wb") as f:
                f.write(np.array([len(q), len(d)], np.int32).tobytes())
                f.write(q.tobytes()); f.write(d.tobytes()); f.write(ids.astype("<u8").tobytes()); f.write(mref.match(q, d, ids).tobytes())
            out["host_check"] = step([exe, "check", case], 60, "the host baseline's check against the reference")
        for s in sizes:
            reps = args.calls if s <= (1 << 17) else 5
            out["host"].append(json.loads(step([exe, "bench", str(args.queries), str(s), str(HOST_THREADS), str(reps)], 600, "the host baseline at %d rows" % s)))
    for s in sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(s), "--queries", str(args.queries), "--calls", str(args.calls), "--chunk-rows", str(args.chunk_rows)]
        out["gpu"].append(json.loads(step(cmd, 300, "the GPU search at %d rows" % s)))
    if out["host"]:
        out["host_over_gpu_wall"] = {str(g["size"]): h["median_ms"] / g["wall_ms_median"] for g, h in zip(out["gpu"], out["host"])}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
