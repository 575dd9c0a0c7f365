#!/usr/bin/env python3
"""Throughput of rectifying contexts at the bench shape (bench.py's workload: KITTI-00-shaped 1241x376, LK 21x21, maxLevel 3,
two contexts x 256 sequences, frames resident in HBM, 4 frames in flight per context).  Three cases on the same frames:
  (a) plain contexts (bench.py's own path), (b) one shared map pair per context, (c) a private map pair per sequence.
The raw frames are bench.py's rendered frames (same size as the rectified ones); the maps come from a mildly distorted
calibration (per-sequence variants in (c)).  Prints one JSON line: frame-pairs/s and svo_get_stage_timing ms[0]
(ingest + pyramids) per case, and the ratios of (b) and (c) to (a)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def calib(K, variant):
    v = variant
    c, s = np.cos(1e-3 * (v % 7)), np.sin(1e-3 * (v % 7))
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    P = np.array([[K[0][0], 0, K[0][2] + 0.25 * (v % 5), 0], [0, K[1][1], K[1][2], 0], [0, 0, 1, 0]])
    return dict(width=1241, height=376, K=K, D=[-0.02 - 1e-4 * (v % 11), 0.004, 1e-4, -1e-4, 0.0], R=R, P=P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seqs", type=int, default=512)
    ap.add_argument("--contexts", type=int, default=2)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of the cases, alternating (a), (b), (c) in every round")
    args = ap.parse_args()

    import torch
    import bench
    from stereo_visual_odometry_amd import api, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("rectify_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    cal = syn.KITTI00
    W, H, F, B, C = cal["width"], cal["height"], args.frames, args.seqs, args.contexts
    Bc = B // C
    pool = bench.render_pool([dict(cal=cal, n_frames=F, seed=0x5EED0002 + g, movers=0.3, step=0.5, cell_px=16.6) for g in range(args.pool)],
                             max(1, min(16, bench.host_cores())))
    left = torch.stack([torch.from_numpy(np.stack(s.left)) for s in pool]).to(dev)
    right = torch.stack([torch.from_numpy(np.stack(s.right)) for s in pool]).to(dev)

    def ping_pong(i):
        p = i % (2 * F - 2)
        return p if p < F else 2 * F - 2 - p

    def ptrs(step, c):
        lp, rp = [], []
        for b in range(c * Bc, (c + 1) * Bc):
            g = b % args.pool
            f = ping_pong(step + (b // args.pool) * 3)
            lp.append(left.data_ptr() + (g * F + f) * W * H)
            rp.append(right.data_ptr() + (g * F + f) * W * H)
        return lp, rp

    K = [[cal["fx"], 0, cal["cx"]], [0, cal["fy"], cal["cy"]], [0, 0, 1]]
    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0, max_level=3, ransac_iterations=100)
    os.environ.setdefault("SVO_GRAPH", "0")
    private = None
    if "c" in args.cases:
        t = time.perf_counter()
        private = []
        for b in range(B):
            ci = calib(K, b)
            cr = dict(ci, D=list(ci["D"][:4]) + [0.001])
            private.append((api.init_rectify_map(ci["K"], ci["D"], ci["R"], ci["P"], W, H), api.init_rectify_map(cr["K"], cr["D"], cr["R"], cr["P"], W, H)))
        print("maps for (c): %.1f s on the host" % (time.perf_counter() - t), file=sys.stderr)

    def run_case(case):
        vos = []
        for c in range(C):
            v = api.BatchVisualOdometry(W, H, Bc, api.default_config(**over))
            v.initalize_projection_matricies(Pl, Pr)
            v.set_stage_timing(True)
            if case == "b":
                ci = calib(K, 0)
                v.set_rectification(ci, dict(ci, D=list(ci["D"][:4]) + [0.001]))
            elif case == "c":
                for i in range(Bc):
                    (a1, a2), (b1, b2) = private[c * Bc + i]
                    v.set_rectification_maps(a1, a2, b1, b2, seq=i, raw_size=(W, H))
            vos.append(v)
        ms0 = []

        def run(first, count, record):
            sub = col = 0
            while col < count:
                while sub < count and sub - col < args.depth:
                    for c, vo in enumerate(vos):
                        lp, rp = ptrs(first + sub, c)
                        vo.submit_device(lp, rp, W)
                    sub += 1
                for vo in vos:
                    vo.collect()
                    if record:
                        ms0.append(vo.stage_timing()["ingest+pyramid"])
                col += 1
        run(0, args.warmup + 1, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.warmup + 1, args.steps, True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for v in vos:
            v.close()
        return dict(frame_pairs_per_s=B * args.steps / dt, ingest_pyramid_ms=float(np.mean(ms0)))

    cases = args.cases.split(",")
    res = {k: [] for k in cases}
    for _ in range(args.repeat):
        for k in cases:
            res[k].append(run_case(k))
    out = dict(shape="1241x376, w21, L3, %d contexts x %d sequences, depth %d, %d steps" % (C, Bc, args.depth, args.steps),
               cases={k: dict(frame_pairs_per_s=[r["frame_pairs_per_s"] for r in v], ingest_pyramid_ms=[r["ingest_pyramid_ms"] for r in v])
                      for k, v in res.items()})
    best = {k: max(r["frame_pairs_per_s"] for r in v) for k, v in res.items()}
    if "a" in best:
        out["ratio_to_a"] = {k: best[k] / best["a"] for k in best if k != "a"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
