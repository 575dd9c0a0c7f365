#!/usr/bin/env python3
"""Cost of detection masks at the bench shape (bench.py's workload: KITTI-00-shaped 1241x376, LK 21x21, maxLevel 3, two contexts x
256 sequences, frames resident in HBM, 4 frames in flight per context): the legs `off` (the library as it is without the setter:
nothing is called), `shared` (one static mask for every sequence, set once) and `per_seq` (a mask of its own for every sequence, set
once) on the same scene, alternating in one process, two rounds.  The masks close the lower quarter of the image (a bonnet) and two
boxes.  Prints one JSON line (and writes it to --out): per leg frame-pairs/s and svo_get_stage_timing's detect stage, the masked
legs as multiples of the `off` leg round by round.  The off leg alone (--legs off --package DIR) runs against a copy of a package
that predates the setter, for an A/B of the untouched path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seqs", type=int, default=512)
    ap.add_argument("--contexts", type=int, default=2)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--legs", default="off,shared,per_seq")
    ap.add_argument("--package", default=None, help="directory holding the stereo_visual_odometry_amd package to import (default: this checkout)")
    ap.add_argument("--repeat", type=int, default=2, help="rounds of the legs, alternating them in every round")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    if args.package:
        sys.path.insert(0, os.path.abspath(args.package))
    import torch
    import bench
    from stereo_visual_odometry_amd import api, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("detect_mask_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    cal = syn.KITTI00
    W, H, F, B, C = cal["width"], cal["height"], args.frames, args.seqs, args.contexts
    Bc = B // C
    pool = bench.render_pool([dict(cal=cal, n_frames=F, seed=0x5EED0002 + g, movers=0.3, step=0.5, cell_px=16.6) for g in range(args.pool)],
                             max(1, min(16, bench.host_cores())))
    legs = args.legs.split(",")
    left = torch.stack([torch.from_numpy(np.stack(s.left)) for s in pool]).to(dev).contiguous()
    right = torch.stack([torch.from_numpy(np.stack(s.right)) for s in pool]).to(dev).contiguous()
    torch.cuda.synchronize()
    img = W * H

    def ping_pong(i):
        p = i % (2 * F - 2)
        return p if p < F else 2 * F - 2 - p

    def ptrs(step, c):
        lp, rp = [], []
        for b in range(c * Bc, (c + 1) * Bc):
            g = b % args.pool
            f = ping_pong(step + (b // args.pool) * 3)
            lp.append(left.data_ptr() + (g * F + f) * img)
            rp.append(right.data_ptr() + (g * F + f) * img)
        return lp, rp

    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0, max_level=3, ransac_iterations=100)
    os.environ.setdefault("SVO_GRAPH", "0")

    def mask_of(i):
        m = np.full((H, W), 255, np.uint8)
        m[H - H // 4:, :] = 0
        rng = np.random.default_rng(77 + i)
        for _ in range(2):
            x, y = int(rng.integers(0, W - 200)), int(rng.integers(0, H - 120))
            m[y:y + 100, x:x + 180] = 0
        return m

    def run_leg(leg):
        vos = []
        for c in range(C):
            v = api.BatchVisualOdometry(W, H, Bc, api.default_config(**over))
            v.initalize_projection_matricies(Pl, Pr)
            v.set_stage_timing(True)
            if leg == "shared":                                       # the off leg is the library as it is without the setter
                v.set_detection_mask(mask_of(0))
            elif leg == "per_seq":
                for i in range(Bc):
                    v.set_detection_mask(mask_of(c * Bc + i), i)
            vos.append(v)
        det_ms, inl, n_masked = [], [], 0

        def run(first, count, record):
            nonlocal n_masked
            sub = col = 0
            while col < count:
                while sub < count and sub - col < args.depth:
                    for c, vo in enumerate(vos):
                        lp, rp = ptrs(first + sub, c)
                        vo.submit_device(lp, rp, W)
                        if record and leg != "off":
                            n_masked += bool(vo.last_frame_path() & 256)   # SVO_PATH_DETECT_MASKED
                    sub += 1
                for vo in vos:
                    vo.collect()
                    if record:
                        det_ms.append(vo.stage_timing()["detect"])
                        inl.append(sum(s.n_inliers for s in vo.stats))
                col += 1
        run(0, args.warmup + 1, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.warmup + 1, args.steps, True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for v in vos:
            v.close()
        return dict(frame_pairs_per_s=B * args.steps / dt, detect_ms=float(np.mean(det_ms)), inliers=int(np.sum(inl)), masked=n_masked)

    res = {k: [] for k in legs}
    for _ in range(args.repeat):
        for k in legs:
            res[k].append(run_leg(k))
    out = dict(shape="1241x376, w21, L3, %d contexts x %d sequences, depth %d, %d steps" % (C, Bc, args.depth, args.steps),
               legs={k: dict(frame_pairs_per_s=[r["frame_pairs_per_s"] for r in v], detect_ms=[r["detect_ms"] for r in v],
                             inliers=[r["inliers"] for r in v], masked_frames=[r["masked"] for r in v]) for k, v in res.items()})
    if "off" in res:
        out["ratio_to_off_per_round"] = {k: [r["frame_pairs_per_s"] / m["frame_pairs_per_s"] for r, m in zip(res[k], res["off"])]
                                         for k in res if k != "off"}
        out["off_round_to_round_spread"] = (max(r["frame_pairs_per_s"] for r in res["off"]) / min(r["frame_pairs_per_s"] for r in res["off"])) - 1
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
