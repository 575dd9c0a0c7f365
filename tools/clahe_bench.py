#!/usr/bin/env python3
"""Throughput of CLAHE contexts at the bench shape (bench.py's workload: KITTI-00-shaped 1241x376, LK 21x21, maxLevel 3, two
contexts x 256 sequences, frames resident in HBM, 4 frames in flight per context).  Legs: off (bench.py's own path, no setter
called), on (set_clahe(2.0, (8, 8)) on mono8 frames) and on_bgr8 (the same with bgr8 frames, converted inside the CLAHE launches).
A discarded warm-up leg (off) runs first: the first leg a process runs is measured 2 - 3 % faster than the same leg later.  The
equalised frames hold other features than the plain ones, so the on legs' later stages do not do the off leg's work: the ratio
is the cost of the feature to a user, not of the two launches alone (svo_get_stage_timing ms[0] is the front's).  Prints one JSON
line (and writes it to --out): per leg frame-pairs/s per round, ms[0], inliers; the on legs as multiples of the same run's off leg,
round by round and best against best; the off leg's run-to-run spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = dict(off=("mono8", False), on=("mono8", True), on_bgr8=("bgr8", True))       # leg -> (frame format, CLAHE)
BPP = dict(mono8=1, bgr8=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seqs", type=int, default=512)
    ap.add_argument("--contexts", type=int, default=2)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--legs", default="off,on,on_bgr8")
    ap.add_argument("--repeat", type=int, default=3, help="rounds of the legs, alternating them in every round")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import bench
    from stereo_visual_odometry_amd import api, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("clahe_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    cal = syn.KITTI00
    W, H, F, B, C = cal["width"], cal["height"], args.frames, args.seqs, args.contexts
    Bc = B // C
    pool = bench.render_pool([dict(cal=cal, n_frames=F, seed=0x5EED0002 + g, movers=0.3, step=0.5, cell_px=16.6) for g in range(args.pool)],
                             max(1, min(16, bench.host_cores())))
    legs = args.legs.split(",")
    gen = torch.Generator(device="cpu"); gen.manual_seed(1)

    def frames_of(side, fmt):
        """[pool][F] frames of one camera in `fmt`, on the device: (pool, F, H, W * bpp) uint8."""
        a = torch.stack([torch.from_numpy(np.stack(getattr(s, side))) for s in pool]).to(dev)             # the rendered scene
        bgr = torch.stack([a, a.roll(1, dims=-2), 255 - a], -1)
        c = bgr.to(torch.int32)
        grey = ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).to(torch.uint8)
        noise = torch.randint(0, 256, a.shape, generator=gen, dtype=torch.uint8).to(dev)
        if fmt == "mono8":
            out = grey
        elif fmt == "bgr8":
            out = bgr
        else:
            raise SystemExit("unknown leg %s" % fmt)
        return out.contiguous()

    def ping_pong(i):
        p = i % (2 * F - 2)
        return p if p < F else 2 * F - 2 - p

    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0, max_level=3, ransac_iterations=100)
    os.environ.setdefault("SVO_GRAPH", "0")

    def run_leg(leg):
        fmt, clahe = LEGS[leg]
        left, right = frames_of("left", fmt), frames_of("right", fmt)
        torch.cuda.synchronize()
        img = W * H * BPP[fmt]

        def ptrs(step, c):
            lp, rp = [], []
            for b in range(c * Bc, (c + 1) * Bc):
                g = b % args.pool
                f = ping_pong(step + (b // args.pool) * 3)
                lp.append(left.data_ptr() + (g * F + f) * img)
                rp.append(right.data_ptr() + (g * F + f) * img)
            return lp, rp

        vos = []
        for c in range(C):
            v = api.BatchVisualOdometry(W, H, Bc, api.default_config(**over))
            v.initalize_projection_matricies(Pl, Pr)
            v.set_stage_timing(True)
            if fmt != "mono8":
                v.set_input_format(fmt)
            if clahe:                                                 # the off leg is the library as it is without the setter
                v.set_clahe(2.0, (8, 8))
            vos.append(v)
        ms0, inl = [], []

        def run(first, count, record):
            sub = col = 0
            while col < count:
                while sub < count and sub - col < args.depth:
                    for c, vo in enumerate(vos):
                        lp, rp = ptrs(first + sub, c)
                        vo.submit_device(lp, rp, W * BPP[fmt])
                    sub += 1
                for vo in vos:
                    vo.collect()
                    if record:
                        ms0.append(vo.stage_timing()["ingest+pyramid"])
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
        del left, right
        return dict(frame_pairs_per_s=B * args.steps / dt, ingest_pyramid_ms=float(np.mean(ms0)), inliers=int(np.sum(inl)))

    run_leg("off")                                                    # discarded: a process's first leg measures fast
    res = {k: [] for k in legs}
    for _ in range(args.repeat):
        for k in legs:
            res[k].append(run_leg(k))
    out = dict(shape="1241x376, w21, L3, %d contexts x %d sequences, depth %d, %d steps, clip 2.0, tiles 8x8" % (C, Bc, args.depth, args.steps),
               legs={k: dict(frame_pairs_per_s=[r["frame_pairs_per_s"] for r in v], ingest_pyramid_ms=[r["ingest_pyramid_ms"] for r in v],
                             inliers=[r["inliers"] for r in v]) for k, v in res.items()})
    best = {k: max(r["frame_pairs_per_s"] for r in v) for k, v in res.items()}
    if "off" in best:
        rates = [r["frame_pairs_per_s"] for r in res["off"]]
        out["off_spread"] = (max(rates) - min(rates)) / max(rates)
        out["ratio_to_off"] = {k: best[k] / best["off"] for k in best if k != "off"}
        out["ratio_to_off_per_round"] = {k: [r["frame_pairs_per_s"] / m["frame_pairs_per_s"] for r, m in zip(res[k], res["off"])] for k in best if k != "off"}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
