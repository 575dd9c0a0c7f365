#!/usr/bin/env python3
"""Ragged and continuous batching, measured: one context at the bench shape (1241x376, LK 21x21, maxLevel 3, 100 RANSAC
iterations) holding 256 sequences whose lengths are the KITTI 00-07 frame counts / 10, repeated 32 times.

  (a) refed      finished sequences are fed their last frame again until the longest one ends (the only option before
                 svo_submit_batch_masked); their outputs are thrown away
  (b) masked     finished sequences are idle (svo_submit_batch_masked): the grids cover the active sequences only
  (c) continuous a queue of 1024 sequences of random lengths (fixed seed) served through the 256 slots: a slot whose sequence
                 ends is reset with new projection matrices (svo_reset_sequence, stream-ordered, no sync) and takes the next
                 one; its useful rate is reported next to the all-active rate of the same context

Frames are rendered once (a pool of synthetic KITTI-00-shaped sequences, as bench.py) and replayed from device memory, so the
tool times the GPU, not the renderer.  Prints one JSON line.

  python tools/ragged_batch.py [--depth 4] [--queue 1024] [--seed 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KITTI_00_07 = (4541, 1101, 4661, 801, 271, 2761, 1101, 1101)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--depth", type=int, default=4, help="frames in flight (<= 8)")
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10, help="frames rendered per pool sequence (ping-pong replay)")
    ap.add_argument("--queue", type=int, default=1024, help="sequences served in continuous mode")
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=200)
    ap.add_argument("--all-active-steps", type=int, default=40)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    from bench import host_cores, render_pool
    from stereo_visual_odometry_amd import api, synthetic as syn

    dev = torch.device("cuda", 0)
    cal = syn.KITTI00
    W, H = cal["width"], cal["height"]
    B, F = args.seqs, args.frames
    pool = render_pool([dict(cal=cal, n_frames=F, seed=0x5EED0002 + g, step=0.5, cell_px=16.6, movers=0.3) for g in range(args.pool)],
                       max(1, host_cores()))
    left = torch.stack([torch.from_numpy(np.stack(s.left)) for s in pool]).to(dev)      # (G, F, H, W) u8, resident in HBM
    right = torch.stack([torch.from_numpy(np.stack(s.right)) for s in pool]).to(dev)
    lbase, rbase, fb = left.data_ptr(), right.data_ptr(), W * H

    def frame(uid, k):
        """frame k of sequence uid: a pool sequence replayed ping-pong from a phase of its own"""
        p = (k + 3 * (uid // args.pool)) % (2 * F - 2)
        f = p if p < F else 2 * F - 2 - p
        g = uid % args.pool
        return lbase + (g * F + f) * fb, rbase + (g * F + f) * fb

    os.environ.setdefault("SVO_GRAPH", "0")
    over = dict(win_w=21, win_h=21, max_level=3, ransac_iterations=100, max_translation_norm=2.0)
    Pl, Pr = syn.projection_matrices(cal)
    vo = api.BatchVisualOdometry(W, H, B, api.default_config(**over))
    vo.initalize_projection_matricies(Pl, Pr)

    def drive(n_steps, step_fn):
        """submit n_steps frames (step_fn(k) -> (lp, rp, active)) with `depth` in flight; wall seconds"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sub = col = 0
        while col < n_steps:
            while sub < n_steps and sub - col < args.depth:
                lp, rp, act = step_fn(sub)
                vo.submit_device(lp, rp, W, active=act)
                sub += 1
            vo.collect()
            col += 1
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def all_active(k):
        lp, rp = zip(*[frame(i, k) for i in range(B)])
        return list(lp), list(rp), None

    drive(6, all_active)                                              # warm-up: kernels loaded, LK grid hint settled
    vo.reset_sequence(-1)
    t_all = drive(args.all_active_steps, all_active)
    all_fps = B * args.all_active_steps / t_all

    lengths = [KITTI_00_07[i % 8] // 10 for i in range(B)]
    T = max(lengths)
    useful = sum(lengths)

    def refed(k):                                                     # a finished sequence repeats its last frame
        lp, rp = zip(*[frame(i, min(k, lengths[i] - 1)) for i in range(B)])
        return list(lp), list(rp), None

    def masked(k):
        act = np.array([k < n for n in lengths], np.uint8)
        lp, rp = [], []
        for i in range(B):
            a, b = frame(i, k) if act[i] else (None, None)
            lp.append(a); rp.append(b)
        return lp, rp, act

    vo.reset_sequence(-1)
    t_refed = drive(T, refed)
    vo.reset_sequence(-1)
    t_masked = drive(T, masked)

    # (c) continuous: slots take sequences from a queue as they free up
    rng = np.random.default_rng(args.seed)
    qlen = rng.integers(args.min_len, args.max_len + 1, size=args.queue).tolist()
    scale = rng.uniform(0.98, 1.02, size=args.queue)
    vo.reset_sequence(-1)
    slot_uid = [-1] * B; slot_k = [0] * B
    nxt = 0
    resets = 0
    plan = []                                                          # planned on the host as the frames are submitted

    def cont(k):
        nonlocal nxt, resets
        act = np.zeros(B, np.uint8)
        lp, rp = [None] * B, [None] * B
        for i in range(B):
            if slot_uid[i] >= 0 and slot_k[i] >= qlen[slot_uid[i]]:
                slot_uid[i] = -1
            if slot_uid[i] < 0 and nxt < args.queue:
                u = nxt; nxt += 1
                if k > 0:                                              # a new sequence in a used slot: start over, its own camera
                    P1 = Pl.copy(); P2 = Pr.copy()
                    P1[0, 0] *= scale[u]; P2[0, 0] *= scale[u]; P2[0, 3] *= scale[u]
                    vo.reset_sequence(i, P1, P2)
                    resets += 1
                slot_uid[i], slot_k[i] = u, 0
            if slot_uid[i] >= 0:
                act[i] = 1
                lp[i], rp[i] = frame(slot_uid[i], slot_k[i])
                slot_k[i] += 1
        plan.append(int(act.sum()))
        return lp, rp, act

    # the number of steps is known once the queue is drained: simulate the schedule first (host only)
    sim_uid, sim_k, sim_n, steps_c = [-1] * B, [0] * B, 0, 0
    while True:
        busy = 0
        for i in range(B):
            if sim_uid[i] >= 0 and sim_k[i] >= qlen[sim_uid[i]]:
                sim_uid[i] = -1
            if sim_uid[i] < 0 and sim_n < args.queue:
                sim_uid[i], sim_k[i] = sim_n, 0; sim_n += 1
            if sim_uid[i] >= 0:
                sim_k[i] += 1; busy += 1
        if busy == 0:
            break
        steps_c += 1
    t_cont = drive(steps_c, cont)
    useful_c = int(sum(qlen))
    assert sum(plan) == useful_c
    vo.close()

    print(json.dumps({
        "tool": "ragged_batch", "shape": "%dx%d w21 L3, one context of %d sequences, %d frames in flight" % (W, H, B, args.depth),
        "lengths": "KITTI 00-07 / 10 x %d" % (B // 8), "steps": T, "useful_frame_pairs": useful,
        "refed": {"wall_s": round(t_refed, 3), "processed_frame_pairs": B * T, "useful_frame_pairs_per_s": round(useful / t_refed, 1)},
        "masked": {"wall_s": round(t_masked, 3), "processed_frame_pairs": useful, "useful_frame_pairs_per_s": round(useful / t_masked, 1)},
        "masked_over_refed_wall": round(t_masked / t_refed, 3), "useful_fraction": round(useful / (B * T), 3),
        "continuous": {"queue": args.queue, "lengths": "uniform %d..%d, seed %d" % (args.min_len, args.max_len, args.seed), "steps": steps_c,
                       "resets": resets, "wall_s": round(t_cont, 3), "useful_frame_pairs": useful_c,
                       "useful_frame_pairs_per_s": round(useful_c / t_cont, 1)},
        "all_active_frame_pairs_per_s": round(all_fps, 1),
        "continuous_over_all_active": round(useful_c / t_cont / all_fps, 3),
    }))


if __name__ == "__main__":
    main()
