#!/usr/bin/env python3
"""What putting a many-sequence frame into a descriptor index costs (include/svo.h, "Batched insertion"): the batch call beside the
loop of single calls it replaces:

    python tools/insert_bench.py [--out FILE] [--seqs 256,512] [--rounds 7] [--max-rows 2048]

One process.  Per context size, one context at the bench shape (KITTI-00 1241 x 376, LK 21 x 21, max_level 3, as bench.py's cfg2)
with the track and descriptor outputs on at --max-rows, fed three frames from a small pool of rendered sequences; then, on the last
collected frame, for the points call and the plain call:

  loop    svo_desc_index_add_frame[_points] once per sequence (the host path: copy, pack, transform, three uploads and a wait each)
  batch   svo_desc_index_add_frames[_points] once (the ring path: the kernels read the host-mapped rings in place)
  staged  svo_desc_index_add_obs on the same rows read back by the host, 1 << 18 rows a call (the same kernels behind a pinned
          upload: what copying the rows to the device first costs, the host's packing of the list included)

Both indices are truncated (untimed) before every run; loop and batch alternate, a warm-up of each first, --rounds rounds; the
medians and the rounds' spread (min, max) of the synchronous calls' wall time are reported, the batch call's kernels beside it (HIP
events: svo_desc_index_set_timing, svo_desc_index_get_insert_stats), and the indices are compared byte for byte once.
link_bytes is computed from the shapes, not counted: 4 bytes of flags per scanned row plus 52 (id, xyz, descriptor) per kept row —
the bytes the kernels ask for; the link moves whole 64-byte requests at least, so this is a lower bound on the traffic, and
link_gbps_asked = link_bytes / kernels time stands beside the link's 63 GB/s specification as that and nothing more.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOL, FRAMES = 4, 3


def spread(walls):
    return dict(median=float(np.median(walls)), min=float(min(walls)), max=float(max(walls)))


def one_context(api, syn, torch, n_seq, max_rows, rounds, pool):
    cal = syn.KITTI00
    W, H = cal["width"], cal["height"]
    vo = api.BatchVisualOdometry(W, H, n_seq, api.default_config(win_w=21, win_h=21, max_translation_norm=2.0, max_level=3, ransac_iterations=100))
    vo.initalize_projection_matricies(*syn.projection_matrices(cal))
    vo.set_track_output(max_rows)
    vo.set_descriptor_output(True)
    for k in range(FRAMES):
        vo.process_device([pool[b % POOL][0][k].data_ptr() for b in range(n_seq)], [pool[b % POOL][1][k].data_ptr() for b in range(n_seq)], W)
    obs = [vo.last_track_obs(s) for s in range(n_seq)]
    desc = [vo.last_track_descriptors(s) for s in range(n_seq)]
    scanned = sum(len(o) for o in obs)
    T = np.tile(np.eye(4), (n_seq, 1, 1)); T[:, :3, 3] = np.arange(n_seq)[:, None]
    out = dict(n_seq=n_seq, max_rows=max_rows, rounds=rounds, rows_scanned=scanned, legs={})
    for points in (True, False):
        a, b = [api.DescriptorIndex(scanned + 16, points=points) for _ in range(2)]
        b.set_timing(True)

        def loop():
            for s in range(n_seq):
                a.add_frame_points(vo, T[s], tag=1, seq=s) if points else a.add_frame(vo, s)

        def batch():
            return b.add_frames_points(vo, T, [1] * n_seq) if points else b.add_frames(vo)

        def staged():                                     # add_obs takes 1 << 18 rows a call: whole sequences up to that
            ms, s0 = 0.0, 0
            while s0 < n_seq:
                s1, m = s0, 0
                while s1 < n_seq and (s1 == s0 or m + len(obs[s1]) <= api._lib.INSERT_MAX_OBS_ROWS):
                    m += len(obs[s1]); s1 += 1
                b.add_obs(obs[s0:s1], desc[s0:s1], with_points=points, cam_to_map=T[s0:s1] if points else None, tags=[1] * (s1 - s0) if points else None)
                ms += b.insert_stats()["last_kernels_ms"]
                s0 = s1
            return ms
        walls, kern = dict(loop=[], batch=[], staged=[]), dict(batch=[], staged=[])
        for r in range(rounds + 1):                       # round 0 warms both up
            for name, ix, call in (("loop", a, loop), ("batch", b, batch), ("staged", b, staged)):
                ix.truncate(0)
                t0 = time.perf_counter()
                ms = call()
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    walls[name].append(dt)
                    if name in kern:
                        kern[name].append(ms if name == "staged" else b.insert_stats()["last_kernels_ms"])
            if r == 0:
                b.truncate(0); batch()
                st = b.insert_stats()
                assert st["last_path"] == api._lib.INSERT_PATH_RING and st["rows_scanned"] == scanned
                want = ("desc", "ids", "xyz", "tags") if points else ("desc", "ids")
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a.read_rows(want=want), b.read_rows(want=want)) if x is not None), "the batch call's index differs from the loop's"
                added = st["rows_added"]
        link_bytes = 4 * scanned + 52 * added
        k_ms = float(np.median(kern["batch"]))
        out["legs"]["points" if points else "plain"] = dict(
            rows_added=int(added), wall_ms={k: spread(v) for k, v in walls.items()}, kernels_ms={k: spread(v) for k, v in kern.items()},
            loop_over_batch_wall=float(np.median(walls["loop"]) / np.median(walls["batch"])),
            loop_ms_per_sequence=float(np.median(walls["loop"]) / n_seq),
            link_bytes=int(link_bytes), link_gbps_asked=float(link_bytes / (k_ms * 1e-3) / 1e9) if k_ms > 0 else None, link_gbps_spec=63.0)
        a.close(); b.close()
    vo.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="256,512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-rows", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from stereo_visual_odometry_amd import api, synthetic as syn
    seqs = [syn.StereoSequence(cal=syn.KITTI00, n_frames=FRAMES, seed=0x5EED0002 + g, step=0.5, cell_px=16.6, movers=0.3) for g in range(POOL)]
    pool = [([torch.from_numpy(np.ascontiguousarray(l)).cuda() for l in s.left], [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in s.right]) for s in seqs]
    torch.cuda.synchronize()
    out = dict(shape="KITTI-00 1241x376, LK 21x21, max_level 3, track + descriptor output, the third frame's rows; need_flags = INLIER",
               read_strategy="the kernels read the host-mapped rings in place; the keep bits stay in device memory between count and put",
               contexts=[one_context(api, syn, torch, int(s), args.max_rows, args.rounds, pool) for s in args.seqs.split(",")])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
