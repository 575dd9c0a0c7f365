#!/usr/bin/env python3
"""Cost of one optional feature at the bench shape (bench.py's workload: KITTI-00-shaped 1241x376, LK 21x21, maxLevel 3, two
contexts x 256 sequences, frames resident in HBM, 4 frames in flight per context):

    python tools/feature_bench.py FEATURE [options]        FEATURE: rectify | input_format | pose_cov | detect_mask | clahe | tracks | prior | descriptors

A feature is one entry of FEATURES: its legs (the baseline first: the library as it is without the feature's setter, nothing is
called), per leg the frame format and a setup(vo, context_index), the svo_get_stage_timing stage it reports, and optionally a
counter that shows the leg took its path (and `stats`: fields of svo_frame_stats summed over the round).  A setup may return a
function called before every submit with (vo, T0 frame index per sequence or -1, T1 frame index per sequence): per-frame setters,
such as the motion prior's.  Everything else is shared, so every feature is measured the same way: one discarded run
of the baseline leg first (the first leg a process runs is measured 2 - 3 % faster than the same leg later), then --repeat rounds
with the legs alternating inside every round.  Prints one JSON line (and writes it to --out): per leg and round frame-pairs/s, the
stage's milliseconds, inliers and the counter; the other legs as multiples of the baseline, round by round and best against best;
the baseline's round-to-round spread, max / min - 1.  The baseline alone (--legs off --package DIR) runs against a copy of a package
that predates the setter, for an A/B of the untouched path."""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# frame format -> bytes per pixel.  "rendered" is bench.py's rendered frame itself; the others are made from it (B = a, G = a rolled
# one row, R = 255 - a; alpha and chroma are noise) and convert to one grey image, which is the mono8 frame of those features
BPP = dict(rendered=1, mono8=1, bgr8=3, bgra8=4, yuv422=2)


def rect_calib(variant):
    """a mildly distorted calibration of the KITTI-00 camera, (left, right), one per variant"""
    from stereo_visual_odometry_amd import synthetic as syn
    cal, v = syn.KITTI00, variant
    K = [[cal["fx"], 0, cal["cx"]], [0, cal["fy"], cal["cy"]], [0, 0, 1]]
    c, s = np.cos(1e-3 * (v % 7)), np.sin(1e-3 * (v % 7))
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    P = np.array([[K[0][0], 0, K[0][2] + 0.25 * (v % 5), 0], [0, K[1][1], K[1][2], 0], [0, 0, 1, 0]])
    ci = dict(width=1241, height=376, K=K, D=[-0.02 - 1e-4 * (v % 11), 0.004, 1e-4, -1e-4, 0.0], R=R, P=P)
    return ci, dict(ci, D=list(ci["D"][:4]) + [0.001])


@functools.lru_cache(maxsize=None)
def rect_maps(variant):
    """the four map planes of rect_calib(variant), made on the host once per process"""
    from stereo_visual_odometry_amd import api
    return tuple(m for ci in rect_calib(variant) for m in api.init_rectify_map(ci["K"], ci["D"], ci["R"], ci["P"], ci["width"], ci["height"]))


def rectify_shared(vo, c):
    vo.set_rectification(*rect_calib(0))


def rectify_private(vo, c):
    for i in range(vo.n_seq):
        vo.set_rectification_maps(*rect_maps(c * vo.n_seq + i), seq=i, raw_size=(vo.width, vo.height))


def bonnet_mask(w, h, i):
    """closes the lower quarter of the image (a bonnet) and two boxes"""
    m = np.full((h, w), 255, np.uint8)
    m[h - h // 4:, :] = 0
    rng = np.random.default_rng(77 + i)
    for _ in range(2):
        x, y = int(rng.integers(0, w - 200)), int(rng.integers(0, h - 120))
        m[y:y + 100, x:x + 180] = 0
    return m


def mask_shared(vo, c):
    vo.set_detection_mask(bonnet_mask(vo.width, vo.height, 0))


def mask_per_seq(vo, c):
    for i in range(vo.n_seq):
        vo.set_detection_mask(bonnet_mask(vo.width, vo.height, c * vo.n_seq + i), i)


def nothing(vo, c):
    pass


def clahe_on(vo, c):
    vo.set_clahe(2.0, (8, 8))


def descriptors_on(vo, c):
    """the descriptor leg: the track output at the `tracks` feature's max_rows, and a 32-byte descriptor beside every row"""
    vo.set_track_output(2048)
    vo.set_descriptor_output(True)


def prior_setup(kind):
    """the motion-prior legs: before every submit, every sequence with a previous frame gets a prior — the identity (the mechanism's
    cost: same tracks, one more copy, the prior kernel) or the rotation between the two frames it is about to track (what it buys)"""
    def setup(vo, c):
        from stereo_visual_odometry_amd import api
        table = {}

        def before(vo, f0, f1):
            Hs, His = np.zeros((vo.n_seq, 3, 3), np.float32), np.zeros((vo.n_seq, 3, 3), np.float32)
            for i, (a, b) in enumerate(zip(f0, f1)):
                if a < 0:
                    continue
                if (a, b) not in table:
                    R = np.eye(3) if kind == "identity" else (np.linalg.inv(POSES[a]) @ POSES[b])[:3, :3].T
                    table[(a, b)] = api.motion_prior_from_rotation(PL, R)
                Hs[i], His[i] = table[(a, b)]
            vo.set_motion_priors(Hs, has=[a >= 0 for a in f0], His=His)
        return before
    return setup


def prior_auto(vo, c):
    """the leg without a host prior: every frame predicts one on the device from each sequence's last pose (SVO_PRIOR_LAST_ROTATION) —
    read against `rotation`, the ground truth, as its ceiling and `off` as its floor"""
    vo.set_motion_prior_mode("last_rotation")


POSES, PL = [], None                                 # the pool's camera poses per frame and the left projection matrix (main fills them)

# legs: name -> (frame format, setup), the baseline first.  evidence: (name, f(vo, leg, frame_bytes) read after every recorded
# collect and summed over the round, whether the sum is divided by the round's frame pairs)
FEATURES = dict(
    rectify=dict(stage="ingest+pyramid", evidence=None,
                 legs=dict(a=("rendered", nothing), b=("rendered", rectify_shared), c=("rendered", rectify_private))),
    input_format=dict(stage="ingest+pyramid", evidence=("source_bytes_per_pair", lambda vo, leg, nbytes: 2 * nbytes * vo.n_seq, True),
                      legs={f: (f, nothing) for f in ("mono8", "bgr8", "bgra8", "yuv422")}),
    pose_cov=dict(stage="pnp",                        # last_pose_covariance() is an error for a frame issued with the mode off
                  evidence=("valid_covariances", lambda vo, leg, nbytes: int(vo.last_pose_covariance()[2].sum()) if leg != "off" else 0, False),
                  legs=dict(off=("rendered", nothing), residual=("rendered", lambda vo, c: vo.set_pose_covariance("residual")))),
    detect_mask=dict(stage="detect", evidence=("masked_frames", lambda vo, leg, nbytes: int(bool(vo.last_frame_path() & 256)), False),   # SVO_PATH_DETECT_MASKED
                     legs=dict(off=("rendered", nothing), shared=("rendered", mask_shared), per_seq=("rendered", mask_per_seq))),
    clahe=dict(stage="ingest+pyramid", evidence=None,
               legs=dict(off=("mono8", nothing), on=("mono8", clahe_on), on_bgr8=("bgr8", clahe_on))),
    tracks=dict(stage="pnp",                          # the rows of sequence 0 only: reading all of them would be timed with the leg
                evidence=("rows_of_sequence_0", lambda vo, leg, nbytes: len(vo.last_track_obs(0)) if leg != "off" else 0, False),
                legs=dict(off=("rendered", nothing), on=("rendered", lambda vo, c: vo.set_track_output(2048)))),
    descriptors=dict(stage="pnp",                     # k_track_desc runs behind the pose stage; the rows of sequence 0 only, as for tracks
                     evidence=("descriptor_rows_of_sequence_0", lambda vo, leg, nbytes: len(vo.last_track_descriptors(0)) if leg == "descriptors" else 0, False),
                     legs=dict(off=("rendered", nothing), tracks=("rendered", lambda vo, c: vo.set_track_output(2048)), descriptors=("rendered", descriptors_on))),
    prior=dict(stage="lk", evidence=("prior_frames", lambda vo, leg, nbytes: int(bool(vo.last_frame_path() & 2048)), False),   # SVO_PATH_MOTION_PRIOR
               stats=("n_after_circular", "lk_newton_steps"),
               legs=dict(off=("rendered", nothing), identity=("rendered", prior_setup("identity")), rotation=("rendered", prior_setup("rotation")),
                         auto=("rendered", prior_auto)),
               on_request=("auto",)),                 # run when --legs names it: the default set stays off, identity, rotation
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("feature", choices=sorted(FEATURES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seqs", type=int, default=512)
    ap.add_argument("--contexts", type=int, default=2)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--legs", default=None, help="comma-separated, default: every leg of the feature but those it runs on request (prior: auto)")
    ap.add_argument("--repeat", type=int, default=3, help="rounds of the legs, alternating them in every round")
    ap.add_argument("--package", default=None, help="directory holding the stereo_visual_odometry_amd package to import (default: this checkout)")
    ap.add_argument("--yaw-amp", type=float, default=None, help="yaw_amp_deg of the rendered scenes (default: the bench's); the per-frame yaw step is at most yaw_amp * 2 pi / 16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    if args.package:
        sys.path.insert(0, os.path.abspath(args.package))
    import torch
    import bench
    from stereo_visual_odometry_amd import api, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("feature_bench.py needs a GPU")
    feature = FEATURES[args.feature]
    base = next(iter(feature["legs"]))
    legs = args.legs.split(",") if args.legs else [k for k in feature["legs"] if k not in feature.get("on_request", ())]
    unknown = [k for k in legs if k not in feature["legs"]]
    if unknown:
        raise SystemExit("%s has no leg %s (it has %s)" % (args.feature, ",".join(unknown), ",".join(feature["legs"])))
    stage_field = feature["stage"].replace("+", "_") + "_ms"
    dev = torch.device("cuda", 0)
    cal = syn.KITTI00
    W, H, F, B, C = cal["width"], cal["height"], args.frames, args.seqs, args.contexts
    Bc = B // C
    scene = dict(cal=cal, n_frames=F, movers=0.3, step=0.5, cell_px=16.6)
    if args.yaw_amp is not None:
        scene["yaw_amp_deg"] = args.yaw_amp
    pool = bench.render_pool([dict(scene, seed=0x5EED0002 + g) for g in range(args.pool)], max(1, min(16, bench.host_cores())))
    global PL
    POSES[:] = pool[0].poses                           # the same trajectory in every scene of the pool: the seed only draws the texture
    PL = syn.projection_matrices(cal)[0]
    gen = torch.Generator(device="cpu"); gen.manual_seed(1)

    def frames_of(side, fmt):
        """[pool][F] frames of one camera in `fmt`, on the device: (pool, F, H, W * bpp) uint8."""
        a = torch.stack([torch.from_numpy(np.stack(getattr(s, side))) for s in pool]).to(dev)             # the rendered scene
        if fmt == "rendered":
            return a.contiguous()
        bgr = torch.stack([a, a.roll(1, dims=-2), 255 - a], -1)
        c = bgr.to(torch.int32)
        grey = ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).to(torch.uint8)
        if fmt == "mono8":
            return grey.contiguous()
        if fmt == "bgr8":
            return bgr.contiguous()
        noise = torch.randint(0, 256, a.shape, generator=gen, dtype=torch.uint8).to(dev)
        return (torch.cat([bgr, noise[..., None]], -1) if fmt == "bgra8" else torch.stack([noise, grey], -1)).contiguous()   # yuv422 is UYVY: chroma, then Y

    def ping_pong(i):
        p = i % (2 * F - 2)
        return p if p < F else 2 * F - 2 - p

    Pl, Pr = syn.projection_matrices(cal)
    over = dict(win_w=21, win_h=21, max_translation_norm=2.0, max_level=3, ransac_iterations=100)
    os.environ.setdefault("SVO_GRAPH", "0")

    def run_leg(leg):
        fmt, setup = feature["legs"][leg]
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

        def frame_ids(step, c):
            return [ping_pong(step + (b // args.pool) * 3) for b in range(c * Bc, (c + 1) * Bc)]

        vos, hooks = [], []
        for c in range(C):
            v = api.BatchVisualOdometry(W, H, Bc, api.default_config(**over))
            v.initalize_projection_matricies(Pl, Pr)
            v.set_stage_timing(True)
            if BPP[fmt] != 1:
                v.set_input_format(fmt)
            hooks.append(setup(v, c))
            vos.append(v)
        ms, inl, seen = [], [], 0
        sums = {k: 0 for k in feature.get("stats", ())}
        ok_frames = 0

        def run(first, count, record):
            nonlocal seen, ok_frames
            sub = col = 0
            while col < count:
                while sub < count and sub - col < args.depth:
                    for c, vo in enumerate(vos):
                        lp, rp = ptrs(first + sub, c)
                        if hooks[c]:
                            s = first + sub
                            hooks[c](vo, frame_ids(s - 1, c) if s > 0 else [-1] * Bc, frame_ids(s, c))
                        vo.submit_device(lp, rp, W * BPP[fmt])
                    sub += 1
                for vo in vos:
                    vo.collect()
                    if record:
                        ms.append(vo.stage_timing()[feature["stage"]])
                        inl.append(sum(s.n_inliers for s in vo.stats))
                        ok_frames += sum(s.fail_reason == 0 for s in vo.stats)
                        for k in sums:
                            sums[k] += sum(getattr(s, k) for s in vo.stats)
                        if feature["evidence"]:
                            seen += feature["evidence"][1](vo, leg, img)
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
        r = {"frame_pairs_per_s": B * args.steps / dt, stage_field: float(np.mean(ms)), "inliers": int(np.sum(inl))}
        if sums:
            r.update(sums, ok_frames=int(ok_frames))
        if feature["evidence"]:
            r[feature["evidence"][0]] = seen // (B * args.steps) if feature["evidence"][2] else seen
        return r

    run_leg(base)                                                     # discarded: a process's first leg measures fast
    res = {k: [] for k in legs}
    for _ in range(args.repeat):
        for k in legs:
            res[k].append(run_leg(k))
    out = dict(feature=args.feature, shape="1241x376, w21, L3, %d contexts x %d sequences, depth %d, %d steps" % (C, Bc, args.depth, args.steps),
               legs={k: {field: [r[field] for r in v] for field in v[0]} for k, v in res.items()})
    if base in res:
        rates = {k: [r["frame_pairs_per_s"] for r in v] for k, v in res.items()}
        out["ratio_to_%s_per_round" % base] = {k: [r / m for r, m in zip(rates[k], rates[base])] for k in rates if k != base}
        out["ratio_to_%s" % base] = {k: max(rates[k]) / max(rates[base]) for k in rates if k != base}
        out["%s_round_to_round_spread" % base] = max(rates[base]) / min(rates[base]) - 1
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
