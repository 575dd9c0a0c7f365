#!/usr/bin/env python3
"""What a relocalisation costs (include/svo.h, "Relocalisation"), against the path it replaces on the same library:

    python tools/reloc_bench.py [--out FILE] [--sizes 65536,1048576] [--queries 2048] [--rounds 15] [--guided RADIUS]

Per index size: an index of random rows with points in which the first --queries rows are landmarks of a scene
(tests/reloc_cases.py: exact projections, an eighth of the pixels moved), and the queries are those rows' descriptors with three bits
flipped.  Timed in alternating rounds, medians reported:
  localize   one svo_desc_index_localize call;
  by hand    svo_desc_index_match, then the host filter INTEGRATION.md used to describe (threshold, ratio, one pixel per landmark, the
             points from a host-side mirror of the rows; vectorised numpy), then svo_camera_to_world.
Both paths must return the same pose bits before anything is timed.  Then the device time of k_reloc_select alone (HIP events around
it: svo_desc_index_set_timing) on that input, and on the dedupe's worst case: 4096 queries, all accepted, all of different
landmarks.  One child python per index size, one after the other, each under its own time limit; the first failure ends the run.
Prints one JSON line.

--guided RADIUS runs the guided leg instead (include/svo.h, "Guided search"): every row of the index is a point spread over a
1241 x 376 view (KITTI's, 4 .. 40 m deep), the first --queries rows are the landmarks the frame sees, and the prior is the true pose
off by 0.005 rad and 0.05 m, so that RADIUS px admits the fraction of the rows a tracker's frame would.  In one process and
alternating rounds: the unguided localize, and localize_guided with the query sort on and off — the whole call, and the search
kernels alone (svo_desc_index_set_timing: k_desc_match + merge for the unguided search, k_guide_project + k_desc_match_guided + merge
for the guided one).

--batch B[,B...] runs the batched leg (include/svo.h, "Batched relocalisation") on the guided leg's index and frame: one
svo_desc_index_localize_batch call of B cameras — each camera the frame's queries under a prior of its own — against a loop of B
single calls, through the C entries with the arguments prepared, in the same process and alternating rounds, guided (at --guided,
24 px by default) and unguided.  Before any timing both paths must return the same result records, byte for byte.  Per leg: the
medians with the rounds' minimum and maximum beside them, their ratio, and the batch call's device span (last_kernels_ms), so that
the host's share of the call shows.  The issue's sweep: --batch 1,8,64,256,512."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_filter(m, xy, xyz, max_dist=40, num=7, den=10):
    """rules 1 - 3 on the host from the match rows and a mirror of the points -> (pixels, points) of the candidates"""
    ok = (m["row"] >= 0) & (m["dist"] <= max_dist) & (m["dist"].astype(np.int64) * den < m["dist2"].astype(np.int64) * num)
    j = np.flatnonzero(ok)
    order = np.lexsort((j, m["dist"][j], m["id"][j]))             # per id the smallest (dist, j) first
    first = np.ones(len(j), bool)
    first[1:] = m["id"][j][order][1:] != m["id"][j][order][:-1]
    keep = np.sort(j[order][first])
    return xy[keep], xyz[m["row"][keep]]


def child(size, n, rounds):
    import reloc_cases as cases
    from stereo_visual_odometry_amd import api
    s = cases.scene(n, size, outliers=n // 8)
    rng = np.random.default_rng(size)
    ix = api.DescriptorIndex(size, points=True)
    ix.add_points(s["desc"], s["ids"], s["xyz"], s["tags"])
    rest = size - n
    mirror, head = [s["xyz"]], [s["desc"]]                        # head: the descriptors of the index's first rows, for the worst case below
    for i0 in range(0, rest, 1 << 16):
        m = min(1 << 16, rest - i0)
        p, d = rng.normal(size=(m, 3)).astype(np.float32), rng.integers(0, 256, (m, 32), dtype=np.uint8)
        ix.add_points(d, (1 << 32) + i0 + np.arange(m, dtype=np.uint64), p)
        mirror.append(p)
        if i0 == 0:
            head.append(d)
    xyz = np.concatenate(mirror)
    prm = ix.reloc_params()

    def by_hand():
        cxy, cxyz = host_filter(ix.match(s["query"]), s["xy"], xyz)
        return api.cameraToWorld(s["K"], cxy, cxyz, np.eye(3), np.zeros(3), prm.ransac_iterations, prm.reproj_error, prm.confidence), len(cxy)

    def localize():
        return ix.localize(s["K"], s["query"], s["xy"], params=prm)

    for _ in range(3):
        ((inl, ok), R, t, iters), k = by_hand()
        res, cand = localize()
    assert ok and res.success and res.n_candidates == k and res.R.tobytes() == R.tobytes() and res.t.tobytes() == t.tobytes(), "the two paths differ"
    t_loc, t_hand = [], []
    for _ in range(rounds):
        t0 = time.perf_counter(); localize(); t_loc.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); by_hand(); t_hand.append((time.perf_counter() - t0) * 1e3)
    ix.set_timing(True)
    kern = []
    for _ in range(rounds):
        ix.select(s["query"], s["xy"], params=prm)
        kern.append(ix.stats()["last_kernels_ms"])
    r = dict(size=size, queries=n, rounds=rounds, candidates=k, inliers=int(res.n_inliers), iters_run=int(res.iters_run),
             localize_ms_median=float(np.median(t_loc)), localize_ms_min=float(min(t_loc)),
             by_hand_ms_median=float(np.median(t_hand)), by_hand_ms_min=float(min(t_hand)),
             select_kernel_ms_median=float(np.median(kern)), select_kernel_ms_min=float(min(kern)))
    all_desc = np.concatenate(head)[:4096]
    if len(all_desc) == 4096:                                     # the dedupe's worst case: the first 4096 rows found again, all accepted, all distinct
        wide = ix.reloc_params(max_dist=256, ratio_num=1 << 20, ratio_den=1, row_lo=0, row_hi=4096)
        kern = []
        for _ in range(rounds):
            got = ix.select(all_desc, np.zeros((4096, 2), np.float32), params=wide)
            kern.append(ix.stats()["last_kernels_ms"])
        assert len(got["query"]) == 4096, len(got["query"])
        r.update(worst_case_candidates=4096, worst_case_select_kernel_ms_median=float(np.median(kern)), worst_case_select_kernel_ms_min=float(min(kern)))
    ix.close()
    print(json.dumps(r))


def child_guided(size, n, rounds, radius):
    import guide_cases as gcases
    from reloc_cases import flip
    from stereo_visual_odometry_amd import api
    rng = np.random.default_rng(size)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)
    ix = api.DescriptorIndex(size, points=True)
    head = None
    for i0 in range(0, size, 1 << 16):
        m = min(1 << 16, size - i0)
        z = rng.uniform(4, 40, m)
        px = np.stack([rng.uniform(0, 1241, m), rng.uniform(0, 376, m)], 1)
        p = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1).astype(np.float32)
        d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        ix.add_points(d, (1 << 32) + i0 + np.arange(m, dtype=np.uint64), p)
        if i0 == 0:
            head = (d[:n], p[:n])
    query = np.stack([flip(rng, d, 3) for d in head[0]])
    c = head[1].astype(np.float64)                                # the true pose is the identity
    xy = (c[:, :2] / c[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)
    xy[:n // 8] += 50                                             # an eighth of the pixels moved: outside the gate, or outliers
    R0, t0 = gcases.rot(0.003, -0.003, 0.002), np.array([0.03, -0.03, 0.03])
    prm = ix.reloc_params()
    guide = (K, R0, t0, radius)

    def unguided():
        return ix.localize(K, query, xy, R0, t0, params=prm)

    def guided():
        return ix.localize_guided(*guide, query, xy, params=prm)

    uv = ix.project(K, R0, t0, 0, min(size, 1 << 16))
    adm = (np.abs(uv[None, :, 0] - xy[:64, None, 0]) <= radius) & (np.abs(uv[None, :, 1] - xy[:64, None, 1]) <= radius)
    legs = {}
    for _ in range(3):
        ru, _ = unguided()
        rg, _ = guided()
    assert ru.success and rg.success, "a leg does not localize"
    times = dict(unguided=[], guided_sort_on=[], guided_sort_off=[])
    for _ in range(rounds):
        t0_ = time.perf_counter(); unguided(); times["unguided"].append((time.perf_counter() - t0_) * 1e3)
        ix.set_guided_sort(True)
        t0_ = time.perf_counter(); guided(); times["guided_sort_on"].append((time.perf_counter() - t0_) * 1e3)
        ix.set_guided_sort(False)
        t0_ = time.perf_counter(); roff, _ = guided(); times["guided_sort_off"].append((time.perf_counter() - t0_) * 1e3)
    assert roff.R.tobytes() == rg.R.tobytes() and roff.n_candidates == rg.n_candidates, "the sort changed the result"
    ix.set_timing(True)
    kern = dict(unguided=[], guided_sort_on=[], guided_sort_off=[], project=[])
    for _ in range(rounds):
        ix.match(query); kern["unguided"].append(ix.stats()["last_kernels_ms"])
        ix.set_guided_sort(True)
        ix.select_guided(*guide, query, xy, params=prm); kern["guided_sort_on"].append(ix.stats()["last_kernels_ms"])
        ix.set_guided_sort(False)
        ix.select_guided(*guide, query, xy, params=prm); kern["guided_sort_off"].append(ix.stats()["last_kernels_ms"])
        ix.project(K, R0, t0); kern["project"].append(ix.stats()["last_kernels_ms"])
    r = dict(size=size, queries=n, rounds=rounds, radius=radius, admitted_fraction_of_rows=float(adm.mean()),
             unguided_candidates=int(ru.n_candidates), unguided_inliers=int(ru.n_inliers), guided_candidates=int(rg.n_candidates), guided_inliers=int(rg.n_inliers))
    for k, v in times.items():
        r["%s_call_ms_median" % k] = float(np.median(v)); r["%s_call_ms_min" % k] = float(min(v))
    for k, v in kern.items():
        r["%s_kernels_ms_median" % k] = float(np.median(v)); r["%s_kernels_ms_min" % k] = float(min(v))
    ix.close()
    print(json.dumps(r))


def child_batch(size, n, rounds, radius, counts):
    """svo_desc_index_localize_batch against a loop of B single calls, guided and unguided, on child_guided's index and frame"""
    import ctypes as C
    import guide_cases as gcases
    from reloc_cases import flip
    from stereo_visual_odometry_amd import _lib, api
    lib, ptr = _lib.lib, _lib.ptr
    rng = np.random.default_rng(size)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)
    ix = api.DescriptorIndex(size, points=True)
    head = None
    for i0 in range(0, size, 1 << 16):
        m = min(1 << 16, size - i0)
        z = rng.uniform(4, 40, m)
        px = np.stack([rng.uniform(0, 1241, m), rng.uniform(0, 376, m)], 1)
        p = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1).astype(np.float32)
        d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        ix.add_points(d, (1 << 32) + i0 + np.arange(m, dtype=np.uint64), p)
        if i0 == 0:
            head = (d[:n], p[:n])
    query = np.stack([flip(rng, d, 3) for d in head[0]])
    c = head[1].astype(np.float64)
    xy = (c[:, :2] / c[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]).astype(np.float32)
    xy[:n // 8] += 50
    prm = ix.reloc_params()
    legs = []
    for B in counts:
        # every camera its own prior: the true pose off by about 0.005 rad and 0.05 m, differently per camera
        guides = [ix.guide(gcases.rot(0.003 + 1e-5 * b, -0.003 + 2e-5 * b, 0.002), np.array([0.03, -0.03, 0.03]) + 1e-4 * b, radius) for b in range(B)]
        g = (_lib.SvoRelocGuide * B)(*guides)
        Kf = np.ascontiguousarray(np.broadcast_to(K.reshape(1, 9), (B, 9)))
        q_all, xy_all = np.ascontiguousarray(np.tile(query, (B, 1))), np.ascontiguousarray(np.tile(xy, (B, 1)))
        begin = (np.arange(B + 1) * n).astype(np.int32)
        res_b, res_s = (_lib.SvoRelocResult * B)(), (_lib.SvoRelocResult * B)()

        def guess(res):
            for b in range(B):
                res[b].R[:] = guides[b].R[:]; res[b].t[:] = guides[b].t[:]

        def batch(guided):
            guess(res_b)
            t0 = time.perf_counter()
            rc = lib.svo_desc_index_localize_batch(ix._h, B, ptr(Kf), g if guided else None, ptr(begin), ptr(q_all), ptr(xy_all), C.byref(prm), res_b, None, None, None)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, _lib.lib.svo_last_error()
            return dt

        def loop(guided):
            guess(res_s)
            t0 = time.perf_counter()
            for b in range(B):
                if guided:
                    rc = lib.svo_desc_index_localize_guided(ix._h, ptr(K), C.byref(guides[b]), n, ptr(query), ptr(xy), C.byref(prm), C.byref(res_s[b]), None, None, None)
                else:
                    rc = lib.svo_desc_index_localize(ix._h, ptr(K), n, ptr(query), ptr(xy), C.byref(prm), C.byref(res_s[b]), None, None, None)
                assert rc == 0, _lib.lib.svo_last_error()
            return (time.perf_counter() - t0) * 1e3

        for guided in (True, False):
            batch(guided); loop(guided)
            assert bytes(res_b) == bytes(res_s), "the batch call and the loop of single calls differ (B = %d, guided = %s)" % (B, guided)
            assert all(r.success for r in res_b), "a camera does not localize"
            r_n = max(3, min(rounds, 4096 // B))                  # fewer rounds where one takes long
            tb, tl, kb = [], [], []
            ix.set_timing(True)
            for _ in range(r_n):
                tb.append(batch(guided)); kb.append(ix.stats()["last_kernels_ms"])
                ix.set_timing(False)
                tl.append(loop(guided))
                ix.set_timing(True)
            ix.set_timing(False)
            legs.append(dict(cameras=B, guided=guided, rounds=r_n, batch_call_ms_median=float(np.median(tb)), batch_call_ms_min=float(min(tb)),
                             batch_call_ms_max=float(max(tb)), batch_kernels_ms_median=float(np.median(kb)), loop_ms_median=float(np.median(tl)),
                             loop_ms_min=float(min(tl)), loop_ms_max=float(max(tl)), loop_over_batch=float(np.median(tl) / np.median(tb)),
                             per_camera_batch_ms=float(np.median(tb) / B), per_camera_loop_ms=float(np.median(tl) / B)))
    ix.close()
    print(json.dumps(dict(size=size, queries=n, radius=radius, legs=legs)))


def step(cmd, limit, what):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("%s failed (exit status %s):\n%s\n%s" % (what, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    lines = r.stdout.strip().splitlines()
    return lines[-1] if lines else ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--guided", type=float, default=None, metavar="RADIUS", help="the guided leg at this radius in pixels, beside the unguided one")
    ap.add_argument("--batch", default=None, metavar="B[,B...]", help="svo_desc_index_localize_batch of B cameras against a loop of B single calls (guided at --guided, default 24 px, and unguided)")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.batch is not None and args.guided is None:
        args.guided = 24.0
    if args.child is not None and args.batch is not None:
        return child_batch(args.child, args.queries, args.rounds, args.guided, [int(b) for b in args.batch.split(",")])
    if args.child is not None:
        return child_guided(args.child, args.queries, args.rounds, args.guided) if args.guided is not None else child(args.child, args.queries, args.rounds)
    out = dict(shape="%d queries of a scene inside an index of random rows with points; alternating rounds" % args.queries, sizes=[])
    if args.batch is not None:
        out["shape"] = ("one batch call of B cameras against a loop of B single calls in the same process, alternating rounds; %d queries per camera of a frame "
                        "inside an index of points spread over a 1241 x 376 view; every camera its own prior; guided at %g px, and unguided" % (args.queries, args.guided))
    elif args.guided is not None:
        out["shape"] = "%d queries of a frame inside an index of points spread over a 1241 x 376 view; guided at %g px; alternating rounds" % (args.queries, args.guided)
    for s in (int(x) for x in args.sizes.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(s), "--queries", str(args.queries), "--rounds", str(args.rounds)]
        if args.guided is not None:
            cmd += ["--guided", str(args.guided)]
        if args.batch is not None:
            cmd += ["--batch", args.batch]
        out["sizes"].append(json.loads(step(cmd, 900 if args.batch else 400, "the relocalisation at %d rows" % s)))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
