"""The frames of tests/pyr_walk_cases.py through the library, for tests/test_gpu_pyr_walk.py: run() feeds a case's frames (host,
pinned or device frames, 1 .. 3 in flight), optionally checks every stored pyramid and derivative plane against the references, and
returns what every frame reported.  As a script (a fresh process: SVO_PYR_WALK is read once per process) it runs the cases given
as JSON with the parent's kernels (SVO_PYR_WALK=0) and saves those reports to the .npz file named on the command line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import deriv_ref  # noqa: E402
import pyr_walk_cases as pw  # noqa: E402
import test_gpu_pyramids as tp  # noqa: E402

N_STREAMS = 3     # sequence i replays stream i % N_STREAMS: the references are computed once per stream, frame and camera


class Planes:
    """Reference derivative planes of a context's reference pyramids, computed once per (image, camera, level)."""

    def __init__(self, ctx):
        self.ctx, self._ref = ctx, {}

    def check(self, seq, which, pair, what):
        vo, pad = self.ctx.vo, pw.lk_pad_for(self.ctx.win)
        for cam, img in enumerate(pair):
            levels = self.ctx.reference(img, cam)[0]
            for lv in range(1, len(levels)):
                key = (id(img), cam, lv)
                if key not in self._ref:
                    self._ref[key] = deriv_ref.planes(levels[lv], pad)
                gx, gy, gpad = vo.derivatives(seq, which, cam, lv)
                assert gpad == pad
                for name, got, exp in (("Ix", gx, self._ref[key][0]), ("Iy", gy, self._ref[key][1])):
                    assert got.dtype == np.int16 and got.shape == exp.shape, (what, name, got.shape, exp.shape)
                    bad = np.argwhere(got != exp)
                    assert not len(bad), "%s: seq %d %s cam %d level %d %s: %d samples differ, first (y, x) %s" % (what, seq, which, cam, lv, name, len(bad), bad[:4].tolist())


def report(vo, ok, T, settled):
    """One frame of every sequence as arrays: flags, pose bits, every statistics field and — when no later frame is in flight, so
    that the sequence's state is this frame's — the feature sets."""
    B = vo.n_seq
    stats = np.array([[getattr(vo.stats[i], f[0]) for f in vo.stats[i]._fields_] for i in range(B)], np.int64)
    feats = [vo.features(i) if settled else (np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)) for i in range(B)]
    return {"ok": np.asarray(ok, np.uint8), "T": np.ascontiguousarray(T, np.float64).view(np.uint64).reshape(B, 16), "stats": stats,
            "n_feat": np.array([len(f[0]) for f in feats], np.int64),
            "xy": np.concatenate([f[0].view(np.uint32).reshape(-1, 2) for f in feats]), "age": np.concatenate([f[1] for f in feats]),
            "strength": np.concatenate([f[2] for f in feats])}


def run(api, case, check):
    route, (w, h), win, ml, B, inp, ex = case
    what = pw.case_id(case)
    ctx = tp.Ctx(api, w, h, win, ml, B)
    vo, planes = ctx.vo, Planes(ctx)
    assert vo.has_derivatives(), what
    depth = ex.get("depth", 1)
    n = 2 + depth
    base = [tp.make_stream(w, h, n, 1000 * win + 17 * j + w, 1, black=(1,) if j == 0 else ()) for j in range(N_STREAMS)]
    streams = [base[i % N_STREAMS] for i in range(B)]
    ll = tp.LastLeft(B)
    out = []

    def after(k, ok, T, settled):
        out.append(report(vo, ok, T, settled))
        for i in range(B):
            ll.update(i, k, vo.stats[i])
        if check and settled:
            for i in range(B):
                for which, j in (("t1", k), ("last_left", ll.frame[i])):
                    pair = (streams[i][0][j], streams[i][1][j])
                    ctx.check(i, which, pair, (what, k, which, j))
                    planes.check(i, which, pair, (what, k, which, j))

    if inp.startswith("dev"):
        extra = int(inp[4:])
        dev = [[tp.device_frames([s[0][k], s[1][k]], extra) for k in range(n)] for s in base]
        stride = dev[0][0][1]
        sub = 0
        for k in range(n):
            while sub < n and sub - k < depth:
                vo.submit_device([dev[i % N_STREAMS][sub][0][0].data_ptr() for i in range(B)], [dev[i % N_STREAMS][sub][0][1].data_ptr() for i in range(B)], stride)
                tp.assert_route(api, vo, route, (what, sub))
                sub += 1
            ok, T = vo.collect()
            after(k, ok, T, sub == k + 1)
        del dev
    else:
        for k in range(n):
            Ls, Rs = [s[0][k] for s in streams], [s[1][k] for s in streams]
            if inp == "pinned":
                pin = [api.PinnedImage(a.shape) for a in Ls + Rs]
                for p, a in zip(pin, Ls + Rs):
                    p.array[...] = a
                Ls, Rs = [p.array for p in pin[:B]], [p.array for p in pin[B:]]
            ok, T = vo.stereo_callback_batch(Ls, Rs)
            tp.assert_route(api, vo, route, (what, k))
            after(k, ok, T, True)
    ctx.close()
    return out


def main():
    assert os.environ.get("SVO_PYR_WALK") == "0", "run with SVO_PYR_WALK=0"
    from stereo_visual_odometry_amd import api
    cases = [(c[0], tuple(c[1]), c[2], c[3], c[4], c[5], c[6]) for c in json.loads(sys.argv[1])]
    saved = {}
    for c in cases:
        for k, fr in enumerate(run(api, c, check=False)):
            for name, a in fr.items():
                saved["%s/%d/%s" % (pw.case_id(c), k, name)] = a
        print("ok", pw.case_id(c), flush=True)
    np.savez(sys.argv[2], **saved)
    print("pyr walk child ok: %d cases" % len(cases))


if __name__ == "__main__":
    main()
