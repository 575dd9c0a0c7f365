"""What the GPU tests (test_gpu_*.py), their child scripts and reference modules share: the `api` fixture, bit views of results,
snapshots of a sequence's state, the synthetic calibration and streams, and the one way a test starts a child python.  A test module
takes the fixture by name (`from gpu_kit import api  # noqa: F401`): pytest finds fixtures in the module's namespace."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def api():
    from stereo_visual_odometry_amd import api as a
    assert a._lib.device_count() >= 1, "no HIP device"
    return a


def f32_bits(a):
    """the float32 bits of `a`, cast to float32 first"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw_bits(a):
    """the bits of `a` as it is: uint32 words of a float32 array, bytes of anything else"""
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def snap(vo, i):
    """Everything a frame leaves behind for sequence i: the feature set and the compacted tracks."""
    f = vo.features(i); t = vo.last_tracks(i)
    return [raw_bits(f[0]), f[1], f[2]] + [raw_bits(t[k]) for k in ("pl0", "pr0", "pl1", "pr1", "world")] + [t["inlier"]]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def calib(w, h):
    """the KITTI-00 camera with a w x h image and its principal point at the centre"""
    from stereo_visual_odometry_amd import synthetic as syn
    return dict(syn.KITTI00, width=w, height=h, cx=w / 2.0, cy=h / 2.0)


def projections(w, h):
    from stereo_visual_odometry_amd import synthetic as syn
    Pl, Pr = syn.projection_matrices(calib(w, h))
    return Pl.astype(np.float32), Pr.astype(np.float32)


def streams(n_seq, n_frames, seed0, w, h, cn=1, cal=None):
    """n_seq independent synthetic stereo sequences of calib(w, h) (or `cal`) -> [(lefts, rights)]; cn == 3: interleaved BGR frames."""
    from stereo_visual_odometry_amd import synthetic as syn
    out = []
    for i in range(n_seq):
        s = syn.StereoSequence(cal=cal or calib(w, h), n_frames=n_frames, seed=seed0 + 31 * i, step=0.3)
        L, R = list(s.left), list(s.right)
        if cn == 3:
            bgr = lambda a: np.ascontiguousarray(np.stack([a, np.roll(a, 1, 0), 255 - a], -1))
            L, R = [bgr(a) for a in L], [bgr(a) for a in R]
        out.append((L, R))
    return out


def run_child(script, *args, env=None, timeout=300, cwd=None):
    """A fresh python on tests/<script> (or on an absolute path) with `args`, once -> the completed process; a non-zero exit status
    fails the test with what the child printed."""
    r = subprocess.run([sys.executable, os.path.join(HERE, script)] + [str(a) for a in args], env=env, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "%s: exit status %s\n%s\n%s" % (script, r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    return r
