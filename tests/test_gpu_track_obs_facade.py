"""The C++ facade's track output (include/svo/visual_odometry.hpp): tests/cpp/track_obs_test.cpp compiles with plain g++ against
the C-ABI, and on a GPU its rows agree with the C-ABI's frame by frame.  And the CLI: `svo_cli --tracks` on the committed run1
frames writes one line per observation row, and a persisting id's T0 point is where its previous line left it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "track_obs_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "track_obs_test")
FIX = os.path.join(ROOT, "tests", "golden", "run1_frames_0_7.npz")


def build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])


def test_track_obs_facade_compiles_and_links_with_gxx():
    build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_track_obs_facade_agrees_with_the_c_abi(tmp_path):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=4, seed=3, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([seq.n_frames, 160, 320], np.int32).tobytes())
        f.write(np.ascontiguousarray(Pl, np.float32).tobytes()); f.write(np.ascontiguousarray(Pr, np.float32).tobytes())
        for l, r in zip(seq.left, seq.right):
            f.write(l.tobytes()); f.write(r.tobytes())
    build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "TRACK OBS OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cli_tracks_csv_on_run1(tmp_path):
    from test_run1_cli import build_cli
    from stereo_visual_odometry_amd import api, synthetic as syn
    d = np.load(FIX)
    folder = tmp_path / "run1"
    (folder / "left").mkdir(parents=True); (folder / "right").mkdir()
    for k in range(8):
        for side in ("left", "right"):
            im = d[side][k]
            with open(folder / side / ("frame%06d.pgm" % k), "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0])); f.write(im.tobytes())
    csv = tmp_path / "tracks.csv"
    out = subprocess.run([build_cli(), "8", str(folder), "--gray", "1", "--tracks", str(csv)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "processed 8 frame pairs" in out.stdout, out.stdout + out.stderr
    lines = csv.read_text().splitlines()
    assert lines[0] == "frame,id,ul,vl,ur,vr,x,y,z,age,inlier,has_xyz"
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    # one line per row: the same frames through the Python API
    vo = api.VisualOdometry(cfg=api.default_config()); vo.initalize_projection_matricies(*syn.projection_matrices(syn.RUN1))
    vo.set_track_output(14080)
    prev, checked = {}, 0
    for k in range(8):
        vo.stereo_callback(d["left"][k], d["right"][k])
        obs = vo.last_track_obs()
        mine = rows[rows[:, 0] == k]
        assert len(mine) == len(obs) == vo.stats.n_after_bounds, k
        assert np.array_equal(mine[:, 1].astype(np.int64), obs["id"])
        assert np.array_equal(mine[:, 2:4].astype(np.float32), obs["l1"]) and np.array_equal(mine[:, 4:6].astype(np.float32), obs["r1"])
        assert np.array_equal(mine[:, 6:9].astype(np.float32), obs["xyz"]) and np.array_equal(mine[:, 9].astype(np.int32), obs["age"])
        assert np.array_equal(mine[:, 10].astype(np.int32), obs["flags"] & 1) and np.array_equal(mine[:, 11].astype(np.int32), (obs["flags"] >> 1) & 1)
        # a persisting id's l0 is the previous line's l1 for that id, where that line was an inlier (the feature set keeps the inliers)
        for o in obs:
            p = prev.get(int(o["id"]))
            if p is not None and p[2]:
                assert np.array_equal(np.float32(p[:2]), o["l0"]), (k, int(o["id"]))
                checked += 1
        prev = {int(r[1]): (r[2], r[3], int(r[10])) for r in mine}
    assert len(rows) > 500 and checked > 200, (len(rows), checked)
