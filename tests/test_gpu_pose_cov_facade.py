"""The C++ facade's pose covariance (include/svo/visual_odometry.hpp): tests/cpp/pose_cov_test.cpp compiles with plain g++
against the C-ABI, and on a GPU its setter and getter agree with the C-ABI frame by frame."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pose_cov_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "pose_cov_test")


def build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])


def test_pose_cov_facade_compiles_and_links_with_gxx():
    build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_pose_cov_facade_agrees_with_the_c_abi(tmp_path):
    from stereo_visual_odometry_amd import synthetic as syn
    cal = dict(syn.KITTI00, width=320, height=160, cx=160.0, cy=80.0)
    seq = syn.StereoSequence(cal=cal, n_frames=3, seed=3, step=0.3)
    Pl, Pr = syn.projection_matrices(cal)
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([seq.n_frames, 160, 320], np.int32).tobytes())
        f.write(np.ascontiguousarray(Pl, np.float32).tobytes()); f.write(np.ascontiguousarray(Pr, np.float32).tobytes())
        for l, r in zip(seq.left, seq.right):
            f.write(l.tobytes()); f.write(r.tobytes())
    build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "POSE COV OK" in out.stdout, out.stdout + out.stderr
