"""The C++ facade's CLAHE (include/svo/visual_odometry.hpp, set_clahe / clear_clahe) and svo_cli --clahe: tests/cpp/clahe_test.cpp
compiles with plain g++ against the C-ABI and, on a GPU, agrees frame by frame with a plain object fed the numpy-equalised frames;
svo_cli --clahe on the committed run1 frames prints the rows the Python API gives."""
import os
import subprocess

import numpy as np
import pytest

import clahe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "clahe_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "clahe_test")
CLI = os.path.join(ROOT, "tools", "svo_cli")
W, H = 320, 160


def build(src=SRC, exe=EXE):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip", "-lz",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])


def test_clahe_facade_and_cli_compile_and_link_with_gxx():
    build()
    build(os.path.join(ROOT, "tools", "svo_cli.cpp"), CLI)
    assert os.path.exists(EXE) and os.path.exists(CLI)


@pytest.mark.gpu
def test_clahe_facade_agrees_with_a_plain_object_on_equalised_frames(tmp_path):
    from test_gpu_input_format import grey_streams
    ((L, R),), (Pl, Pr) = grey_streams(1, 5, 2700, W, H)
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(L), H, W], np.int32).tobytes())
        f.write(np.ascontiguousarray(Pl, np.float32).tobytes()); f.write(np.ascontiguousarray(Pr, np.float32).tobytes())
        for l, r in zip(L, R):
            for a in (l, r, clahe_ref.clahe_ref(l, 3.0, (6, 4)), clahe_ref.clahe_ref(r, 3.0, (6, 4))):
                f.write(np.ascontiguousarray(a).tobytes())
    build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CLAHE FACADE OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cli_clahe_prints_the_python_api_rows(tmp_path):
    from stereo_visual_odometry_amd import api, synthetic as syn
    d = np.load(os.path.join(ROOT, "tests", "golden", "run1_frames_0_7.npz"))
    n = 8
    for side in ("left", "right"):
        os.makedirs(tmp_path / side)
        for k in range(n):
            a = d[side][k]
            with open(tmp_path / side / ("frame%06d.pgm" % k), "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0])); f.write(np.ascontiguousarray(a, np.uint8).tobytes())
    build(os.path.join(ROOT, "tools", "svo_cli.cpp"), CLI)

    def cli(*extra):
        res = tmp_path / "r.csv"
        p = subprocess.run([CLI, str(n), str(tmp_path), "--gray", "1", "--identity-start", "1", "--out", str(res)] + list(extra), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "processed %d frame pairs" % n in p.stdout, p.stdout + p.stderr
        return res.read_text().splitlines()[1:], [ln for ln in p.stdout.splitlines() if ln.startswith("Frame")]
    rows, frames = cli("--clahe", "2.0,8,8")
    plain_rows, plain_frames = cli()
    assert frames != plain_frames                                     # the equalisation changes what is tracked
    vo = api.VisualOdometry(cfg=api.default_config())                 # the CLI's configuration: the reference defaults
    vo.initalize_projection_matricies(*syn.projection_matrices(syn.RUN1))
    vo.set_clahe(2.0, (8, 8))
    pose = np.eye(4)
    want_rows, want_frames = [], []
    for k in range(n):
        ok, T = vo.stereo_callback(d["left"][k], d["right"][k])
        nxt = np.zeros((4, 4))
        for i in range(4):                                            # the CLI's matmul4: the same sums in the same order
            for j in range(4):
                s = 0.0
                for m in range(4):
                    s += pose[i, m] * T[m, j]
                nxt[i, j] = s
        pose = nxt
        want_rows.append("%.9g,%.9g,%.9g,%.9g,%.9g" % (pose[0, 3], pose[1, 3], pose[2, 3], 0, 0))
        want_frames.append("Frame %d: ok=%d tracks=%d inliers=%d" % (k, int(ok), vo.stats.n_after_bounds, vo.stats.n_inliers))
    vo.close()
    assert frames == want_frames and rows == want_rows
    assert any("ok=1" in ln for ln in frames)
    p = subprocess.run([CLI, str(n), str(tmp_path), "--gray", "1", "--clahe", "2.0,8"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--clahe" in p.stderr
