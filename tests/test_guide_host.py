"""tests/cpp/guide_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_guide.hpp, the guided search's projection
and gate compiled for the host from the text the kernels and the index's host code run — built with AddressSanitizer and UBSan
(-ffp-contract=off, as the library) and run as its own process on tables tests/guide_ref.py wrote: random poses and points at scales
1 and 1e3 (rows in front of the camera and behind it, some without a point), the planned rows for every clause of rule 1 under both
of guide_cases' priors (Zc == 0, Zc < 0, a Zc so small that u overflows f32, an infinite quotient times fx = 0, no point), and gate
tables for every clause of rule 2 (|u - x| equal to the radius and one f32 beyond it, radius 0 with u == x, radius 0.25, NaN and infinite
pixels, invisible rows) and for random pixels.  The program's projections and gate bits must equal the tables' byte for byte.
Nothing goes through Python or LD_PRELOAD.  And the facade test (tests/cpp/guide_facade_test.cpp) compiles and links with g++;
tests/test_gpu_guide_facade.py runs it."""
import os
import subprocess

import numpy as np

import guide_cases as cases
import guide_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def put_projection(f, K, R, t, xyz, tags):
    uv = gref.project(K, R, t, xyz, tags)
    pts = np.zeros(len(xyz), np.dtype([("xyz", "<f4", 3), ("tag", "<i4")]))
    pts["xyz"], pts["tag"] = xyz, tags
    f.write(np.array([1, len(xyz)], np.int32).tobytes())
    f.write(np.asarray(K, np.float32).reshape(9).tobytes()); f.write(np.asarray(R, np.float64).reshape(9).tobytes())
    f.write(np.asarray(t, np.float64).reshape(3).tobytes()); f.write(pts.tobytes()); f.write(uv.tobytes())
    return uv


def put_gate(f, uv, xy, radius):
    adm = gref.admissible(uv, xy, radius)
    f.write(np.array([2, len(uv), len(xy)], np.int32).tobytes()); f.write(np.float32(radius).tobytes())
    f.write(np.asarray(uv, np.float32).tobytes()); f.write(np.asarray(xy, np.float32).tobytes()); f.write(adm.astype(np.uint8).tobytes())
    return adm


def write_tables(path):
    rng = np.random.default_rng(12)
    points = gates = 0
    K = np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32)
    with open(path, "wb") as f:
        for scale in (1.0, 1e3):
            for _ in range(3):
                R, t = np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(size=3) * scale
                xyz = (rng.normal(size=(500, 3)) * scale).astype(np.float32)
                tags = np.where(rng.random(500) < 0.1, -1, rng.integers(0, 9, 500)).astype(np.int32)
                uv = put_projection(f, K, R, t, xyz, tags)
                vis = np.isfinite(uv).all(1)
                k = min(40, int(vis.sum()))
                assert 10 < vis.sum() < 490                                                    # rows in front of the camera, and rows not
                xy = (uv[vis][:k] + rng.choice([-3, -2.5, 0, 2.5, 3, 40], (k, 2))).astype(np.float32)   # on the radius, inside and outside
                adm = put_gate(f, uv, xy, 3.0)
                assert adm.sum() >= 5 and not adm.all()
                points += len(xyz); gates += adm.size
        xyz, tags = cases.clause_rows()
        for (Kc, R, t), want in zip(cases.CLAUSE_GUIDES, cases.CLAUSE_VISIBLE):
            uv = put_projection(f, Kc, R, t, xyz, tags)
            assert np.isfinite(uv).all(1).tolist() == want
            points += len(xyz)
            for radius in (24.0, 0.0, 0.25):
                xy, plan = cases.clause_pixels(uv[0, 0], uv[0, 1], radius)
                adm = put_gate(f, uv, xy, radius)
                assert adm[:, 0].tolist() == plan.tolist()
                gates += adm.size
    return points, gates


def test_guide_rules_under_sanitizers(tmp_path):
    exe, table = str(tmp_path / "guide_host"), str(tmp_path / "tables.bin")
    points, gates = write_tables(table)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "guide_host.cpp"), "-o", exe])
    out = subprocess.run([exe, table], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "GUIDE HOST OK (20 tables, %d points, %d gates)" % (points, gates) in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "guide_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "guide_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
