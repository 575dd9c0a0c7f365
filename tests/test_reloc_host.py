"""tests/cpp/reloc_select_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_reloc.hpp, the relocaliser's rules
compiled for the host from the text k_reloc_select and the index's host code run — built with AddressSanitizer and UBSan and run on
tables tests/reloc_ref.py wrote: randomised result rows with heavy ties (few distances, few ids, distances on both sides of max_dist,
ratio terms on both sides of equality, rows without points, empty rows), and the f64 transform of add_frame_points on random poses.
Nothing goes through LD_PRELOAD.  And the facade test (tests/cpp/reloc_facade_test.cpp) compiles and links with g++;
tests/test_gpu_reloc_facade.py runs it."""
import os
import subprocess

import numpy as np

import desc_match_ref as mref
import reloc_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def random_rows(rng, n, m):
    """n result rows over an index of m rows: ties everywhere, every clause of rule 1 on both sides"""
    out = np.zeros(n, mref.DTYPE)
    out["row"] = rng.integers(0, m, n)
    out["id"] = rng.integers(0, max(2, n // 3), n).astype(np.uint64) * np.uint64(0x100000001)   # both halves of an id matter
    out["dist"] = rng.choice([0, 7, 14, 39, 40, 41, 256], n)
    out["dist2"] = np.maximum(out["dist"], rng.choice([0, 10, 11, 20, 21, 57, 58, 256, mref.NO_DIST], n))
    out["row2"] = np.where(out["dist2"] == mref.NO_DIST, mref.NONE, 0)
    empty = rng.random(n) < 0.05
    out["row"][empty] = out["row2"][empty] = mref.NONE
    out["dist"][empty] = out["dist2"][empty] = mref.NO_DIST
    out["id"][empty] = 0
    return out


def write_cases(path):
    rng = np.random.default_rng(11)
    kept = 0
    with open(path, "wb") as f:
        for n in (0, 1, 2, 63, 64, 65, 1023, 1025, 4096):
            for rule in ((40, 7, 10), (256, 1 << 20, 1), (0, 1, 1 << 20), (39, 7, 10)):
                m = max(1, n // 2)
                rows = random_rows(rng, n, m)
                tags = np.where(rng.random(m) < 0.2, rref.POINT_NONE, rng.integers(0, 1000, m)).astype(np.int32)
                q, r = rref.select(rows, tags, *rule)
                kept += len(q)
                f.write(np.array([n, m, *rule, len(q)], np.int32).tobytes())
                f.write(rows.tobytes()); f.write(tags.tobytes()); f.write(q.tobytes()); f.write(r.tobytes())
        for scale in (1.0, 1e3):
            T = np.eye(4)
            T[:3] = rng.normal(size=(3, 4)) * [1, 1, 1, scale]
            p = (rng.normal(size=(500, 3)) * scale).astype(np.float32)
            f.write(np.array([-1, len(p)], np.int32).tobytes())
            f.write(T.tobytes()); f.write(p.tobytes()); f.write(rref.map_points(T, p).tobytes())
    return kept


def test_reloc_rules_under_sanitizers(tmp_path):
    exe, table = str(tmp_path / "reloc_select_host"), str(tmp_path / "cases.bin")
    assert write_cases(table) > 1000                  # the tables keep something, and (the rules' clauses) drop something
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "reloc_select_host.cpp"), "-o", exe])
    out = subprocess.run([exe, table], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "RELOC HOST OK (36 cases, 1000 points)" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "reloc_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "reloc_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
