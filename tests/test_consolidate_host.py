"""tests/cpp/consolidate_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_consolidate.hpp, the rules of the
landmark consolidation compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as
tests/test_place_host.py does for the place candidates': every refusal of a call, the scratch layout's sizes, the small rules, and
against the numpy reference's vectors (written into the program's input) the medoid, the mean point and the far views of planted
groups: one view, two, a tie, identical descriptors, 63 and 64 views, radius 0, a radius that cuts views off, and the group whose sum
depends on its order.  And the facade round trip (tests/cpp/consolidate_facade_test.cpp) compiles and links with g++;
tests/test_gpu_consolidate_facade.py runs it."""
import os
import subprocess

import numpy as np

import consolidate_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def planted_groups():
    """-> [(rows, desc (n, 32) uint8, xyz (n, 3) float32, radius)]"""
    rng = np.random.default_rng(11)
    out = []
    for n, radius in ((1, 0.5), (2, 0.1), (2, 100.0), (3, 0.0), (5, 0.3), (8, 0.3), (8, 0.0), (30, 0.25), (63, 0.3), (64, 0.3), (64, 0.0), (17, 1e6)) * 2:
        c = cr.group_sizes_case([n], seed=int(rng.integers(1 << 20)))
        rows = np.sort(rng.choice(100000, n, replace=False)).astype(np.int32)
        out.append((rows, c["desc"], c["xyz"], radius))
    same = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 9, 0)            # every sum is 0: the latest view
    out.append((np.arange(9, dtype=np.int32) * 7, same, rng.uniform(-1, 1, (9, 3)).astype(np.float32), 0.5))
    order = np.zeros((4, 3), np.float32)
    order[:, 0] = [4.0, 2.0 ** -22, 2.0 ** -51, 2.0 ** -51]
    out.append((np.arange(4, dtype=np.int32), np.zeros((4, 32), np.uint8), order, 8.0))
    return out


def write_vectors(path):
    groups = planted_groups()
    with open(path, "wb") as f:
        f.write(np.array([len(groups)], np.int32).tobytes())
        for rows, desc, xyz, radius in groups:
            n = len(rows)
            m = cr.medoid(list(range(n)), desc)
            near = (np.abs(xyz - xyz[m]) <= np.float32(radius)).all(1)
            want = cr.mean_point(xyz, near)
            whole = cr.consolidate(desc, np.full(n, 5, np.uint64), xyz, np.zeros(n, np.int32), radius)      # the same through the five rules
            if n > 1:
                assert whole["xyz"][0].tobytes() == want.tobytes() and np.array_equal(whole["desc"][0], desc[m]) and whole["result"].n_far_views == (~near).sum()
            f.write(np.array([n, m, (~near).sum()], np.int32).tobytes()); f.write(np.float32(radius).tobytes())
            f.write(rows.astype("<i4").tobytes()); f.write(np.ascontiguousarray(desc).view("<u4").tobytes())
            f.write(xyz.astype("<f4").tobytes()); f.write(want.astype("<f4").tobytes())


def test_consolidate_rules_under_sanitizers(tmp_path):
    exe, vec = str(tmp_path / "consolidate_host"), str(tmp_path / "vectors.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "consolidate_host.cpp"), "-o", exe])
    write_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "CONSOLIDATE HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "consolidate_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "consolidate_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
