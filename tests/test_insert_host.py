"""tests/cpp/insert_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_insert.hpp, the rules of the batched
insertion compiled for the host from the text the library runs — built with AddressSanitizer and UBSan and run, as
tests/test_consolidate_host.py does for the consolidation's: the keep predicate, the id rule, the point rule, the plan of tiles,
the masks' ranks, the layout, and against the numpy reference's vectors (written into the program's input) whole calls, once as a
sequential program and once tile by tile and lane by lane as the kernels run them.  And the facade round trip
(tests/cpp/insert_facade_test.cpp) compiles and links with g++ -Wall -Werror; tests/test_gpu_insert_facade.py runs it."""
import os
import subprocess

import numpy as np

import insert_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def cases():
    """-> [(entries, need_flags, with_points, cam_to_map or None, id_base, tags)]"""
    rng = np.random.default_rng(3)
    out = []
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 513]
    for pattern in ("none", "all", "alternate", "tile_last", "lanes_63_64", "random"):
        e = [ir.make_entry(r, ir.flag_pattern(pattern, r, 40 + b), 7 * b + 1, id0=1000 * b) for b, r in enumerate(sizes)]
        base = rng.integers(0, 1 << 63, len(e), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        out.append((e, ir.OBS_INLIER, True, [ir.pose(b) for b in range(len(e))], base, list(range(len(e)))))
        out.append((e, ir.OBS_INLIER, False, None, base, [0] * len(e)))
        out.append((e, 0, True, None, np.zeros(len(e), np.uint64), [5] * len(e)))
    many = [ir.make_entry(1 + b % 3, ir.flag_pattern("random", 1 + b % 3, b), b) for b in range(ir.MAX_ENTRIES)]
    out.append((many, ir.OBS_INLIER, True, [ir.pose(b % 7) for b in range(len(many))], np.arange(len(many), dtype=np.uint64) << np.uint64(48), [b % 5 for b in range(len(many))]))
    out.append(([ir.make_entry(300, ir.flag_pattern("random", 300, 2), 8)] * 3, ir.OBS_INLIER, True, [ir.pose(1), ir.pose(2, 1e38), ir.pose(3)], np.zeros(3, np.uint64), [1, 2, 3]))
    return out


def write_vectors(path):
    cs = cases()
    refused = 0
    with open(path, "wb") as f:
        f.write(np.array([len(cs)], np.int32).tobytes())
        for entries, need, with_points, T, base, tags in cs:
            n, rows = len(entries), [len(o) for o, _ in entries]
            try:
                want = ir.insert(entries, need, base, with_points, T, tags)
                total, added = int(want["n_added"].sum()), want["n_added"]
            except ir.Refused:
                want, total, refused = None, -1, refused + 1
                added = ir.insert(entries, need, base, False)["n_added"] if not with_points else ir.insert(entries, need | ir.OBS_HAS_XYZ, base, False)["n_added"]
            f.write(np.array([n, need, int(with_points), int(T is not None), sum(rows), total], np.int32).tobytes())
            f.write(np.array(rows, np.int32).tobytes())
            f.write(np.concatenate([o for o, _ in entries]).tobytes()); f.write(np.concatenate([d for _, d in entries]).tobytes())
            f.write(np.asarray(base, "<u8").tobytes()); f.write(np.array(tags, np.int32).tobytes())
            f.write((np.array(T, np.float64) if T is not None else np.zeros((n, 16))).reshape(n, 16).tobytes())
            f.write(np.asarray(added, np.int32).tobytes())
            if want is not None:
                f.write(want["desc"].tobytes()); f.write(want["ids"].astype("<u8").tobytes())
                if with_points:
                    f.write(want["xyz"].astype("<f4").tobytes()); f.write(want["tags"].astype("<i4").tobytes())
    assert refused == 1


def test_insert_rules_under_sanitizers(tmp_path):
    exe, vec = str(tmp_path / "insert_host"), str(tmp_path / "vectors.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "insert_host.cpp"), "-o", exe])
    write_vectors(vec)
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "INSERT HOST OK" in out.stdout, out.stdout + out.stderr


def build_facade_test():
    exe = os.path.join(CPP, "insert_facade_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(CPP, "insert_facade_test.cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "stereo_visual_odometry_amd"), "-lsvo_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "stereo_visual_odometry_amd")])
    return exe


def test_facade_test_compiles_and_links_with_gxx():
    assert os.path.exists(build_facade_test())
