"""tools/camera_info_yaml.hpp (svo_cli --rectify) reads ROS camera_calibration_parsers YAML files: compiled with g++ like the
other host-only C++ tests, it must give the matrices of the fixtures under tests/golden/ and refuse what it does not cover."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run(tmp_path, *files):
    exe = str(tmp_path / "camera_info_yaml_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tools"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "camera_info_yaml_test.cpp"), "-o", exe])
    return subprocess.check_output([exe] + list(files)).decode().splitlines()


def parsed(line):
    v = line.split()
    w, h, nd = int(v[0]), int(v[1]), int(v[2])
    x = np.array([float(t) for t in v[3:]])
    return dict(width=w, height=h, K=x[:9].reshape(3, 3), D=x[9:9 + nd], R=x[9 + nd:18 + nd].reshape(3, 3), P=x[18 + nd:].reshape(3, 4))


def test_fixtures(tmp_path):
    left, right = run(tmp_path, os.path.join(GOLDEN, "camera_info_left.yaml"), os.path.join(GOLDEN, "camera_info_right.yaml"))
    a, b = parsed(left), parsed(right)
    assert (a["width"], a["height"]) == (1280, 720) and (b["width"], b["height"]) == (1280, 720)
    assert np.array_equal(a["K"], [[699.5, 0, 652.7], [0, 699.1, 362.3], [0, 0, 1]])
    assert np.array_equal(a["D"], [-0.1711, 0.0257, 0.00031, -0.00042, 0])
    assert np.array_equal(a["R"], [[0.99998, 0.00211, -0.00562], [-0.00213, 0.99999, -0.00302], [0.00561, 0.00303, 0.99998]])
    assert np.array_equal(a["P"], [[684.37, 0, 689.89, 0], [0, 684.37, 406.87, 0], [0, 0, 1, 0]])
    assert np.array_equal(b["K"], [[701.2, 0, 648.1], [0, 700.9, 359.8], [0, 0, 1]])               # data over three lines
    assert np.array_equal(b["D"], [0.41, -0.12, 4e-4, -3e-4, 0.02, 0.75, -0.05, 0.08])           # flow mapping, rational_polynomial
    assert np.array_equal(b["R"], [[0.99995, -0.00442, 0.00893], [0.00440, 0.99999, 0.00221], [-0.00894, -0.00217, 0.99996]])
    assert np.array_equal(b["P"], [[684.37, 0, 689.89, -82.124], [0, 684.37, 406.87, 0], [0, 0, 1, 0]])


def test_refuses_unsupported(tmp_path):
    txt = open(os.path.join(GOLDEN, "camera_info_left.yaml")).read()
    bad = [txt.replace("plumb_bob", "equidistant"), txt.replace("data: [684.37, 0, 689.89, 0, 0, 684.37, 406.87, 0, 0, 0, 1, 0]", "data: [1, 2]"),
           txt.replace("image_width: 1280\n", "")]
    paths = []
    for i, t in enumerate(bad):
        p = tmp_path / ("bad%d.yaml" % i); p.write_text(t); paths.append(str(p))
    out = run(tmp_path, *paths)
    assert len(out) == 3 and all(o.startswith("ERROR") for o in out), out
