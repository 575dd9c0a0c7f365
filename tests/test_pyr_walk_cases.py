"""The guard of the case matrix tests/test_gpu_pyr_walk.py runs (tests/pyr_walk_cases.py), and the walk itself without a GPU:
stereo_visual_odometry_amd/csrc/svo_pyr_walk.hpp — the plan and the per-thread routine k_pyr_walk runs — compiles with plain g++
(tests/cpp/pyr_walk_host.cpp restates v_perm and v_alignbyte), so

- the packed arithmetic: every work item of a level run on the host, level after level, equals tests/pyramid_ref.py byte for byte
  on random and on 0 / 255 images of the matrix sizes (and 1241 x 376), with rows 0, 1, 3 and 64 bytes wider than the image, the
  ingest form's level-0 copy included; the program places the image against inaccessible pages on either side, so a load outside
  the caller's image ends it with a fault;
- the load plan: for every level of every size the bytes an item loads lie inside the h rows of w bytes, and every pixel of the
  destination level and of level 0 belongs to exactly one item."""
import os
import re
import subprocess

import numpy as np
import pytest

import pyr_walk_cases as pw
import pyramid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_visual_odometry_amd", "csrc")
ALL = pw.CASES + pw.MANY_CASES


# --------------------------------------------------------------------------------------------------------------- the matrix
def test_the_restated_constants_are_the_kernels():
    text = open(os.path.join(CSRC, "svo_pyr_walk.hpp")).read()
    define = lambda name: re.search(r"^#define %s (.+?)\s*(//.*)?$" % name, text, re.M).group(1)
    assert (int(define("PW_VEC")), int(define("PW_ROWS")), int(define("PW_ROWS_INGEST"))) == (pw.WALK_V, pw.WALK_ROWS, pw.WALK_ROWS_INGEST)
    assert define("PW_SPAN") == "(2 * PW_VEC + 4)" and pw.WALK_SPAN == 2 * pw.WALK_V + 4
    assert define("PW_LOAD") == "(PW_SPAN + 4)" and pw.WALK_LOAD == pw.WALK_SPAN + 4
    assert "PW_VEC * v - p.c" in text and "p.c = pad & 7" in text, "the vectors' origin moved: restate it in pyr_walk_cases.py"
    assert int(re.search(r"^#define SVO_LONE_MAX_SEQ (\d+)", open(os.path.join(CSRC, "svo_internal.hpp")).read(), re.M).group(1)) == 8


def test_the_contexts_are_the_smallest_many_sequence_ones():
    assert all(9 <= c[4] <= 12 for c in ALL) and {c[4] for c in pw.CASES} >= {9, 10, 11, 12}
    assert all(len(pw.levels_of(c)) >= 2 for c in ALL)
    assert sum(c[1] == (1241, 376) and c[4] == 9 for c in pw.CASES) == 1


def test_widths_and_heights_hit_the_plan_edges():
    V, R, R1 = pw.WALK_V, pw.WALK_ROWS, pw.WALK_ROWS_INGEST
    w0, w1, rows, rows1, origins, odd = set(), set(), set(), set(), set(), False
    for c in pw.CASES:
        sizes = pw.levels_of(c)
        origins.add(pw.lk_pad_for(c[2]) & 7)
        w0.add(sizes[0][0] % V); w1.add(sizes[1][0] % V)
        rows |= {h % R for w, h in sizes[2:]}
        rows1.add(sizes[1][1] % R1)
        odd |= sizes[0][1] % 2 == 1 and any(h % 2 == 1 for w, h in sizes[1:-1])
    assert w0 >= {V - 1, 0, 1} and w1 >= {V - 1, 0, 1}, (w0, w1)
    assert rows >= {0, 1, R - 1} and rows1 >= {0, 1, R1 - 1} and odd, (rows, rows1)
    assert origins == {0, 4}
    assert {pw.lk_pad_for(21) & 7, pw.lk_pad_for(15) & 7} == {0, 4} and {pw.lk_pad_for(5) & 7, pw.lk_pad_for(10) & 7} == {0, 4}


def test_small_levels_are_there():
    narrow_vec = below_pad = double_fold = edge_only = False
    for c in pw.CASES:
        pad = pw.lk_pad_for(c[2])
        sizes = pw.levels_of(c)
        for (sw, sh), (w, h) in zip(sizes, sizes[1:]):
            narrow_vec |= w < pw.WALK_V
            edge_only |= not pw.fast_vectors(sw, pad)                 # a level no vector of which takes the fast form
        below_pad |= any(w < pad or h < pad for w, h in sizes)
        double_fold |= any(min(w, h) <= (pad + 1) // 2 for w, h in sizes)
    assert narrow_vec and below_pad and double_fold and edge_only
    assert pw.levels_of(pw.CASES[1])[-1] == (9, 7) and pw.levels_of(pw.CASES[2])[-1] == (18, 10)      # 142 x 78: 9 x 5 stops the chain
    assert any(h <= 2 for w, h in pw.HOST_ONLY_SIZES) and (1, 1) in pw.HOST_ONLY_SIZES
    assert {w for w, h in pw.HOST_ONLY_SIZES} >= {pw.WALK_SPAN - 1, pw.WALK_SPAN, pw.WALK_SPAN + 1, 2 * 4 - 2 + pw.WALK_LOAD - 1, 2 * 4 - 2 + pw.WALK_LOAD}


def test_inputs_and_routes():
    inputs = {c[5] for c in pw.CASES}
    assert inputs >= {"host", "dev+0", "dev+1", "dev+3", "dev+64"}
    assert {c[6].get("depth", 1) for c in pw.CASES if c[5].startswith("dev")} == {1, 2, 3}
    assert all(c[0] == "ahead" for c in pw.CASES) and pw.MANY_CASES and all(c[0] == "many" for c in pw.MANY_CASES)
    assert set(pw.ROW_EXTRA) == {0, 1, 3, 64}


# ---------------------------------------------------------------------------------------------------- the walk on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pyr_walk") / "pyr_walk_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "pyr_walk_host.cpp"), "-o", exe])
    return exe


def sizes_and_pads():
    """(w, h, pad, walk length) of every source level of the matrix, the host-only sizes at both vector origins and both walk
    lengths, and the bench image."""
    out = set()
    for c in ALL:
        pad = pw.lk_pad_for(c[2])
        out |= {(w, h, pad, pw.WALK_ROWS if l else pw.WALK_ROWS_INGEST) for l, (w, h) in enumerate(pw.levels_of(c)[:-1])}
    for w, h in pw.HOST_ONLY_SIZES + [(1241, 376)]:
        out |= {(w, h, pad, R) for pad in (12, 16, 28) for R in (pw.WALK_ROWS, pw.WALK_ROWS_INGEST)}
    return sorted(out)


def test_load_plan_stays_inside_the_image(host):
    assert (1241, 376, 28, pw.WALK_ROWS_INGEST) in sizes_and_pads()
    for w, h, pad, R in sizes_and_pads():
        r = subprocess.run([host, "plan", str(w), str(h), str(pad), str(R)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (w, h, pad, r.stderr)
        items, fast, loads, outside, min_x, max_x, min_r, max_r, d0, d2, z0, z2 = map(int, r.stdout.split())
        what = (w, h, pad, R, r.stdout.strip())
        assert items == pw.vectors((w + 1) // 2, pad) * -(-((h + 1) // 2) // R), what
        assert fast == len(pw.fast_vectors(w, pad)) * -(-((h + 1) // 2) // R), what
        assert loads > 0 and outside == 0 and 0 <= min_x <= max_x < w and 0 <= min_r <= max_r < h, what
        assert (d0, d2, z0, z2) == (0, 0, 0, 0), what


def chain(img, n):
    levels = [img]
    for _ in range(n):
        levels.append(ref.pyr_down(levels[-1]))
    return levels


@pytest.mark.parametrize("kind", ["random", "0-255"])
def test_host_walk_equals_the_reference(host, tmp_path, kind):
    rng = np.random.default_rng(7 if kind == "random" else 8)
    jobs = []
    for c in ALL:
        jobs.append((c[1], pw.lk_pad_for(c[2]), len(pw.levels_of(c)) - 1))
    jobs += [((w, h), pad, 2 if min(w, h) > 2 else 1) for w, h in pw.HOST_ONLY_SIZES for pad in (12, 16)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for k, ((w, h), pad, n) in enumerate(sorted(set(jobs))):
        img = rng.integers(0, 256, (h, w)).astype(np.uint8) if kind == "random" else (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        want = chain(img, n)
        for extra in pw.ROW_EXTRA if (w, h) != (1241, 376) else pw.ROW_EXTRA[k % 4:][:1]:
            buf = np.full((h, w + extra), 0x5A, np.uint8)
            buf[:, :w] = img
            with open(fin, "wb") as f:
                f.write(buf.tobytes()[:(h - 1) * (w + extra) + w])
            r = subprocess.run([host, "run", fin, fout, str(w), str(h), str(w + extra), str(pad), str(n)], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, ((w, h), pad, extra, "exit status", r.returncode, r.stderr)
            got = np.fromfile(fout, np.uint8)
            assert got.size == sum(lv.size for lv in want)
            o = 0
            for l, lv in enumerate(want):
                g = got[o:o + lv.size].reshape(lv.shape); o += lv.size
                bad = np.argwhere(g != lv)
                assert not len(bad), "%dx%d pad %d rows +%d %s: level %d: %d bytes differ, first (y, x) %s" % (w, h, pad, extra, kind, l, len(bad), bad[:4].tolist())
