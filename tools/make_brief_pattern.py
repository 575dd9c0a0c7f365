#!/usr/bin/env python3
"""Writes stereo_visual_odometry_amd/csrc/svo_brief_pattern.hpp: the 256 point pairs of the library's steered BRIEF descriptor
(include/svo.h, "Binary descriptors").

The pattern is the project's own, not OpenCV's learned ORB table.  Both points of a test are drawn from an isotropic Gaussian with
sigma = 31 / 5 pixels (BRIEF's G-II sampling, Calonder et al. 2010), rounded to integers and rejected outside the disc of radius 13
(x^2 + y^2 <= 169: the rotated point must keep its 5 x 5 box inside the 31 x 31 patch); a test with a == b, or one already drawn,
is rejected too.

Everything is integer arithmetic, so the table regenerates byte for byte on any machine:
  * the generator is a 64-bit linear congruential generator (Knuth's MMIX constants), seeded with SEED; a draw is its top 16 bits;
  * a standard normal deviate is the sum of twelve draws minus its mean (Irwin-Hall: variance 12 * 65536^2 / 12), so a coordinate is
    round(s * 31 / (5 * 65536)) of that sum s, rounded half away from zero with integer division.

    python tools/make_brief_pattern.py            # rewrite the header
    python tools/make_brief_pattern.py --check    # exit status 1 if the committed header differs
"""
import os
import sys

SEED = 0x5356304252494546          # "SV0BRIEF" in ASCII
N_TESTS = 256
R2_MAX = 169
MASK = (1 << 64) - 1
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo_visual_odometry_amd", "csrc", "svo_brief_pattern.hpp")


class Lcg:
    def __init__(self, seed):
        self.s = seed & MASK

    def u16(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & MASK
        return self.s >> 48


def coordinate(rng):
    s = sum(rng.u16() for _ in range(12)) - 6 * 65536      # N(0, 65536^2), to Irwin-Hall's accuracy
    num, den = abs(s) * 31 * 2 + 5 * 65536, 2 * 5 * 65536  # |s| * 31 / (5 * 65536) + 1/2, floored
    v = num // den
    return v if s >= 0 else -v


def point(rng):
    while True:
        x, y = coordinate(rng), coordinate(rng)
        if x * x + y * y <= R2_MAX:
            return x, y


def pattern():
    rng = Lcg(SEED)
    tests, seen = [], set()
    while len(tests) < N_TESTS:
        a, b = point(rng), point(rng)
        t = a + b
        if a == b or t in seen:
            continue
        seen.add(t)
        tests.append(t)
    return tests


def header_text():
    lines = [
        "// svo_brief_pattern.hpp — the 256 tests (ax, ay, bx, by) of the steered BRIEF descriptor (include/svo.h, \"Binary descriptors\").",
        "// WRITTEN BY tools/make_brief_pattern.py — do not edit; tests/test_descriptor_ref.py regenerates it and compares the bytes.",
        "// The project's own table: Gaussian point pairs (sigma = 31 / 5) inside the disc of radius 13, not OpenCV's learned ORB pattern.",
        "#pragma once",
        "#define SVO_BRIEF_TESTS %d" % N_TESTS,
        "#define SVO_BRIEF_PATTERN_VALUES \\",
    ]
    tests = pattern()
    for i in range(0, N_TESTS, 4):
        row = ",  ".join("%3d,%3d,%3d,%3d" % t for t in tests[i:i + 4])
        lines.append("    %s%s" % (row, ", \\" if i + 4 < N_TESTS else ""))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv[1:]:
        same = os.path.exists(OUT) and open(OUT, encoding="utf-8").read() == text
        print("svo_brief_pattern.hpp is %s" % ("up to date" if same else "STALE"))
        sys.exit(0 if same else 1)
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text)
    print("wrote %s" % OUT)
