#!/usr/bin/env python3
"""Generates the colour fixture of BASELINE.json configs[0] (`vo 400 run1`) from the reference's bundled data set.
Data only — no reference source is copied:
  * run1_bgr_{left,right}_<first>_<last>.npy.xz : all 128 stereo pairs as the reference CLI feeds them to stereo_callback —
    512x288 8-bit BGR, interleaved (cv::imread default, main.cpp:38-46) — in chunks of 8 frames, each an xz-compressed .npy
    of shape (8, 288, 512, 3) (delta + LZMA2 filters, so that every file stays under 1 MiB; tests/golden_run1.py reads them);
  * run1_recorded.npz : ALL rows of run1/result.csv (the trajectory the reference recorded, 6 significant digits) and of
    run1/gt.csv.
usage: python tests/golden/make_run1_color_fixture.py <the reference's run1/ directory>
"""
import glob
import lzma
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
N, CHUNK, LIMIT = 128, 8, 1 << 20
FILTERS = [{"id": lzma.FILTER_DELTA, "dist": 3}, {"id": lzma.FILTER_LZMA2, "preset": 9 | lzma.PRESET_EXTREME}]


def bgr(path):
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[..., ::-1])


def main(ref):
    for old in glob.glob(os.path.join(HERE, "run1_bgr_*.npy.xz")):
        os.remove(old)
    for cam in ("left", "right"):
        for a in range(0, N, CHUNK):
            b = min(N, a + CHUNK) - 1
            frames = np.stack([bgr("%s/%s/frame%06d.png" % (ref, cam, i)) for i in range(a, b + 1)])
            out = os.path.join(HERE, "run1_bgr_%s_%03d_%03d.npy.xz" % (cam, a, b))
            with lzma.open(out, "wb", format=lzma.FORMAT_XZ, filters=FILTERS) as f:
                np.save(f, frames, allow_pickle=False)
            assert os.path.getsize(out) < LIMIT, (out, os.path.getsize(out))
            print(out, os.path.getsize(out), frames.shape)
    res = np.loadtxt(ref + "/result.csv", delimiter=",", skiprows=1)
    gt = np.loadtxt(ref + "/gt.csv", delimiter=",", skiprows=1)
    out = os.path.join(HERE, "run1_recorded.npz")
    np.savez_compressed(out, result_csv=res, gt_csv=gt, result_header="x,y,z,gtx,gty", gt_header="time,x,y,dx,dy")
    print(out, os.path.getsize(out), res.shape, gt.shape)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1].rstrip("/"))
