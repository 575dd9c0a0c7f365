#!/usr/bin/env python3
"""Generates tests/golden/run1_frames_0_7.npz from the reference's bundled data set (run1/, the input of
BASELINE.json configs[0] `vo 400 run1`).  Data only — no reference source is copied:
  * left/right frames 0..7 (512x288 RGB PNG) decoded with PIL and converted to 8-bit gray with OpenCV's
    BGR2GRAY integer formula: (B*1868 + G*9617 + R*4899 + 8192) >> 14;
  * rows 0..7 of run1/result.csv (the trajectory the reference recorded) and of run1/gt.csv.
The .npz members are LZMA-compressed (np.load reads them like any .npz), so that the file stays under 1 MiB.
usage: python tests/golden/make_run1_fixture.py <the reference's run1/ directory>
"""
import io
import os
import sys
import zipfile

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "run1_frames_0_7.npz")


def gray(path):
    a = np.asarray(Image.open(path).convert("RGB")).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def main(REF):
    n = 8
    left = np.stack([gray("%s/left/frame%06d.png" % (REF, i)) for i in range(n)])
    right = np.stack([gray("%s/right/frame%06d.png" % (REF, i)) for i in range(n)])
    res = np.loadtxt(REF + "/result.csv", delimiter=",", skiprows=1)[:n]
    gt = np.loadtxt(REF + "/gt.csv", delimiter=",", skiprows=1)[:n]
    arrays = dict(left=left, right=right, result_csv=res, gt_csv=gt, result_header=np.array("x,y,z,gtx,gty"),
                  gt_header=np.array("time,x,y,dx,dy"))
    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_LZMA) as z:
        for name, a in arrays.items():
            b = io.BytesIO()
            np.save(b, a, allow_pickle=False)
            z.writestr(name + ".npy", b.getvalue())
    print(OUT, os.path.getsize(OUT), left.shape)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1].rstrip("/"))
