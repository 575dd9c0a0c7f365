"""Reader of the committed colour fixture of the reference's run1/ set (tests/golden/run1_bgr_<cam>_<first>_<last>.npy.xz,
written by tests/golden/make_run1_color_fixture.py): 512x288 8-bit interleaved BGR stereo pairs, in chunks of frames."""
import glob
import lzma
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_FRAMES = 128


def bgr_frames(n=48):
    """The first n stereo pairs -> (left, right), each an (n, 288, 512, 3) uint8 array."""
    assert 0 < n <= N_FRAMES, n
    out = []
    for cam in ("left", "right"):
        parts, have = [], 0
        for p in sorted(glob.glob(os.path.join(GOLD, "run1_bgr_%s_*.npy.xz" % cam))):
            if have >= n:
                break
            with lzma.open(p, "rb") as f:
                parts.append(np.load(f, allow_pickle=False))
            have += len(parts[-1])
        assert have >= n, "tests/golden holds %d %s frames of run1, %d asked for" % (have, cam, n)
        out.append(np.concatenate(parts)[:n])
    return out[0], out[1]
