"""numpy restatement of the derivative planes the many-sequence grey contexts keep beside every pyramid (k_deriv_levels writes them,
the LK kernel loads them at the levels >= 1), written from the definition and not from the kernel's column sums: what
cv::buildOpticalFlowPyramid stores with withDerivatives = true (calcScharrDeriv on the level with its REFLECT_101 border, derivBorder =
BORDER_CONSTANT), at 4 x the Scharr value.  int64 arithmetic, so the library must equal it sample for sample.

- scharr4: pad the level by one pixel with REFLECT_101, correlate with the full 3x3 kernels 4 Scharr_x and 4 Scharr_y.
- planes: the two results embedded in zero arrays of (h + 2 pad, w + 2 pad) int16, as svo_get_derivatives returns them.
- CASES: the matrix tests/test_gpu_deriv_planes.py runs; tests/test_deriv_ref.py guards what it covers on the CPU."""
import numpy as np

import pyramid_ref

KX = np.array([[-12, 0, 12], [-40, 0, 40], [-12, 0, 12]], np.int64)      # 4 x [[-3 0 3] [-10 0 10] [-3 0 3]]
KY = KX.T.copy()
BOUND = 16320                                                            # 255 * (12 + 40 + 12)


def scharr4(level):
    """(Ix, Iy) of one level, int64 (h, w): 4 x the Scharr derivatives of the level on a REFLECT_101 border."""
    level = np.asarray(level, np.uint8)
    h, w = level.shape
    p = pyramid_ref.padded(level, 1).astype(np.int64)
    ix, iy = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for r in range(3):
        for c in range(3):
            win = p[r:r + h, c:c + w]
            ix += KX[r, c] * win
            iy += KY[r, c] * win
    assert np.abs(ix).max() <= BOUND and np.abs(iy).max() <= BOUND, "a derivative left int16's range"
    return ix, iy


def planes(level, pad):
    """(Ix, Iy) as they are stored: int16 (h + 2 pad, w + 2 pad), zero outside the level."""
    h, w = np.asarray(level).shape
    out = []
    for d in scharr4(level):
        a = np.zeros((h + 2 * pad, w + 2 * pad), np.int16)
        a[pad:pad + h, pad:pad + w] = d
        out.append(a)
    return out[0], out[1]


# --------------------------------------------------------------------------------------------------------------- the case matrix
# ((w, h), win, max_level, n_seq, input, extra, the levels >= 1 the stop rule builds): every case is a grey context of 9 .. 12 sequences
# in the exact-sums mode (the contexts that keep planes).  input = host | pinned | dev+K (device frames, rows K bytes wider);
# extra: depth (frames in flight, device inputs), frames, mask (the frame a third of the sequences sit out), reset (sequence 1 is reset
# before the masked frame, which it sits out: refused until the frame after), rect, fmt (input format), clahe.
CASES = [
    ((134, 70), 5, 3, 12, "pinned", {"frames": 5, "mask": 2, "reset": 1}, [(67, 35), (34, 18), (17, 9)]),
    ((130, 66), 5, 5, 10, "dev+3", {"frames": 5, "depth": 2, "mask": 2}, [(65, 33), (33, 17), (17, 9)]),
    ((128, 64), 7, 2, 9, "host", {"frames": 3, "fmt": "bgr8"}, [(64, 32), (32, 16)]),
    ((258, 97), 10, 3, 9, "dev+1", {"frames": 5, "depth": 3}, [(129, 49), (65, 25), (33, 13)]),
    ((300, 129), 21, 1, 9, "host", {"frames": 3, "rect": 1}, [(150, 65)]),
    ((419, 201), 7, 5, 10, "dev+0", {"frames": 3, "depth": 1}, [(210, 101), (105, 51), (53, 26), (27, 13)]),
    ((255, 129), 15, 4, 9, "host", {"frames": 3, "clahe": 1}, [(128, 65), (64, 33), (32, 17)]),
    ((520, 96), 31, 1, 11, "pinned", {"frames": 4, "mask": 2}, [(260, 48)]),
    ((1241, 376), 21, 4, 9, "host", {"frames": 2}, [(621, 188), (311, 94), (156, 47), (78, 24)]),      # the bench shape
]


def case_id(c):
    (w, h), win, ml, B, inp, ex, _ = c
    return "%dx%d-w%d-l%d-B%d-%s%s" % (w, h, win, ml, B, inp, "".join("-%s%s" % kv for kv in sorted(ex.items())))
