"""numpy restatement of the image pyramids the frame pipeline keeps, written independently of the HIP code: the level chain of
cv::buildOpticalFlowPyramid (withDerivatives = false, pyrBorder = BORDER_REFLECT_101) and the REFLECT_101 border stored
around every level.  Integer arithmetic only, so the library must equal it byte for byte.

- pyr_down: cv::pyrDown, the separable [1 4 6 4 1] kernel on REFLECT_101 source borders, (sum + 128) >> 8, destination
  ((w + 1) / 2, (h + 1) / 2).
- pyramid: level 0 = the image; no next level once (w + 1) / 2 <= win or (h + 1) / 2 <= win; at most max_level levels after
  level 0 (capped by SVO_MAX_LEVELS).
- padded: one level with `pad` border pixels on every side, each from the iterated cv::borderInterpolate(BORDER_REFLECT_101)
  — a single rule for the whole pad, also where the pad is wider than the level.
- For interleaved BGR frames one pyramid per colour plane; raw frames are rectified first (rectify_ref.remap)."""
import numpy as np

SVO_MAX_LEVELS = 8
KERNEL = (1, 4, 6, 4, 1)


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) on an int array: the rule repeats with period 2n - 2."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    j = np.mod(i, p)
    return np.where(j < n, j, p - j)


def pyr_down(img):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    src = img.astype(np.int64)
    xs, ys = 2 * np.arange(dw), 2 * np.arange(dh)
    rows = np.zeros((h, dw), np.int64)
    for k, c in enumerate(KERNEL):
        rows += c * src[:, reflect101(xs + k - 2, w)]
    acc = np.zeros((dh, dw), np.int64)
    for k, c in enumerate(KERNEL):
        acc += c * rows[reflect101(ys + k - 2, h), :]
    return ((acc + 128) >> 8).astype(np.uint8)


def level_sizes(w, h, win, max_level):
    """[(w, h)] of every level the stop rule builds."""
    out = [(w, h)]
    for _ in range(min(max_level, SVO_MAX_LEVELS - 1)):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
        out.append((w, h))
    return out


def pyramid(img, win, max_level):
    """Levels of one single-channel image."""
    img = np.asarray(img, np.uint8)
    levels = [img]
    for _ in level_sizes(img.shape[1], img.shape[0], win, max_level)[1:]:
        levels.append(pyr_down(levels[-1]))
    return levels


def pyramids(frame, win, max_level, maps=None):
    """[plane][level] of one frame: (H, W) grey or (H, W, 3) interleaved BGR; maps = (map1, map2): a RAW frame, rectified first."""
    frame = np.asarray(frame, np.uint8)
    if maps is not None:
        import rectify_ref
        frame = rectify_ref.remap(frame, *maps)
    planes = [frame] if frame.ndim == 2 else [frame[:, :, c] for c in range(frame.shape[2])]
    return [pyramid(np.ascontiguousarray(p), win, max_level) for p in planes]


def padded(level, pad):
    """The level with its REFLECT_101 border: (h + 2 pad, w + 2 pad)."""
    h, w = level.shape
    return level[np.ix_(reflect101(np.arange(-pad, h + pad), h), reflect101(np.arange(-pad, w + pad), w))]


# The shapes the pyramid tests run (tests/test_pyramid_ref.py on the CPU, tests/test_gpu_pyramids.py through the library).  Between
# them their level chains hold every level width residue mod 4, levels narrower and shorter than the pad, and levels no wider or
# taller than (pad + 1) / 2, where the left / top border needs a second fold.
SHAPES = [(417, 203), (418, 202), (419, 201), (420, 200), (1241, 376), (255, 129), (130, 66), (165, 83), (90, 46), (67, 35)]
WINDOWS = [5, 7, 10, 15, 21, 31]
