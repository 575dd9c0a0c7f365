"""numpy restatement of the input formats of include/svo.h (svo_set_input_format): the grey image of a frame in one of the seven
formats, and the inverse direction the tests need — frames in every format that hold a given scene.

    grey = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14        

for the colour formats (alpha ignored); the Y byte for the two YUV 4:2:2 packings (UYVY: byte 2x + 1 of the row, YUY2: byte 2x)."""
import numpy as np

FORMATS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8", "yuv422", "yuv422_yuy2")
BPP = dict(mono8=1, bgr8=3, rgb8=3, bgra8=4, rgba8=4, yuv422=2, yuv422_yuy2=2)
WB, WG, WR, ROUND, SHIFT = 1868, 9617, 4899, 8192, 14


def to_grey(frame, fmt):
    """frame: (H, W) for mono8, else (H, W, BPP[fmt]) uint8 -> (H, W) uint8."""
    a = np.asarray(frame)
    assert a.dtype == np.uint8 and fmt in FORMATS, (a.dtype, fmt)
    if fmt == "mono8":
        assert a.ndim == 2, a.shape
        return a.copy()
    assert a.ndim == 3 and a.shape[2] == BPP[fmt], (a.shape, fmt)
    if fmt == "yuv422":
        return a[:, :, 1].copy()
    if fmt == "yuv422_yuy2":
        return a[:, :, 0].copy()
    c = a.astype(np.int64)
    b, g, r = (c[:, :, 0], c[:, :, 1], c[:, :, 2]) if fmt in ("bgr8", "bgra8") else (c[:, :, 2], c[:, :, 1], c[:, :, 0])
    return ((b * WB + g * WG + r * WR + ROUND) >> SHIFT).astype(np.uint8)


def colour_of(a, fmt, rng):
    """A frame in `fmt` made from the grey scene a: B = a, G = a rolled one row, R = 255 - a; alpha and the chroma bytes are
    random, so that a wrong byte pick or weight order shows.  The YUV frames carry the BGR frame's grey value as Y, so every
    format of one scene converts to the same grey image except through a wrong kernel.  -> (frame, its grey image)."""
    a = np.asarray(a, np.uint8)
    bgr = np.ascontiguousarray(np.stack([a, np.roll(a, 1, 0), 255 - a], -1))
    grey = to_grey(bgr, "bgr8")
    noise = rng.integers(0, 256, a.shape).astype(np.uint8)
    if fmt == "mono8":
        out = grey.copy()
    elif fmt == "bgr8":
        out = bgr
    elif fmt == "rgb8":
        out = np.ascontiguousarray(bgr[:, :, ::-1])
    elif fmt == "bgra8":
        out = np.ascontiguousarray(np.concatenate([bgr, noise[..., None]], -1))
    elif fmt == "rgba8":
        out = np.ascontiguousarray(np.concatenate([bgr[:, :, ::-1], noise[..., None]], -1))
    elif fmt == "yuv422":
        out = np.ascontiguousarray(np.stack([noise, grey], -1))
    elif fmt == "yuv422_yuy2":
        out = np.ascontiguousarray(np.stack([grey, noise], -1))
    else:
        raise ValueError(fmt)
    assert np.array_equal(to_grey(out, fmt), grey)
    return out, grey
