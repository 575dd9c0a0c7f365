"""tests/clahe_ref.py (the numpy restatement of the CLAHE section of include/svo.h) against cases small enough to check by hand, and
against an independent scalar-loop implementation kept in this file (plain Python numbers, f32 rounding through struct)."""
import struct

import numpy as np

import clahe_ref as ref


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def scalar_clahe(img, clip_limit, tiles):
    """The definition with loops and Python numbers only: nothing shared with clahe_ref."""
    h, w = len(img), len(img[0])
    tx_n, ty_n = tiles
    ew, eh = w, h
    if w % tx_n or h % ty_n:
        ew, eh = w + tx_n - w % tx_n, h + ty_n - h % ty_n
    r101 = lambda i, n: i if i < n else 2 * n - 2 - i
    tw, th = ew // tx_n, eh // ty_n
    area = tw * th
    lut = {}
    for ty in range(ty_n):
        for tx in range(tx_n):
            hist = [0] * 256
            for y in range(ty * th, (ty + 1) * th):
                for x in range(tx * tw, (tx + 1) * tw):
                    hist[img[r101(y, h)][r101(x, w)]] += 1
            if clip_limit > 0:
                clip = max(int(clip_limit * area / 256.0), 1)
                clipped = 0
                for i in range(256):
                    if hist[i] > clip:
                        clipped += hist[i] - clip; hist[i] = clip
                batch, residual = clipped // 256, clipped % 256
                hist = [v + batch for v in hist]
                if residual > 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        hist[i] += 1; i += step; residual -= 1
            scale = f32(255.0 / area)
            s, row = 0, []
            for i in range(256):
                s += hist[i]
                row.append(min(max(int(round(f32(f32(s) * scale))), 0), 255))
            lut[ty, tx] = row
    inv_tw, inv_th = f32(1.0 / tw), f32(1.0 / th)
    out = [[0] * w for _ in range(h)]
    for y in range(h):
        tyf = f32(f32(y * inv_th) - 0.5)
        ty1 = int(np.floor(tyf)); ya = f32(tyf - ty1); ya1 = f32(1.0 - ya)
        ty2 = min(ty1 + 1, ty_n - 1); ty1 = max(ty1, 0)
        for x in range(w):
            txf = f32(f32(x * inv_tw) - 0.5)
            tx1 = int(np.floor(txf)); xa = f32(txf - tx1); xa1 = f32(1.0 - xa)
            tx2 = min(tx1 + 1, tx_n - 1); tx1 = max(tx1, 0)
            v = img[y][x]
            top = f32(f32(lut[ty1, tx1][v] * xa1) + f32(lut[ty1, tx2][v] * xa))
            bot = f32(f32(lut[ty2, tx1][v] * xa1) + f32(lut[ty2, tx2][v] * xa))
            res = f32(f32(top * ya1) + f32(bot * ya))
            out[y][x] = min(max(int(round(res)), 0), 255)
    return np.array(out, np.uint8)


def test_one_tile_without_clipping_is_plain_equalisation():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (12, 20)).astype(np.uint8)
    img[:3] //= 4                                                     # a lopsided histogram
    cdf = np.cumsum(np.bincount(img.reshape(-1), minlength=256))
    lut = np.clip(np.rint(cdf.astype(np.float32) * (np.float32(255.0) / np.float32(img.size))), 0, 255).astype(np.uint8)
    assert np.array_equal(ref.luts(img, 0, (1, 1))[0, 0], lut)
    assert np.array_equal(ref.clahe_ref(img, 0, (1, 1)), lut[img])     # one tile: all four taps are the same LUT, the weights sum to 1
    assert np.array_equal(ref.clahe_ref(img, -3.0, (1, 1)), lut[img])  # clip_limit <= 0: no clipping


def test_constant_image_lut_by_hand():
    # 16 x 16 pixels of value 100, one tile, clip_limit 2: area = 256, clip = max((int)(2 * 256 / 256), 1) = 2.
    # hist[100] = 256 is cut to 2: clipped = 254, batch = 254 / 256 = 0, residual = 254, step = max(256 / 254, 1) = 1, so the loop
    # adds 1 to bins 0 .. 253.  hist = 1 on 0 .. 253 except hist[100] = 3, and 0 on 254, 255 (sum 256).  Running sum: i + 1 below 100,
    # i + 3 on 100 .. 253, 256 on 254 and 255; lut = rint(sum * 255 / 256).
    img = np.full((16, 16), 100, np.uint8)
    s = np.array([i + 1 if i < 100 else (i + 3 if i <= 253 else 256) for i in range(256)])
    want = np.rint(s.astype(np.float32) * (np.float32(255) / np.float32(256))).astype(np.uint8)
    assert want[100] == 103 and want[0] == 1 and want[255] == 255     # 103 * 255 / 256 = 102.6; 1 * 255 / 256 = 0.996
    assert np.array_equal(ref.luts(img, 2.0, (1, 1))[0, 0], want)
    assert np.array_equal(ref.clahe_ref(img, 2.0, (1, 1)), np.full((16, 16), 103, np.uint8))
    # without clipping every sum from bin 100 on is the area: the image maps to 255
    assert np.array_equal(ref.clahe_ref(img, 0, (1, 1)), np.full((16, 16), 255, np.uint8))


IMG8 = np.array([
    [10, 10, 20, 20, 200, 200, 210, 210],
    [10, 30, 20, 40, 200, 220, 210, 230],
    [50, 50, 60, 60, 240, 240, 250, 250],
    [50, 70, 60, 80, 240, 255, 250, 0],
    [5, 15, 25, 35, 45, 55, 65, 75],
    [85, 95, 105, 115, 125, 135, 145, 155],
    [165, 175, 185, 195, 205, 215, 225, 235],
    [245, 255, 0, 128, 128, 128, 64, 64]], np.uint8)
# scalar_clahe(IMG8, 0, (2, 2)), typed in
OUT8 = np.array([
    [48, 48, 96, 76, 160, 112, 112, 112],
    [48, 112, 96, 100, 160, 160, 112, 143],
    [175, 175, 223, 171, 223, 207, 239, 239],
    [151, 199, 187, 167, 227, 255, 243, 12],
    [16, 48, 80, 74, 60, 50, 48, 56],
    [136, 148, 160, 147, 130, 138, 135, 147],
    [175, 191, 207, 215, 215, 223, 239, 255],
    [239, 255, 16, 155, 151, 147, 64, 64]], np.uint8)


def test_literal_8x8_two_by_two_tiles():
    assert np.array_equal(scalar_clahe(IMG8.tolist(), 0, (2, 2)), OUT8)
    assert np.array_equal(ref.clahe_ref(IMG8, 0, (2, 2)), OUT8)
    # by hand: a corner pixel lies in the outer half of its tile and reads that tile's LUT alone.  Pixel (0, 0) = 10: three of the
    # 16 pixels of tile (0, 0) are <= 10 -> rint(3 * 255 / 16) = rint(47.8) = 48.  Pixel (7, 7) = 64 of tile (1, 1): four of 16
    # pixels (45, 55, 64, 64) are <= 64 -> rint(4 * 15.9375) = 64.
    assert OUT8[0, 0] == 48 and OUT8[7, 7] == 64


def test_scalar_loops_agree_on_clipped_odd_sizes():
    rng = np.random.default_rng(2)
    for (w, h), tiles, clip in [((13, 9), (3, 2), 2.0), ((16, 11), (4, 4), 0.01), ((11, 7), (2, 3), 40.0), ((9, 9), (3, 3), 1.5)]:
        img = rng.integers(0, 256, (h, w)).astype(np.uint8)
        img[: h // 2] = (img[: h // 2] // 32) * 3                       # a few heavy bins, so that clipping cuts something
        assert np.array_equal(ref.clahe_ref(img, clip, tiles), scalar_clahe(img.tolist(), clip, tiles)), (w, h, tiles, clip)


def test_padding_quirk_extends_a_divisible_width_by_a_whole_tile_count():
    assert ref.geometry(320, 160, (8, 8)) == (320, 160, 40, 20)
    assert ref.geometry(320, 163, (8, 8)) == (328, 168, 41, 21)         # w divisible, h not: ext_w = w + tiles_x
    assert ref.geometry(323, 160, (8, 8)) == (328, 168, 41, 21)
    assert ref.geometry(323, 163, (8, 8)) == (328, 168, 41, 21)
    assert ref.geometry(37, 21, (16, 16)) == (48, 32, 3, 2)
    assert ref.geometry(8, 9, (8, 8)) is None                            # the width would grow by 8 > w - 1
    assert ref.geometry(4, 4, (8, 8)) is None
    # the extension is REFLECT_101: with one tile column the tile's histogram counts the mirrored columns
    img = np.arange(20, dtype=np.uint8).reshape(4, 5) * 10               # 5 x 4, tiles (2, 2): ext 6 x 6 (the quirk adds two rows), tiles 3 x 3
    assert ref.geometry(5, 4, (2, 2)) == (6, 6, 3, 3)
    L = ref.luts(img, 0, (2, 2))
    right_top = np.concatenate([img[:3, 3:5].reshape(-1), img[:3, 3]])  # rows 0 .. 2 of columns 3, 4 and of column 5 = the mirrored column 3
    cdf = np.cumsum(np.bincount(right_top, minlength=256))
    assert np.array_equal(L[0, 1], np.rint(cdf.astype(np.float32) * (np.float32(255) / np.float32(9))).astype(np.uint8))
    left_bottom = np.concatenate([img[3, :3], img[2, :3], img[1, :3]])  # row 3, then rows 4 and 5 = the mirrored rows 2 and 1
    cdf = np.cumsum(np.bincount(left_bottom, minlength=256))
    assert np.array_equal(L[1, 0], np.rint(cdf.astype(np.float32) * (np.float32(255) / np.float32(9))).astype(np.uint8))


def test_tiny_clip_limit_reaches_the_floor_of_one():
    assert ref.clip_of(0.01, 40 * 20) == 1 and ref.clip_of(1e-9, 4) == 1 and ref.clip_of(2.0, 800) == 6 and ref.clip_of(0, 800) == 0
    # clip = 1 on a 16 x 16 one-tile image of two values (128 pixels each): both bins are cut to 1, clipped = 254, residual = 254,
    # step = 1: bins 0 .. 253 get + 1 -> hist = 1 everywhere on 0 .. 253 but 2 on the two values
    img = np.zeros((16, 16), np.uint8); img[:, 8:] = 200
    s = np.cumsum([0 if i > 253 else (2 if i in (0, 200) else 1) for i in range(256)])
    want = np.rint(s.astype(np.float32) * (np.float32(255) / np.float32(256))).astype(np.uint8)
    assert np.array_equal(ref.luts(img, 0.001, (1, 1))[0, 0], want)
