"""numpy restatement of the CLAHE section of include/svo.h (svo_set_clahe / svo_clahe): cv::CLAHE::apply for 8-bit images as that
section defines it, rule by rule.  The GPU tests pin the kernels to this file bit for bit; tests/test_clahe_ref.py pins this file
to hand-checkable cases.

    geometry(w, h, tiles)          rule 1: (ext_w, ext_h, tw, th), or None when the rule rejects the geometry
    tile_lut(hist, area, clip)     rules 2 and 3 for one tile's histogram
    luts(img, clip_limit, tiles)   (tiles_y, tiles_x, 256) uint8
    clahe_ref(img, ...)            the equalised image"""
import numpy as np

F = np.float32


def geometry(w, h, tiles):
    tx, ty = tiles
    ew, eh = w, h
    if w % tx != 0 or h % ty != 0:
        ex, ey = tx - w % tx, ty - h % ty          # a divisible dimension is extended by a whole tiles_* (OpenCV's quirk)
        if ex > w - 1 or ey > h - 1:               # REFLECT_101 is undefined there
            return None
        ew, eh = w + ex, h + ey
    tw, th = ew // tx, eh // ty
    if tw == 0 or th == 0:
        return None
    return ew, eh, tw, th


def clip_of(clip_limit, area):
    """rule 2's integer clip, or 0 for no clipping."""
    if not clip_limit > 0:
        return 0
    return max(int(float(clip_limit) * area / 256.0), 1)


def tile_lut(hist, area, clip):
    """hist: 256 counts that sum to area -> 256 uint8 (rules 2 and 3)."""
    hist = np.array(hist, np.int64)
    if clip > 0:
        clipped = int(np.maximum(hist - clip, 0).sum())
        hist = np.minimum(hist, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        hist += batch
        if residual > 0:
            step = max(256 // residual, 1)
            i = 0
            while i < 256 and residual > 0:
                hist[i] += 1
                i += step
                residual -= 1
    scale = F(255.0) / F(area)
    s = np.cumsum(hist)
    return np.clip(np.rint(s.astype(F) * scale), 0, 255).astype(np.uint8)


def luts(img, clip_limit, tiles):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    g = geometry(w, h, tiles)
    assert g is not None, "rule 1 rejects %dx%d with tiles %s" % (w, h, tiles)
    ew, eh, tw, th = g
    ext = np.pad(img, ((0, eh - h), (0, ew - w)), mode="reflect") if (ew, eh) != (w, h) else img    # numpy's reflect is REFLECT_101
    area = tw * th
    clip = clip_of(clip_limit, area)
    out = np.zeros((tiles[1], tiles[0], 256), np.uint8)
    for ty in range(tiles[1]):
        for tx in range(tiles[0]):
            t = ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            out[ty, tx] = tile_lut(np.bincount(t.reshape(-1), minlength=256), area, clip)
    return out


def clahe_ref(img, clip_limit=2.0, tiles=(8, 8)):
    img = np.asarray(img)
    L = luts(img, clip_limit, tiles)
    h, w = img.shape
    _, _, tw, th = geometry(w, h, tiles)
    inv_tw, inv_th = F(1.0) / F(tw), F(1.0) / F(th)

    def axis(n, inv, nt):
        f = np.arange(n).astype(F) * inv - F(0.5)
        t1 = np.floor(f)
        a = f - t1
        a1 = F(1.0) - a
        t1 = t1.astype(np.int64)
        return np.maximum(t1, 0), np.minimum(t1 + 1, nt - 1), a, a1
    tx1, tx2, xa, xa1 = axis(w, inv_tw, tiles[0])
    ty1, ty2, ya, ya1 = axis(h, inv_th, tiles[1])
    assert xa.dtype == F and ya1.dtype == F
    v = img.astype(np.int64)
    look = lambda ty, tx: L[ty[:, None], tx[None, :], v].astype(F)
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (look(ty1, tx1) * xa1 + look(ty1, tx2) * xa) * ya1 + (look(ty2, tx1) * xa1 + look(ty2, tx2) * xa) * ya
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)
