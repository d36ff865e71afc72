"""The numpy model of idn's exposure correction: cvt_color_yuv, equalize_hist, clahe and the tone
part of correct_exposure (Automold's exposure_process before its non-local means).

The arithmetic is OpenCV 3.4's 8-bit code as recalled, written out in include/idn.h next to the
entry points; cv2 is not importable here, so parity with cv2 itself is unpinned and this model
defines the result.  The kernels of csrc/exposure.hip are tested against it bit for bit
(tests/test_exposure_gpu.py).  Every function takes one image: a (H, W) uint8 plane or a (H, W, 3)
uint8 BGR / YUV image.
"""
import numpy as np

F32 = np.float32
CLIP_LIMIT = 2.0      # exposure_process: createCLAHE(clipLimit=2.0, tileGridSize=(4, 4))
TILE_GRID = (4, 4)
TONE_ABOVE = 150      # luma strictly above this is scaled by 0.85


def _descale(v):
    return (v + 8192) >> 14  # arithmetic shift on numpy's signed integers


def _sat(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def bgr2yuv(x):
    """cv2.cvtColor(x, COLOR_BGR2YUV) on 8 bits"""
    b, g, r = (x[..., k].astype(np.int64) for k in range(3))
    y = _descale(1868 * b + 9617 * g + 4899 * r)
    u = _descale((b - y) * 8061 + (128 << 14))
    v = _descale((r - y) * 14369 + (128 << 14))
    return np.stack([_sat(y), _sat(u), _sat(v)], axis=-1)


def yuv2bgr(x):
    """cv2.cvtColor(x, COLOR_YUV2BGR) on 8 bits"""
    y = x[..., 0].astype(np.int64)
    u = x[..., 1].astype(np.int64) - 128
    v = x[..., 2].astype(np.int64) - 128
    b = y + _descale(33292 * u)
    g = y + _descale(-6472 * u - 9519 * v)
    r = y + _descale(18678 * v)
    return np.stack([_sat(b), _sat(g), _sat(r)], axis=-1)


def tone(y):
    """exposure_process's luma step: trunc(Y * 0.85) in float64 where Y > 150, as integers"""
    y = y.astype(np.int64)
    return np.where(y > TONE_ABOVE, (17 * y) // 20, y).astype(np.uint8)


def tone_float(y):
    """the same step as the reference writes it: a float64 product stored into uint8"""
    ones = np.ones(y.shape)
    ones[y > TONE_ABOVE] = 0.85
    return (y * ones).astype(np.uint8)


def _lut_from_sums(sums, scale):
    """sat(rne((float)sums * scale)): float32 product, round half to even"""
    return _sat(np.rint(sums.astype(F32) * F32(scale)).astype(np.int64))


def equalize_lut(hist, total):
    """cv2.equalizeHist's table from the image's 256-bin histogram"""
    hist = np.asarray(hist, np.int64)
    i0 = int(np.flatnonzero(hist)[0])
    if hist[i0] == total:
        return np.full(256, i0, np.uint8)
    scale = F32(255.0) / F32(total - hist[i0])
    sums = np.cumsum(hist) - hist[i0]  # sum over i0 < k <= i; bins below i0 are empty
    lut = _lut_from_sums(np.maximum(sums, 0), scale)
    lut[:i0 + 1] = 0
    return lut


def equalize_hist(x):
    hist = np.bincount(x.ravel(), minlength=256)
    return equalize_lut(hist, x.size)[x]


def clahe_extent(h, w, tiles_x, tiles_y):
    """(Hext, Wext): the image as CLAHE tiles it.  Both pads are applied whenever either dimension
    fails to divide, so a dimension that divides grows by a whole tile count (OpenCV's behaviour)"""
    if w % tiles_x == 0 and h % tiles_y == 0:
        return h, w
    return h + (tiles_y - h % tiles_y), w + (tiles_x - w % tiles_x)


def clahe_clip(clip_limit, area):
    if clip_limit == 0:
        return 0
    return max(int(float(clip_limit) * area / 256), 1)


def clip_histogram(hist, clip):
    """clip, spread the excess evenly, then the residual rule: one more count in every step-th bin"""
    h = np.asarray(hist, np.int64).copy()
    if clip <= 0:
        return h
    excess = int(np.maximum(h - clip, 0).sum())
    h = np.minimum(h, clip)
    h += excess // 256
    r = excess % 256
    if r > 0:
        step = max(256 // r, 1)
        i = 0
        while i < 256 and r > 0:
            h[i] += 1
            r -= 1
            i += step
    return h


def clahe_tables(x, clip_limit=CLIP_LIMIT, tile_grid=TILE_GRID):
    """((tiles_y, tiles_x, 256) uint8 tables, tile_h, tile_w) of one plane"""
    tiles_x, tiles_y = tile_grid
    h, w = x.shape
    assert h > tiles_y and w > tiles_x
    hext, wext = clahe_extent(h, w, tiles_x, tiles_y)
    ext = np.pad(x, ((0, hext - h), (0, wext - w)), mode="reflect")  # BORDER_REFLECT_101
    th, tw = hext // tiles_y, wext // tiles_x
    area = th * tw
    scale = F32(255.0) / F32(area)
    clip = clahe_clip(clip_limit, area)
    luts = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for j in range(tiles_y):
        for i in range(tiles_x):
            tile = ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            hist = clip_histogram(np.bincount(tile.ravel(), minlength=256), clip)
            luts[j, i] = _lut_from_sums(np.cumsum(hist), scale)
    return luts, th, tw


def _interp_axis(n, tile, tiles):
    """(first tile, second tile, weight of the second, weight of the first) along one axis"""
    f = np.arange(n).astype(F32) * (F32(1.0) / F32(tile)) - F32(0.5)
    t1 = np.floor(f).astype(np.int64)
    a = (f - t1.astype(F32)).astype(F32)
    a1 = (F32(1.0) - a).astype(F32)
    t2 = np.minimum(t1 + 1, tiles - 1)
    t1 = np.maximum(t1, 0)
    return t1, t2, a, a1


def clahe_apply(x, luts, th, tw):
    tiles_y, tiles_x = luts.shape[:2]
    h, w = x.shape
    ty1, ty2, ya, ya1 = _interp_axis(h, th, tiles_y)
    tx1, tx2, xa, xa1 = _interp_axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = (v[:, None] for v in (ty1, ty2, ya, ya1))
    tx1, tx2, xa, xa1 = (v[None, :] for v in (tx1, tx2, xa, xa1))
    l11 = luts[ty1, tx1, x].astype(F32)
    l12 = luts[ty1, tx2, x].astype(F32)
    l21 = luts[ty2, tx1, x].astype(F32)
    l22 = luts[ty2, tx2, x].astype(F32)
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya  # every step rounds to fp32
    assert res.dtype == F32
    return _sat(np.rint(res).astype(np.int64))


def clahe(x, clip_limit=CLIP_LIMIT, tile_grid=TILE_GRID):
    """cv2.createCLAHE(clip_limit, tile_grid).apply(x), tile_grid = (tiles_x, tiles_y)"""
    luts, th, tw = clahe_tables(x, clip_limit, tile_grid)
    return clahe_apply(x, luts, th, tw)


def exposure_tone(x):
    """exposure_process up to and including COLOR_YUV2BGR (before fastNlMeansDenoisingColored)"""
    yuv = bgr2yuv(x)
    y = tone(yuv[..., 0])
    y = clahe(y, CLIP_LIMIT, TILE_GRID)
    y = equalize_hist(y)
    y = clahe(y, CLIP_LIMIT, TILE_GRID)
    yuv[..., 0] = y
    return yuv2bgr(yuv)


# ---- the issue's formula inputs ----------------------------------------------------------------------

def plane(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return ((37 * y + 11 * x + ((y * x) % 17) * 5) % 256).astype(np.uint8)


def bgr(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(90 + 5 * y + ((x * y) % 7) * 3) % 256,
                     (40 + 6 * x + (y % 5) * 4) % 256,
                     (200 - 3 * y + 2 * x + ((x + y) % 3) * 9) % 256], axis=-1).astype(np.uint8)
