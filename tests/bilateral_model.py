"""Host model of idn.bilateral_filter: OpenCV 3.4.2's bilateralFilter_8u with BORDER_CONSTANT 0,
restated in numpy float64 from the definition (not from oracle/filters.c).

cv2 is not importable where this project is built, so parity with cv2 itself is unpinned; this
model is the exact value the kernels (csrc/bilateral_u8.hip) and the fp32 oracle are held to.

  sigma_color, sigma_space <= 0 count as 1
  radius = d // 2 for d > 0, else int(rint(1.5 * sigma_space)) (half to even); at least 1
  taps   = {(i, j): i*i + j*j <= radius*radius}; pixels outside the image are 0 in every channel
  ws     = float32(exp((i*i + j*j) * -0.5 / sigma_space^2))
  wc     = float32(exp(dist^2 * -0.5 / sigma_color^2)),  dist = sum over channels |tap - centre|
  pre[c] = sum(ws * wc * tap[c]) / sum(ws * wc)           in float64
  out[c] = clip(rint(pre[c]), 0, 255)                     (cvRound: half to even)

`bilateral` returns pre, shape (N, H, W, C).  `rule` is the project's 1-LSB contract with pre as
the exact value.  The input families and the parameter tables below are shared by
tests/test_bilateral_model.py (CPU) and tests/test_bilateral_gpu.py, so that the oracle is
checked on exactly the inputs the kernels are."""
import functools

import numpy as np

MAX_RADIUS = 8  # idn_bilateral_u8 takes radius 1..8


def radius_of(d, sigma_space):
    """the window radius OpenCV derives from (d, sigma_space)"""
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    r = int(d) // 2 if d > 0 else int(np.rint(1.5 * ss))
    return max(r, 1)


def taps(radius):
    """the (i, j) offsets of the window, row-major"""
    return [(i, j) for i in range(-radius, radius + 1) for j in range(-radius, radius + 1)
            if i * i + j * j <= radius * radius]


def bilateral(img, d, sigma_color, sigma_space, drop=None):
    """float64 pre-round value of every output sample, shape (N, H, W, C).  img: uint8
    (N, H, W, C).  drop = (i, j) leaves that tap out (only for the tests' sensitivity proof)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 4
    n, h, w, c = img.shape
    sc = float(sigma_color) if sigma_color > 0 else 1.0
    ss = float(sigma_space) if sigma_space > 0 else 1.0
    r = radius_of(d, sigma_space)
    cw = np.exp(np.arange(255 * c + 1, dtype=np.float64) ** 2 * (-0.5 / (sc * sc)))
    cw = cw.astype(np.float32).astype(np.float64)
    centre = img.astype(np.int64)
    pad = np.zeros((n, h + 2 * r, w + 2 * r, c), np.int64)
    pad[:, r:r + h, r:r + w] = centre
    num = np.zeros((n, h, w, c), np.float64)
    den = np.zeros((n, h, w, 1), np.float64)
    for i, j in taps(r):
        if drop is not None and (i, j) == tuple(drop):
            continue
        ws = float(np.float32(np.exp((i * i + j * j) * (-0.5 / (ss * ss)))))
        nb = pad[:, r + i:r + i + h, r + j:r + j + w]
        wt = ws * cw[np.abs(nb - centre).sum(axis=3)][..., None]
        num += wt * nb
        den += wt
    return num / den


def to_u8(pre):
    return np.clip(np.rint(pre), 0, 255).astype(np.uint8)


# ---- the 1-LSB rule ------------------------------------------------------------------------------
BOUNDARY = 1e-3  # a differing byte's exact value lies this close to a half-integer
SHARE = 1e-3     # differing bytes per sample (at least 2 are allowed)


def rule(got, pre):
    """(violations, stats) of bytes `got` against the exact values `pre` (same shape; or lists of
    such arrays, pooled).  violations is a list of strings, empty when the rule holds:
      |got - rint(pre)| <= 1; every differing byte has pre within BOUNDARY of a half-integer;
      differing bytes number at most max(2, SHARE * samples)."""
    if isinstance(got, (list, tuple)):
        got = np.concatenate([np.asarray(g).ravel() for g in got])
        pre = np.concatenate([np.asarray(p).ravel() for p in pre])
    got = np.asarray(got)
    pre = np.asarray(pre, np.float64)
    assert got.shape == pre.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(np.int64) - to_u8(pre).astype(np.int64))
    mis = diff > 0
    frac = np.abs(pre - np.floor(pre) - 0.5)  # distance from the rounding boundary
    cap = max(2, SHARE * got.size)
    stats = {"samples": int(got.size), "mismatches": int(mis.sum()), "cap": cap,
             "max_diff": int(diff.max()) if got.size else 0,
             "max_boundary_dist": float(frac[mis].max()) if mis.any() else 0.0}
    bad = []
    if stats["max_diff"] > 1:
        bad.append(f"{int((diff > 1).sum())} bytes differ by more than 1 (max {stats['max_diff']})")
    off = int((frac[mis] >= BOUNDARY).sum())
    if off:
        bad.append(f"{off} differing bytes lie {stats['max_boundary_dist']:.3g} (max) from a "
                   f"rounding boundary, allowed < {BOUNDARY}")
    if stats["mismatches"] > cap:
        bad.append(f"{stats['mismatches']} differing bytes of {got.size}, allowed {cap:g}")
    return bad, stats


# ---- inputs --------------------------------------------------------------------------------------
FAMILIES = ("textured", "bytes", "saltpepper")


def make_input(family, shape, seed):
    """uint8 (N, H, W, C): 'textured' = conftest.textured (128 +- 64 +- 32); 'bytes' = i.i.d.
    0..255 (colour distances up to 765); 'saltpepper' = textured with 20 % zeros and 20 % 255,
    the first image with two bright rows and columns at its top left edge (against the zero
    border) and a black block"""
    from conftest import textured
    n, h, w, c = shape
    rs = np.random.RandomState(seed + 7919)
    if family == "textured":
        return textured(n, h, w, c=c, seed=seed)
    if family == "bytes":
        return rs.randint(0, 256, size=shape).astype(np.uint8)
    assert family == "saltpepper"
    img = textured(n, h, w, c=c, seed=seed)
    m = rs.random_sample(img.shape)
    img[m < 0.2] = 0
    img[(m >= 0.2) & (m < 0.4)] = 255
    img[0, :2] = 255
    img[0, :, :2] = 255
    img[0, h // 2:h // 2 + 5, w // 3:w // 3 + 9] = 0
    return img


def seed_of(family, shape, params):
    d, sc, ss = params
    return 1000 * FAMILIES.index(family) + 31 * (d + 2) + int(sc) + int(10 * ss) + sum(shape)


@functools.lru_cache(maxsize=None)
def case(family, shape, params):
    """(img, pre) of a case, computed once per process and shared read-only"""
    img = make_input(family, shape, seed_of(family, shape, params))
    pre = bilateral(img, *params)
    img.setflags(write=False)
    pre.setflags(write=False)
    return img, pre


# ---- parameter tables ----------------------------------------------------------------------------
WIDE = tuple((d, 200.0, 100.0) for d in (3, 5, 7, 9, 11, 13, 15, 17))        # radius 1..8
NARROW = ((7, 25.0, 3.0), (11, 50.0, 4.0), (15, 30.0, 5.0), (17, 20.0, 100.0))
SEAM_SHAPES = ((2, 33, 129, 3), (2, 33, 129, 1))  # odd w past a 128 tile, h past a 32-row tile
COLUMN_SHAPE = (2, 20, 1, 3)                      # w == 1: the generic 3-channel kernel
EVEN_D = ((1, 3), (2, 3), (4, 5), (6, 7), (10, 11), (12, 13), (16, 17))  # d, the odd d it equals
EVEN_SHAPES = ((1, 19, 70, 3), (1, 19, 70, 1))
EVEN_SIGMAS = (60.0, 3.0)
# (d, sigma_color, sigma_space), the radius OpenCV derives
DERIVED = (((0, 60.0, 1.0), 2), ((0, 60.0, 3.0), 4), ((0, 60.0, 3.4), 5), ((0, 60.0, 5.0), 8),
           ((-1, 60.0, 0.3), 1))
SIGMA_CLAMPS = ((5, 0.0, 0.0), (5, -1.0, -1.0))  # give the bytes of (5, 1, 1)
DERIVED_SHAPES = ((2, 19, 70, 3), (2, 19, 70, 1))
TINY_SHAPES = ((2, 3, 5), (1, 1, 2), (1, 2, 1), (3, 7, 2))  # (n, h, w), smaller than the window
TINY_D = (7, 11, 17)
PERSISTENT_HW = (4, 6)
PERSISTENT_D = (5, 9, 11)
BATCH_D = (7, 11, 17)
BATCH_SHAPES = ((3, 33, 129, 3), (3, 20, 70, 1))
PAD_CASES = ((3, 5), (3, 11), (3, 15), (1, 7))  # (C, d) on PAD_SHAPE with PADS extra row bytes
PAD_SHAPE = (2, 9, 70)
PADS = (1, 5, 8)
TUNING_D = (3, 5, 7, 9, 11)


def tuning_params(d):
    return ((d, 200.0, 100.0), (d, 30.0, 3.0))


def persistent_n(cus):
    return 5 * cus + 3


def all_cases(cus=256):
    """every (family, shape, params) that tests/test_bilateral_gpu.py holds against the model
    (the persistent-loop batch at a device of `cus` compute units)"""
    out = []
    for shape in SEAM_SHAPES:
        for p in WIDE + NARROW:
            out += [(f, shape, p) for f in FAMILIES]
    out += [("bytes", COLUMN_SHAPE, p) for p in WIDE[:5]]
    for shape in EVEN_SHAPES:
        for d, dd in EVEN_D:
            out += [("bytes", shape, (d,) + EVEN_SIGMAS)]
    for shape in DERIVED_SHAPES:
        out += [("saltpepper", shape, p) for p, _ in DERIVED]
        out += [("textured", shape, (5, 1.0, 1.0))]
    for c in (1, 3):
        for n, h, w in TINY_SHAPES:
            for d in TINY_D:
                out += [(f, (n, h, w, c), (d, 200.0, 100.0)) for f in ("bytes", "saltpepper")]
    out += [("bytes", (persistent_n(cus),) + PERSISTENT_HW + (3,), (d, 200.0, 100.0))
            for d in PERSISTENT_D]
    for shape in BATCH_SHAPES:
        out += [("saltpepper", shape, (d, 75.0, 75.0)) for d in BATCH_D]
    out += [("bytes", PAD_SHAPE + (c,), (d, 200.0, 100.0)) for c, d in PAD_CASES]
    for d in TUNING_D:
        for p in tuning_params(d):
            out += [(f, SEAM_SHAPES[0], p) for f in FAMILIES]
    return list(dict.fromkeys(out))
