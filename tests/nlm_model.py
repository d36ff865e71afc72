"""Host model of idn.nl_means: OpenCV 3.4's 8-bit non-local means (fastNlMeansDenoising,
fast_nlmeans_denoising_invoker.hpp with DistSquared, IT = int, WT = int) restated in numpy.

cv2 is not importable where this project is built, so parity with cv2 itself is unpinned; this
model is the contract the kernel (csrc/nlmeans.hip) is held to bit for bit.

  fpm    = INT_MAX // (s*s*255)                      fixed-point weight of an identical patch
  shift  = smallest p with 2^p >= t*t;  mult = 2^shift / (t*t)
  wt[a]  = rint(fpm * exp(-(a*mult) / (h*h*C))), 0 where below 0.001*fpm;  a < int(65025*C/mult + 1)
  E      = the image padded by t//2 + s//2 with BORDER_REFLECT_101
  per pixel p and each of the s*s offsets o:  ssd = sum over the t x t template and the channels
  of (E[p+q] - E[p+o+q])^2;  w = wt[ssd >> shift];  wsum += w;  est[c] += w * E[p+o][c]
  out[c] = min(255, (est[c] + wsum//2) // wsum)

`nl_means` is the vectorised form (one pass per offset, the box sum from a 2-D cumulative sum);
`nl_means_direct` is the five-loop definition, for small images only."""
import functools
import math

import numpy as np

INT_MAX = 2 ** 31 - 1


def params(t, s):
    """(fpm, shift, mult) of a template size t and a search size s"""
    if not (t % 2 == 1 and 3 <= t <= 7 and s % 2 == 1 and 5 <= s <= 21):
        raise ValueError(f"template {t} / search {s}: odd sizes in 3..7 / 5..21")
    fpm = min(INT_MAX // (s * s * 255), INT_MAX)
    shift = 0
    while (1 << shift) < t * t:
        shift += 1
    return fpm, shift, (1 << shift) / (t * t)


@functools.lru_cache(maxsize=None)
def weights(h, c, t, s):
    """(nonzero prefix of the weight table as int64, full table length, shift, fpm).  exp is libm's
    (math.exp), evaluated per entry; the tail behind the prefix is checked to be all zero."""
    if not h > 0:
        raise ValueError("h must be positive")
    fpm, shift, mult = params(t, s)
    n = int(255 * 255 * c / mult + 1)
    den = float(h) * float(h) * c
    thr = 0.001 * fpm
    wt = []
    for a in range(n):
        w = round(fpm * math.exp(-(a * mult) / den))  # round(): half to even, like rint
        if w < thr:
            break
        wt.append(w)
    tail = np.rint(fpm * np.exp(-(np.arange(len(wt), n) * mult) / den))
    assert np.all(tail < thr), "the table is a nonzero prefix followed by zeros"
    wt = np.array(wt, dtype=np.int64)
    assert len(wt) >= 1 and wt[0] == fpm and np.all(np.diff(wt) <= 0)
    wt.setflags(write=False)
    return wt, n, shift, fpm


def _check(img, t, s):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (1, 3):
        raise ValueError("expected a uint8 (H, W, C) image with C in {1, 3}")
    b = t // 2 + s // 2
    if min(img.shape[:2]) < b + 1:
        raise ValueError(f"image {img.shape[:2]} smaller than {b + 1}")
    return img, b


def _finish(est, wsum, fpm, s):
    assert est.max() <= s * s * fpm * 255 <= INT_MAX
    assert wsum.min() >= fpm
    return np.minimum(255, (est + (wsum // 2)[..., None]) // wsum[..., None]).astype(np.uint8)


def nl_means(img, h=3.0, t=7, s=21, return_wsum=False):
    """vectorised model of one (H, W, C) uint8 image"""
    img, b = _check(img, t, s)
    H, W, C = img.shape
    tr, sr = t // 2, s // 2
    wt, _, shift, fpm = weights(float(h), C, t, s)
    nw = len(wt)
    E = np.pad(img.astype(np.int64), ((b, b), (b, b), (0, 0)), mode="reflect")
    A = E[sr:sr + H + 2 * tr, sr:sr + W + 2 * tr]          # every pixel a template touches
    est = np.zeros((H, W, C), np.int64)
    wsum = np.zeros((H, W), np.int64)
    cs = np.zeros((H + 2 * tr + 1, W + 2 * tr + 1), np.int64)
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            B = E[sr + dy:sr + dy + H + 2 * tr, sr + dx:sr + dx + W + 2 * tr]
            d = A - B
            cs[1:, 1:] = np.cumsum(np.cumsum((d * d).sum(axis=2), axis=0), axis=1)
            ssd = cs[t:, t:] - cs[:-t, t:] - cs[t:, :-t] + cs[:-t, :-t]
            idx = ssd >> shift
            w = np.where(idx < nw, wt[np.minimum(idx, nw - 1)], 0)
            wsum += w
            est += w[..., None] * E[b + dy:b + dy + H, b + dx:b + dx + W]
    out = _finish(est, wsum, fpm, s)
    return (out, wsum) if return_wsum else out


def nl_means_direct(img, h=3.0, t=7, s=21):
    """the definition, loop by loop (pixel, offset, template, channel); small images only"""
    img, b = _check(img, t, s)
    H, W, C = img.shape
    tr, sr = t // 2, s // 2
    wt, n, shift, fpm = weights(float(h), C, t, s)
    full = np.zeros(n, np.int64)
    full[:len(wt)] = wt
    E = np.pad(img.astype(np.int64), ((b, b), (b, b), (0, 0)), mode="reflect")
    est = np.zeros((H, W, C), np.int64)
    wsum = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            for dy in range(-sr, sr + 1):
                for dx in range(-sr, sr + 1):
                    ssd = 0
                    for qy in range(-tr, tr + 1):
                        for qx in range(-tr, tr + 1):
                            for c in range(C):
                                d = int(E[b + y + qy, b + x + qx, c]) - int(E[b + y + dy + qy, b + x + dx + qx, c])
                                ssd += d * d
                    w = int(full[ssd >> shift])
                    wsum[y, x] += w
                    for c in range(C):
                        est[y, x, c] += w * int(E[b + y + dy, b + x + dx, c])
    return _finish(est, wsum, fpm, s)


def nl_means_batch(x, h=3.0, t=7, s=21):
    return np.stack([nl_means(im, h, t, s) for im in x])


def changed_share(x, y):
    """share of bytes in which two arrays differ"""
    return float(np.mean(np.asarray(x) != np.asarray(y)))


# ---- the inputs of the GPU cases (tests/test_nlmeans_gpu.py) -------------------------------------

def flat_noisy(h, w, c=3, level=120, sd=6.0, seed=7):
    rs = np.random.RandomState(seed)
    return np.clip(np.rint(level + rs.normal(0.0, sd, (h, w, c))), 0, 255).astype(np.uint8)


def steps(h, w, c=3, sd=4.0, seed=9):
    """steps of 32 every 8 columns (wrapping below 256) plus N(0, sd)"""
    rs = np.random.RandomState(seed)
    base = ((np.arange(w) // 8) * 32 % 224 + 16)[None, :, None]
    return np.clip(np.rint(base + rs.normal(0.0, sd, (h, w, c))), 0, 255).astype(np.uint8)


def checkerboard(h, w, c=3):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], c, axis=2)
