"""The definition of idn.wiener: scipy.signal.wiener on every channel plane of a uint8 image, with
the window sums carried as integers so that every value has one bit pattern.

For a sample x and its kh x kw window (both odd, n = kh*kw):
  S1 = sum t, S2 = sum t^2 over the taps, integers; a tap outside the image is 0 under
       border="zero" (scipy's correlate(..., 'same')) and the mirrored sample under
       border="reflect101" (np.pad(mode="reflect"), cv2's default border)
  m = float64(S1) / n
  v = float64(S2) / n - m*m            (the product rounds, then the difference)
  noise: given per (image, channel), or float64(Q) / float64(n*n*H*W) with the exact integer
         Q = sum over the plane of (n*S2 - S1*S1)  (scipy's mean(lVar) without its rounding order)
  r = m where v == 0, else m where v < noise, else (x - m) * (1 - noise / v) + m
out="f64" is r, out="u8" is clip(rint(r), 0, 255) (round half to even; r lies between m and x).
v == 0 -> m is the one departure from scipy, which returns NaN there when noise is 0 as well.
"""
import numpy as np

BORDERS = ("zero", "reflect101")
Q_MAX_PLANE = 1 << 28  # samples per plane for which Q stays below 2^64


def _ksize(ksize):
    kh, kw = (ksize, ksize) if np.isscalar(ksize) else ksize
    kh, kw = int(kh), int(kw)
    if not (1 <= kh <= 31 and 1 <= kw <= 31 and kh % 2 == 1 and kw % 2 == 1):
        raise ValueError(f"window sides must be odd and in 1..31, got {ksize!r}")
    return kh, kw


def window_sums(plane, ksize, border="zero"):
    """(S1, S2) of a 2-D uint8 plane as int64 arrays of its shape, from integer integral images"""
    kh, kw = _ksize(ksize)
    p = np.asarray(plane)
    if p.dtype != np.uint8 or p.ndim != 2:
        raise ValueError("a 2-D uint8 plane is expected")
    h, w = p.shape
    rh, rw = kh // 2, kw // 2
    if border == "zero":
        e = np.pad(p.astype(np.int64), ((rh, rh), (rw, rw)), mode="constant")
    elif border == "reflect101":
        if rh >= h or rw >= w:
            raise ValueError("reflect101 needs kh//2 < H and kw//2 < W")
        e = np.pad(p.astype(np.int64), ((rh, rh), (rw, rw)), mode="reflect")
    else:
        raise ValueError(f"unknown border {border!r}")

    def box(a):
        ii = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
        ii[1:, 1:] = a.cumsum(0).cumsum(1)
        return ii[kh:, kw:] - ii[:-kh, kw:] - ii[kh:, :-kw] + ii[:-kh, :-kw]

    return box(e), box(e * e)


def q_sum(s1, s2, n):
    """Q = sum (n*S2 - S1*S1) as a Python int (every term is in 0 .. 961^2 * 65025)"""
    if s1.size > Q_MAX_PLANE:
        raise ValueError("plane too large for the 64-bit Q")
    terms = n * s2 - s1 * s1
    assert terms.min() >= 0
    return int(terms.astype(np.uint64).sum(dtype=np.uint64))


def estimate_noise(plane, ksize, border="zero"):
    """the noise scipy would estimate (noise=None), as float64(Q) / float64(n*n*H*W)"""
    kh, kw = _ksize(ksize)
    s1, s2 = window_sums(plane, (kh, kw), border)
    n = kh * kw
    h, w = s1.shape
    return np.float64(float(q_sum(s1, s2, n))) / np.float64(float(n * n * h * w))


def stats(plane, ksize, border="zero"):
    """(m, v) of a plane, float64"""
    kh, kw = _ksize(ksize)
    s1, s2 = window_sums(plane, (kh, kw), border)
    n = np.float64(kh * kw)
    m = s1.astype(np.float64) / n
    v = s2.astype(np.float64) / n - m * m
    return m, v


def wiener_plane(plane, ksize, noise=None, border="zero"):
    """(r float64, noise used) of one 2-D uint8 plane"""
    m, v = stats(plane, ksize, border)
    nz = estimate_noise(plane, ksize, border) if noise is None else np.float64(noise)
    x = np.asarray(plane).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = x - m
        res = res * (1.0 - nz / v)
        res = res + m
        r = np.where(v == 0, m, np.where(v < nz, m, res))
    return r, nz


def to_u8(r):
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def wiener(x, ksize=3, noise=None, border="zero", out="u8", return_noise=False):
    """idn.wiener on a numpy uint8 array (N,)H,W,C.  noise: None, a number, C numbers, or an array
    (C,) / (N, C).  Returns the result (uint8 or float64, x's shape) and, with return_noise, the
    float64 (N, C) ((C,) for one image) noise used."""
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim not in (3, 4):
        raise ValueError("uint8 (N,)H,W,C expected")
    if out not in ("u8", "f64"):
        raise ValueError(f"out must be 'u8' or 'f64', got {out!r}")
    xb = x[None] if x.ndim == 3 else x
    n, h, w, c = xb.shape
    nz = None if noise is None else np.broadcast_to(np.asarray(noise, np.float64), (n, c))
    res = np.empty(xb.shape, np.float64)
    used = np.empty((n, c), np.float64)
    for i in range(n):
        for ch in range(c):
            res[i, ..., ch], used[i, ch] = wiener_plane(
                xb[i, ..., ch], ksize, None if nz is None else nz[i, ch], border)
    y = to_u8(res) if out == "u8" else res
    if x.ndim == 3:
        y, used = y[0], used[0]
    return (y, used) if return_noise else y


def smooth_image(h=96, w=128):
    """the clean test image: clip(rint(96 + 64 sin(x/17) cos(y/23) + 60 ((x//32 + y//32) % 2)))"""
    y, x = np.mgrid[0:h, 0:w]
    v = 96 + 64 * np.sin(x / 17) * np.cos(y / 23) + 60 * ((x // 32 + y // 32) % 2)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def noisy_image(clean, sd=15.0, seed=0):
    """clean (H,W) replicated to three channels plus rint(N(0, sd)) from default_rng(seed)"""
    c3 = np.repeat(np.asarray(clean)[..., None], 3, axis=2)
    g = np.random.default_rng(seed).normal(0.0, sd, c3.shape)
    return np.clip(c3.astype(np.float64) + np.rint(g), 0, 255).astype(np.uint8)


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10.0 * np.log10(65025.0 / np.mean(d * d))
