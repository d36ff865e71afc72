"""The definition of idn.blur and idn.gaussian_blur at every odd window 3..31 (numpy, integers).

Both work per channel plane under BORDER_REFLECT_101, the reflection repeated until the index is
inside the image (cv::borderInterpolate), so images smaller than the radius are legal.

Box.  S = the sum of the k x k window; the result is (2 S + k^2) // (2 k^2).  k^2 is odd, so
S / k^2 is never a tie: cv2.blur's value whichever rounding it applies.  The sums here come from an
integral image, not from the oracle.

Gaussian.  Q8 taps t[0..k-1], unsigned integers that sum to 256 (gaussian_taps), and
(sum_i sum_j t[i] t[j] x[y+i-r, x+j-r] + 32768) >> 16.
  sigma <= 0 and k in {3, 5, 7}: OpenCV's fixed dyadic kernels, cv2.GaussianBlur(x, (k, k), 0) bit
    for bit.
  otherwise s = sigma, or 0.3 * ((k - 1) * 0.5 - 1) + 0.8 for sigma <= 0; g[i] = exp(-(i - k//2)^2
    / (2 s^2)) in float64, t = rint(256 g / sum(g)), and 256 - sum(t) goes to the centre tap.
    This model, not cv2, is the definition there: OpenCV does not renormalise its rounded taps.
A constant image comes back unchanged, a row pass fits 16 bits and the full sum 32 bits.
"""
import numpy as np

MAX_KSIZE = 31
SMALL = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}


def check_ksize(k):
    k = int(k)
    if not (3 <= k <= MAX_KSIZE and k % 2 == 1):
        raise ValueError(f"ksize must be odd and in 3..{MAX_KSIZE}, got {k}")
    return k


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) for an integer array i"""
    i = np.asarray(i, np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)


def pad101(plane, r):
    """the plane extended by r samples on every side"""
    h, w = plane.shape
    ys = reflect101(np.arange(-r, h + r), h)
    xs = reflect101(np.arange(-r, w + r), w)
    return np.asarray(plane)[np.ix_(ys, xs)]


def gaussian_weights(ksize, sigma=0.0):
    """256 v[i] in float64, before rounding (None for the dyadic kernels)"""
    k = check_ksize(ksize)
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma < 0:
        raise ValueError(f"sigma must be finite and >= 0, got {sigma}")
    if sigma <= 0 and k in SMALL:
        return None
    s = sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    d = np.arange(k, dtype=np.float64) - (k // 2)
    with np.errstate(all="ignore"):
        g = np.exp(-(d * d) / (2.0 * s * s))
    g[k // 2] = 1.0
    return 256.0 * (g / g.sum())


def gaussian_taps(ksize, sigma=0.0):
    """uint16 taps that sum to 256"""
    k = check_ksize(ksize)
    v = gaussian_weights(k, sigma)
    if v is None:
        return np.array(SMALL[k], np.uint16)
    t = np.rint(v).astype(np.int64)
    t[k // 2] += 256 - int(t.sum())
    assert t.min() >= 0 and t.sum() == 256
    return t.astype(np.uint16)


def _planes(x):
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim not in (3, 4):
        raise ValueError("uint8 (N,)H,W,C expected")
    return x[None] if x.ndim == 3 else x


def box_sum(plane, ksize):
    """int64 window sums of a 2-D plane from an integral image"""
    k = check_ksize(ksize)
    e = pad101(plane, k // 2).astype(np.int64)
    ii = np.zeros((e.shape[0] + 1, e.shape[1] + 1), np.int64)
    ii[1:, 1:] = e.cumsum(0).cumsum(1)
    return ii[k:, k:] - ii[:-k, k:] - ii[k:, :-k] + ii[:-k, :-k]


def blur(x, ksize=3):
    k = check_ksize(ksize)
    xb = _planes(x)
    out = np.empty_like(xb)
    for i in range(xb.shape[0]):
        for ch in range(xb.shape[3]):
            s = box_sum(xb[i, :, :, ch], k)
            out[i, :, :, ch] = (2 * s + k * k) // (2 * k * k)
    return out[0] if np.asarray(x).ndim == 3 else out


def gaussian_plane(plane, taps):
    t = np.asarray(taps, np.int64)
    k = t.size
    h, w = plane.shape
    e = pad101(plane, k // 2).astype(np.int64)
    rows = sum(t[j] * e[:, j:j + w] for j in range(k))          # (h + 2r, w), <= 255 * 256
    assert rows.max(initial=0) <= 65280
    full = sum(t[i] * rows[i:i + h, :] for i in range(k))       # <= 255 * 65536
    return ((full + 32768) >> 16).astype(np.uint8)


def gaussian_blur(x, ksize=5, sigma=0.0):
    t = gaussian_taps(ksize, sigma)
    xb = _planes(x)
    out = np.empty_like(xb)
    for i in range(xb.shape[0]):
        for ch in range(xb.shape[3]):
            out[i, :, :, ch] = gaussian_plane(xb[i, :, :, ch], t)
    return out[0] if np.asarray(x).ndim == 3 else out
