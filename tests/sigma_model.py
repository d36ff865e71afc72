"""The definition of idn.estimate_sigma: numpy float64, no other imports.

skimage.restoration.estimate_sigma (unchanged between 0.14.2 and 0.18.3) of one channel plane is
median(|d|, d != 0) / norm.ppf(0.75) over d = pywt.dwtn(plane, 'db2')['dd'], the finest diagonal
detail band.  There is no img_as_float: the scale of the result is the scale of the input.  This
file restates pywt's arithmetic, tap order included, so that the result is bit-equal to the real
libraries (tests/golden/sigma.npz holds their values; tests/test_estimate_sigma.py compares) and
the kernel (csrc/estimate_sigma.hip) is bit-equal to this file.

Per plane p, taken as float64 (a uint8 value converts exactly, nothing is divided by 255):

  filter    g = pywt.Wavelet('db2').dec_hi
  transform one decimating high-pass along axis 0, then the same along axis 1 of that result.
            Along a length-n axis there are (n + 3) // 2 outputs; output o is centred at
            i = 2 o + 1 and is sum_j g[j] X(i - j) over the half-sample symmetric extension
            X(-1 - m) = x[m], X(n + m) = x[n - 1 - m]
  order     the sum starts from 0.0 and every step is one multiply, then one add (no FMA).  For
            i < n the taps go j = 0, 1, 2, 3.  For i >= n (the right overhang) the overhanging
            taps go first in descending order j = i - n, ..., 0, and the rest follow,
            j = i - n + 1, ..., 3.  Only i = n + 2 (odd n, the last output) differs from plain
            ascending order in its value: 2, 1, 0, 3
  keys      k = |d| over the coefficients that are not +-0.0
  result    median(k) / 0.6744897501960817, (a + b) / 2 for an even count, NaN for no key

A flat region of a nonzero value does not cancel to zero under this arithmetic (a constant 200
gives |d| ~ 1e-31) and every such position counts towards the rank; only true zeros drop out.
"""
import numpy as np

DEC_HI = (-0.48296291314453416, 0.8365163037378079, -0.2241438680420134, -0.12940952255126037)
PPF75 = 0.6744897501960817  # scipy.stats.norm.ppf(0.75)
MIN_SIDE = 4                # the symmetric extension reflects once


def tap_order(i, n):
    """the order in which output i = 2 o + 1 of a length-n axis adds its taps"""
    if i < n:
        return [0, 1, 2, 3]
    k = i - n
    return list(range(k, -1, -1)) + list(range(k + 1, 4))


def _extended(i, n):
    """index into x of X(i) for -n <= i < 2 n"""
    if i < 0:
        return -1 - i
    if i >= n:
        return 2 * n - 1 - i
    return i


def highpass_axis0(x):
    """the decimating db2 high-pass along axis 0 of a 2-D float64 array"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n < MIN_SIDE:
        raise ValueError(f"axis of length {n} < {MIN_SIDE}")
    out = np.empty(((n + 3) // 2,) + x.shape[1:], dtype=np.float64)
    for o in range(out.shape[0]):
        i = 2 * o + 1
        s = np.zeros(x.shape[1:], dtype=np.float64)
        for j in tap_order(i, n):
            s = s + DEC_HI[j] * x[_extended(i - j, n)]
        out[o] = s
    return out


def dd_band(plane):
    """pywt.dwtn(plane, 'db2')['dd'] of a 2-D array (uint8 or float64)"""
    p = np.asarray(plane).astype(np.float64)
    if p.ndim != 2:
        raise ValueError("dd_band takes one 2-D plane")
    v = highpass_axis0(p)
    return np.ascontiguousarray(highpass_axis0(np.ascontiguousarray(v.T)).T)


def keys(plane):
    """|d| over the coefficients of the dd band that are not +-0.0, in raster order"""
    d = dd_band(plane).ravel()
    return np.abs(d[d != 0.0])


def sigma_of_keys(k):
    k = np.sort(np.asarray(k, dtype=np.float64))
    m = k.size
    if m == 0:
        return np.float64(np.nan)
    a, b = k[(m - 1) // 2], k[m // 2]
    return np.float64((a + b) / 2.0) / np.float64(PPF75)


def plane_sigma(plane):
    return sigma_of_keys(keys(plane))


def estimate_sigma(x, average_sigmas=False):
    """skimage.restoration.estimate_sigma(x[i], multichannel=True, average_sigmas=...) per image of
    x, (N,)H,W,C: float64 (N, C) ((C,) for one image); (N,) (a numpy scalar) with average_sigmas"""
    x = np.asarray(x)
    one = x.ndim == 3
    xb = x[None] if one else x
    n, h, w, c = xb.shape
    out = np.empty((n, c), dtype=np.float64)
    for i in range(n):
        for ch in range(c):
            out[i, ch] = plane_sigma(xb[i, :, :, ch])
    if average_sigmas:
        out = average(out)
    return out[0] if one else out


def average(s):
    """numpy's mean over the last axis of 1 or 3 sigmas: ((s0 + s1) + s2) / 3"""
    s = np.asarray(s, dtype=np.float64)
    if s.shape[-1] == 1:
        return s[..., 0].copy()
    return ((s[..., 0] + s[..., 1]) + s[..., 2]) / 3.0
