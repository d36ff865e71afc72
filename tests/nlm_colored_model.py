"""Host model of idn.nl_means_colored: OpenCV 3.4's cv2.fastNlMeansDenoisingColored for CV_8UC3,
restated in numpy.

  lab = cvtColor(src, COLOR_LBGR2Lab)                      lbgr2lab
  L'  = fastNlMeansDenoising(lab[..., 0:1], h, t, s)       nl_means_c, C = 1
  ab' = fastNlMeansDenoising(lab[..., 1:3], hColor, t, s)  nl_means_c, C = 2 (a, b jointly)
  dst = cvtColor(merge(L', ab'), COLOR_Lab2LBGR)           lab2lbgr

The two conversions are oracle/cvlab.py's integer RGB2Lab_b / Lab2RGBinteger with OpenCV's linear
gamma tables in place of the sRGB ones: linearGammaTab_b[i] = i << 3 on the way in,
linearInvGammaTab_b[v] = (255 * v) >> 12 on the way out (both recalled from initLabTabs()).  The
non-local means is the scheme of tests/nlm_model.py for any channel count; its weight tables and
constants come from there.  cv2 is not importable where this project is built, so parity with cv2
itself is unpinned; this model is the contract the kernels are held to bit for bit."""
import numpy as np

import nlm_model as nm
from oracle import cvlab


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def lbgr2lab(img):
    """cv2.cvtColor(img, COLOR_LBGR2Lab) for uint8 BGR (..., 3)"""
    t = cvlab.tables()
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    B, G, R = (a[..., k].astype(np.int64) << cvlab.GAMMA_SHIFT for k in range(3))
    C, cb = t["c_fwd"], t["cbrt_b"]
    fX = cb[_descale(B * C[0] + G * C[1] + R * C[2], cvlab.LAB_SHIFT)]
    fY = cb[_descale(B * C[3] + G * C[4] + R * C[5], cvlab.LAB_SHIFT)]
    fZ = cb[_descale(B * C[6] + G * C[7] + R * C[8], cvlab.LAB_SHIFT)]
    s2 = cvlab.LAB_SHIFT2
    Lscale = (116 * 255 + 50) // 100
    Lshift = -((16 * 255 * (1 << s2) + 50) // 100)
    L = _descale(Lscale * fY + Lshift, s2)
    aa = _descale(500 * (fX - fY) + 128 * (1 << s2), s2)
    bb = _descale(200 * (fY - fZ) + 128 * (1 << s2), s2)
    return np.stack([np.clip(v, 0, 255) for v in (L, aa, bb)], axis=-1).astype(np.uint8)


def lab2lbgr(lab):
    """cv2.cvtColor(lab, COLOR_Lab2LBGR) for uint8 Lab (..., 3)"""
    t = cvlab.tables()
    a = np.asarray(lab)
    assert a.dtype == np.uint8 and a.shape[-1] == 3
    L, A, Bv = (a[..., k].astype(np.int64) for k in range(3))
    y, ify = t["y_b"][L], t["ify_b"][L]
    base = cvlab.BASE
    adiv = A * base // 500 - 128 * base // 500
    bdiv = Bv * base // 200 - 128 * base // 200
    x = t["ab_to_xz"][ify + adiv - cvlab.MIN_AB]
    z = t["ab_to_xz"][ify - bdiv - cvlab.MIN_AB]
    C = t["c_inv"]
    out = []
    for row in (2, 1, 0):  # B, G, R rows of the XYZ -> RGB matrix
        v = _descale(C[row * 3] * x + C[row * 3 + 1] * y + C[row * 3 + 2] * z, cvlab.LAB_SHIFT + 2)
        v = np.clip(v, 0, cvlab.INV_GAMMA_TAB_SIZE - 1)
        out.append((255 * v) >> 12)
    return np.stack(out, axis=-1).astype(np.uint8)


def nl_means_c(img, h, t=7, s=21):
    """tests/nlm_model.py's vectorised scheme for a uint8 (H, W, C) image of any channel count"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("expected a uint8 (H, W, C) image")
    H, W, C = img.shape
    tr, sr = t // 2, s // 2
    b = tr + sr
    if min(H, W) < b + 1:
        raise ValueError(f"image {(H, W)} smaller than {b + 1}")
    wt, _, shift, fpm = nm.weights(float(h), C, t, s)
    nw = len(wt)
    E = np.pad(img.astype(np.int64), ((b, b), (b, b), (0, 0)), mode="reflect")
    A = E[sr:sr + H + 2 * tr, sr:sr + W + 2 * tr]
    est = np.zeros((H, W, C), np.int64)
    wsum = np.zeros((H, W), np.int64)
    cs = np.zeros((H + 2 * tr + 1, W + 2 * tr + 1), np.int64)
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            d = A - E[sr + dy:sr + dy + H + 2 * tr, sr + dx:sr + dx + W + 2 * tr]
            cs[1:, 1:] = np.cumsum(np.cumsum((d * d).sum(axis=2), axis=0), axis=1)
            ssd = cs[t:, t:] - cs[:-t, t:] - cs[t:, :-t] + cs[:-t, :-t]
            idx = ssd >> shift
            w = np.where(idx < nw, wt[np.minimum(idx, nw - 1)], 0)
            wsum += w
            est += w[..., None] * E[b + dy:b + dy + H, b + dx:b + dx + W]
    assert est.max() <= s * s * fpm * 255 <= nm.INT_MAX and wsum.min() >= fpm
    return np.minimum(255, (est + (wsum // 2)[..., None]) // wsum[..., None]).astype(np.uint8)


def nl_means_c_direct(img, h, t=7, s=21):
    """the definition, loop by loop (pixel, offset, template, channel), any C; small images only"""
    img = np.asarray(img)
    H, W, C = img.shape
    tr, sr = t // 2, s // 2
    b = tr + sr
    wt, n, shift, fpm = nm.weights(float(h), C, t, s)
    full = np.zeros(n, np.int64)
    full[:len(wt)] = wt
    E = np.pad(img.astype(np.int64), ((b, b), (b, b), (0, 0)), mode="reflect")
    out = np.zeros((H, W, C), np.uint8)
    for y in range(H):
        for x in range(W):
            wsum, est = 0, [0] * C
            for dy in range(-sr, sr + 1):
                for dx in range(-sr, sr + 1):
                    ssd = 0
                    for qy in range(-tr, tr + 1):
                        for qx in range(-tr, tr + 1):
                            for c in range(C):
                                d = int(E[b + y + qy, b + x + qx, c]) - \
                                    int(E[b + y + dy + qy, b + x + dx + qx, c])
                                ssd += d * d
                    w = int(full[ssd >> shift])
                    wsum += w
                    for c in range(C):
                        est[c] += w * int(E[b + y + dy, b + x + dx, c])
            for c in range(C):
                out[y, x, c] = min(255, (est[c] + wsum // 2) // wsum)
    return out


def nl_means_colored(img, h=3.0, h_color=3.0, t=7, s=21, return_lab=False):
    """model of one (H, W, 3) uint8 BGR image; return_lab: also the Lab image before and after"""
    lab = lbgr2lab(img)
    den = np.concatenate([nl_means_c(lab[..., 0:1], h, t, s), nl_means_c(lab[..., 1:3], h_color, t, s)],
                         axis=2)
    out = lab2lbgr(den)
    return (out, lab, den) if return_lab else out


def nl_means_colored_batch(x, h=3.0, h_color=3.0, t=7, s=21):
    return np.stack([nl_means_colored(im, h, h_color, t, s) for im in x])
