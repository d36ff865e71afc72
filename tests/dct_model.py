"""The definition of idn.denoise_dct: the sliding 8x8 DCT hard-threshold denoiser (Yu & Sapiro,
"DCT image denoising: a simple and effective image denoising algorithm", IPOL 2011), numpy float64.

For a uint8 image (H, W, C), C 1 or 3, H, W >= 8, a strength sigma per channel (0..255 scale) and
a factor:
  1. f = x.astype(float64)
  2. colour transform (color and C == 3): g[..., k] = sum_j M[k, j] f[..., j], M the orthonormal
     3-point DCT on the channels as stored: rows [1,1,1]/sqrt3, [1,0,-1]/sqrt2, [1,-2,1]/sqrt6;
     otherwise g = f
  3. thresholds: s'_k = sqrt(sum_j M[k,j]^2 s_j^2) with the transform (exact noise propagation),
     else s'_k = s_k;  T_k = factor * s'_k
  4. for every plane k and every patch P with top-left (i, j), 0 <= i <= H-8, 0 <= j <= W-8:
     D = Cm P Cm^T (Cm: the orthonormal 8-point DCT-II matrix);
     D'[u,v] = D[u,v] if (u,v) == (0,0) or |D[u,v]| >= T_k, else 0;   R = Cm^T D' Cm
  5. r_k[y,x] = the sum of R at (y,x) over the patches that contain it, divided by their count
     (min(y,H-8) - max(y-7,0) + 1) * (min(x,W-8) - max(x-7,0) + 1)
  6. inverse colour transform: r_j = sum_k M[k,j] r_k
out "f" is r, "u8" is clip(rint(r), 0, 255), round half to even.

Not cv2.xphoto.dctDenoising and not the IPOL code, and parity with them is unpinned: the DC term
is always kept, the patch is 8, the colour transform is fixed and there is no PCA.

dtype=np.float32 runs the same steps in fp32 (it sizes the tolerance of the device kernel).
risk_mask marks the samples whose value hangs on a threshold decision that rounding could flip.
"""
import numpy as np

PATCH = 8
_K = np.arange(PATCH)
CM = np.sqrt(2.0 / PATCH) * np.cos(np.pi * (2 * _K[None, :] + 1) * _K[:, None] / (2 * PATCH))
CM[0, :] = np.sqrt(1.0 / PATCH)
M3 = np.array([[1.0, 1.0, 1.0], [1.0, 0.0, -1.0], [1.0, -2.0, 1.0]])
M3 /= np.sqrt((M3 * M3).sum(axis=1, keepdims=True))


def to_u8(r):
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def counts(h, w):
    """(H, W) number of patches that cover each sample"""
    y, x = np.arange(h), np.arange(w)
    cy = np.minimum(y, h - PATCH) - np.maximum(y - (PATCH - 1), 0) + 1
    cx = np.minimum(x, w - PATCH) - np.maximum(x - (PATCH - 1), 0) + 1
    return cy[:, None] * cx[None, :]


def _sigmas(sigma, n, c):
    s = np.asarray(sigma, np.float64)
    if s.ndim == 2 and s.shape == (n, 1):
        s = np.repeat(s, c, axis=1)
    return np.array(np.broadcast_to(s, (n, c)))


def thresholds(sigma, factor, color):
    """T_k of one image from its (C,) sigmas, float64"""
    s = np.asarray(sigma, np.float64)
    if color and s.shape[0] == 3:
        w = M3 * M3
        s = np.sqrt(w[:, 0] * s[0] ** 2 + w[:, 1] * s[1] ** 2 + w[:, 2] * s[2] ** 2)
    return factor * s


def planes(x, color, dtype=np.float64):
    """step 1 and 2 of one image (H, W, C): (H, W, C) of dtype"""
    f = np.asarray(x).astype(dtype)
    if color and f.shape[-1] == 3:
        m = M3.astype(dtype)
        return np.stack([m[k, 0] * f[..., 0] + m[k, 1] * f[..., 1] + m[k, 2] * f[..., 2]
                         for k in range(3)], axis=-1)
    return f


def patch_dct(plane, dtype=np.float64):
    """D of every patch of a 2-D plane: (H-7, W-7, 8, 8)"""
    cm = CM.astype(dtype)
    p = np.lib.stride_tricks.sliding_window_view(plane, (PATCH, PATCH))
    return np.einsum("uy,ijyx,vx->ijuv", cm, p, cm, optimize=False).astype(dtype)


def _keep(d, t):
    keep = np.abs(d) >= t
    keep[..., 0, 0] = True
    return keep


def denoise_plane(plane, t, dtype=np.float64):
    """steps 4 and 5 of one 2-D plane with the threshold t"""
    plane = np.asarray(plane, dtype)
    h, w = plane.shape
    cm = CM.astype(dtype)
    d = patch_dct(plane, dtype)
    d = np.where(_keep(d, dtype(t)), d, dtype(0))
    r = np.einsum("uy,ijuv,vx->ijyx", cm, d, cm, optimize=False).astype(dtype)
    acc = np.zeros((h, w), dtype)
    for dy in range(PATCH):
        for dx in range(PATCH):
            acc[dy:dy + h - PATCH + 1, dx:dx + w - PATCH + 1] += r[:, :, dy, dx]
    return acc / counts(h, w).astype(dtype)


def _check(x):
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] not in (1, 3):
        raise ValueError("uint8 (N,)H,W,C with C 1 or 3 expected")
    if x.shape[-3] < PATCH or x.shape[-2] < PATCH:
        raise ValueError("H and W must be at least 8")
    return x


def denoise_dct(x, sigma, factor=3.0, color=True, patch=8, out="u8", dtype=np.float64):
    """idn.denoise_dct on a numpy uint8 array (N,)H,W,C.  sigma: a number, C numbers, or an array
    (C,), (N, C) or (N, 1).  out: 'u8' | 'f' (the float result in dtype, not clipped) | 'both'."""
    x = _check(x)
    if patch != PATCH:
        raise ValueError("only patch 8 is defined")
    if out not in ("u8", "f", "both"):
        raise ValueError(f"out must be 'u8', 'f' or 'both', got {out!r}")
    xb = x[None] if x.ndim == 3 else x
    n, h, w, c = xb.shape
    sg = _sigmas(sigma, n, c)
    use_color = bool(color) and c == 3
    res = np.empty(xb.shape, dtype)
    for i in range(n):
        t = thresholds(sg[i], float(factor), use_color)
        g = planes(xb[i], use_color, dtype)
        r = np.stack([denoise_plane(g[..., k], t[k], dtype) for k in range(c)], axis=-1)
        if use_color:
            m = M3.astype(dtype)
            r = np.stack([m[0, j] * r[..., 0] + m[1, j] * r[..., 1] + m[2, j] * r[..., 2]
                          for j in range(3)], axis=-1)
        res[i] = r
    if x.ndim == 3:
        res = res[0]
    if out == "f":
        return res
    return to_u8(res) if out == "u8" else (to_u8(res), res)


def risk_mask(x, sigma, factor=3.0, color=True, margin=2e-3):
    """bool, x's shape: the samples covered by at least one patch (of any plane, under the colour
    transform, which mixes the planes into every channel) that has a non-DC coefficient with
    ||D| - T| < margin: a decision another rounding could flip"""
    x = _check(x)
    xb = x[None] if x.ndim == 3 else x
    n, h, w, c = xb.shape
    sg = _sigmas(sigma, n, c)
    use_color = bool(color) and c == 3
    mask = np.zeros(xb.shape, bool)
    for i in range(n):
        t = thresholds(sg[i], float(factor), use_color)
        g = planes(xb[i], use_color)
        for k in range(c):
            near = np.abs(np.abs(patch_dct(g[..., k])) - t[k]) < margin
            near[..., 0, 0] = False
            bad = near.any(axis=(2, 3))
            cover = np.zeros((h, w), bool)
            for dy in range(PATCH):
                for dx in range(PATCH):
                    cover[dy:dy + h - PATCH + 1, dx:dx + w - PATCH + 1] |= bad
            if use_color:
                mask[i] |= cover[..., None]
            else:
                mask[i, ..., k] |= cover
    return mask[0] if x.ndim == 3 else mask
