"""Host model of idn.denoise_tv_chambolle: skimage 0.14.2's
restoration.denoise_tv_chambolle(x, weight, eps, n_iter_max, multichannel=True) on a uint8 image,
restated in numpy float64.

skimage is not importable where this project is built, so parity with skimage itself is unpinned;
this model is the contract the kernels (csrc/tv.hip) are held to.

Every channel is a 2-D image im = x[..., c] / 255.0 with its own stopping iteration.  With the dual
planes p0, p1 and d at 0 and i = 0, while i < n_iter_max:
  i > 0:  d = -(p0 + p1);  d[1:, :] += p0[:-1, :];  d[:, 1:] += p1[:, :-1];  out = im + d
  i = 0:  out = im
  E = sum(d^2)
  g0[:-1, :] = out[1:, :] - out[:-1, :];  g1[:, :-1] = out[:, 1:] - out[:, :-1]   (last row / column 0)
  norm = sqrt(g0^2 + g1^2);  E += weight * sum(norm);  norm = norm * (0.25 / weight) + 1
  p0 = (p0 - 0.25 g0) / norm;  p1 = (p1 - 0.25 g1) / norm;  E /= H * W
  i = 0:  E_init = E_prev = E
  i > 0:  break if |E_prev - E| < eps * E_init, else E_prev = E
  i += 1
The result is `out` and iters = i: the loop index on a break (the image returned was then formed
from the duals before that iteration's update), n_iter_max on exhaustion.  A constant channel has
E_init = 0, never breaks and returns im; eps = 0 never breaks either.

`tv_chambolle` is the vectorised form on a batch; `tv_channel_direct` is the per-pixel loop, for
small images only.  Both return, per iteration i >= 1, r_i = |E_prev - E| / (eps * E_init): the
stopping rule is r_i < 1, and a test case is only meaningful where no r_i is close to 1."""
import numpy as np


def _ratio(e_prev, e, eps, e_init):
    den = eps * e_init
    return abs(e_prev - e) / den if den > 0 else np.inf


def tv_channel(im, weight=0.1, eps=2e-4, n_iter_max=200):
    """(out, iters, r) of one float64 2-D image; r[k] belongs to iteration k + 1"""
    im = np.asarray(im, dtype=np.float64)
    h, w = im.shape
    p0 = np.zeros_like(im)
    p1 = np.zeros_like(im)
    d = np.zeros_like(im)
    out = im
    r = []
    e_init = e_prev = 0.0
    i = 0
    while i < n_iter_max:
        if i > 0:
            d = -(p0 + p1)
            d[1:, :] += p0[:-1, :]
            d[:, 1:] += p1[:, :-1]
            out = im + d
        else:
            out = im
        e = (d ** 2).sum()
        g0 = np.zeros_like(im)
        g1 = np.zeros_like(im)
        g0[:-1, :] = out[1:, :] - out[:-1, :]
        g1[:, :-1] = out[:, 1:] - out[:, :-1]
        norm = np.sqrt(g0 ** 2 + g1 ** 2)
        e += weight * norm.sum()
        norm = norm * (0.25 / weight) + 1.0
        p0 = (p0 - 0.25 * g0) / norm
        p1 = (p1 - 0.25 * g1) / norm
        e /= float(h * w)
        if i == 0:
            e_init = e_prev = e
        else:
            r.append(_ratio(e_prev, e, eps, e_init))
            if abs(e_prev - e) < eps * e_init:
                break
            e_prev = e
        i += 1
    return out, i, np.array(r)


def tv_channel_direct(im, weight=0.1, eps=2e-4, n_iter_max=200):
    """tv_channel with every array expression written as a loop over the pixels.  The two energy
    sums add the per-pixel terms with the same numpy reduction as the vectorised form, so that E,
    and with it the stopping iteration, is the same number and not one a few ulps away."""
    im = np.asarray(im, dtype=np.float64)
    h, w = im.shape
    p0 = np.zeros((h, w))
    p1 = np.zeros((h, w))
    out = im.copy()
    r = []
    e_init = e_prev = 0.0
    i = 0
    while i < n_iter_max:
        d = np.zeros((h, w))
        out = np.empty((h, w))
        for y in range(h):
            for x in range(w):
                if i > 0:
                    v = -(p0[y, x] + p1[y, x])
                    if y > 0:
                        v += p0[y - 1, x]
                    if x > 0:
                        v += p1[y, x - 1]
                    d[y, x] = v
                    out[y, x] = im[y, x] + v
                else:
                    out[y, x] = im[y, x]
        d2 = np.empty((h, w))
        nrm = np.empty((h, w))
        q0 = np.empty((h, w))
        q1 = np.empty((h, w))
        for y in range(h):
            for x in range(w):
                g0 = out[y + 1, x] - out[y, x] if y + 1 < h else 0.0
                g1 = out[y, x + 1] - out[y, x] if x + 1 < w else 0.0
                d2[y, x] = d[y, x] * d[y, x]
                nv = np.sqrt(g0 * g0 + g1 * g1)
                nrm[y, x] = nv
                den = nv * (0.25 / weight) + 1.0
                q0[y, x] = (p0[y, x] - 0.25 * g0) / den
                q1[y, x] = (p1[y, x] - 0.25 * g1) / den
        e = d2.sum()
        e += weight * nrm.sum()
        p0, p1 = q0, q1
        e /= float(h * w)
        if i == 0:
            e_init = e_prev = e
        else:
            r.append(_ratio(e_prev, e, eps, e_init))
            if abs(e_prev - e) < eps * e_init:
                break
            e_prev = e
        i += 1
    return out, i, np.array(r)


def tv_chambolle(x, weight=0.1, eps=2e-4, n_iter_max=200, channel=tv_channel):
    """(out float64 like x, iters int32 (N, C), r[n][c] arrays) of a uint8 (N,H,W,C) batch"""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 4
    n, h, w, c = x.shape
    out = np.empty(x.shape, dtype=np.float64)
    iters = np.empty((n, c), dtype=np.int32)
    r = []
    for i in range(n):
        r.append([])
        for ch in range(c):
            o, it, rr = channel(x[i, :, :, ch] / 255.0, weight, eps, n_iter_max)
            out[i, :, :, ch] = o
            iters[i, ch] = it
            r[i].append(rr)
    return out, iters, r


def to_u8(out):
    """the op's uint8 output: clip(rint(255 * out), 0, 255)"""
    return np.clip(np.rint(255.0 * out), 0, 255).astype(np.uint8)


def near_half(out, tol=255e-5):
    """pixels whose 255 * out lies within tol of a half-integer (their byte may round either way
    under an error of 1e-5 in out)"""
    v = 255.0 * out
    return np.abs(v - np.floor(v) - 0.5) <= tol


def total_variation(a):
    """isotropic total variation of a (H, W) image, with the model's forward differences"""
    g0 = np.zeros_like(a)
    g1 = np.zeros_like(a)
    g0[:-1, :] = a[1:, :] - a[:-1, :]
    g1[:, :-1] = a[:, 1:] - a[:, :-1]
    return np.sqrt(g0 ** 2 + g1 ** 2).sum()


def noisy(n, h, w, c, seed, sd):
    """conftest.textured plus rounded Gaussian noise of standard deviation sd, clipped"""
    from conftest import textured
    rs = np.random.RandomState(seed + 1000)
    x = textured(n, h, w, c, seed=seed).astype(np.float64)
    return np.clip(np.rint(x + rs.normal(0.0, sd, size=x.shape)), 0, 255).astype(np.uint8)
