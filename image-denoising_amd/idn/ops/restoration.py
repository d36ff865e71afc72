"""Restoration: total-variation denoising (Chambolle), the noise level estimate, adaptive Wiener,
the sliding-DCT denoiser."""
from __future__ import annotations

import numbers
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._args import (_as_batch, _finish, _image_layout, _one_or_tuple, _ptr, _stream, _workspace,
                    check_image, check_not_empty, check_out_u8, require_gpu)

# ---- total-variation denoising -------------------------------------------------------------------

TV_MAX_ITER = 1000  # IDN_TV_MAX_ITER of include/idn.h


def _tv_check(x, weight, eps, n_iter_max, out, out_u8) -> None:
    """argument errors of denoise_tv_chambolle, raised before the device is looked at"""
    name = "denoise_tv_chambolle"
    check_image(name, x)
    check_not_empty(name, x)
    if not (isinstance(weight, numbers.Real) and 0 < weight < float("inf")):
        raise ValueError(f"{name}: weight must be positive and finite, got {weight!r}")
    if not (isinstance(eps, numbers.Real) and 0 <= eps < float("inf")):
        raise ValueError(f"{name}: eps must be finite and not negative, got {eps!r}")
    if not (isinstance(n_iter_max, numbers.Integral) and 1 <= n_iter_max <= TV_MAX_ITER):
        raise ValueError(f"{name}: n_iter_max must be an integer in 1..{TV_MAX_ITER}, "
                         f"got {n_iter_max!r}")
    if out not in ("u8", "f32", "both"):
        raise ValueError(f"{name}: out must be 'u8', 'f32' or 'both', got {out!r}")
    if out_u8 is not None:
        if out == "f32":
            raise ValueError(f"{name}: out_u8 given with out='f32'")
        check_out_u8(name, x, out_u8, "out_u8", any_object=True)


def denoise_tv_chambolle(x: torch.Tensor, weight: float = 0.1, eps: float = 2e-4,
                         n_iter_max: int = 200, out: str = "u8",
                         out_u8: Optional[torch.Tensor] = None, return_iters: bool = False):
    """skimage.restoration.denoise_tv_chambolle(x, weight, eps, n_iter_max, multichannel=True) of
    skimage 0.14.2 on uint8 images, 1 or 3 channels: every channel of every image is denoised on
    its own as x[..., c] / 255 and stops at its own iteration.  A larger weight removes more (and
    flattens more texture); eps = 0 runs exactly n_iter_max iterations.
    out: 'u8' (clip(rint(255 * result))) | 'f32' (the float result, not clipped) | 'both'.
    return_iters=True appends the int32 (N, C) device tensor ((C,) for one image) of the iteration
    each (image, channel) stopped at.  Within 1e-5 of the numpy float64 model tests/tv_model.py,
    with the same iteration counts wherever the stopping rule is not within rounding of a tie, and
    the same bits on every call and in every batch.  x may be contiguous or have padded rows;
    out_u8, if given, must then share x's layout.  The scratch is 48 bytes per pixel at 3
    channels."""
    _tv_check(x, weight, eps, n_iter_max, out, out_u8)
    want_u8 = out in ("u8", "both")
    want_f32 = out in ("f32", "both")
    xb, y8, pitch, sq = _image_layout("denoise_tv_chambolle", x, out_u8, want_u8)
    n, h, w, c = xb.shape
    y32 = torch.empty((n, h, w, c), dtype=torch.float32, device=xb.device) if want_f32 else None
    its = torch.empty((n, c), dtype=torch.int32, device=xb.device) if return_iters else None
    if n > 0:
        lib = _lib.load()
        nbytes = lib.idn_tv_chambolle_workspace_size(n, h, w, c)
        ws = _workspace(nbytes, xb.device)
        rc = lib.idn_tv_chambolle_u8(xb.data_ptr(), _ptr(y8), _ptr(y32), _ptr(its), n, h, w, c,
                                     pitch, float(weight), float(eps), int(n_iter_max),
                                     ws.data_ptr(), nbytes, _stream())
        _lib.check(rc, "idn_tv_chambolle_u8")
    res = []
    if want_u8:
        res.append(out_u8 if out_u8 is not None else _finish(y8, sq))
    if want_f32:
        res.append(_finish(y32, sq))
    if return_iters:
        res.append(_finish(its, sq))
    return _one_or_tuple(res)


# ---- noise level -------------------------------------------------------------------------------

def _sigma_check(x) -> None:
    """argument errors of estimate_sigma, raised before the device is looked at"""
    check_image("estimate_sigma", x, dtypes=(torch.uint8, torch.float64))
    require_gpu("estimate_sigma", x)


def estimate_sigma(x: torch.Tensor, average_sigmas: bool = False) -> torch.Tensor:
    """skimage.restoration.estimate_sigma(x[i], multichannel=True, average_sigmas=...) per image:
    the noise standard deviation of every channel, from the median absolute finest diagonal db2
    wavelet coefficient over norm.ppf(0.75).  x: uint8 or float64, (N,)H,W,C with C 1 or 3, H and
    W at least 4.  Returns float64 on the device: (N, C), or (C,) for one image; with
    average_sigmas (N,) or 0-d, ((s0 + s1) + s2) / 3 as numpy's mean adds them.
    The scale is the input's, as in skimage: a uint8 batch is estimated on 0..255 (the scale of
    nl_means' h; divide by 255 for denoise_tv_chambolle and denoise_wavelet), a float64 batch in
    [0, 1] on that scale.  A channel with no nonzero coefficient (an all-zero channel) gives NaN.
    Bit-equal to the numpy float64 model tests/sigma_model.py, which is pinned bit for bit to
    the real skimage and pywt; the same bits on every call and in every batch."""
    _sigma_check(x)
    xb, sq = _as_batch(x, "estimate_sigma")
    if not xb.is_contiguous():
        xb = xb.contiguous()
    n, h, w, c = xb.shape
    out = torch.empty((n, c), dtype=torch.float64, device=xb.device)
    if n > 0:
        lib = _lib.load()
        is_f64 = xb.dtype == torch.float64
        nbytes = lib.idn_estimate_sigma_workspace_size(n, h, w, c, int(is_f64))
        ws = _workspace(nbytes, xb.device)
        src = (None, xb.data_ptr()) if is_f64 else (xb.data_ptr(), None)  # (uint8, float64)
        rc = lib.idn_estimate_sigma(*src, out.data_ptr(), n, h, w, c, w * c, ws.data_ptr(), nbytes,
                                    _stream())
        _lib.check(rc, "idn_estimate_sigma")
    if average_sigmas:
        if c == 3:
            # a tensor divisor: torch turns a division by a Python scalar into a multiplication
            three = torch.full((), 3.0, dtype=torch.float64, device=out.device)
            out = ((out[:, 0] + out[:, 1]) + out[:, 2]) / three
        else:
            out = out[:, 0]
    return _finish(out, sq)


# ---- adaptive Wiener filter ----------------------------------------------------------------------

WIENER_MAX_KSIZE = 31                              # idn_wiener_u8: odd window sides 1..31
WIENER_BORDERS = {"zero": 0, "reflect101": 1}      # idn_wiener_border
WIENER_TILE = (128, 256)  # output rows x interleaved byte columns (W*C) of one workgroup


def _wiener_check(x, ksize, noise, border, out, out_u8):
    """argument errors of wiener, raised before the device is looked at; returns (kh, kw)"""
    name = "wiener"
    check_image(name, x)
    check_not_empty(name, x)
    h, w, c = x.shape[-3:]
    ks = (ksize, ksize) if isinstance(ksize, numbers.Integral) else ksize
    try:
        kh, kw = ks
        ok = all(isinstance(k, numbers.Integral) and 1 <= k <= WIENER_MAX_KSIZE and k % 2 == 1
                 for k in (kh, kw))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name}: ksize must be an odd integer in 1..{WIENER_MAX_KSIZE} or a "
                         f"pair (kh, kw) of them, got {ksize!r}")
    kh, kw = int(kh), int(kw)
    if border not in WIENER_BORDERS:
        raise ValueError(f"{name}: border must be one of {sorted(WIENER_BORDERS)}, got {border!r}")
    if border == "reflect101" and (kh // 2 >= h or kw // 2 >= w):
        raise ValueError(f"{name}: border='reflect101' needs kh//2 < H and kw//2 < W "
                         f"(window {kh} x {kw}, image {h} x {w})")
    if out not in ("u8", "f64"):
        raise ValueError(f"{name}: out must be 'u8' or 'f64', got {out!r}")
    if out_u8 is not None:
        if out != "u8":
            raise ValueError(f"{name}: out_u8 given with out={out!r}")
        check_out_u8(name, x, out_u8, "out_u8", any_object=True)
    n = x.shape[0] if x.dim() == 4 else 1
    if isinstance(noise, torch.Tensor):
        if noise.dtype != torch.float64:
            raise TypeError(f"{name}: a noise tensor must be float64, got {noise.dtype}")
        if noise.device != x.device:
            raise ValueError(f"{name}: a noise tensor must be on x's device ({x.device}), "
                             f"got {noise.device}")
        if tuple(noise.shape) not in ((c,), (n, c)):
            raise ValueError(f"{name}: a noise tensor must have shape ({c},) or ({n}, {c}), "
                             f"got {tuple(noise.shape)}")
    elif noise is not None:
        if isinstance(noise, (str, bytes)):
            raise TypeError(f"{name}: noise must be None, a number, {c} numbers or a tensor")
        try:
            vals = np.asarray(noise, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"{name}: noise must be None, a number, {c} numbers or a tensor, "
                            f"got {type(noise).__name__}") from None
        if vals.shape not in ((), (c,)):
            raise ValueError(f"{name}: noise must be one number or {c} (one per channel), "
                             f"got shape {vals.shape}")
        if not (np.isfinite(vals).all() and (vals >= 0).all()):
            raise ValueError(f"{name}: noise must be finite and not negative, got {noise!r}")
    require_gpu(name, x)
    return kh, kw


def wiener(x: torch.Tensor, ksize=3, noise=None, *, border: str = "zero", out: str = "u8",
           out_u8: Optional[torch.Tensor] = None, return_noise: bool = False):
    """scipy.signal.wiener(x[i][..., ch].astype(float64), (kh, kw), noise) on every channel plane
    of uint8 images, (N,)H,W,C with C 1 or 3: the adaptive local-statistics (Lee, Matlab wiener2)
    filter.  With the window's mean m and variance v (exact: integer sums, divided once),
    r = m where v < noise, else (x - m) * (1 - noise / v) + m: flat regions are averaged, edges
    and texture are kept.  ksize: an odd int or (kh, kw), each 1..31; the cost does not grow with
    the window's area.
    noise, on the 0..255 scale squared (estimate_sigma(x) ** 2 is that scale): None estimates it
    per (image, channel) as scipy does, the mean of v over the plane, which counts the signal and
    so overestimates on structured images; a float; C floats; or a float64 device tensor (C,) or
    (N, C), which is not validated (host values must be finite and not negative).
    border: 'zero' is scipy's (taps outside the image are 0, which dims the rim), 'reflect101'
    mirrors the image (cv2's default border; needs kh//2 < H and kw//2 < W).
    out: 'u8' (clip(rint(r), 0, 255), round half to even) | 'f64' (r).  Where v == 0 the result is
    m; scipy gives NaN there when noise is 0 as well (an all-zero image with noise=None).
    return_noise=True also returns the float64 (N, C) device tensor ((C,) for one image) of the
    noise used.  Bit-equal to the numpy model tests/wiener_model.py, which tests/golden/wiener.npz
    pins to scipy 1.15.3; the same bits on every call and in every batch.  x may be contiguous or
    have padded rows; out_u8, if given, must then share x's layout."""
    kh, kw = _wiener_check(x, ksize, noise, border, out, out_u8)
    xb, y8, pitch, sq = _image_layout("wiener", x, out_u8, out == "u8")
    n, h, w, c = xb.shape
    y64 = torch.empty((n, h, w, c), dtype=torch.float64, device=xb.device) if out == "f64" else None
    nz, nz_stride = None, 0
    if isinstance(noise, torch.Tensor):
        nz = noise.contiguous()
        nz_stride = c if nz.dim() == 2 else 0
    elif noise is not None:
        vals = np.array(np.broadcast_to(np.asarray(noise, dtype=np.float64), (c,)))
        nz = torch.from_numpy(vals).to(xb.device)
    used = torch.empty((n, c), dtype=torch.float64, device=xb.device) if return_noise else None
    if n > 0:
        lib = _lib.load()
        nbytes = lib.idn_wiener_workspace_size(n, c) if nz is None else 0
        ws = _workspace(nbytes, xb.device) if nbytes else None
        rc = lib.idn_wiener_u8(xb.data_ptr(), _ptr(y8), _ptr(y64), n, h, w, c, pitch, kh, kw,
                               WIENER_BORDERS[border], _ptr(nz), nz_stride, _ptr(used), _ptr(ws),
                               nbytes, _stream())
        _lib.check(rc, "idn_wiener_u8")
    if out == "u8":
        res = out_u8 if out_u8 is not None else _finish(y8, sq)
    else:
        res = _finish(y64, sq)
    return (res, _finish(used, sq)) if return_noise else res


# ---- sliding DCT denoiser ------------------------------------------------------------------------

DCT_PATCH = 8            # the one patch side idn_dct_denoise_u8 is built for
DCT_TILE = (128, 57)     # output rows x output columns of one workgroup


def _dct_check(x, sigma, factor, color, patch, out, out_u8) -> None:
    """argument errors of denoise_dct, raised before the device is looked at"""
    name = "denoise_dct"
    check_image(name, x)
    check_not_empty(name, x)
    h, w, c = x.shape[-3:]
    n = x.shape[0] if x.dim() == 4 else 1
    if not (isinstance(factor, numbers.Real) and 0 <= factor < float("inf")):
        raise ValueError(f"{name}: factor must be finite and not negative, got {factor!r}")
    if not isinstance(color, (bool, np.bool_)):
        raise TypeError(f"{name}: color must be a bool, got {color!r}")
    if patch != DCT_PATCH or isinstance(patch, bool):
        raise _lib.IdnError(f"{name}: unsupported patch {patch!r}: only {DCT_PATCH} is built "
                            "(16 is not)")
    if h < DCT_PATCH or w < DCT_PATCH:
        raise _lib.IdnError(f"{name}: unsupported image {h} x {w}: a patch is {DCT_PATCH} x "
                            f"{DCT_PATCH}")
    if out not in ("u8", "f32", "both"):
        raise ValueError(f"{name}: out must be 'u8', 'f32' or 'both', got {out!r}")
    if out_u8 is not None:
        if out == "f32":
            raise ValueError(f"{name}: out_u8 given with out='f32'")
        check_out_u8(name, x, out_u8, "out_u8", any_object=True)
    if isinstance(sigma, torch.Tensor):
        if sigma.dtype != torch.float64:
            raise TypeError(f"{name}: a sigma tensor must be float64, got {sigma.dtype}")
        if sigma.device != x.device:
            raise ValueError(f"{name}: a sigma tensor must be on x's device ({x.device}), "
                             f"got {sigma.device}")
        if tuple(sigma.shape) not in ((c,), (n, c), (n, 1)):
            raise ValueError(f"{name}: a sigma tensor must have shape ({c},), ({n}, {c}) or "
                             f"({n}, 1), got {tuple(sigma.shape)}")
    else:
        if sigma is None or isinstance(sigma, (str, bytes)):
            raise TypeError(f"{name}: sigma must be a number, {c} numbers or a tensor")
        try:
            vals = np.asarray(sigma, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"{name}: sigma must be a number, {c} numbers or a tensor, "
                            f"got {type(sigma).__name__}") from None
        if vals.shape not in ((), (c,)):
            raise ValueError(f"{name}: sigma must be one number or {c} (one per channel), "
                             f"got shape {vals.shape}")
        if not (np.isfinite(vals).all() and (vals >= 0).all()):
            raise ValueError(f"{name}: sigma must be finite and not negative, got {sigma!r}")
    require_gpu(name, x)


def denoise_dct(x: torch.Tensor, sigma, *, factor: float = 3.0, color: bool = True,
                patch: int = 8, out: str = "u8", out_u8: Optional[torch.Tensor] = None):
    """Sliding-window DCT denoising (Yu & Sapiro, IPOL 2011) of uint8 images, (N,)H,W,C with C 1
    or 3 and H, W >= 8: every overlapping 8x8 patch of a plane is transformed by the orthonormal
    DCT, the coefficients below factor * sigma are zeroed (the DC term always stays), the patch is
    transformed back, and every sample is the mean of the up to 64 patches that cover it.  Nothing
    is decimated: no block artefacts.  For Gaussian noise it is the strongest cheap filter of the
    bank.
    sigma, the noise standard deviation on the 0..255 scale (estimate_sigma(x) passes straight
    in): a float; C floats; or a float64 device tensor (C,), (N, C) or (N, 1) (one strength per
    image), which is not validated (host values must be finite and not negative).  sigma = 0
    returns the input.
    color: with three channels, denoise in the orthonormal 3-point DCT of the channels (rows
    [1,1,1]/sqrt3, [1,0,-1]/sqrt2, [1,-2,1]/sqrt6 on the channels as stored), each plane with
    the noise level the transform gives it; where the channels are correlated, as in photographs,
    this gains up to about 4 dB.  Ignored for one channel.
    patch: 8; anything else raises IdnError (16 is not built), and so does an image below 8 x 8.
    out: 'u8' (clip(rint(r), 0, 255), round half to even) | 'f32' (r, not clipped) | 'both'.
    fp32 on the device, against the numpy float64 model tests/dct_model.py: within a few 1e-4
    wherever no coefficient lies within rounding of its threshold, and the same bits on every
    call and in every batch.  Not cv2.xphoto.dctDenoising: parity with it is unpinned.  x may be
    contiguous or have padded rows; out_u8, if given, must then share x's layout."""
    _dct_check(x, sigma, factor, color, patch, out, out_u8)
    want_u8 = out in ("u8", "both")
    want_f32 = out in ("f32", "both")
    xb, y8, pitch, sq = _image_layout("denoise_dct", x, out_u8, want_u8)
    n, h, w, c = xb.shape
    y32 = torch.empty((n, h, w, c), dtype=torch.float32, device=xb.device) if want_f32 else None
    if isinstance(sigma, torch.Tensor):
        sg = sigma.expand(n, c) if sigma.dim() == 2 else sigma
        sg = sg.contiguous()
        sg_stride = c if sg.dim() == 2 else 0
    else:
        vals = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (c,)))
        sg, sg_stride = torch.from_numpy(vals).to(xb.device), 0
    if n > 0:
        lib = _lib.load()
        nbytes = lib.idn_dct_denoise_workspace_size(n, h, w, c)
        ws = _workspace(nbytes, xb.device) if nbytes else None
        rc = lib.idn_dct_denoise_u8(xb.data_ptr(), _ptr(y8), _ptr(y32), n, h, w, c, pitch,
                                    int(patch), int(bool(color) and c == 3), sg.data_ptr(),
                                    sg_stride, float(factor), _ptr(ws), nbytes, _stream())
        _lib.check(rc, "idn_dct_denoise_u8")
    res = []
    if want_u8:
        res.append(out_u8 if out_u8 is not None else _finish(y8, sq))
    if want_f32:
        res.append(_finish(y32, sq))
    return _one_or_tuple(res)
