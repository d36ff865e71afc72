"""The window filters: Gaussian, box, median, adaptive median, bilateral, and the float64 forms."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._args import _f64_batch, _finish, _ptr, _stream, _u8_batch

MEDIAN_MAX_KSIZE = 31  # idn_median_blur_u8: odd ksize 3..MEDIAN_MAX_KSIZE
ADAPTIVE_MEDIAN_MAX_KSIZE = 31  # idn_adaptive_median_u8: odd max_ksize 3..31
BLUR_MAX_KSIZE = 31    # idn_gaussian_blur_u8 / idn_box_blur_u8: odd ksize 3..BLUR_MAX_KSIZE
# strip rows x byte columns (W*C) of one workgroup of the wide kernels: the box, and the Gaussian
# by channel count (whole groups of 4 pixels)
BLUR_TILE = {"box": (128, 256),
             "gaussian": {1: (128, 256), 2: (128, 256), 3: (128, 252), 4: (128, 256)}}


def _filter_io(fn_name: str, x: torch.Tensor, out: Optional[torch.Tensor]):
    """(source batch, destination batch, squeeze) of a filter call"""
    xb, sq = _u8_batch(x, fn_name)
    y = torch.empty_like(xb) if out is None else out.view(xb.shape)
    return xb, y, sq


def _filter_launch(fn_name: str, xb: torch.Tensor, dst: tuple, *args) -> None:
    """fn(src, *dst, n, h, w, c, pitch, *args, stream) on a batch that is not empty (an empty
    tensor has no storage: its null data_ptr() is not for the C ABI)"""
    n, h, w, c = xb.shape
    rc = getattr(_lib.load(), fn_name)(xb.data_ptr(), *dst, n, h, w, c, w * c, *args, _stream())
    _lib.check(rc, fn_name)


def _filter(fn_name: str, x: torch.Tensor, *args, out: Optional[torch.Tensor] = None):
    xb, y, sq = _filter_io(fn_name, x, out)
    if xb.shape[0] != 0:
        _filter_launch(fn_name, xb, (y.data_ptr(),), *args)
    return _finish(y, sq)


def gaussian_taps(ksize: int, sigma: float = 0.0) -> np.ndarray:
    """The ksize Q8 taps of gaussian_blur (numpy uint16, sum 256); host only (idn_gaussian_taps).

    sigma 0 at 3, 5, 7: OpenCV's dyadic kernels.  Otherwise rint(256 g / sum g) of the sampled
    Gaussian with the given sigma (0: 0.3*((ksize-1)*0.5 - 1) + 0.8), the centre tap adjusted so
    that the sum is 256.  tests/blur_model.py is the definition."""
    taps = np.zeros(32, np.uint16)
    rc = _lib.load().idn_gaussian_taps(int(ksize), float(sigma), taps.ctypes.data)
    _lib.check(rc, "idn_gaussian_taps")
    return taps[:int(ksize)].copy()


def gaussian_blur(x: torch.Tensor, ksize: int = 5, out: Optional[torch.Tensor] = None, *,
                  sigma: float = 0.0) -> torch.Tensor:
    """cv2.GaussianBlur(x, (ksize, ksize), sigma); odd ksize in 3..BLUR_MAX_KSIZE (31).

    Q8 taps t = gaussian_taps(ksize, sigma) and (sum t[i] t[j] x[..] + 32768) >> 16 under
    BORDER_REFLECT_101, images smaller than the window included; bit-equal to tests/blur_model.py.
    With sigma 0 at 3, 5 and 7 that is cv2's result bit for bit; for every other kernel the model
    is the definition and parity with cv2 is unpinned (the taps are renormalised to 256, so a
    constant image comes back unchanged).  (3, 0) and (5, 0) run the stencil kernels, everything
    else a separable LDS kernel whose cost grows with ksize, not ksize**2 (MI355X, 256 images of
    600x1000x3: 1.01 / 1.41 / 2.11 ms at 7 / 15 / 31, the copy of the batch 0.165 ms).  An even
    ksize, 1, anything above 31, or a negative, NaN or infinite sigma raises IdnError."""
    if float(sigma) == 0.0:
        return _filter("idn_gaussian_blur_u8", x, int(ksize), out=out)
    return _filter("idn_gaussian_blur_sigma_u8", x, int(ksize), float(sigma), out=out)


def blur(x: torch.Tensor, ksize: int = 3, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.blur(x, (ksize, ksize)); odd ksize in 3..BLUR_MAX_KSIZE (31); bit-exact.

    (2 S + ksize**2) // (2 ksize**2) of the window sum S under BORDER_REFLECT_101, images smaller
    than the window included.  3 runs the stencil kernel, 5..31 running column sums whose cost
    does not grow with the window's area (MI355X, 256 images of 600x1000x3: 1.12 / 1.25 / 1.48 /
    1.70 ms at 5 / 7 / 15 / 31).  Any other ksize raises IdnError."""
    return _filter("idn_box_blur_u8", x, int(ksize), out=out)


def median_blur(x: torch.Tensor, ksize: int = 3, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.medianBlur(x, ksize); odd ksize in 3..MEDIAN_MAX_KSIZE (31); bit-exact.

    The exact per-channel median (rank ksize*ksize // 2) of the ksize x ksize window,
    BORDER_REPLICATE, images smaller than the window included.  3 and 5 run the sorting-network
    kernels, 7..31 a histogram kernel whose cost per output grows with ksize, not ksize**2.
    Any other ksize (even, 1, above 31) raises IdnError."""
    return _filter("idn_median_blur_u8", x, int(ksize), out=out)


def adaptive_median(x: torch.Tensor, max_ksize: int = 15, out: Optional[torch.Tensor] = None, *,
                    return_ksize: bool = False):
    """The adaptive median filter for salt & pepper (Hwang & Haddad 1995; Gonzalez & Woods §5.3).

    Per channel plane, BORDER_REPLICATE, images smaller than the window included; for a sample z
        for k = 3, 5, .., max_ksize:  mn, mx, md = min, max, median of the k x k window
            if mn < md < mx:  out = z if mn < z < mx else md;  ksize = k;  stop
        no k passed:  out = md of the max_ksize window;  ksize = 0
    (the fall-through rule of the 3rd and later editions of Gonzalez & Woods; the 2nd outputs z).
    max_ksize, odd in 3..ADAPTIVE_MEDIAN_MAX_KSIZE (31), is a cap on the window, not a strength:
    the window grows only where the impulses are dense, and a clean sample comes back unchanged.
    Bit-equal to tests/adaptive_median_model.py.  return_ksize=True returns (y, ksize) with the
    uint8 map of x's shape of the level that decided each sample (0: the fall-through).
    Any other max_ksize (even, 1, above 31, negative) raises IdnError."""
    fn_name = "idn_adaptive_median_u8"
    xb, y, sq = _filter_io(fn_name, x, out)
    km = torch.empty_like(xb) if return_ksize else None
    if xb.shape[0] != 0:
        _filter_launch(fn_name, xb, (y.data_ptr(), _ptr(km)), int(max_ksize))
    if return_ksize:
        return _finish(y, sq), _finish(km, sq)
    return _finish(y, sq)


def bilateral_filter(x: torch.Tensor, d: int = 9, sigma_color: float = 20.0,
                     sigma_space: float = 100.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.bilateralFilter(x, d, sigma_color, sigma_space, borderType=BORDER_CONSTANT)."""
    return _filter("idn_bilateral_u8", x, int(d), float(sigma_color), float(sigma_space), out=out)


def gaussian_blur_f64(x: torch.Tensor, ksize: int = 3) -> torch.Tensor:
    """cv2.GaussianBlur on a float64 image (the train_v0 post hook after a float64 noise branch)."""
    xb, sq = _f64_batch(x, "gaussian_blur_f64")
    n, h, w, c = xb.shape
    y = torch.empty_like(xb)
    _lib.check(_lib.load().idn_gaussian_blur_f64(xb.data_ptr(), y.data_ptr(), n, h, w, c, int(ksize),
                                                 _stream()), "idn_gaussian_blur_f64")
    return _finish(y, sq)


def blur_f64(x: torch.Tensor, ksize: int = 3) -> torch.Tensor:
    """cv2.blur on a float64 image (test_v0 default branch, train_v0 'mean' post hook)."""
    xb, sq = _f64_batch(x, "blur_f64")
    n, h, w, c = xb.shape
    y = torch.empty_like(xb)
    _lib.check(_lib.load().idn_box_blur_f64(xb.data_ptr(), y.data_ptr(), n, h, w, c, int(ksize),
                                            _stream()), "idn_box_blur_f64")
    return _finish(y, sq)
