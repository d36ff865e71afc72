"""The blob epilogue and the small ops around it: resize, the flat copy, shader, bloom."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ._args import _as_batch, _f64_batch, _finish, _mean3, _stream, _u8_batch
from .filters import gaussian_blur

PIXEL_MEANS = (102.9801, 115.9465, 122.7717)  # lib/model/config.py:252 (BGR)


def blob(x: torch.Tensor, pixel_means=PIXEL_MEANS, out_hw: Optional[Tuple[int, int]] = None,
         flip: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """prep_im_for_blob (scale 1.0) + im_list_to_blob: float32 NHWC, mean-subtracted, zero-padded."""
    xb, _ = _u8_batch(x, "blob")
    n, h, w, c = xb.shape
    oh, ow = out_hw if out_hw is not None else (h, w)
    y = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=xb.device) if out is None else out
    m = _mean3(pixel_means)
    rc = _lib.load().idn_blob_f32(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c, oh, ow, m,
                                  1 if flip else 0, _stream())
    _lib.check(rc, "idn_blob_f32")
    return y


def gaussian_blob(x: torch.Tensor, ksize: int = 5, pixel_means=PIXEL_MEANS,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """blob(gaussian_blur(x, ksize)) at scale 1.0 in one pass: float32 (N, H, W, 3)
    float32(float64(v) - mean[ch]) written by the filter (idn_gaussian_blob_f32)."""
    xb, _ = _u8_batch(x, "gaussian_blob")
    n, h, w, c = xb.shape
    y = torch.empty((n, h, w, c), dtype=torch.float32, device=xb.device) if out is None else out
    m = _mean3(pixel_means)
    rc = _lib.load().idn_gaussian_blob_f32(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c,
                                           int(ksize), m, _stream())
    if rc == -2:
        return blob(gaussian_blur(xb, ksize), pixel_means, out=y)
    _lib.check(rc, "idn_gaussian_blob_f32")
    return y


def blob_from_f64(x: torch.Tensor, pixel_means=PIXEL_MEANS, out_hw: Optional[Tuple[int, int]] = None,
                  flip: bool = False) -> torch.Tensor:
    """prep_im_for_blob on a float64 image (the reference's float64 plain-noise branches)."""
    xb, _ = _f64_batch(x, "blob_from_f64")
    n, h, w, c = xb.shape
    oh, ow = out_hw if out_hw is not None else (h, w)
    y = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=xb.device)
    m = _mean3(pixel_means)
    _lib.check(_lib.load().idn_blob_from_f64(xb.data_ptr(), y.data_ptr(), n, h, w, oh, ow, m,
                                             1 if flip else 0, _stream()), "idn_blob_from_f64")
    return y


def resize_linear(x: torch.Tensor, fx: float, fy: float) -> torch.Tensor:
    """cv2.resize(x, None, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) on float32 NHWC."""
    xb, sq = _as_batch(x, "resize_linear")
    if xb.dtype != torch.float32:
        raise TypeError("resize_linear: expected float32")
    xb = xb.contiguous()
    n, h, w, c = xb.shape
    oh, ow = int(round(h * fy)), int(round(w * fx))  # cv::Size(saturate_cast<int>(...))
    if (oh, ow) == (h, w):
        return _finish(xb.clone(), sq)  # cv2.resize copies when the size is unchanged
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=xb.device)
    _lib.check(_lib.load().idn_resize_linear_f32(xb.data_ptr(), y.data_ptr(), n, h, w, c, oh, ow,
                                                 float(fx), float(fy), _stream()),
               "idn_resize_linear_f32")
    return _finish(y, sq)


def copy_flat(x: torch.Tensor, out: torch.Tensor, policy: int = 0) -> torch.Tensor:
    """out <- x as one flat byte copy (the bench's copy ceiling; policy 1 = nontemporal)."""
    if x.device.type != "cuda" or out.device != x.device:
        raise ValueError("copy_flat: both tensors must be on the same GPU")
    if not (x.is_contiguous() and out.is_contiguous()) or x.nbytes != out.nbytes:
        raise ValueError("copy_flat: contiguous tensors of equal byte size required")
    rc = _lib.load().idn_copy_u8(x.data_ptr(), out.data_ptr(), x.nbytes, int(policy), _stream())
    _lib.check(rc, "idn_copy_u8")
    return out


def shader(x: torch.Tensor, factor: float = 3.0) -> torch.Tensor:
    """add_shader: PIL ImageEnhance.Brightness(factor) of the image, returned in RGB order."""
    xb, sq = _u8_batch(x, "shader")
    n, h, w, c = xb.shape
    y = torch.empty_like(xb)
    _lib.check(_lib.load().idn_shader_u8(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c, float(factor),
                                         _stream()), "idn_shader_u8")
    return _finish(y, sq)


def bloom(x: torch.Tensor, rng=None, circles=None, **flare_kw) -> torch.Tensor:
    """add_bloom: Automold.add_sun_flare(img, flare_center=(100,100), angle=-pi/4) per image, the
    random draws taken from `rng` (default: the global `random`, like the reference), or given
    per image as `circles` = [(circles int32 [k, 8], weights float32 [k, 2]), ...] (what
    automold.sun_flare_circles returns; plans carry them, idn.noise_spec.plan(hw=...))."""
    import math
    from .. import automold
    xb, sq = _u8_batch(x, "bloom")
    n, h, w, c = xb.shape
    if circles is not None:
        if len(circles) != n:
            raise ValueError(f"bloom: {len(circles)} circle sets for {n} images")
        circ = np.stack([np.asarray(a, np.int32).reshape(-1, 8) for a, _ in circles])
        wts = np.stack([np.asarray(b, np.float32).reshape(-1, 2) for _, b in circles])
    else:
        kw = dict(flare_center=(100, 100), angle=-math.pi / 4)
        kw.update(flare_kw)
        circ, wts = zip(*[automold.sun_flare_circles(h, w, rng=rng, **kw) for _ in range(n)])
        circ, wts = np.stack(circ), np.stack(wts)
    rmax = int(circ[..., 2].max()) if circ.size else 0
    spans = torch.from_numpy(automold.span_table(max(rmax, 1))).to(xb.device)
    circ_t = torch.from_numpy(np.ascontiguousarray(circ)).to(xb.device)
    wts_t = torch.from_numpy(np.ascontiguousarray(wts)).to(xb.device)
    y = torch.empty_like(xb)
    _lib.check(_lib.load().idn_bloom_u8(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c,
                                        circ_t.data_ptr(), wts_t.data_ptr(), circ.shape[1],
                                        spans.data_ptr(), _stream()), "idn_bloom_u8")
    return _finish(y, sq)
