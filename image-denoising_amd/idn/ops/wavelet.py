"""Wavelet denoising: skimage's denoise_wavelet on the tuned and the general kernels."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._args import _as_batch, _finish, _ptr, _stream, _workspace

WAVELETS = {"db1": 0, "haar": 0, "bior1.5": 1, "db2": 2, "sym4": 3, "coif5": 4}  # idn_wavelet
WAVELET_METHODS = {"BayesShrink": 0, "VisuShrink": 1}  # idn_wavelet_method
WAVELET_MODES = {"soft": 0, "hard": 1}                  # idn_wavelet_mode


def _wavelet_sigma(sigma, n: int, c: int, device) -> Optional[torch.Tensor]:
    """sigma as the (n, c) float64 device tensor idn_wavelet_denoise_general reads, or None"""
    if sigma is None:
        return None
    if isinstance(sigma, torch.Tensor):
        if sigma.dtype != torch.float64 or sigma.device != device:
            raise ValueError("denoise_wavelet: a sigma tensor must be float64 on x's device")
        if tuple(sigma.shape) not in ((c,), (n, c)):
            raise ValueError(f"denoise_wavelet: sigma tensor of shape {tuple(sigma.shape)}, "
                             f"expected ({c},) or ({n}, {c})")
        return sigma.expand(n, c).contiguous()  # stays on the device: no value is read here
    if isinstance(sigma, (int, float)) and not isinstance(sigma, bool):
        vals = [float(sigma)] * c
    else:
        try:
            vals = [float(v) for v in sigma]
        except TypeError:
            raise TypeError("denoise_wavelet: sigma must be None, a float, a sequence of C floats "
                            "or a float64 device tensor") from None
        if len(vals) != c:
            raise ValueError(f"denoise_wavelet: {len(vals)} sigmas for {c} channels")
    return torch.tensor(vals, dtype=torch.float64).to(device).expand(n, c).contiguous()


def denoise_wavelet(x: torch.Tensor, wavelet: str = "bior1.5", levels: Optional[int] = None,
                    out: str = "u8", out_u8: Optional[torch.Tensor] = None,
                    ycc_keys: Optional[torch.Tensor] = None, *, sigma=None, mode: str = "soft",
                    method: str = "BayesShrink", convert2ycbcr: bool = True):
    """Per image, skimage 0.14.2's denoise_wavelet(x_i, sigma, wavelet, mode,
    wavelet_levels=levels, multichannel=True, convert2ycbcr=convert2ycbcr, method=method),
    followed for out='u8' by the caller's (255 * r).astype(uint8).
    x: uint8 (N,)H,W,C or float64 (N,)H,W,C in [0, 1] (a precondition: skimage clips a float image
    with negative values to (-1, 1) instead, which this does not do).
    wavelet: 'db1' / 'haar', 'bior1.5', 'db2', 'sym4', 'coif5', extension 'symmetric'; levels
    defaults to max(min(dwt_max_level(h, F), dwt_max_level(w, F)) - 3, 1).
    method: 'BayesShrink' (a threshold per band) | 'VisuShrink' (sigma sqrt(2 log(h w)) for all).
    mode: 'soft' | 'hard' (pywt.threshold).
    sigma: None (estimated per channel from the finest diagonal band of `wavelet`), a float, a
    sequence of C floats, or a float64 device tensor of shape (C,) or (N, C) -- a strength per
    image, read on the device.  sigma is on the scale of what is transformed: with
    convert2ycbcr=False the image on 0..1 (idn.estimate_sigma(u8) / 255 is that scale); with
    convert2ycbcr=True skimage passes sigma[i] to the Y / Cb / Cr channel after it has been
    normalised to [0, 1] by its own range, and so does this -- it is not the noise level of the
    RGB image.
    convert2ycbcr: True (the default here, unlike skimage's, so that no earlier call changes)
    denoises in YCbCr and needs C = 3; False denoises each channel of the float image on its own
    and clips once to [0, 1]; C may then be 1 (skimage's multichannel=False on the 2-D image) or 3.
    out: 'u8' | 'f32' (float result before the cast) | 'both'.
    ycc_keys: float64 x only, with every option above at its default and wavelet db1 / bior1.5 --
    the colour range random_noise_ycc reduced while writing x (the same result, one read fewer).
    With every keyword option at its default and wavelet db1 / bior1.5 this runs the tuned kernels
    (idn_wavelet_denoise_u8 / _ycc), as before; any other option or wavelet runs the general
    path (idn_wavelet_denoise_general), which is slower."""
    wv = WAVELETS.get(wavelet)
    if wv is None:
        raise ValueError(f"denoise_wavelet: unsupported wavelet {wavelet!r} "
                         "(db1/haar/bior1.5/db2/sym4/coif5)")
    if method not in WAVELET_METHODS:
        raise ValueError(f"denoise_wavelet: method {method!r} (BayesShrink/VisuShrink)")
    if mode not in WAVELET_MODES:
        raise ValueError(f"denoise_wavelet: mode {mode!r} (soft/hard)")
    convert2ycbcr = bool(convert2ycbcr)
    general = (wv > 1 or sigma is not None or mode != "soft" or method != "BayesShrink"
               or not convert2ycbcr)
    if general and ycc_keys is not None:
        raise ValueError("denoise_wavelet: ycc_keys goes with the default options and wavelet "
                         "db1 / bior1.5 only")
    # (the argument checks come before the device is looked at)
    c = x.shape[-1] if isinstance(x, torch.Tensor) and x.dim() in (3, 4) else 3
    if convert2ycbcr and c != 3:
        raise ValueError("denoise_wavelet: the YCbCr path needs 3 channels (pass "
                         "convert2ycbcr=False to denoise a 1- or 3-channel image per channel)")
    if c not in (1, 3):
        raise ValueError(f"denoise_wavelet: {c} channels (1 or 3)")
    xb, sq = _as_batch(x, "denoise_wavelet")
    n, h, w, c = xb.shape
    if xb.dtype == torch.uint8:
        src, src64 = xb.contiguous(), None
    elif xb.dtype == torch.float64:
        src, src64 = None, xb.contiguous()
    else:
        raise TypeError(f"denoise_wavelet: expected uint8 or float64, got {xb.dtype}")
    want_u8 = out in ("u8", "both")
    want_f32 = out in ("f32", "both")
    y8 = (out_u8.view(n, h, w, c) if out_u8 is not None else
          torch.empty((n, h, w, c), dtype=torch.uint8, device=xb.device)) if want_u8 else None
    y32 = torch.empty((n, h, w, c), dtype=torch.float32, device=xb.device) if want_f32 else None
    lib = _lib.load()
    lv = -1 if levels is None else int(levels)

    def result():
        if out == "u8":
            return _finish(y8, sq)
        if out == "f32":
            return _finish(y32, sq)
        return _finish(y8, sq), _finish(y32, sq)

    if general:
        sig = _wavelet_sigma(sigma, n, c, xb.device)
        nbytes = lib.idn_wavelet_general_workspace_size(n, h, w, c, wv, lv)
        ws = _workspace(nbytes, xb.device)
        rc = lib.idn_wavelet_denoise_general(
            _ptr(src), _ptr(src64), _ptr(y8), _ptr(y32), n, h, w, c, w * c, wv, lv,
            WAVELET_METHODS[method], WAVELET_MODES[mode], int(convert2ycbcr), _ptr(sig),
            ws.data_ptr(), nbytes, _stream())
        _lib.check(rc, "idn_wavelet_denoise_general")
        return result()
    nbytes = lib.idn_wavelet_workspace_size(n, h, w, wv, lv)
    ws = _workspace(nbytes, xb.device)
    if ycc_keys is not None:
        if src64 is None:
            raise ValueError("denoise_wavelet: ycc_keys applies to float64 input")
        if (ycc_keys.dtype != torch.int64 or ycc_keys.device != xb.device
                or tuple(ycc_keys.shape) != (n, 6)):
            raise ValueError("denoise_wavelet: ycc_keys must be the (N, 6) int64 device tensor of "
                             "random_noise_ycc")
        rc = lib.idn_wavelet_denoise_ycc(src64.data_ptr(), ycc_keys.contiguous().data_ptr(),
                                         _ptr(y8), _ptr(y32), n, h, w, wv, lv, ws.data_ptr(),
                                         nbytes, _stream())
        _lib.check(rc, "idn_wavelet_denoise_ycc")
        return result()
    rc = lib.idn_wavelet_denoise_u8(_ptr(src), _ptr(src64), _ptr(y8), _ptr(y32), n, h, w, w * 3,
                                    wv, lv, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "idn_wavelet_denoise_u8")
    return result()
