"""Quality metrics of an image pair: mse, psnr, ssim."""
from __future__ import annotations

import torch

from .. import _lib
from ._args import _finish, _ptr, _stream, _u8_batch, _workspace, check_shape, check_tensor


def _check_pair(x, y, name: str) -> None:
    """dtype and shape errors of a metric's image pair, raised before the device is looked at"""
    check_tensor(name, x, role=" for x")
    check_tensor(name, y, role=" for y")
    if x.shape != y.shape:
        raise ValueError(f"{name}: shape mismatch {tuple(x.shape)} vs {tuple(y.shape)}")
    check_shape(name, x)
    if x.device != y.device:
        raise ValueError(f"{name}: images on different devices ({x.device} vs {y.device})")


def mse(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """skimage.measure.compare_mse(x[i], y[i]) per image pair: float64 (N,) on the device (0-d for
    one (H,W,C) pair), bit-equal to numpy's float64 mean of the squared differences."""
    _check_pair(x, y, "mse")
    xb, sq = _u8_batch(x, "mse")
    yb, _ = _u8_batch(y, "mse")
    n, h, w, c = xb.shape
    out = torch.empty((n,), dtype=torch.float64, device=xb.device)
    if n == 0:
        return out
    lib = _lib.load()
    nbytes = lib.idn_metrics_workspace_size(n, h, w, c, 0)
    ws = _workspace(nbytes, xb.device)
    rc = lib.idn_mse_u8(xb.data_ptr(), yb.data_ptr(), out.data_ptr(), n, h, w, c, w * c, w * c,
                        ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "idn_mse_u8")
    return _finish(out, sq)


def psnr(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """skimage.measure.compare_psnr(x[i], y[i]) (data_range 255) per image pair: float64 on the
    device, +inf for identical images."""
    return 10.0 * torch.log10(65025.0 / mse(x, y))


def ssim(x: torch.Tensor, y: torch.Tensor, win_size: int = 7, *, per_channel: bool = False,
         return_mse: bool = False):
    """skimage.measure.compare_ssim(x[i], y[i], win_size=win_size, multichannel=True) per image
    pair (uniform window, sample covariance, data_range 255): float64 (N,) on the device, (N, C)
    with per_channel=True (0-d / (C,) for one (H,W,C) pair).  win_size odd, 3..11.
    return_mse=True returns (ssim, mse), the mse from the same pass over the images."""
    _check_pair(x, y, "ssim")
    win = int(win_size)
    if win != win_size or win % 2 == 0 or not 3 <= win <= 11:
        raise ValueError(f"ssim: win_size must be odd and in 3..11, got {win_size!r}")
    if min(x.shape[-3], x.shape[-2]) < win:
        raise ValueError(f"ssim: win_size {win} exceeds the image ({x.shape[-3]} x {x.shape[-2]})")
    xb, sq = _u8_batch(x, "ssim")
    yb, _ = _u8_batch(y, "ssim")
    n, h, w, c = xb.shape
    out = torch.empty((n,), dtype=torch.float64, device=xb.device)
    out_ch = torch.empty((n, c), dtype=torch.float64, device=xb.device) if per_channel else None
    out_mse = torch.empty((n,), dtype=torch.float64, device=xb.device) if return_mse else None
    if n == 0:
        res = out_ch if per_channel else out
        return (res, out_mse) if return_mse else res
    lib = _lib.load()
    nbytes = lib.idn_metrics_workspace_size(n, h, w, c, win)
    ws = _workspace(nbytes, xb.device)
    rc = lib.idn_ssim_u8(xb.data_ptr(), yb.data_ptr(), out.data_ptr(), _ptr(out_ch), _ptr(out_mse),
                         n, h, w, c, w * c, w * c, win, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "idn_ssim_u8")
    res = _finish(out_ch if per_channel else out, sq)
    return (res, _finish(out_mse, sq)) if return_mse else res
