"""Exposure correction: equalizeHist, CLAHE, BGR <-> YUV, and Automold's correct_exposure."""
from __future__ import annotations

import numbers
from typing import Optional, Tuple

import torch

from .. import _lib
from ._args import _finish, _image_layout, _stream, _workspace, check_image
from .nlmeans import nl_means_colored

CLAHE_MAX_TILES = 16            # idn_clahe_u8: tiles per axis
EXPOSURE_TILE_GRID = (4, 4)     # exposure_process: createCLAHE(clipLimit=2.0, tileGridSize=(4,4))
EXPOSURE_NLM = (3.0, 3.0, 7, 21)  # its fastNlMeansDenoisingColored(., None, 3, 3, 7, 21)


def _exposure_check(name: str, x, channels: int, min_hw=(1, 1)) -> None:
    """argument errors of the exposure wrappers, raised before the device is looked at"""
    check_image(name, x, channels=channels, min_hw=min_hw)


def _exposure_call(fn: str, name: str, x, out, grid, *params) -> torch.Tensor:
    """one histogram op of the C ABI: fn(src, dst, n, h, w, pitch, *params, workspace, bytes, stream)"""
    xb, y, pitch, sq = _image_layout(name, x, out)
    n, h, w, _ = xb.shape
    if n:
        lib = _lib.load()
        nbytes = lib.idn_exposure_workspace_size(n, h, w, *grid)
        ws = _workspace(nbytes, xb.device)
        rc = getattr(lib, fn)(xb.data_ptr(), y.data_ptr(), n, h, w, pitch, *params, ws.data_ptr(),
                              nbytes, _stream())
        _lib.check(rc, fn)
    return out if out is not None else _finish(y, sq)


def equalize_hist(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.equalizeHist(x) per image on uint8 single-channel images (H,W,1) or (N,H,W,1).  Bit-equal
    to the numpy model tests/exposure_model.py (OpenCV 3.4's arithmetic as recalled; parity with
    cv2 itself is unpinned).  x may be contiguous or have padded rows; out, if given, must then
    share x's layout."""
    _exposure_check("equalize_hist", x, 1)
    return _exposure_call("idn_equalize_hist_u8", "equalize_hist", x, out, (1, 1))


def clahe(x: torch.Tensor, clip_limit: float = 2.0, tile_grid: Tuple[int, int] = (4, 4),
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.createCLAHE(clip_limit, tile_grid).apply(x) per image on uint8 single-channel images.
    tile_grid = (tiles_x, tiles_y) as in cv2's Size, each in 1..16; H > tiles_y and W > tiles_x.
    clip_limit >= 0 and finite, 0 meaning no clipping.  When either dimension fails to divide by
    its tile count the image is extended by reflection in both (OpenCV's rule: a dimension that
    divides then grows by a whole tile count).  Bit-equal to tests/exposure_model.py."""
    name = "clahe"
    try:
        tx, ty = tile_grid
        ok = all(isinstance(v, numbers.Integral) and 1 <= v <= CLAHE_MAX_TILES for v in (tx, ty))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name}: tile_grid must be (tiles_x, tiles_y) with each in "
                         f"1..{CLAHE_MAX_TILES}, got {tile_grid!r}")
    if not (isinstance(clip_limit, numbers.Real) and 0 <= clip_limit < float("inf")):
        raise ValueError(f"{name}: clip_limit must be finite and not negative, got {clip_limit!r}")
    tx, ty = int(tx), int(ty)
    _exposure_check(name, x, 1, (ty + 1, tx + 1))
    return _exposure_call("idn_clahe_u8", name, x, out, (tx, ty), float(clip_limit), tx, ty)


def cvt_color_yuv(x: torch.Tensor, to_yuv: bool = True,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.cvtColor(x, COLOR_BGR2YUV) (to_yuv) or (x, COLOR_YUV2BGR) on 8-bit 3-channel images.
    The round trip is not the identity: V saturates and every channel rounds."""
    name = "cvt_color_yuv"
    _exposure_check(name, x, 3)
    xb, y, pitch, sq = _image_layout(name, x, out)
    n, h, w, _ = xb.shape
    if n:
        fn = "idn_bgr2yuv_u8" if to_yuv else "idn_yuv2bgr_u8"
        rc = getattr(_lib.load(), fn)(xb.data_ptr(), y.data_ptr(), n, h, w, pitch, _stream())
        _lib.check(rc, fn)
    return out if out is not None else _finish(y, sq)


def correct_exposure(x: torch.Tensor, denoise: bool = True,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Automold's correct_exposure / exposure_process per uint8 BGR image: BGR -> YUV, luma * 0.85
    where it is above 150, clahe(2.0, (4, 4)), equalize_hist, clahe(2.0, (4, 4)), YUV -> BGR with
    the original U and V, then nl_means_colored(., 3, 3, 7, 21).  denoise=False stops before the
    non-local means and returns the tone-corrected image.  Byte for byte the composition of
    cvt_color_yuv, clahe, equalize_hist and nl_means_colored; the tone part is one C call that
    stores no YUV image.  H, W > 4, and with denoise min(H, W) >= 14."""
    name = "correct_exposure"
    h_nlm, hc_nlm, t_nlm, s_nlm = EXPOSURE_NLM
    need = t_nlm // 2 + s_nlm // 2 + 1 if denoise else EXPOSURE_TILE_GRID[0] + 1
    _exposure_check(name, x, 3, (need, need))
    if not denoise:
        return _exposure_call("idn_correct_exposure_u8", name, x, out, EXPOSURE_TILE_GRID)
    xb, y, pitch, sq = _image_layout(name, x, out)
    if xb.shape[0] == 0:
        return out if out is not None else _finish(y, sq)
    toned = torch.empty_strided(y.shape, y.stride(), dtype=torch.uint8, device=y.device)
    _exposure_call("idn_correct_exposure_u8", name, xb, toned, EXPOSURE_TILE_GRID)
    nl_means_colored(toned, h_nlm, hc_nlm, t_nlm, s_nlm, out=y)
    return out if out is not None else _finish(y, sq)
