"""The argument layer of every op family: tensors to batches and pointers, the checks and the
messages the ops share, the row layout of an image and its destination, the scratch cache.

The messages the ops share (no CPU path, the image shape, a uint8 destination like x) are spelled
here and nowhere else.  The order in which an op's checks fire is the op's own: some reject bad
arguments before they look at the device (check_image ... require_gpu), the others look at the
device first (_as_batch)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _seed64(seed) -> int:
    """the seed as the uint64 the C ABI takes"""
    return int(seed) & (2 ** 64 - 1)


def _mean3(pixel_means):
    """the per-channel means as the double[3] of the blob entry points"""
    return (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1)])


def _one_or_tuple(res: list):
    return res[0] if len(res) == 1 else tuple(res)


# ---- checks --------------------------------------------------------------------------------------

def require_gpu(name: str, x: torch.Tensor) -> None:
    if x.device.type != "cuda":
        raise ValueError(f"{name}: idn runs on the GPU only; got a {x.device} tensor "
                         "(move it with .cuda(); there is no CPU fallback)")


def _shape_error(name: str, x: torch.Tensor) -> ValueError:
    return ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")


def check_tensor(name: str, x, dtypes=(torch.uint8,), role: str = "") -> None:
    """x is a tensor, of one of dtypes unless that is None; role (' for x') names it where an op
    takes two images"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor{role}, got {type(x).__name__}")
    if dtypes is not None and x.dtype not in dtypes:
        kinds = " or ".join(str(d).split(".")[-1] for d in dtypes)
        raise TypeError(f"{name}: expected {kinds} images, got {x.dtype}{role}")


def check_shape(name: str, x: torch.Tensor, channels=(1, 3), min_hw=None) -> None:
    """x is 3-D or 4-D with an allowed channel count, and at least min_hw = (rows, columns) if
    that is given.  channels: a tuple of the counts supported, or an int for an op that needs
    exactly that many (the two wordings of the ops)."""
    if x.dim() not in (3, 4):
        raise _shape_error(name, x)
    c = x.shape[-1]
    if isinstance(channels, int):
        if c != channels:
            raise ValueError(f"{name}: needs {channels} channel{'s' if channels > 1 else ''}, got {c}")
    elif c not in channels:
        raise ValueError(f"{name}: {' or '.join(map(str, channels))} channels supported, got {c}")
    if min_hw is not None:
        h, w = x.shape[-3], x.shape[-2]
        if h < min_hw[0] or w < min_hw[1]:
            raise ValueError(f"{name}: image {h} x {w} is smaller than the {min_hw[0]} x "
                             f"{min_hw[1]} this call needs")


def check_image(name: str, x, dtypes=(torch.uint8,), channels=(1, 3), min_hw=None) -> None:
    """the checks every image argument gets before the device is looked at"""
    check_tensor(name, x, dtypes)
    check_shape(name, x, channels, min_hw)


def check_not_empty(name: str, x: torch.Tensor) -> None:
    if x.shape[-3] < 1 or x.shape[-2] < 1:
        raise ValueError(f"{name}: empty image {x.shape[-3]} x {x.shape[-2]}")


def check_out_u8(name: str, x: torch.Tensor, out, what: str = "out", any_object: bool = False) -> None:
    """out is a uint8 tensor shaped like x on x's device.  any_object: out is whatever the caller
    passed and is checked to be a tensor first; otherwise it is taken to be one."""
    if (any_object and not isinstance(out, torch.Tensor)) or out.dtype != torch.uint8 \
            or out.shape != x.shape or out.device != x.device:
        raise ValueError(f"{name}: {what} must be a uint8 tensor shaped like x on x's device")


# ---- batches -------------------------------------------------------------------------------------

def _as_batch(x: torch.Tensor, name: str) -> Tuple[torch.Tensor, bool]:
    check_tensor(name, x, None)
    require_gpu(name, x)
    squeeze = False
    if x.dim() == 3:
        x = x.unsqueeze(0)
        squeeze = True
    if x.dim() != 4:
        raise _shape_error(name, x)
    return x, squeeze


def _u8_batch(x: torch.Tensor, name: str) -> Tuple[torch.Tensor, bool]:
    x, sq = _as_batch(x, name)
    check_tensor(name, x)
    if not x.is_contiguous():
        x = x.contiguous()
    return x, sq


def _f64_batch(x: torch.Tensor, name: str):
    xb, sq = _as_batch(x, name)
    if xb.dtype != torch.float64:
        raise TypeError(f"{name}: expected float64, got {xb.dtype}")
    return xb.contiguous(), sq


def _finish(out: torch.Tensor, squeeze: bool) -> torch.Tensor:
    return out[0] if squeeze else out


def _row_pitch(t: torch.Tensor):
    """row pitch in bytes of a (N,H,W,C) uint8 tensor whose rows are compact or padded (images
    h*pitch apart), or None for any other layout"""
    n, h, w, c = t.shape
    sn, sh, sw, sc = t.stride()
    if sc == 1 and sw == c and sh >= w * c and (n == 1 or sn == h * sh):
        return sh
    return None


def _image_layout(name: str, x: torch.Tensor, out: Optional[torch.Tensor], want_u8: bool = True):
    """(source batch, destination batch, their common row pitch, squeeze) of x and out.
    want_u8=False: the call writes no uint8 image; the destination is None and x stays where it
    lies if its rows are compact or padded."""
    xb, sq = _as_batch(x, name)
    n, hh, w, c = xb.shape
    if not want_u8:
        pitch = _row_pitch(xb)
        if pitch is None:
            xb = xb.contiguous()
            pitch = w * c
        return xb, None, pitch, sq
    if out is not None:
        check_out_u8(name, x, out)
        y = out.unsqueeze(0) if sq else out
        pitch = _row_pitch(y)
        if pitch is None:
            raise ValueError(f"{name}: out must have compact or padded rows")
        if _row_pitch(xb) != pitch:
            if pitch != w * c:
                raise ValueError(f"{name}: a padded out needs x in the same layout")
            xb = xb.contiguous()
        if y.data_ptr() == xb.data_ptr():
            raise ValueError(f"{name}: in-place filtering is not supported (out is x)")
    else:
        pitch = w * c
        xb = xb.contiguous()
        y = torch.empty_like(xb)
    return xb, y, pitch, sq


# ---- per-image ids and batch slots ---------------------------------------------------------------

def _ids_tensor(image_ids, n: int, device) -> torch.Tensor:
    """device uint64 (int64 storage) array of n image ids for the *_ids_u8 entry points.  An
    int64 tensor already on the device is used as is (no host copy, no sync; the caller owns its
    validity); anything else is checked on the host and copied over."""
    if isinstance(image_ids, torch.Tensor) and image_ids.device == device \
            and image_ids.dtype == torch.int64:
        t = image_ids.reshape(-1)
        if t.numel() != n:
            raise ValueError(f"image_ids has {t.numel()} entries for a batch of {n}")
        return t.contiguous()
    t = torch.as_tensor(image_ids, dtype=torch.int64).reshape(-1)
    if t.numel() != n:
        raise ValueError(f"image_ids has {t.numel()} entries for a batch of {n}")
    if bool((t < 0).any()):
        raise ValueError("image_ids must be non-negative")
    return t.to(device).contiguous()


def _slots_tensor(slots, device) -> torch.Tensor:
    """The caller owns slot validity (0 <= slot < batch size, as for device image-id tensors):
    checking a device tensor's values would cost a host sync per launch."""
    if not (isinstance(slots, torch.Tensor) and slots.device == device
            and slots.dtype == torch.int64):
        raise ValueError("slots must be an int64 tensor on the batch's device")
    return slots.reshape(-1).contiguous()


# ---- scratch -------------------------------------------------------------------------------------

_WS_CACHE: dict = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    """grow-only scratch per (device, current stream) (the C-ABI never allocates): calls on one
    stream are ordered, so they may share it; calls on two streams get separate buffers."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _WS_CACHE[key] = ws
    return ws
