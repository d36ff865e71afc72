"""Colour: quantisation by k-means in 8-bit Lab, and the BGR <-> Lab conversions."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._args import (_finish, _ids_tensor, _one_or_tuple, _ptr, _seed64, _stream, _u8_batch,
                    _workspace)


def quantize(x: torch.Tensor, k: int, *, seed: int = 0, offset: int = 0, image_ids=None,
             centers: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             return_labels: bool = False, return_centers: bool = False):
    """The reference's `quant` noise (lib/model/test.py:592-765): per image
    LAB2BGR(MiniBatchKMeans(n_clusters=k).fit(BGR2LAB(x)).cluster_centers_.astype(uint8)[labels]).

    centers None: device k-means (greedy k-means++ + Lloyd, Philox draws keyed by (seed, image
    id = offset + i or image_ids[i])).  centers (float64 (N, k, 3) on the device, e.g. sklearn's
    cluster_centers_): replay -- labels exactly as sklearn assigns them.
    Returns out, plus labels (uint8 (N, H, W)) and / or the centres used ((N, k, 3) float64)."""
    xb, sq = _u8_batch(x, "quantize")
    n, h, w, c = xb.shape
    if c != 3:
        raise ValueError("quantize: needs 3-channel BGR images")
    k = int(k)
    y = torch.empty_like(xb) if out is None else out.view(n, h, w, c)
    lab = torch.empty((n, h, w), dtype=torch.uint8, device=xb.device) if return_labels else None
    cen_out = (torch.empty((n, k, 3), dtype=torch.float64, device=xb.device)
               if return_centers else None)
    cin = None
    if centers is not None:
        if centers.device != xb.device or centers.dtype != torch.float64 or \
                tuple(centers.shape) != (n, k, 3):
            raise ValueError(f"quantize: centers must be float64 {(n, k, 3)} on the batch's device")
        cin = centers.contiguous()
    ids = _ids_tensor(image_ids, n, xb.device) if image_ids is not None else None
    lib = _lib.load()
    ws_bytes = lib.idn_quant_workspace_size(n, k)
    ws = _workspace(ws_bytes, xb.device) if ws_bytes else None
    rc = lib.idn_quant_u8(xb.data_ptr(), y.data_ptr(), _ptr(lab), n, h, w, w * 3, k, _seed64(seed),
                          int(offset), _ptr(ids), _ptr(cin), _ptr(cen_out), _ptr(ws), ws_bytes,
                          _stream())
    _lib.check(rc, "idn_quant_u8")
    res = [_finish(y, sq)]
    if return_labels:
        res.append(_finish(lab, sq))
    if return_centers:
        res.append(_finish(cen_out, sq))
    return _one_or_tuple(res)


def cvt_color_lab(x: torch.Tensor, to_lab: bool = True, linear: bool = False) -> torch.Tensor:
    """cv2.cvtColor(x, COLOR_BGR2LAB) (to_lab) or (x, COLOR_LAB2BGR) on 8-bit 3-channel images;
    linear=True: COLOR_LBGR2Lab / COLOR_Lab2LBGR (no sRGB gamma; nl_means_colored's conversions)."""
    xb, sq = _u8_batch(x, "cvt_color_lab")
    n, h, w, c = xb.shape
    if c != 3:
        raise ValueError("cvt_color_lab: needs 3 channels")
    y = torch.empty_like(xb)
    if linear:
        fn = "idn_lbgr2lab_u8" if to_lab else "idn_lab2lbgr_u8"
    else:
        fn = "idn_bgr2lab_u8" if to_lab else "idn_lab2bgr_u8"
    _lib.check(getattr(_lib.load(), fn)(xb.data_ptr(), y.data_ptr(), n, h, w, w * 3, _stream()), fn)
    return _finish(y, sq)
