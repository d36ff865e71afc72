"""Non-local means in OpenCV's 8-bit integer scheme: grey / joint, and the Lab-coloured form."""
from __future__ import annotations

import ctypes
import numbers
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ._args import _finish, _image_layout, _stream, _workspace, check_image

NLMEANS_MAX_WEIGHTS = 24576  # IDN_NLMEANS_MAX_WEIGHTS of include/idn.h

_NLM_CACHE: dict = {}


def nl_means_weights(h: float, channels: int, template_window: int = 7, search_window: int = 21):
    """The nonzero prefix of OpenCV's fixed-point weight table as an int32 numpy array, with the
    shift and the fixed-point multiplier (idn_nlmeans_weights; host only, no GPU needed)."""
    lib = _lib.load()
    n, shift, fpm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    args = (float(h), int(channels), int(template_window), int(search_window))
    refs = (ctypes.byref(n), ctypes.byref(shift), ctypes.byref(fpm))
    _lib.check(lib.idn_nlmeans_weights(*args, None, 0, *refs), "idn_nlmeans_weights")
    wt = np.empty(n.value, dtype=np.int32)
    _lib.check(lib.idn_nlmeans_weights(*args, wt.ctypes.data, wt.size, *refs), "idn_nlmeans_weights")
    return wt, shift.value, fpm.value


def _nlm_check(name: str, x, channels, t, s, strengths) -> None:
    """argument errors of the non-local means wrappers, raised before the device is looked at"""
    check_image(name, x, channels=channels)
    if t not in (3, 5, 7):
        raise ValueError(f"{name}: template_window must be odd and in 3..7, got {t!r}")
    if s not in range(5, 22, 2):
        raise ValueError(f"{name}: search_window must be odd and in 5..21, got {s!r}")
    for what, h in strengths:
        if not (isinstance(h, numbers.Real) and 0 < h < float("inf")):
            raise ValueError(f"{name}: {what} must be positive and finite, got {h!r}")
    need = t // 2 + s // 2 + 1
    if min(x.shape[-3], x.shape[-2]) < need:
        raise ValueError(f"{name}: image {x.shape[-3]} x {x.shape[-2]} smaller than the {need} "
                         "pixels the template and search windows need")


def _nlm_table(name: str, device, what: str, h, c: int, t: int, s: int) -> torch.Tensor:
    """the weight table of (h, c, t, s) on the device, built once per device and key"""
    key = (str(device), float(h), c, t, s)
    wt = _NLM_CACHE.get(key)
    if wt is None:
        if c == 2:
            host = nl_means_colored_weights(1.0, h, t, s)[1]
        else:
            host, _, _ = nl_means_weights(h, c, t, s)
        if host.size > NLMEANS_MAX_WEIGHTS:
            raise _lib.IdnError(f"{name}: unsupported: {what} = {h} gives a weight table of "
                                f"{host.size} entries, above NLMEANS_MAX_WEIGHTS "
                                f"({NLMEANS_MAX_WEIGHTS})")
        wt = torch.from_numpy(host).to(device)
        _NLM_CACHE[key] = wt
    return wt


def nl_means(x: torch.Tensor, h: float = 3.0, template_window: int = 7, search_window: int = 21,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.fastNlMeansDenoising(x, None, h, template_window, search_window) in OpenCV 3.4's 8-bit
    integer scheme, per image; 1 or 3 channels (3 channels are denoised jointly, as cv2 does for a
    3-channel input: this is not fastNlMeansDenoisingColored, which is nl_means_colored).  Bit-equal
    to the numpy model tests/nlm_model.py.  h must be of the order of the noise's standard
    deviation on the 0..255 scale: far below it every patch but the pixel's own gets weight 0 and
    the input comes back.  x may be contiguous or have padded rows; out, if given, must then share
    x's layout."""
    t, s = template_window, search_window
    _nlm_check("nl_means", x, (1, 3), t, s, (("h", h),))
    t, s = int(t), int(s)
    xb, y, pitch, sq = _image_layout("nl_means", x, out)
    n, hh, w, c = xb.shape
    wt = _nlm_table("nl_means", xb.device, "h", h, c, t, s)
    rc = _lib.load().idn_nlmeans_u8(xb.data_ptr(), y.data_ptr(), n, hh, w, c, pitch, t, s,
                                    wt.data_ptr(), wt.numel(), _stream())
    _lib.check(rc, "idn_nlmeans_u8")
    return out if out is not None else _finish(y, sq)


def nl_means_colored_weights(h: float, h_color: float, template_window: int = 7,
                             search_window: int = 21):
    """The two weight tables of nl_means_colored as int32 numpy arrays, (h, 1 channel) for L and
    (h_color, 2 channels) for (a, b), with the shift and the fixed-point multiplier
    (idn_nlmeans_colored_weights; host only, no GPU needed)."""
    lib = _lib.load()
    nl, nab, shift, fpm = (ctypes.c_int(0) for _ in range(4))
    args = (float(h), float(h_color), int(template_window), int(search_window))
    tail = (ctypes.byref(shift), ctypes.byref(fpm))
    rc = lib.idn_nlmeans_colored_weights(*args, None, 0, ctypes.byref(nl), None, 0,
                                         ctypes.byref(nab), *tail)
    _lib.check(rc, "idn_nlmeans_colored_weights")
    wl = np.empty(nl.value, dtype=np.int32)
    wab = np.empty(nab.value, dtype=np.int32)
    rc = lib.idn_nlmeans_colored_weights(*args, wl.ctypes.data, wl.size, ctypes.byref(nl),
                                         wab.ctypes.data, wab.size, ctypes.byref(nab), *tail)
    _lib.check(rc, "idn_nlmeans_colored_weights")
    return wl, wab, shift.value, fpm.value


def nl_means_colored(x: torch.Tensor, h: float = 3.0, h_color: float = 3.0,
                     template_window: int = 7, search_window: int = 21,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.fastNlMeansDenoisingColored(x, None, h, h_color, template_window, search_window) on
    uint8 BGR images, per image: to 8-bit Lab with OpenCV's linear conversion (COLOR_LBGR2Lab),
    nl_means on L with h and on (a, b) jointly with h_color, and back (COLOR_Lab2LBGR).  Bit-equal
    to the numpy model tests/nlm_colored_model.py.  The 8-bit Lab round trip is not the identity:
    with strengths too small to change anything the result is still up to (4, 2, 5) away from x in
    (B, G, R).  h and h_color are on the 0..255 scale of the Lab bytes and of the order of the
    noise there.  x may be contiguous or have padded rows; out, if given, must then share x's
    layout."""
    t, s = template_window, search_window
    _nlm_check("nl_means_colored", x, (3,), t, s, (("h", h), ("h_color", h_color)))
    t, s = int(t), int(s)
    xb, y, pitch, sq = _image_layout("nl_means_colored", x, out)
    n, hh, w, _ = xb.shape
    wl = _nlm_table("nl_means_colored", xb.device, "h", h, 1, t, s)
    wab = _nlm_table("nl_means_colored", xb.device, "h_color", h_color, 2, t, s)
    lib = _lib.load()
    nbytes = lib.idn_nlmeans_colored_workspace_size(n, hh, w)
    ws = _workspace(nbytes, xb.device)
    rc = lib.idn_nlmeans_colored_u8(xb.data_ptr(), y.data_ptr(), n, hh, w, pitch, t, s,
                                    wl.data_ptr(), wl.numel(), wab.data_ptr(), wab.numel(),
                                    ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "idn_nlmeans_colored_u8")
    return out if out is not None else _finish(y, sq)
