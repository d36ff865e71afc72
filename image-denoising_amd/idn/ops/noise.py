"""The noise generators: skimage's random_noise, the reference's additive noises, the periodic
pattern, the slot forms for mixed batches, and the noise -> filter step."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ._args import (_as_batch, _finish, _ids_tensor, _ptr, _seed64, _slots_tensor, _stream,
                    _u8_batch, _workspace)
from .filters import blur, gaussian_blur

NOISE_KINDS = {"gaussian": 0, "speckle": 1, "s&p": 2, "sap": 2, "poisson": 3}


def _empty_like_img(xb: torch.Tensor, dtype) -> torch.Tensor:
    return torch.empty(xb.shape, dtype=dtype, device=xb.device)


def _noise_kind(mode: str, mean, var, amount, salt_vs_pepper):
    """random_noise's mode -> (kind, p0, p1) of idn_noise_u8"""
    kind = NOISE_KINDS.get(mode.lower())
    if kind is None:
        raise ValueError(f"random_noise: unsupported mode {mode!r}; supported: {sorted(NOISE_KINDS)}")
    if kind in (0, 1):
        return kind, float(mean), float(var)
    if kind == 2:
        return kind, float(amount), float(salt_vs_pepper)
    return kind, 0.0, 0.0


def _noise_outputs(name: str, xb: torch.Tensor, out: str, out_u8: Optional[torch.Tensor]):
    """out = 'u8' / 'f64' / 'both' -> (y8, y64), each a batch shaped like xb or None"""
    want_u8 = out in ("u8", "both")
    want_f64 = out in ("f64", "both")
    if not (want_u8 or want_f64):
        raise ValueError(f"{name}: out must be 'u8', 'f64' or 'both'")
    y8 = (out_u8.view(xb.shape) if out_u8 is not None else _empty_like_img(xb, torch.uint8)) if want_u8 else None
    y64 = _empty_like_img(xb, torch.float64) if want_f64 else None
    return y8, y64


def _noise_result(out: str, y8, y64, squeeze: bool):
    if out == "u8":
        return _finish(y8, squeeze)
    if out == "f64":
        return _finish(y64, squeeze)
    return _finish(y8, squeeze), _finish(y64, squeeze)


def _replay_field(replay, xb: torch.Tensor, need: int, bad: str, bad_count: Optional[str] = None):
    """the replayed random field, contiguous: float64 on xb's device with `need` elements (the
    messages are the caller's; bad_count may name {got} and {need})"""
    if replay is None:
        return None
    if replay.device != xb.device or replay.dtype != torch.float64:
        raise ValueError(bad)
    if replay.numel() != need:
        raise ValueError((bad_count or bad).format(got=replay.numel(), need=need))
    return replay.contiguous()


def _stream_ids(name: str, image_ids, replay, n: int, device) -> Optional[torch.Tensor]:
    if image_ids is None:
        return None
    if replay is not None:
        raise ValueError(f"{name}: image_ids applies to the Philox stream, not to replay")
    return _ids_tensor(image_ids, n, device)


def random_noise(x: torch.Tensor, mode: str = "gaussian", *, mean: float = 0.0, var: float = 0.01,
                 amount: float = 0.05, salt_vs_pepper: float = 0.5, seed: int = 0,
                 offset: int = 0, replay: Optional[torch.Tensor] = None, out: str = "u8",
                 out_u8: Optional[torch.Tensor] = None, image_ids=None, slots=None):
    """skimage.util.random_noise(x, mode, ...) on a uint8 batch, plus the caller's U8 cast.

    out="u8"   -> (255 * random_noise(...)).astype(np.uint8)   (denoise-branch input)
    out="f64"  -> random_noise(...) as float64 in [0, 1]        ("plain" branch result)
    out="both" -> (u8, f64)
    replay: None draws from the Philox stream keyed by (seed, offset + image index); otherwise the
    random field numpy would have drawn (gaussian/speckle: N(mean, sqrt(var)) field of x.shape;
    s&p: float64 [2, *x.shape] random_sample fields for `flipped` then `salted`; poisson: the
    Poisson draws), which makes the result bit-exact with the reference.
    image_ids: optional per-image ids (Philox stream only) instead of offset + index -- one launch
    for any subset of a batch, drawing what per-image calls with offset = id would.
    slots: with image_ids, an int64 device tensor of batch positions: only images x[slots] are
    noised, written to out_u8[slots] (out="u8", out_u8 required, the rest of out_u8 untouched) --
    a mixed batch's per-type group with no gather / scatter of its images.
    """
    if slots is not None:
        return _random_noise_slots(x, mode, mean, var, amount, salt_vs_pepper, seed, out, out_u8,
                                   image_ids, slots)
    kind, p0, p1 = _noise_kind(mode, mean, var, amount, salt_vs_pepper)
    xb, sq = _u8_batch(x, "random_noise")
    n, h, w, c = xb.shape
    y8, y64 = _noise_outputs("random_noise", xb, out, out_u8)
    rp = _replay_field(replay, xb, (2 if kind == 2 else 1) * xb.numel(),
                       "random_noise: replay must be a float64 tensor on the same device",
                       "random_noise: replay has {got} elements, expected {need}")
    lib = _lib.load()
    ws_bytes = lib.idn_noise_workspace_size(kind, n)
    ws = _workspace(ws_bytes, xb.device) if ws_bytes else None
    ids = _stream_ids("random_noise", image_ids, rp, n, xb.device)
    head = (xb.data_ptr(), _ptr(y8), _ptr(y64), n, h, w, c, w * c, kind, p0, p1, _seed64(seed))
    if ids is not None:
        rc = lib.idn_noise_ids_u8(*head, ids.data_ptr(), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "idn_noise_ids_u8")
    else:
        rc = lib.idn_noise_u8(*head, int(offset), _ptr(rp), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "idn_noise_u8")
    return _noise_result(out, y8, y64, sq)


def ycc_fusable(x: torch.Tensor) -> bool:
    """random_noise_ycc takes this batch: uint8, 3 channels, an even pixel count per image, and
    not a contiguous view that starts at an odd address (idn_noise_ycc_u8 reads byte pairs; a
    batch that is not contiguous is copied first, to an aligned address)"""
    return (x.dtype == torch.uint8 and x.shape[-1] == 3 and (x.shape[-3] * x.shape[-2]) % 2 == 0
            and not (x.is_contiguous() and x.data_ptr() % 2))


def random_noise_ycc(x: torch.Tensor, mode: str = "gaussian", *, mean: float = 0.0,
                     var: float = 0.01, seed: int = 0, offset: int = 0,
                     replay: Optional[torch.Tensor] = None, image_ids=None):
    """random_noise(x, mode, out='f64') for gaussian / speckle, fused with the wavelet's colour
    range (idn_noise_ycc_u8; lib/model/test.py:1678-1684 -> 1807-1810: the float64 image goes
    straight into denoise_wavelet).  Returns (the float64 image -- the same values as
    random_noise(..., out='f64') -- and an (N, 6) int64 device tensor of per-image YCbCr min / max
    keys for denoise_wavelet(..., ycc_keys=...))."""
    kind = NOISE_KINDS.get(mode.lower())
    if kind not in (0, 1):
        raise ValueError(f"random_noise_ycc: gaussian or speckle only (got {mode!r})")
    xb, sq = _u8_batch(x, "random_noise_ycc")
    n, h, w, c = xb.shape
    if c != 3:
        raise ValueError("random_noise_ycc: needs 3 channels")
    xb = xb.contiguous()
    y64 = _empty_like_img(xb, torch.float64)
    keys = torch.empty((n, 6), dtype=torch.int64, device=xb.device)
    rp = _replay_field(replay, xb, xb.numel(),
                       "random_noise_ycc: replay must be a float64 field of x's shape on its device")
    ids = _stream_ids("random_noise_ycc", image_ids, rp, n, xb.device)
    rc = _lib.load().idn_noise_ycc_u8(xb.data_ptr(), None, y64.data_ptr(), n, h, w, kind,
                                      float(mean), float(var), _seed64(seed), int(offset),
                                      _ptr(ids), _ptr(rp), keys.data_ptr(), _stream())
    _lib.check(rc, "idn_noise_ycc_u8")
    return _finish(y64, sq), keys


def _random_noise_slots(x, mode, mean, var, amount, salt_vs_pepper, seed, out, out_u8, image_ids,
                        slots):
    kind, p0, p1 = _noise_kind(mode, mean, var, amount, salt_vs_pepper)
    if out != "u8" or out_u8 is None or image_ids is None:
        raise ValueError("random_noise: slots needs out='u8', out_u8 and image_ids")
    xb, _ = _u8_batch(x, "random_noise")
    nb, h, w, c = xb.shape
    if not (isinstance(out_u8, torch.Tensor) and out_u8.dtype == torch.uint8
            and out_u8.device == xb.device and out_u8.is_contiguous()
            and tuple(out_u8.shape) in ((nb, h, w, c), (h, w, c) if nb == 1 else ())):
        raise ValueError("random_noise: slots needs out_u8 = a contiguous uint8 tensor shaped "
                         "like x on x's device")
    y8 = out_u8.view(nb, h, w, c)
    sl = _slots_tensor(slots, xb.device)
    n = sl.numel()
    ids = _ids_tensor(image_ids, n, xb.device)
    lib = _lib.load()
    ws_bytes = lib.idn_noise_workspace_size(kind, n)
    ws = _workspace(ws_bytes, xb.device) if ws_bytes else None
    rc = lib.idn_noise_slots_u8(xb.data_ptr(), y8.data_ptr(), None, n, h, w, c, w * c, kind, p0, p1,
                                _seed64(seed), ids.data_ptr(), sl.data_ptr(), _ptr(ws), ws_bytes,
                                _stream())
    _lib.check(rc, "idn_noise_slots_u8")
    return out_u8


ADD_NOISE_KINDS = {"uniform": 4, "gamma": 5, "rayleigh": 6, "brownian": 7}
GAMMA_SHAPE = 1.99  # a = 1.99 in every gamma closure (lib/model/test.py:1303)


def noise_add(x: torch.Tensor, mode: str, level: float, *, seed: int = 0, offset: int = 0,
              replay: Optional[torch.Tensor] = None, out: str = "u8",
              out_u8: Optional[torch.Tensor] = None, shape: float = GAMMA_SHAPE, image_ids=None):
    """The reference's own additive noises (lib/model/test.py:767-1572), u8 batch in:
      uniform  level = high:  out = img_as_float(x) + np.random.uniform(0, high)
      gamma    level = scale: out = x + scipy.stats.gamma.rvs(1.99, scale=level)
      rayleigh level = scale: out = x + scipy.stats.rayleigh.rvs(scale=level)
      brownian level = dt:    u8 = cv2.add(img, U8(255 * cumsum-walk)), f64 = the walk B
    cv2.add(float64, float64) does not clip: out="f64" is the unclipped sum (what train_v0's plain
    branches return), out="u8" is (255 * out).astype(np.uint8) with its modulo-256 wrap.
    replay: numpy's unit draws (random_sample / standard_gamma(1.99) / sqrt(chisquare(2)) /
    for brownian the normals with element e holding z[e-1]), float64 of x's shape.
    image_ids: optional per-image ids (Philox stream only), as in random_noise."""
    kind = ADD_NOISE_KINDS.get(mode.lower())
    if kind is None:
        raise ValueError(f"noise_add: unsupported mode {mode!r}; supported: {sorted(ADD_NOISE_KINDS)}")
    xb, sq = _u8_batch(x, "noise_add")
    n, h, w, c = xb.shape
    y8, y64 = _noise_outputs("noise_add", xb, out, out_u8)
    p0, p1 = (float(shape), float(level)) if kind == 5 else (float(level), 0.0)
    rp = _replay_field(replay, xb, xb.numel(),
                       "noise_add: replay must be float64, on the same device, one value per element")
    lib = _lib.load()
    ws_bytes = lib.idn_noise_add_workspace_size(kind, n, h, w, c)
    ws = _workspace(ws_bytes, xb.device) if ws_bytes else None
    ids = _stream_ids("noise_add", image_ids, rp, n, xb.device)
    head = (xb.data_ptr(), _ptr(y8), _ptr(y64), n, h, w, c, w * c, kind, p0, p1, _seed64(seed))
    if ids is not None:
        rc = lib.idn_noise_add_ids_u8(*head, ids.data_ptr(), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "idn_noise_add_ids_u8")
    else:
        rc = lib.idn_noise_add_u8(*head, int(offset), _ptr(rp), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "idn_noise_add_u8")
    return _noise_result(out, y8, y64, sq)


_PATTERN_CACHE: dict = {}


def periodic_pattern(h: int, w: int, c: int, amplitude: float, device=None) -> torch.Tensor:
    """U8(255*sin(linspace(-A, A, h*w*c))).reshape(h, w, c); cached per (h, w, c, A, device)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    key = (h, w, c, float(amplitude), str(dev))
    pat = _PATTERN_CACHE.get(key)
    if pat is None:
        pat = torch.empty((h, w, c), dtype=torch.uint8, device=dev)
        rc = _lib.load().idn_periodic_pattern_u8(pat.data_ptr(), h, w, c, float(amplitude), _stream())
        _lib.check(rc, "idn_periodic_pattern_u8")
        _PATTERN_CACHE[key] = pat
    return pat


def add_pattern(x: torch.Tensor, pattern: torch.Tensor, out: Optional[torch.Tensor] = None,
                slots=None) -> torch.Tensor:
    """cv2.add(x, pattern) (u8 saturating), pattern broadcast over the batch.  slots (int64 device
    tensor, out required): only images x[slots] -> out[slots]."""
    xb, sq = _u8_batch(x, "add_pattern")
    n, h, w, c = xb.shape
    if tuple(pattern.shape) != (h, w, c) or pattern.dtype != torch.uint8:
        raise ValueError(f"add_pattern: pattern must be uint8 {(h, w, c)}, got {tuple(pattern.shape)}")
    if slots is not None:
        if out is None:
            raise ValueError("add_pattern: slots needs out")
        sl = _slots_tensor(slots, xb.device)
        rc = _lib.load().idn_add_pattern_slots_u8(xb.data_ptr(), pattern.contiguous().data_ptr(),
                                                  out.data_ptr(), sl.numel(), h, w, c,
                                                  sl.data_ptr(), _stream())
        _lib.check(rc, "idn_add_pattern_slots_u8")
        return out
    y = torch.empty_like(xb) if out is None else out.view(n, h, w, c)
    rc = _lib.load().idn_add_pattern_u8(xb.data_ptr(), pattern.contiguous().data_ptr(), y.data_ptr(),
                                        n, h, w, c, w * c, _stream())
    _lib.check(rc, "idn_add_pattern_u8")
    return _finish(y, sq)


def periodic_noise(x: torch.Tensor, amplitude: float, out: Optional[torch.Tensor] = None,
                   slots=None) -> torch.Tensor:
    """add_periodic_noise: cv2.add(img, U8(255*sin(linspace(-A, A, img.size))).reshape(h,w,3))."""
    xb, _ = _as_batch(x, "periodic_noise")
    _, h, w, c = xb.shape
    return add_pattern(x, periodic_pattern(h, w, c, amplitude, xb.device), out=out, slots=slots)


def copy_slots(x: torch.Tensor, out: torch.Tensor, slots) -> torch.Tensor:
    """out[slots] = x[slots] for a uint8 batch (the noise-free members of a mixed batch)."""
    xb, _ = _u8_batch(x, "copy_slots")
    if out.shape != x.shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("copy_slots: out must be a contiguous uint8 tensor shaped like x")
    sl = _slots_tensor(slots, xb.device)
    per_img = xb[0].numel() if xb.shape[0] else 1
    rc = _lib.load().idn_copy_slots_u8(xb.data_ptr(), out.data_ptr(), sl.numel(), per_img,
                                       sl.data_ptr(), _stream())
    _lib.check(rc, "idn_copy_slots_u8")
    return out


# ---- fused steps -------------------------------------------------------------------------------

FILTERS = {"gaus_blur": 0, "mean": 1}


def noise_filter(x: torch.Tensor, mode: str, filter: str, ksize: int, *, var: float = 0.01,
                 amount: float = 0.05, salt_vs_pepper: float = 0.5, seed: int = 0,
                 offset: int = 0, image_ids=None, out: Optional[torch.Tensor] = None,
                 form: str = "serial"):
    """random_noise(x, mode, ...) -> U8 -> cv2.GaussianBlur (filter 'gaus_blur') or cv2.blur
    ('mean'); the result is identical in every form (Philox u8 stream keyed by (seed, image id)).
      form 'serial'    the noise launch, then the filter launch (the default: fastest measured,
                       profiles/r02/README.md -- the noise is VALU-bound; a one-pass fused LDS-ring
                       form measured slower and was removed in round 3)
      form 'pipelined' the batch in chunks: the noise of chunk k+1 (VALU-bound) runs on a side
                       stream beside the filter of chunk k (HBM-bound), whose input is still in
                       the 256 MB Infinity Cache"""
    if form == "pipelined":
        return _noise_filter_pipelined(x, mode, filter, ksize, var=var, amount=amount,
                                       salt_vs_pepper=salt_vs_pepper, seed=seed, offset=offset,
                                       image_ids=image_ids, out=out)
    if form != "serial":
        raise ValueError("noise_filter: form must be 'serial' or 'pipelined'")
    kind = NOISE_KINDS.get(mode.lower())
    if kind is None or kind == 3:
        raise ValueError(f"noise_filter: mode {mode!r} not supported (gaussian, speckle, s&p)")
    if filter not in FILTERS:
        raise ValueError(f"noise_filter: filter must be one of {sorted(FILTERS)}")
    xb, sq = _u8_batch(x, "noise_filter")
    n, h, w, c = xb.shape
    y = torch.empty_like(xb) if out is None else out.view(n, h, w, c)
    kw = dict(amount=amount, salt_vs_pepper=salt_vs_pepper) if kind == 2 else dict(var=var)
    t = random_noise(xb, mode, seed=seed, offset=offset, image_ids=image_ids, out="u8", **kw)
    return _finish((gaussian_blur if filter == "gaus_blur" else blur)(t, ksize, out=y), sq)


_PIPE_STREAMS: dict = {}


def _noise_filter_pipelined(x, mode, filter, ksize, *, var, amount, salt_vs_pepper, seed, offset,
                            image_ids, out, chunk: int = 32):
    xb, sq = _u8_batch(x, "noise_filter")
    n = xb.shape[0]
    y = torch.empty_like(xb) if out is None else out.view(xb.shape)
    main = torch.cuda.current_stream(xb.device)
    side = _PIPE_STREAMS.get(xb.device)
    if side is None:
        side = _PIPE_STREAMS[xb.device] = torch.cuda.Stream(device=xb.device)
    tmp = _workspace(xb.numel(), xb.device)[: xb.numel()].view(xb.shape)
    kw = dict(amount=amount, salt_vs_pepper=salt_vs_pepper) if mode in ("s&p", "sap") else \
        dict(var=var)
    flt = gaussian_blur if filter == "gaus_blur" else blur
    side.wait_stream(main)  # inputs / outputs are ready on the caller's stream
    ids_all = _ids_tensor(image_ids, n, xb.device) if image_ids is not None else None
    prev = None
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        with torch.cuda.stream(side):
            if ids_all is None:
                random_noise(xb[lo:hi], mode, seed=seed, offset=offset + lo, out="u8",
                             out_u8=tmp[lo:hi], **kw)
            else:
                random_noise(xb[lo:hi], mode, seed=seed, image_ids=ids_all[lo:hi], out="u8",
                             out_u8=tmp[lo:hi], **kw)
            ev = torch.cuda.Event()
            ev.record(side)
        if prev is not None:
            main.wait_event(prev[2])
            flt(tmp[prev[0]:prev[1]], ksize, out=y[prev[0]:prev[1]])
        prev = (lo, hi, ev)
    if prev is not None:
        main.wait_event(prev[2])
        flt(tmp[prev[0]:prev[1]], ksize, out=y[prev[0]:prev[1]])
    side.wait_stream(main)  # tmp (shared scratch) is not reused by the side stream early
    return _finish(y, sq)
