"""Tensor-level ops over the HIP C-ABI (device tensors in, device tensors out).

Every function takes uint8 images shaped (H, W, C) or (N, H, W, C) living on a ROCm device
(torch "cuda" tensors) and launches on torch's current stream.  Names and argument meaning follow
the OpenCV / scikit-image calls the reference makes on its preprocessing path:

  gaussian_blur(x, ksize, sigma=0)        cv2.GaussianBlur(x, (ksize, ksize), sigma), odd 3..31
  blur(x, ksize=3)                        cv2.blur(x, (ksize, ksize)), odd ksize 3..31
  median_blur(x, ksize)                   cv2.medianBlur(x, ksize), odd ksize 3..31
  adaptive_median(x, max_ksize)           the window-growing median (Gonzalez & Woods §5.3)
  bilateral_filter(x, d, sc, ss)          cv2.bilateralFilter(x, d, sc, ss, BORDER_CONSTANT)
  random_noise(x, mode, ...)              skimage.util.random_noise (+ U8 cast)
  periodic_pattern / add_pattern          add_periodic_noise's linspace/sin pattern, cv2.add
  denoise_wavelet(x, wavelet, levels)     skimage.restoration.denoise_wavelet (0.14.2 wrapper)
  blob(x, ...)                            lib/utils/blob.py prep_im_for_blob + im_list_to_blob
  mse / psnr / ssim(x, y)                 skimage.measure.compare_mse / _psnr / _ssim (0.14.2)
  nl_means(x, h, t, s)                    cv2.fastNlMeansDenoising(x, None, h, t, s) (3.4, 8-bit)
  nl_means_colored(x, h, h_color, t, s)   cv2.fastNlMeansDenoisingColored(x, None, h, h_color, t, s)
  denoise_tv_chambolle(x, weight, eps, n) skimage.restoration.denoise_tv_chambolle (0.14.2)
  estimate_sigma(x, average_sigmas)       skimage.restoration.estimate_sigma (multichannel=True)
  wiener(x, ksize, noise, border=...)     scipy.signal.wiener per channel plane (1.15.3)
  equalize_hist(x)                        cv2.equalizeHist(x)
  clahe(x, clip_limit, tile_grid)         cv2.createCLAHE(clip_limit, tile_grid).apply(x)
  cvt_color_yuv(x, to_yuv)                cv2.cvtColor(x, COLOR_BGR2YUV / COLOR_YUV2BGR)
  correct_exposure(x, denoise)            Automold.correct_exposure (tools/Automold.py:817-842)

There is no CPU path: a CPU tensor raises, a missing library raises.
"""
from __future__ import annotations

import ctypes
import numbers
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

PIXEL_MEANS = (102.9801, 115.9465, 122.7717)  # lib/model/config.py:252 (BGR)

NOISE_KINDS = {"gaussian": 0, "speckle": 1, "s&p": 2, "sap": 2, "poisson": 3}
MEDIAN_MAX_KSIZE = 31  # idn_median_blur_u8: odd ksize 3..MEDIAN_MAX_KSIZE
ADAPTIVE_MEDIAN_MAX_KSIZE = 31  # idn_adaptive_median_u8: odd max_ksize 3..31
BLUR_MAX_KSIZE = 31    # idn_gaussian_blur_u8 / idn_box_blur_u8: odd ksize 3..BLUR_MAX_KSIZE
# strip rows x byte columns (W*C) of one workgroup of the wide kernels: the box, and the Gaussian
# by channel count (whole groups of 4 pixels)
BLUR_TILE = {"box": (128, 256),
             "gaussian": {1: (128, 256), 2: (128, 256), 3: (128, 252), 4: (128, 256)}}
WAVELETS = {"db1": 0, "haar": 0, "bior1.5": 1, "db2": 2, "sym4": 3, "coif5": 4}  # idn_wavelet


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _as_batch(x: torch.Tensor, name: str) -> Tuple[torch.Tensor, bool]:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.device.type != "cuda":
        raise ValueError(f"{name}: idn runs on the GPU only; got a {x.device} tensor "
                         "(move it with .cuda(); there is no CPU fallback)")
    squeeze = False
    if x.dim() == 3:
        x = x.unsqueeze(0)
        squeeze = True
    if x.dim() != 4:
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    return x, squeeze


def _u8_batch(x: torch.Tensor, name: str) -> Tuple[torch.Tensor, bool]:
    x, sq = _as_batch(x, name)
    if x.dtype != torch.uint8:
        raise TypeError(f"{name}: expected uint8 images, got {x.dtype}")
    if not x.is_contiguous():
        x = x.contiguous()
    return x, sq


def _finish(out: torch.Tensor, squeeze: bool) -> torch.Tensor:
    return out[0] if squeeze else out


def _filter(fn_name: str, x: torch.Tensor, *args, out: Optional[torch.Tensor] = None):
    xb, sq = _u8_batch(x, fn_name)
    n, h, w, c = xb.shape
    y = torch.empty_like(xb) if out is None else out.view(n, h, w, c)
    if n == 0:  # an empty tensor has no storage: its null data_ptr() is not for the C ABI
        return _finish(y, sq)
    lib = _lib.load()
    rc = getattr(lib, fn_name)(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c, *args, _stream())
    _lib.check(rc, fn_name)
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
    xb, sq = _u8_batch(x, fn_name)
    n, h, w, c = xb.shape
    y = torch.empty_like(xb) if out is None else out.view(n, h, w, c)
    km = torch.empty_like(xb) if return_ksize else None
    if n != 0:  # an empty tensor has no storage: its null data_ptr() is not for the C ABI
        rc = _lib.load().idn_adaptive_median_u8(
            xb.data_ptr(), y.data_ptr(), None if km is None else km.data_ptr(), n, h, w, c, w * c,
            int(max_ksize), _stream())
        _lib.check(rc, fn_name)
    if return_ksize:
        return _finish(y, sq), _finish(km, sq)
    return _finish(y, sq)


def bilateral_filter(x: torch.Tensor, d: int = 9, sigma_color: float = 20.0,
                     sigma_space: float = 100.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cv2.bilateralFilter(x, d, sigma_color, sigma_space, borderType=BORDER_CONSTANT)."""
    return _filter("idn_bilateral_u8", x, int(d), float(sigma_color), float(sigma_space), out=out)


# ---- noise generators ------------------------------------------------------------------------

def _empty_like_img(xb: torch.Tensor, dtype) -> torch.Tensor:
    return torch.empty(xb.shape, dtype=dtype, device=xb.device)


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


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return t.data_ptr() if t is not None else None


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
    head = (xb.data_ptr(), _ptr(y8), _ptr(y64), n, h, w, c, w * c, kind, p0, p1,
            int(seed) & (2 ** 64 - 1))
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
                                      float(mean), float(var), int(seed) & (2 ** 64 - 1),
                                      int(offset), _ptr(ids), _ptr(rp), keys.data_ptr(),
                                      _stream())
    _lib.check(rc, "idn_noise_ycc_u8")
    return _finish(y64, sq), keys


def _slots_tensor(slots, device) -> torch.Tensor:
    """The caller owns slot validity (0 <= slot < batch size, as for device image-id tensors):
    checking a device tensor's values would cost a host sync per launch."""
    if not (isinstance(slots, torch.Tensor) and slots.device == device
            and slots.dtype == torch.int64):
        raise ValueError("slots must be an int64 tensor on the batch's device")
    return slots.reshape(-1).contiguous()


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
                                int(seed) & (2 ** 64 - 1), ids.data_ptr(), sl.data_ptr(),
                                _ptr(ws), ws_bytes, _stream())
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
    head = (xb.data_ptr(), _ptr(y8), _ptr(y64), n, h, w, c, w * c, kind, p0, p1,
            int(seed) & (2 ** 64 - 1))
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


def gaussian_blob(x: torch.Tensor, ksize: int = 5, pixel_means=PIXEL_MEANS,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """blob(gaussian_blur(x, ksize)) at scale 1.0 in one pass: float32 (N, H, W, 3)
    float32(float64(v) - mean[ch]) written by the filter (idn_gaussian_blob_f32)."""
    xb, _ = _u8_batch(x, "gaussian_blob")
    n, h, w, c = xb.shape
    y = torch.empty((n, h, w, c), dtype=torch.float32, device=xb.device) if out is None else out
    m = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1)])
    rc = _lib.load().idn_gaussian_blob_f32(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c,
                                           int(ksize), m, _stream())
    if rc == -2:
        return blob(gaussian_blur(xb, ksize), pixel_means, out=y)
    _lib.check(rc, "idn_gaussian_blob_f32")
    return y


# ---- quant: colour quantisation by k-means in 8-bit Lab ----------------------------------------

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
    rc = lib.idn_quant_u8(xb.data_ptr(), y.data_ptr(), lab.data_ptr() if lab is not None else None,
                          n, h, w, w * 3, k, int(seed) & (2 ** 64 - 1), int(offset),
                          ids.data_ptr() if ids is not None else None,
                          cin.data_ptr() if cin is not None else None,
                          cen_out.data_ptr() if cen_out is not None else None,
                          ws.data_ptr() if ws is not None else None, ws_bytes, _stream())
    _lib.check(rc, "idn_quant_u8")
    res = [_finish(y, sq)]
    if return_labels:
        res.append(_finish(lab, sq))
    if return_centers:
        res.append(_finish(cen_out, sq))
    return res[0] if len(res) == 1 else tuple(res)


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


def copy_flat(x: torch.Tensor, out: torch.Tensor, policy: int = 0) -> torch.Tensor:
    """out <- x as one flat byte copy (the bench's copy ceiling; policy 1 = nontemporal)."""
    if x.device.type != "cuda" or out.device != x.device:
        raise ValueError("copy_flat: both tensors must be on the same GPU")
    if not (x.is_contiguous() and out.is_contiguous()) or x.nbytes != out.nbytes:
        raise ValueError("copy_flat: contiguous tensors of equal byte size required")
    rc = _lib.load().idn_copy_u8(x.data_ptr(), out.data_ptr(), x.nbytes, int(policy), _stream())
    _lib.check(rc, "idn_copy_u8")
    return out


# ---- blob epilogue -----------------------------------------------------------------------------

def blob(x: torch.Tensor, pixel_means=PIXEL_MEANS, out_hw: Optional[Tuple[int, int]] = None,
         flip: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """prep_im_for_blob (scale 1.0) + im_list_to_blob: float32 NHWC, mean-subtracted, zero-padded."""
    xb, _ = _u8_batch(x, "blob")
    n, h, w, c = xb.shape
    oh, ow = out_hw if out_hw is not None else (h, w)
    y = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=xb.device) if out is None else out
    m = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1)])
    rc = _lib.load().idn_blob_f32(xb.data_ptr(), y.data_ptr(), n, h, w, c, w * c, oh, ow, m,
                                  1 if flip else 0, _stream())
    _lib.check(rc, "idn_blob_f32")
    return y


# ---- wavelet denoise ---------------------------------------------------------------------------

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
            src.data_ptr() if src is not None else None,
            src64.data_ptr() if src64 is not None else None,
            y8.data_ptr() if y8 is not None else None,
            y32.data_ptr() if y32 is not None else None, n, h, w, c, w * c, wv, lv,
            WAVELET_METHODS[method], WAVELET_MODES[mode], int(convert2ycbcr),
            sig.data_ptr() if sig is not None else None, ws.data_ptr(), nbytes, _stream())
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
                                         y8.data_ptr() if y8 is not None else None,
                                         y32.data_ptr() if y32 is not None else None,
                                         n, h, w, wv, lv, ws.data_ptr(), nbytes, _stream())
        _lib.check(rc, "idn_wavelet_denoise_ycc")
        return result()
    rc = lib.idn_wavelet_denoise_u8(src.data_ptr() if src is not None else None,
                                    src64.data_ptr() if src64 is not None else None,
                                    y8.data_ptr() if y8 is not None else None,
                                    y32.data_ptr() if y32 is not None else None,
                                    n, h, w, w * 3, wv, lv, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "idn_wavelet_denoise_u8")
    return result()


# ---- non-local means -----------------------------------------------------------------------------

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


def _row_pitch(t: torch.Tensor):
    """row pitch in bytes of a (N,H,W,C) uint8 tensor whose rows are compact or padded (images
    h*pitch apart), or None for any other layout"""
    n, h, w, c = t.shape
    sn, sh, sw, sc = t.stride()
    if sc == 1 and sw == c and sh >= w * c and (n == 1 or sn == h * sh):
        return sh
    return None


def _nlm_check(name: str, x, channels, t, s, strengths) -> None:
    """argument errors of the non-local means wrappers, raised before the device is looked at"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.uint8:
        raise TypeError(f"{name}: expected uint8 images, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    if x.shape[-1] not in channels:
        raise ValueError(f"{name}: {' or '.join(map(str, channels))} channels supported, "
                         f"got {x.shape[-1]}")
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


def _nlm_layout(name: str, x: torch.Tensor, out: Optional[torch.Tensor]):
    """(source batch, destination batch, their common row pitch, squeeze) of x and out"""
    xb, sq = _as_batch(x, name)
    n, hh, w, c = xb.shape
    if out is not None:
        if out.dtype != torch.uint8 or out.shape != x.shape or out.device != x.device:
            raise ValueError(f"{name}: out must be a uint8 tensor shaped like x on x's device")
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
    xb, y, pitch, sq = _nlm_layout("nl_means", x, out)
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
    xb, y, pitch, sq = _nlm_layout("nl_means_colored", x, out)
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


# ---- exposure correction -------------------------------------------------------------------------

CLAHE_MAX_TILES = 16            # idn_clahe_u8: tiles per axis
EXPOSURE_TILE_GRID = (4, 4)     # exposure_process: createCLAHE(clipLimit=2.0, tileGridSize=(4,4))
EXPOSURE_NLM = (3.0, 3.0, 7, 21)  # its fastNlMeansDenoisingColored(., None, 3, 3, 7, 21)


def _exposure_check(name: str, x, channels: int, min_hw=(1, 1)) -> None:
    """argument errors of the exposure wrappers, raised before the device is looked at"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.uint8:
        raise TypeError(f"{name}: expected uint8 images, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    if x.shape[-1] != channels:
        raise ValueError(f"{name}: needs {channels} channel{'s' if channels > 1 else ''}, "
                         f"got {x.shape[-1]}")
    h, w = x.shape[-3], x.shape[-2]
    if h < min_hw[0] or w < min_hw[1]:
        raise ValueError(f"{name}: image {h} x {w} is smaller than the {min_hw[0]} x {min_hw[1]} "
                         "this call needs")


def _exposure_call(fn: str, name: str, x, out, grid, *params) -> torch.Tensor:
    """one histogram op of the C ABI: fn(src, dst, n, h, w, pitch, *params, workspace, bytes, stream)"""
    xb, y, pitch, sq = _nlm_layout(name, x, out)
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
    xb, y, pitch, sq = _nlm_layout(name, x, out)
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
    xb, y, pitch, sq = _nlm_layout(name, x, out)
    if xb.shape[0] == 0:
        return out if out is not None else _finish(y, sq)
    toned = torch.empty_strided(y.shape, y.stride(), dtype=torch.uint8, device=y.device)
    _exposure_call("idn_correct_exposure_u8", name, xb, toned, EXPOSURE_TILE_GRID)
    nl_means_colored(toned, h_nlm, hc_nlm, t_nlm, s_nlm, out=y)
    return out if out is not None else _finish(y, sq)


# ---- total-variation denoising -------------------------------------------------------------------

TV_MAX_ITER = 1000  # IDN_TV_MAX_ITER of include/idn.h


def _tv_check(x, weight, eps, n_iter_max, out, out_u8) -> None:
    """argument errors of denoise_tv_chambolle, raised before the device is looked at"""
    name = "denoise_tv_chambolle"
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.uint8:
        raise TypeError(f"{name}: expected uint8 images, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    if x.shape[-1] not in (1, 3):
        raise ValueError(f"{name}: 1 or 3 channels supported, got {x.shape[-1]}")
    if x.shape[-3] < 1 or x.shape[-2] < 1:
        raise ValueError(f"{name}: empty image {x.shape[-3]} x {x.shape[-2]}")
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
        if (not isinstance(out_u8, torch.Tensor) or out_u8.dtype != torch.uint8
                or out_u8.shape != x.shape or out_u8.device != x.device):
            raise ValueError(f"{name}: out_u8 must be a uint8 tensor shaped like x on x's device")


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
    name = "denoise_tv_chambolle"
    want_u8 = out in ("u8", "both")
    want_f32 = out in ("f32", "both")
    if want_u8:
        xb, y8, pitch, sq = _nlm_layout(name, x, out_u8)
    else:
        xb, sq = _as_batch(x, name)
        y8, pitch = None, _row_pitch(xb)
        if pitch is None:
            xb = xb.contiguous()
            pitch = xb.shape[2] * xb.shape[3]
    n, h, w, c = xb.shape
    y32 = torch.empty((n, h, w, c), dtype=torch.float32, device=xb.device) if want_f32 else None
    its = torch.empty((n, c), dtype=torch.int32, device=xb.device) if return_iters else None
    if n > 0:
        lib = _lib.load()
        nbytes = lib.idn_tv_chambolle_workspace_size(n, h, w, c)
        ws = _workspace(nbytes, xb.device)
        rc = lib.idn_tv_chambolle_u8(xb.data_ptr(), y8.data_ptr() if y8 is not None else None,
                                     y32.data_ptr() if y32 is not None else None,
                                     its.data_ptr() if its is not None else None, n, h, w, c,
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
    return res[0] if len(res) == 1 else tuple(res)


# ---- noise level -------------------------------------------------------------------------------

def _sigma_check(x) -> None:
    """argument errors of estimate_sigma, raised before the device is looked at"""
    name = "estimate_sigma"
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype not in (torch.uint8, torch.float64):
        raise TypeError(f"{name}: expected uint8 or float64 images, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    if x.shape[-1] not in (1, 3):
        raise ValueError(f"{name}: 1 or 3 channels supported, got {x.shape[-1]}")
    if x.device.type != "cuda":
        raise ValueError(f"{name}: idn runs on the GPU only; got a {x.device} tensor "
                         "(move it with .cuda(); there is no CPU fallback)")


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
        rc = lib.idn_estimate_sigma(None if is_f64 else xb.data_ptr(),
                                    xb.data_ptr() if is_f64 else None, out.data_ptr(), n, h, w, c,
                                    w * c, ws.data_ptr(), nbytes, _stream())
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
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.uint8:
        raise TypeError(f"{name}: expected uint8 images, got {x.dtype}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    c = x.shape[-1]
    if c not in (1, 3):
        raise ValueError(f"{name}: 1 or 3 channels supported, got {c}")
    h, w = x.shape[-3], x.shape[-2]
    if h < 1 or w < 1:
        raise ValueError(f"{name}: empty image {h} x {w}")
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
        if (not isinstance(out_u8, torch.Tensor) or out_u8.dtype != torch.uint8
                or out_u8.shape != x.shape or out_u8.device != x.device):
            raise ValueError(f"{name}: out_u8 must be a uint8 tensor shaped like x on x's device")
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
    if x.device.type != "cuda":
        raise ValueError(f"{name}: idn runs on the GPU only; got a {x.device} tensor "
                         "(move it with .cuda(); there is no CPU fallback)")
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
    name = "wiener"
    if out == "u8":
        xb, y8, pitch, sq = _nlm_layout(name, x, out_u8)
    else:
        xb, sq = _as_batch(x, name)
        y8, pitch = None, _row_pitch(xb)
        if pitch is None:
            xb = xb.contiguous()
            pitch = xb.shape[2] * xb.shape[3]
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
        rc = lib.idn_wiener_u8(xb.data_ptr(), y8.data_ptr() if y8 is not None else None,
                               y64.data_ptr() if y64 is not None else None, n, h, w, c, pitch,
                               kh, kw, WIENER_BORDERS[border],
                               nz.data_ptr() if nz is not None else None, nz_stride,
                               used.data_ptr() if used is not None else None,
                               ws.data_ptr() if ws is not None else None, nbytes, _stream())
        _lib.check(rc, "idn_wiener_u8")
    if out == "u8":
        res = out_u8 if out_u8 is not None else _finish(y8, sq)
    else:
        res = _finish(y64, sq)
    return (res, _finish(used, sq)) if return_noise else res


# ---- quality metrics ---------------------------------------------------------------------------

def _check_pair(x, y, name: str) -> None:
    """dtype and shape errors of a metric's image pair, raised before the device is looked at"""
    for t, nm in ((x, "x"), (y, "y")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor for {nm}, got {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{name}: expected uint8 images, got {t.dtype} for {nm}")
    if x.shape != y.shape:
        raise ValueError(f"{name}: shape mismatch {tuple(x.shape)} vs {tuple(y.shape)}")
    if x.dim() not in (3, 4):
        raise ValueError(f"{name}: expected (H,W,C) or (N,H,W,C), got shape {tuple(x.shape)}")
    if x.shape[-1] not in (1, 3):
        raise ValueError(f"{name}: 1 or 3 channels supported, got {x.shape[-1]}")
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
    rc = lib.idn_ssim_u8(xb.data_ptr(), yb.data_ptr(), out.data_ptr(),
                         out_ch.data_ptr() if out_ch is not None else None,
                         out_mse.data_ptr() if out_mse is not None else None,
                         n, h, w, c, w * c, w * c, win, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "idn_ssim_u8")
    res = _finish(out_ch if per_channel else out, sq)
    return (res, _finish(out_mse, sq)) if return_mse else res


# ---- float64 filters, shader, bloom ------------------------------------------------------------

def _f64_batch(x: torch.Tensor, name: str):
    xb, sq = _as_batch(x, name)
    if xb.dtype != torch.float64:
        raise TypeError(f"{name}: expected float64, got {xb.dtype}")
    return xb.contiguous(), sq


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
    from . import automold
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


def blob_from_f64(x: torch.Tensor, pixel_means=PIXEL_MEANS, out_hw: Optional[Tuple[int, int]] = None,
                  flip: bool = False) -> torch.Tensor:
    """prep_im_for_blob on a float64 image (the reference's float64 plain-noise branches)."""
    xb, _ = _f64_batch(x, "blob_from_f64")
    n, h, w, c = xb.shape
    oh, ow = out_hw if out_hw is not None else (h, w)
    y = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=xb.device)
    m = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(pixel_means, np.float64).reshape(-1)])
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


# ---- decode front-end (cv2.imread: lib/model/test.py:191, minibatch.py:85) ------------------
def _file_ptrs(files):
    bufs = [bytes(f) for f in files]
    ptrs = (ctypes.c_void_p * len(bufs))(
        *[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in bufs])
    lens = (ctypes.c_size_t * len(bufs))(*[len(b) for b in bufs])
    return bufs, ptrs, lens


def jpeg_orientation(data: bytes) -> int:
    """The EXIF orientation (1..8, 1 = none) cv2.imread (OpenCV 3.4.2) applies to this JPEG after
    decoding (include/idn.h idn_jpeg_orientation)."""
    lib = _lib.load()
    o = ctypes.c_int()
    buf = bytes(data)
    _lib.check(lib.idn_jpeg_orientation(ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p),
                                        len(buf), ctypes.byref(o)), "idn_jpeg_orientation")
    return o.value


def jpeg_info(data: bytes, orientation: bool = True) -> Tuple[int, int, int]:
    """(height, width, components) of a JPEG held in memory, as cv2.imread returns it (the size
    after its EXIF orientation; orientation=False: the decoded size); IdnError if the decoder
    does not take it (lossless, hierarchical, 12-bit, ...)."""
    lib = _lib.load()
    h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    buf = bytes(data)
    _lib.check(lib.idn_jpeg_info(ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p), len(buf),
                                 ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)),
               "idn_jpeg_info")
    if not orientation and jpeg_orientation(buf) >= 5:  # back to the decoded (untransposed) size
        return w.value, h.value, c.value
    return h.value, w.value, c.value


JPEG_MODES = {"libjpeg9": 0, "turbo": 1}  # include/idn.h IDN_JPEG_TURBO
JPEG_IGNORE_ORIENTATION = 2  # include/idn.h IDN_JPEG_IGNORE_ORIENTATION


def jpeg_decode(files, out: Optional[torch.Tensor] = None, device=None, mode: str = "libjpeg9",
                chunk_bits: int = 0, orientation: bool = True) -> torch.Tensor:
    """cv2.imread(path) for a batch of same-size JPEG files (bytes in host memory):
    (n, h, w, 3) uint8 BGR on the GPU.  mode "libjpeg9" (default) is bit-exact with the
    reference's pinned IJG libjpeg 9d (requirements.txt:74, under OpenCV 3.4.2: scaled 16x16 /
    16x8 chroma IDCT); "turbo" with libjpeg-turbo (fancy upsampling).  Each image is turned by its
    EXIF orientation as OpenCV 3.4.2's imread does (orientation=False: cv2's
    IMREAD_IGNORE_ORIENTATION); (h, w) is the size after the turn and must agree across the
    batch.  chunk_bits (0 = default) sets the entropy decoder's chunk size; it does not change
    the output."""
    files = list(files)
    if not files:
        raise ValueError("jpeg_decode: no files")
    if mode not in JPEG_MODES:
        raise ValueError(f"jpeg_decode: mode must be one of {sorted(JPEG_MODES)}")
    flags = JPEG_MODES[mode] | (int(chunk_bits) << 8) | (0 if orientation else JPEG_IGNORE_ORIENTATION)
    h, w, _ = jpeg_info(files[0], orientation)
    n = len(files)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous()
          or out.device.type != "cuda"):
        raise ValueError("jpeg_decode: out must be a contiguous (n, h, w, 3) uint8 CUDA tensor")
    lib = _lib.load()
    bufs, ptrs, lens = _file_ptrs(files)
    ws_bytes = lib.idn_jpeg_workspace_size(ptrs, lens, n, flags)
    if ws_bytes == 0:
        raise _lib.IdnError("jpeg_decode: unsupported or corrupt JPEG in the batch (or bad flags)")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
    with torch.cuda.device(out.device):
        rc = lib.idn_jpeg_decode_u8(ptrs, lens, n, out.data_ptr(), h, w, w * 3, flags,
                                    ws.data_ptr(), ws_bytes, _stream())
    _lib.check(rc, "idn_jpeg_decode_u8")
    del bufs
    return out
