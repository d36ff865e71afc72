"""The definition of idn.denoise_wavelet with every option: numpy float64, no pywt, no skimage.

Per image this is skimage 0.14.2's

    denoise_wavelet(x, sigma, wavelet, mode, wavelet_levels=levels, multichannel=True,
                    convert2ycbcr=convert2ycbcr, method=method)

(for C = 1 with convert2ycbcr=False: multichannel=False on the 2-D image), restated so that the
analysis is bit-equal to PyWavelets 1.1.1 (tests/golden/wavelet_general.npz holds the real
libraries' values; tests/test_wavelet_general.py compares).  The filters come from that file.

  input      uint8 -> x * (1 / 255) (img_as_float), float64 as it is (precondition: in [0, 1])
  colour     convert2ycbcr=True: rgb2ycbcr, each channel (v - min) / (max - min), the transform,
             clip [0, 1], * (max - min) + min, ycbcr2rgb, clip [0, 1] (oracle/wavelet.py's
             wrapper); a given sigma[i] applies to the normalised channel i
             convert2ycbcr=False: the transform on each channel of the float image, one clip [0, 1]
  transform  skimage _wavelet_threshold: pywt.wavedecn(level L, 'symmetric'), thresholds, waverecn,
             crop.  L defaults to max(min(dwt_max_level(h, F), dwt_max_level(w, F)) - 3, 1)
  analysis   pywt's downsampling_convolution, axis 0 then axis 1.  Output o of a length-n axis is
             centred at i = 2 o + 1 and is sum_j f[j] X(i - j) over the half-sample symmetric
             extension X (any overshoot: period 2 n).  The sum starts from 0.0, every step is one
             multiply then one add.  For i < n the taps go j = 0 .. F-1; for i >= n the
             overhanging taps go first in descending order j = i - n .. 0, the rest follow
             j = i - n + 1 .. F-1 (tests/sigma_model.py states the same for db2)
  sigma      None: median(|dd_1| != 0) / 0.6744897501960817 of the finest diagonal band
  thresholds BayesShrink: per band t = var / sqrt(max(mean(d^2) - var, eps))
             VisuShrink: t = sigma sqrt(2 log(h w)) for every band
  shrinkage  soft: pywt.threshold(d, t, 'soft') = d max(1 - t / |d|, 0) (0 where d = 0)
             hard: d where |d| >= t, else 0
  synthesis  pywt's upsampling_convolution_valid_sf per axis (axis 1, then axis 0), the
             approximation cropped to the detail shape before each level
"""
from pathlib import Path

import numpy as np

from oracle import wavelet as ow
from sigma_model import sigma_of_keys

FIXTURE = Path(__file__).resolve().parent / "golden" / "wavelet_general.npz"
WAVELETS = ("db1", "bior1.5", "db2", "sym4", "coif5")
ALIASES = {"haar": "db1"}
EPS = np.finfo(np.float64).eps
_TAPS = {}


def taps(wavelet):
    """(dec_lo, dec_hi, rec_lo, rec_hi) of the fixture file, float64 arrays"""
    wavelet = ALIASES.get(wavelet, wavelet)
    if not _TAPS:
        with np.load(FIXTURE) as z:
            for n in WAVELETS:
                _TAPS[n] = tuple(np.array(r, np.float64) for r in z["taps_" + n])
    return _TAPS[wavelet]


def tap_order(i, n, F):
    if i < n:
        return list(range(F))
    k = i - n
    return list(range(k, -1, -1)) + list(range(k + 1, F))


def dwt_axis0(x, lo, hi):
    """pywt.dwt along axis 0 ('symmetric'), pywt's operation order"""
    n, F = x.shape[0], len(lo)
    nout = (n + F - 1) // 2
    a = np.empty((nout,) + x.shape[1:], np.float64)
    d = np.empty_like(a)
    for o in range(nout):
        i = 2 * o + 1
        sa = np.zeros(x.shape[1:], np.float64)
        sd = np.zeros(x.shape[1:], np.float64)
        for j in tap_order(i, n, F):
            row = x[int(ow._sym_index(i - j, n))]
            sa = sa + lo[j] * row
            sd = sd + hi[j] * row
        a[o], d[o] = sa, sd
    return a, d


def dwt2(x, wavelet):
    """pywt.dwtn of a 2-D array: {'aa', 'ad', 'da', 'dd'}"""
    lo, hi = taps(wavelet)[:2]
    a0, d0 = dwt_axis0(np.ascontiguousarray(x, np.float64), lo, hi)
    out = {}
    for k0, v in (("a", a0), ("d", d0)):
        a1, d1 = dwt_axis0(np.ascontiguousarray(v.T), lo, hi)
        out[k0 + "a"] = np.ascontiguousarray(a1.T)
        out[k0 + "d"] = np.ascontiguousarray(d1.T)
    return out


def idwt_axis0(a, d, rlo, rhi):
    n, h = a.shape[0], len(rlo) // 2
    m = n - h + 1
    out = np.empty((2 * m,) + a.shape[1:], np.float64)
    for o in range(m):
        z = np.zeros(a.shape[1:], np.float64)
        le, lo_, he, ho = z, z, z, z  # the lowpass sums, then the highpass sums added to them
        for j in range(h):
            le = le + rlo[2 * j] * a[o + h - 1 - j]
            lo_ = lo_ + rlo[2 * j + 1] * a[o + h - 1 - j]
            he = he + rhi[2 * j] * d[o + h - 1 - j]
            ho = ho + rhi[2 * j + 1] * d[o + h - 1 - j]
        out[2 * o], out[2 * o + 1] = le + he, lo_ + ho
    return out


def idwt2(c, wavelet):
    rlo, rhi = taps(wavelet)[2:]
    a = idwt_axis0(np.ascontiguousarray(c["aa"].T), np.ascontiguousarray(c["ad"].T), rlo, rhi).T
    d = idwt_axis0(np.ascontiguousarray(c["da"].T), np.ascontiguousarray(c["dd"].T), rlo, rhi).T
    return idwt_axis0(np.ascontiguousarray(a), np.ascontiguousarray(d), rlo, rhi)


def default_levels(h, w, wavelet):
    F = len(taps(wavelet)[0])
    return max(min(ow.dwt_max_level(h, F), ow.dwt_max_level(w, F)) - 3, 1)


def wavedec2(x, wavelet, levels):
    """pywt.wavedecn: [aa_L, {ad, da, dd}_L, ..., {ad, da, dd}_1]"""
    out, a = [], x
    for _ in range(levels):
        c = dwt2(a, wavelet)
        a = c.pop("aa")
        out.append(c)
    return [a] + out[::-1]


def shrink(d, t, mode):
    if mode == "hard":
        return np.where(np.abs(d) >= t, d, 0.0)
    mag = np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.clip(1 - t / mag, 0, None)
    return d * np.where(mag == 0, 0.0, s)


def wavelet_threshold(plane, wavelet, levels=None, sigma=None, mode="soft", method="BayesShrink",
                      info=None):
    """skimage _wavelet_threshold of one 2-D float64 plane.  info (a dict) receives sigma, the
    coefficient list and the thresholds [{band: t} per level, coarsest first]."""
    h, w = plane.shape
    if levels is None:
        levels = default_levels(h, w, wavelet)
    co = wavedec2(plane, wavelet, levels)
    if sigma is None:
        dd = co[-1]["dd"].ravel()
        sigma = sigma_of_keys(np.abs(dd[dd != 0.0]))
    sigma = np.float64(sigma)
    var = sigma * sigma
    thr = []
    for lev in co[1:]:
        if method == "BayesShrink":
            with np.errstate(invalid="ignore"):
                thr.append({k: var / np.sqrt(max(np.mean(d * d) - var, EPS)) for k, d in lev.items()})
        else:
            thr.append({k: sigma * np.sqrt(2 * np.log(plane.size)) for k in lev})
    if info is not None:
        info.update(sigma=sigma, coeffs=co, thr=thr)
    a = co[0]
    for lev, t in zip(co[1:], thr):
        ref = lev["dd"].shape
        c = {k: shrink(d, t[k], mode) for k, d in lev.items()}
        c["aa"] = a[:ref[0], :ref[1]]
        a = idwt2(c, wavelet)
    return a[:h, :w]


def as_float(x):
    x = np.asarray(x)
    return x.astype(np.float64) * (1.0 / 255.0) if x.dtype == np.uint8 else x.astype(np.float64)


def _matmul3(x, M, matmul, pre=None, post=None):
    """(x - pre) @ M.T + post over the last axis.  numpy's matmul rounds this as its build does:
    'fma' is the fused chain of oracle/cv.py (what oracle/wavelet.py and the kernels use), 'plain'
    is (x0 m0 + x1 m1) + x2 m2 in separate operations (what the interpreter that wrote the fixture
    file does)"""
    if matmul == "fma":
        from oracle.cv import matmul3_fma
        zero = (0.0, 0.0, 0.0)
        return matmul3_fma(x, M, pre=zero if pre is None else pre, post=zero if post is None else post)
    if pre is not None:
        x = x - pre
    out = np.stack([(x[..., 0] * M[c, 0] + x[..., 1] * M[c, 1]) + x[..., 2] * M[c, 2]
                    for c in range(3)], axis=-1)
    return out if post is None else out + post


def denoise(x, wavelet="bior1.5", levels=None, sigma=None, mode="soft", method="BayesShrink",
            convert2ycbcr=True, info=None, matmul="fma"):
    """float64 (H, W, C) result in [0, 1] of one image x (H, W, C), uint8 or float64.  info (a
    list) receives one dict per channel (wavelet_threshold).  matmul: _matmul3."""
    img = as_float(x)
    C = img.shape[-1]
    sig = list(np.ravel(sigma)) if sigma is not None and np.ndim(sigma) else [sigma] * C
    kw = dict(levels=levels, mode=mode, method=method)
    infos = [{} for _ in range(C)]
    if convert2ycbcr:
        out = _matmul3(img, ow.YCBCR_FROM_RGB, matmul, post=ow.YCBCR_OFFSET)
        for i in range(3):
            mn, mx = out[..., i].min(), out[..., i].max()
            ch = (out[..., i] - mn) / (mx - mn)
            ch = np.clip(wavelet_threshold(ch, wavelet, sigma=sig[i], info=infos[i], **kw), 0, 1)
            out[..., i] = ch * (mx - mn) + mn
        out = _matmul3(out, ow.RGB_FROM_YCBCR, matmul, pre=ow.YCBCR_OFFSET)
    else:
        out = np.empty_like(img)
        for c in range(C):
            out[..., c] = wavelet_threshold(img[..., c], wavelet, sigma=sig[c], info=infos[c], **kw)
    if info is not None:
        info.extend(infos)
    return np.clip(out, 0, 1)


def to_u8(r):
    return (255 * r).astype(np.uint8)
