#!/opt/conda/bin/python3.9
"""Generate tests/golden/wavelet_general.npz from the real libraries.

Interpreter: python3.9 with scikit-image 0.18.3 and PyWavelets 1.1.1.  The denoise_wavelet wrapper
has skimage 0.14.2's semantics (what the reference pins) around 0.18.3's `_wavelet_threshold`, as
tests/golden/make_fixtures.py does; 0.18.3's own denoise_wavelet is not called (it clips
differently and rescales sigma).

  python3.9 tests/golden/make_wavelet_general_fixtures.py

The file holds, for the cases of tests/wavelet_general_cases.py:
  taps_<wavelet>      (4, F): dec_lo, dec_hi, rec_lo, rec_hi
  crc_<case>          CRC-32 of the input bytes
  sigma_<case>        (C,) the sigma each channel was thresholded with (estimated where not given)
  full_<case>         the float64 result, shapes up to 37 x 53; above that
  crops_<case>        (3, 16, 16, C) crops (wavelet_general_cases.crop_origins) and
  sums_<case>         (C,) per-channel sums of the result
  wavedec_<case>_<k>  pywt.wavedecn of channel 0 as the transform sees it: k = 0 the
                      approximation, then ad, da, dd of every level, coarsest first
"""
import sys
from pathlib import Path

import numpy as np
import pywt
from skimage import color
from skimage.restoration._denoise import _sigma_est_dwt, _wavelet_threshold
from skimage.util import img_as_float

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import wavelet_general_cases as wc  # noqa: E402

OUT = HERE / "wavelet_general.npz"
WAVELETS = ("db1", "bior1.5", "db2", "sym4", "coif5")


def denoise_wavelet_0142(image, sigma, wavelet, mode, wavelet_levels, convert2ycbcr, method,
                         planes):
    """skimage 0.14.2 denoise_wavelet(image, sigma, wavelet, mode, wavelet_levels,
    multichannel=True, convert2ycbcr, method); planes receives what _wavelet_threshold saw"""
    image = img_as_float(image)
    C = image.shape[-1]
    if sigma is None or np.isscalar(sigma):
        sigma = [sigma] * C
    kw = dict(wavelet=wavelet, method=method, mode=mode, wavelet_levels=wavelet_levels)
    if convert2ycbcr:
        out = color.rgb2ycbcr(image)
        for i in range(3):
            mn, mx = out[..., i].min(), out[..., i].max()
            channel = out[..., i] - mn
            channel /= mx - mn
            planes.append(channel.copy())
            ch = np.clip(_wavelet_threshold(channel, sigma=sigma[i], **kw), 0, 1)
            out[..., i] = ch * (mx - mn)
            out[..., i] += mn
        out = color.ycbcr2rgb(out)
    else:
        out = np.empty_like(image)
        for c in range(C):
            planes.append(image[..., c].copy())
            out[..., c] = _wavelet_threshold(image[..., c], sigma=sigma[c], **kw)
    return np.clip(out, 0, 1)


def main():
    z = {}
    for n in WAVELETS:
        w = pywt.Wavelet(n)
        z["taps_" + n] = np.array([w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi], np.float64)
    for case in wc.CASES:
        x = wc.make_input(case)
        h, w = case.shape
        planes = []
        with np.errstate(all="ignore"):
            r = denoise_wavelet_0142(x, case.sigma, case.wavelet, case.mode, case.levels, case.ycc,
                                     case.method, planes)
        z["crc_" + case.name] = np.array(wc.crc(x), np.uint32)
        if case.sigma is None:
            sig = [_sigma_est_dwt(pywt.dwtn(p, case.wavelet)["dd"], distribution="Gaussian")
                   for p in planes]
        else:
            sig = list(np.ravel(case.sigma)) * (1 if np.ndim(case.sigma) else case.c)
        z["sigma_" + case.name] = np.array(sig, np.float64)
        if h <= wc.FULL_MAX[0] and w <= wc.FULL_MAX[1]:
            z["full_" + case.name] = r
        else:
            z["crops_" + case.name] = np.stack([r[y:y + 16, x0:x0 + 16]
                                                for y, x0 in wc.crop_origins(h, w)])
            z["sums_" + case.name] = r.sum(axis=(0, 1))
        if case.name in wc.WAVEDEC:
            lv = case.levels
            if lv is None:
                F = pywt.Wavelet(case.wavelet).dec_len
                lv = max(min(pywt.dwt_max_level(s, F) for s in case.shape) - 3, 1)
            co = pywt.wavedecn(planes[0], case.wavelet, level=lv)
            arrs = [co[0]] + [lev[k] for lev in co[1:] for k in ("ad", "da", "dd")]
            for k, a in enumerate(arrs):
                z["wavedec_%s_%d" % (case.name, k)] = a
    np.savez_compressed(OUT, **z)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
