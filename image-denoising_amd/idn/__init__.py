"""idn — MI355X-native image noise-injection + denoising filter bank.

Drop-in for the preprocessing hot path of mahesh-kashyap-ml/image-denoising (the noise closures
and denoise hooks of lib/roi_data_layer/minibatch.py and lib/model/test.py, and
lib/utils/blob.py), computed by hand-written HIP kernels for gfx950 behind a C-ABI
(include/idn.h).  See DESIGN.md.
"""
from ._lib import IdnError, LIB_PATH  # noqa: F401
from . import ops  # noqa: F401
from .ops import (  # noqa: F401
    gaussian_blur, blur, median_blur, adaptive_median, bilateral_filter, random_noise,
    periodic_pattern,
    add_pattern, periodic_noise, blob, mse, psnr, ssim, nl_means,
    nl_means_colored, denoise_tv_chambolle, estimate_sigma, denoise_wavelet,
    equalize_hist, clahe, cvt_color_yuv, correct_exposure, wiener, denoise_dct,
)
from . import automold  # noqa: F401

__version__ = "0.1.0"
