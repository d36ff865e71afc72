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
  denoise_dct(x, sigma, color=...)        sliding 8x8 DCT hard threshold (Yu & Sapiro, IPOL 2011)
  equalize_hist(x)                        cv2.equalizeHist(x)
  clahe(x, clip_limit, tile_grid)         cv2.createCLAHE(clip_limit, tile_grid).apply(x)
  cvt_color_yuv(x, to_yuv)                cv2.cvtColor(x, COLOR_BGR2YUV / COLOR_YUV2BGR)
  correct_exposure(x, denoise)            Automold.correct_exposure (tools/Automold.py:817-842)

There is no CPU path: a CPU tensor raises, a missing library raises.

One module per family; _args holds what they share (batches, pointers, the common checks and
their messages, the image layout, the scratch cache).  Everything is re-exported here, the
caches as the very objects the ops use.
"""
from ._args import (  # noqa: F401
    _WS_CACHE, _as_batch, _f64_batch, _finish, _ids_tensor, _image_layout, _ptr, _row_pitch,
    _slots_tensor, _stream, _u8_batch, _workspace,
)
from .filters import (  # noqa: F401
    ADAPTIVE_MEDIAN_MAX_KSIZE, BLUR_MAX_KSIZE, BLUR_TILE, MEDIAN_MAX_KSIZE, _filter,
    adaptive_median, bilateral_filter, blur, blur_f64, gaussian_blur, gaussian_blur_f64,
    gaussian_taps, median_blur,
)
from .noise import (  # noqa: F401
    ADD_NOISE_KINDS, FILTERS, GAMMA_SHAPE, NOISE_KINDS, _PATTERN_CACHE, _PIPE_STREAMS,
    _empty_like_img, _noise_filter_pipelined, _noise_kind, _noise_outputs, _noise_result,
    _random_noise_slots, _replay_field, _stream_ids, add_pattern, copy_slots, noise_add,
    noise_filter, periodic_noise, periodic_pattern, random_noise, random_noise_ycc, ycc_fusable,
)
from .misc import (  # noqa: F401
    PIXEL_MEANS, blob, blob_from_f64, bloom, copy_flat, gaussian_blob, resize_linear, shader,
)
from .color import cvt_color_lab, quantize  # noqa: F401
from .wavelet import (  # noqa: F401
    WAVELET_METHODS, WAVELET_MODES, WAVELETS, _wavelet_sigma, denoise_wavelet,
)
from .nlmeans import (  # noqa: F401
    NLMEANS_MAX_WEIGHTS, _NLM_CACHE, _nlm_check, _nlm_table, nl_means, nl_means_colored,
    nl_means_colored_weights, nl_means_weights,
)
from .exposure import (  # noqa: F401
    CLAHE_MAX_TILES, EXPOSURE_NLM, EXPOSURE_TILE_GRID, _exposure_call, _exposure_check, clahe,
    correct_exposure, cvt_color_yuv, equalize_hist,
)
from .restoration import (  # noqa: F401
    DCT_PATCH, DCT_TILE, TV_MAX_ITER, WIENER_BORDERS, WIENER_MAX_KSIZE, WIENER_TILE, _dct_check,
    _sigma_check, _tv_check, _wiener_check, denoise_dct, denoise_tv_chambolle, estimate_sigma,
    wiener,
)
from .metrics import _check_pair, mse, psnr, ssim  # noqa: F401
from .jpeg import (  # noqa: F401
    JPEG_IGNORE_ORIENTATION, JPEG_MODES, _file_ptrs, jpeg_decode, jpeg_info, jpeg_orientation,
)
