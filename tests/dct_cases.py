"""The parity cases of idn.denoise_dct, shared by tests/test_dct_model.py and
tests/test_dct_denoise_gpu.py: noisy smooth images, at which the share of samples that hang on a
threshold decision stays small.  Uniform-random images and sd 5 stay out: their share reached
32 % and 8 %.  Every reference is computed once and handed out read-only."""
import functools

import numpy as np

import dct_model as dm
import wiener_model as wm

PARITY_SHAPES = [(8, 8, 1), (8, 8, 3), (8, 37, 3), (37, 8, 1), (9, 9, 3), (33, 70, 3), (64, 97, 1)]
PARITY_SDS = [15.0, 40.0]
MARGIN = 2e-3      # a coefficient this close to its threshold may fall either way in fp32
MAX_SHARE = 0.05   # of samples covered by a patch with such a coefficient


@functools.lru_cache(maxsize=None)
def parity_image(shape, sd, seed=1):
    """wm.noisy_image(wm.smooth_image(h, w), sd, seed)[..., :c], or a batch of them for a 4-D
    shape (seeds seed, seed + 1, ...)"""
    if len(shape) == 4:
        x = np.stack([parity_image(tuple(shape[1:]), sd, seed + i) for i in range(shape[0])])
    else:
        h, w, c = shape
        x = np.ascontiguousarray(wm.noisy_image(wm.smooth_image(h, w), sd, seed)[..., :c])
    x.setflags(write=False)
    return x


def references(x, sigma, color, factor=3.0):
    """(float64 model, fp32 model, risk mask) of x, read-only"""
    r64 = dm.denoise_dct(x, sigma, factor=factor, color=color, out="f")
    r32 = dm.denoise_dct(x, sigma, factor=factor, color=color, out="f", dtype=np.float32)
    mask = dm.risk_mask(x, sigma, factor=factor, color=color, margin=MARGIN)
    for a in (r64, r32, mask):
        a.setflags(write=False)
    return r64, r32, mask


@functools.lru_cache(maxsize=None)
def parity_case(shape, sd, color):
    """(x, float64 model, fp32 model, risk mask) of one parity case"""
    x = parity_image(shape, sd)
    return (x,) + references(x, sd, color)
