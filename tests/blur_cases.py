"""The cases tests/test_blur_model.py (CPU) and tests/test_blur_large_gpu.py (GPU) share: the
windows, the literal Q8 taps, and the quality thresholds with the figures they are checked on."""
import numpy as np

import blur_model as bm
import philox_model as pm
import wiener_model as wm

KS = list(range(3, 32, 2))
SHAPES = [(13, 17, 3), (2, 3, 3), (1, 40, 3), (3, 4, 1)]
SID = lambda s: "x".join(map(str, s))  # noqa: E731

# the taps of the issue, from its numpy prototype
SYM31_0 = [0, 0, 1, 1, 2, 3, 4, 6, 8, 10, 12, 15, 17, 19, 20, 20]
SYM31_12 = [5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 10, 10, 11, 14]
TAPS = {
    (9, 1.0): [0, 1, 14, 62, 102, 62, 14, 1, 0],
    (15, 2.5): [1, 2, 6, 11, 20, 30, 38, 40, 38, 30, 20, 11, 6, 2, 1],
    (31, 0.0): SYM31_0 + SYM31_0[-2::-1],
    (31, 12.0): SYM31_12 + SYM31_12[-2::-1],
    (3, 0.3): [1, 254, 1],
    (3, 0.1): [0, 256, 0],
    (5, 0.8): [6, 58, 128, 58, 6],
    (3, 0.0): [64, 128, 64],
    (5, 0.0): [16, 64, 96, 64, 16],
    (7, 0.0): [8, 28, 56, 72, 56, 28, 8],
}

# the quality thresholds (dB) that tests/test_blur_large_gpu.py asserts on the device
QUALITY_SEED = 0
QUALITY_VAR = (40.0 / 255.0) ** 2
GAUSS9_OVER_5, GAUSS9_OVER_3, BOX7_OVER_3 = 1.0, 3.0, 1.5


def device_noisy(clean3, seed=QUALITY_SEED):
    """idn.random_noise(clean3, "gaussian", var=QUALITY_VAR, seed=seed, out="u8") from the host
    model of the Philox stream (tests/philox_model.py; the kernel forms the same value in fp32)"""
    v = clean3.reshape(1, -1)
    return pm.gauss_u8(v, seed, pm.image_ids(1), pm.GAUSSIAN, 0.0, QUALITY_VAR)["byte"].reshape(
        clean3.shape)


def quality_figures(clean3, noisy):
    g = {k: wm.psnr(clean3, bm.gaussian_blur(noisy, k)) for k in (3, 5, 9)}
    b = {k: wm.psnr(clean3, bm.blur(noisy, k)) for k in (3, 7)}
    return g, b
