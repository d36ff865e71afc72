"""The named cases of the general wavelet denoiser, shared by the fixture generator
(tests/golden/make_wavelet_general_fixtures.py), tests/test_wavelet_general.py and
tests/test_wavelet_general_gpu.py.  numpy only.

Input recipe (make_input): clip(128 + 64 sin(2 pi x / 97) cos(2 pi y / 61)
+ amp ((x // 16 + y // 16) % 2) + N(0, 6), 0, 255) cast to uint8, the noise from RandomState(3),
per channel.  float64 inputs are (4 u8 + k) / 1023 with k uniform in 0..3 from the same stream:
off the uint8 grid, and exact integer ratios under any numpy.  The fixture file records each
input's CRC-32.
"""
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name shape c dtype wavelet levels method mode sigma ycc kind")


def _c(name, shape, c, dtype, wavelet, levels, method, mode, sigma, ycc, kind="recipe"):
    return Case(name, shape, c, dtype, wavelet, levels, method, mode, sigma, ycc, kind)


B, V, S, H = "BayesShrink", "VisuShrink", "soft", "hard"
CASES = [
    # db2
    _c("db2_64x96_L2_ycc_soft", (64, 96), 3, "u8", "db2", 2, B, S, None, True),
    _c("db2_64x96_L2_ycc_hard", (64, 96), 3, "u8", "db2", 2, B, H, None, True),
    _c("db2_64x96_L3_plain_visu", (64, 96), 3, "f64", "db2", 3, V, S, 0.02, False),
    _c("db2_64x96_L3_plain_bayes", (64, 96), 3, "f64", "db2", 3, B, S, 0.02, False),
    _c("db2_600x1000", (600, 1000), 3, "u8", "db2", None, B, S, None, False),
    _c("db2_130x77_c1", (130, 77), 1, "u8", "db2", None, V, H, (0.015,), False),
    _c("db2_9x11_c1", (9, 11), 1, "f64", "db2", None, B, S, None, False),
    # sym4
    _c("sym4_64x96_L2_ycc_soft", (64, 96), 3, "u8", "sym4", 2, V, S, (0.02, 0.012, 0.015), True),
    _c("sym4_64x96_L2_ycc_hard", (64, 96), 3, "u8", "sym4", 2, V, H, (0.02, 0.012, 0.015), True),
    _c("sym4_64x96_L3_c1", (64, 96), 1, "f64", "sym4", 3, B, H, None, False),
    _c("sym4_64x17", (64, 17), 3, "u8", "sym4", None, B, S, 0.03, False),
    _c("sym4_37x53_ycc", (37, 53), 3, "f64", "sym4", None, B, S, None, True),
    # coif5
    _c("coif5_130x200_L2_bayes", (130, 200), 3, "u8", "coif5", 2, B, S, 0.03, False),
    _c("coif5_130x200_L2_visu", (130, 200), 3, "u8", "coif5", 2, V, S, 0.03, False),
    _c("coif5_9x11_ycc", (9, 11), 3, "u8", "coif5", None, B, H, None, True),
    _c("coif5_37x53_c1", (37, 53), 1, "f64", "coif5", None, V, S, (0.02,), False),
    _c("coif5_64x96_ycc", (64, 96), 3, "f64", "coif5", None, V, H, 0.015, True),
    _c("coif5_130x77_none", (130, 77), 3, "u8", "coif5", None, B, S, None, False),
    # bior1.5 on the general path
    _c("bior15_64x96_visu_soft", (64, 96), 3, "u8", "bior1.5", None, V, S, 0.015, True),
    _c("bior15_64x96_visu_hard", (64, 96), 3, "u8", "bior1.5", None, V, H, 0.015, True),
    _c("bior15_130x77_c1", (130, 77), 1, "f64", "bior1.5", None, B, S, None, False),
    _c("bior15_64x17", (64, 17), 3, "u8", "bior1.5", None, B, H, (0.03, 0.02, 0.025), False),
    # db1 on the general path
    _c("db1_64x96_c1", (64, 96), 1, "u8", "db1", None, B, H, None, False),
    _c("db1_37x53_ycc", (37, 53), 3, "f64", "db1", None, V, S, (0.02, 0.012, 0.015), True),
    _c("db1_130x77", (130, 77), 3, "u8", "db1", None, V, H, 0.02, False),
    # more than half the pixels flat (half 0, a quarter 200), sigma from the data
    _c("db2_64x96_flat", (64, 96), 3, "u8", "db2", None, B, S, None, False, "flat"),
    # channel 1 constant
    _c("sym4_64x96_const", (64, 96), 3, "u8", "sym4", None, B, S, None, False, "const"),
]
BY_NAME = {c.name: c for c in CASES}
# cases that differ in one option only
PAIRS = [("db2_64x96_L2_ycc_soft", "db2_64x96_L2_ycc_hard", "mode"),
         ("sym4_64x96_L2_ycc_soft", "sym4_64x96_L2_ycc_hard", "mode"),
         ("bior15_64x96_visu_soft", "bior15_64x96_visu_hard", "mode"),
         ("db2_64x96_L3_plain_visu", "db2_64x96_L3_plain_bayes", "method"),
         ("coif5_130x200_L2_bayes", "coif5_130x200_L2_visu", "method")]
# one case per new wavelet whose pywt.wavedecn arrays the fixture file holds (channel 0)
WAVEDEC = ("db2_64x96_L3_plain_visu", "sym4_64x96_L3_c1", "coif5_37x53_c1")
FULL_MAX = (37, 53)  # full results are stored up to this shape; above it crops and sums
CROPS = ((0, 0), (1, 2), (2, 1))  # 16 x 16 crops at (fy * (h - 16) // 2, fx * (w - 16) // 2)


def make_u8(h, w, c, amp=40, seed=3):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 64 * np.sin(2 * np.pi * x / 97) * np.cos(2 * np.pi * y / 61) \
        + amp * ((x // 16 + y // 16) % 2)
    img = base[..., None] + rs.normal(0.0, 6.0, size=(h, w, c))
    return np.clip(img, 0, 255).astype(np.uint8), rs


def make_input(case):
    """the case's input image (H, W, C), uint8 or float64"""
    h, w = case.shape
    u8, rs = make_u8(h, w, case.c)
    if case.kind == "flat":
        u8[: h // 2] = 0
        u8[h // 2:, : w // 2] = 200
    elif case.kind == "const":
        u8[..., 1] = 200
    if case.dtype == "u8":
        return u8
    k = rs.randint(0, 4, size=u8.shape)
    return (4.0 * u8 + k) / 1023.0


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes()) & 0xFFFFFFFF


def crop_origins(h, w):
    return [(fy * (h - 16) // 2, fx * (w - 16) // 2) for fy, fx in CROPS]


def kwargs(case):
    """the options as idn.denoise_wavelet / the model take them"""
    return dict(wavelet=case.wavelet, levels=case.levels, sigma=case.sigma, mode=case.mode,
                method=case.method, convert2ycbcr=case.ycc)
