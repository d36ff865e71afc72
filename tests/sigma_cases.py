"""The inputs of the estimate_sigma tests (numpy only; RandomState streams are frozen by numpy).

tests/golden/make_sigma_fixtures.py runs the real skimage / pywt on exactly these arrays and
stores a CRC of each beside the values, so a test can tell that it rebuilt the array the real
library saw.  Every case is (N,)H,W,C; `cases()` yields (name, array).

Shapes: 4x4 (every sample is a boundary), 4x5 / 5x4, 7x9 (odd in both axes: the right-overhang
order matters in both), 16x16, 17x23, 33x35, 64x97 with one channel, 70x1100 (wider than a row
tile), 300x20 (taller than a tile), one batch of five 24x40 images with differing content.
Contents: uniform random bytes; a two-level image (heavy ties in the keys); half 255 / half 0
with a noisy band (a median among the ~1e-31 keys of the flat half, exact zeros in the other); a
single nonzero pixel in a zero image; an all-zero channel (NaN) beside normal channels; a
checkerboard of two amplitudes whose two middle keys differ already in their exponent, the lower
one tied with more than 1024 others.  The float64 form of a case is clip(u8 / 255 + normal, 0, 1).
"""
import zlib

import numpy as np

SHAPES = [(4, 4, 3), (4, 5, 3), (5, 4, 3), (7, 9, 3), (16, 16, 3), (17, 23, 3), (33, 35, 3),
          (64, 97, 1), (70, 1100, 3), (300, 20, 3)]
STORED_INPUT_BYTES = 2048   # inputs up to this size are stored in the fixture file themselves
DD_CASES = ("random-4x4x3-u8", "random-7x9x3-u8", "random-4x5x3-f64")  # real dd bands stored


def _seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def random_bytes(h, w, c):
    return np.random.RandomState(_seed("random", h, w, c)).randint(0, 256, (h, w, c)).astype(np.uint8)


def two_level(h, w, c):
    """40 or 200 per sample: a handful of distinct key values, each shared by many positions"""
    rs = np.random.RandomState(_seed("two", h, w, c))
    return np.where(rs.randint(0, 2, (h, w, c)) == 1, 200, 40).astype(np.uint8)


def half_saturated(h, w, c):
    """the left 3/4 is 255, the rest 0, and rows h//2 .. h//2 + 1 are random bytes"""
    rs = np.random.RandomState(_seed("half", h, w, c))
    x = np.zeros((h, w, c), np.uint8)
    x[:, :(3 * w) // 4] = 255
    x[h // 2:h // 2 + 2] = rs.randint(0, 256, (min(2, h - h // 2), w, c))
    return x


def single_pixel(h, w, c):
    x = np.zeros((h, w, c), np.uint8)
    x[h // 2, w // 3] = 77
    return x


def zero_channel(h, w, c):
    x = random_bytes(h, w, c).copy()
    x[..., c // 2] = 0
    return x


def two_boards(h=122, w=100, split=62):
    """a checkerboard of 40 / 0 above row `split` and of 200 / 0 below: inside either part |d| is
    one value (40.0 and 200.0), and with this split the count of nonzero keys is even, the lower
    middle key is 40.0 (one of 1470) and the upper one 150 (a key of the seam)"""
    i, j = np.indices((h, w))
    x = np.where((i + j) % 2 == 0, np.where(i < split, 40, 200), 0)
    return x.astype(np.uint8)[:, :, None]


def as_f64(u8, sd=0.08):
    """clip(u8 / 255 + N(0, sd), 0, 1); an all-zero channel plane stays all zero (the NaN case)"""
    rs = np.random.RandomState(_seed("f64", u8.shape))
    x = np.clip(u8 / 255.0 + rs.normal(0.0, sd, u8.shape), 0.0, 1.0)
    zero = ~u8.any(axis=(-3, -2), keepdims=True)
    return np.where(zero, 0.0, x)


def batch_u8():
    h, w, c = 24, 40, 3
    return np.stack([random_bytes(h, w, c), two_level(h, w, c), half_saturated(h, w, c),
                     single_pixel(h, w, c), zero_channel(h, w, c)])


def cases():
    out = []
    for h, w, c in SHAPES:
        out.append((f"random-{h}x{w}x{c}-u8", random_bytes(h, w, c)))
    for h, w, c in ((16, 16, 3), (70, 1100, 3)):
        out.append((f"two-{h}x{w}x{c}-u8", two_level(h, w, c)))
    for h, w, c in ((33, 35, 3), (64, 97, 1)):
        out.append((f"half-{h}x{w}x{c}-u8", half_saturated(h, w, c)))
    out.append(("pixel-17x23x3-u8", single_pixel(17, 23, 3)))
    out.append(("zeroch-16x16x3-u8", zero_channel(16, 16, 3)))
    out.append(("boards-122x100x1-u8", two_boards()))
    out.append(("batch-5x24x40x3-u8", batch_u8()))
    for name, x in list(out):
        out.append((name[:-2] + "f64", as_f64(x)))
    return out


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())
