"""The case table of the quant fit's exact model (tests/quant_fit_model.py), shared by the CPU
tests of the model and the GPU tests of the kernel.  Each case names what it reaches in
csrc/quant.hip; the model's fit of a case is computed once per process and never modified.

  A3 A1  16x24, k = 3 and 1        S = 384 < 512: some threads own no sample; k = 1: no seeding loop
  B      64x128, k = 8, id 3       h w = 8192 exactly: no sampling; upper edge of the KM = 8 kernel
  C      3x2731, k = 9, id 1       h w = 8193: Philox sampling; first k of the KM = 16 kernel; the
                                   apply takes its generic path (h w % 16 != 0)
  D      96x128, k = 16, id 2      Q_KMAX, 4 trials, sampled
  E      37x51, k = 7, id 2^32+5   the id's high word
  F      32x32 two colours, k = 5  the potential reaches 0 (no draw), duplicate centres, three
                                   empty clusters
  G      16x16 constant, k = 4     one nonempty cluster
  H I J  40x40, k = 2, 4, 5        the KM = 4 / KM = 8 dispatch edges
  K      2x2, k = 4                k = S

No case reaches the 100-iteration cap of the Lloyd loop (the longest run here takes 85
iterations); the model restates the cap, nothing here exercises it.
"""
import functools

import numpy as np

from conftest import textured

import quant_fit_model as qm

SEED = 3


def _two_colours():
    img = np.empty((32 * 32, 3), np.uint8)
    img[:] = (20, 180, 90)
    img[np.random.RandomState(0).permutation(32 * 32)[:307]] = (200, 30, 60)  # 30 %
    return img.reshape(32, 32, 3)


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "two_colours":
        img = _two_colours()
    elif name == "constant":
        img = np.full((16, 16, 3), 77, np.uint8)
    else:
        h, w = (int(v) for v in name.split("x"))
        img = textured(1, h, w)[0]
    img.setflags(write=False)
    return img


# name -> (image, k, image id)
CASES = {
    "A3": ("16x24", 3, 0),
    "A1": ("16x24", 1, 0),
    "B": ("64x128", 8, 3),
    "C": ("3x2731", 9, 1),
    "D": ("96x128", 16, 2),
    "E": ("37x51", 7, (1 << 32) + 5),
    "F": ("two_colours", 5, 0),
    "G": ("constant", 4, 0),
    "H": ("40x40", 2, 0),
    "I": ("40x40", 4, 0),
    "J": ("40x40", 5, 0),
    "K": ("2x2", 4, 0),
}
DEGENERATE = ("A1", "F", "G")  # no seeding choice to get wrong: k = 1, or the potential reaches 0


@functools.lru_cache(maxsize=None)
def model(img_name, k, image_id, seed=SEED, mutate=None):
    """(centres, runs) of the model; shared between tests, treat as read-only"""
    return qm.fit(image(img_name), k, seed, image_id, _mutate=mutate)


def case_model(name, mutate=None):
    img_name, k, gid = CASES[name]
    return model(img_name, k, gid, SEED, mutate)
