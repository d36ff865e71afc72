"""CPU: the public range of median_blur (odd ksize 3..31), its host-side rejections, and the
yardstick oracle.cv.median_blur pinned to scipy at the window sizes the histogram kernel adds."""
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import textured

ROOT = Path(__file__).resolve().parent.parent


def test_max_ksize_constant():
    from idn import ops
    assert ops.MEDIAN_MAX_KSIZE == 31


def test_header_comment_names_the_range():
    text = (ROOT / "include" / "idn.h").read_text()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int idn_median_blur_u8\(", text, flags=re.S)
    assert m, "idn_median_blur_u8 has no comment"
    assert re.search(r"\b31\b", m.group(1)), m.group(1)


@pytest.mark.parametrize("k", [33, 8, 1])
def test_rejected_on_the_host(k):
    """dummy non-null pointers, never dereferenced: IDN_EUNSUPPORTED (-2) before any launch"""
    from idn import _lib
    lib = _lib.load()
    rc = lib.idn_median_blur_u8(1, 2, 1, 8, 8, 3, 24, k, None)
    assert rc == -2
    msg = lib.idn_last_error().decode()
    assert "supported" in msg and "3..31" in msg, msg


ORACLE_SHAPES = [(2, 5, 7, 3), (1, 9, 1, 3), (1, 1, 40, 3), (2, 23, 64, 3), (1, 37, 53, 1),
                 (1, 20, 70, 4), (1, 40, 129, 3)]


@pytest.mark.parametrize("k", [7, 9, 15, 17, 31])
def test_oracle_equals_scipy(k):
    import oracle
    import scipy.ndimage as ndi
    for shape in ORACLE_SHAPES:
        n, h, w, c = shape
        img = textured(n, h, w, c=c, seed=k + sum(shape))
        m = np.random.RandomState(k).random_sample(img.shape)
        img[m < 0.3] = 0
        img[(m >= 0.3) & (m < 0.6)] = 255
        ref = np.stack([ndi.median_filter(im, size=(k, k, 1), mode="nearest") for im in img])
        got = oracle.cv.median_blur(img, k)
        assert np.array_equal(got, ref), (k, shape, np.argwhere(got != ref)[:6])
