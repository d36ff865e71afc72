"""The adaptive median of tests/adaptive_median_model.py composed from scipy.ndimage's minimum /
maximum / median filters (size=(k, k, 1), mode="nearest"): the installed library the model is
pinned to (tests/test_adaptive_median.py), and the reference where the model is too slow."""
import numpy as np


def adaptive_median(img, max_ksize=15):
    """img: uint8 (N,H,W,C); returns (out, ksize)"""
    import scipy.ndimage as ndi
    assert img.dtype == np.uint8 and img.ndim == 4
    out = img.copy()
    ksize = np.zeros(img.shape, np.uint8)
    for i, im in enumerate(img):
        undecided = np.ones(im.shape, bool)
        md = im
        for k in range(3, max_ksize + 1, 2):
            size = (k, k, 1)
            mn = ndi.minimum_filter(im, size=size, mode="nearest")
            mx = ndi.maximum_filter(im, size=size, mode="nearest")
            md = ndi.median_filter(im, size=size, mode="nearest")
            a = undecided & (mn < md) & (md < mx)
            keep = (mn < im) & (im < mx)
            out[i][a] = np.where(keep, im, md)[a]
            ksize[i][a] = k
            undecided &= ~a
        out[i][undecided] = md[undecided]
    return out, ksize
