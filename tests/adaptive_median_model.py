"""The definition of idn.adaptive_median (idn_adaptive_median_u8) in plain numpy.

Per channel plane of every image, BORDER_REPLICATE (np.pad mode="edge"); K = max_ksize odd, 3..31:

    for k = 3, 5, ..., K:
        mn, mx = min, max of the k x k window;  md = its median (rank k*k // 2 of the sorted window)
        if mn < md < mx:                     # stage A: the median is not an extreme
            out = z if mn < z < mx else md   # stage B, with the mn / mx of this same k
            ksize = k; stop
    if no k passed:  out = md of the K x K window;  ksize = 0

One sort of the window per level; slow and obvious.  The kernel is held to this bit for bit, for
`out` and for `ksize`.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MAX_KSIZE = 31


def levels(plane, k):
    """(mn, md, mx, sorted windows) of the k x k windows of a 2-D uint8 plane, edge-padded"""
    r = k // 2
    p = np.pad(plane, r, mode="edge")
    win = sliding_window_view(p, (k, k)).reshape(plane.shape[0], plane.shape[1], k * k)
    s = np.sort(win, axis=-1)
    return s[..., 0], s[..., k * k // 2], s[..., -1], s


def adaptive_median_plane(plane, max_ksize):
    plane = np.ascontiguousarray(plane)
    assert plane.ndim == 2 and plane.dtype == np.uint8
    out = plane.copy()
    ksize = np.zeros(plane.shape, np.uint8)
    undecided = np.ones(plane.shape, bool)
    md = plane
    for k in range(3, max_ksize + 1, 2):
        mn, md, mx, _ = levels(plane, k)
        a = undecided & (mn < md) & (md < mx)
        keep = (mn < plane) & (plane < mx)
        out[a] = np.where(keep, plane, md)[a]
        ksize[a] = k
        undecided &= ~a
        if not undecided.any():
            break
    out[undecided] = md[undecided]  # the fall-through: the median at max_ksize
    return out, ksize


def adaptive_median(img, max_ksize=15):
    """img: uint8 (H,W,C) or (N,H,W,C); returns (out, ksize), both of img's shape and dtype"""
    if max_ksize < 3 or max_ksize > MAX_KSIZE or max_ksize % 2 == 0:
        raise ValueError("max_ksize %r not supported (odd, 3..31)" % (max_ksize,))
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (3, 4)
    x = img[None] if img.ndim == 3 else img
    out = np.empty_like(x)
    ks = np.empty_like(x)
    for i in range(x.shape[0]):
        for ch in range(x.shape[3]):
            out[i, :, :, ch], ks[i, :, :, ch] = adaptive_median_plane(x[i, :, :, ch], max_ksize)
    return (out[0], ks[0]) if img.ndim == 3 else (out, ks)
