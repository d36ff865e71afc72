"""GPU: idn.blur and idn.gaussian_blur at every odd window 3..31 and with a given sigma, bit for bit
against tests/blur_model.py (and the oracle where it reaches): the seams of the wide kernels'
tiles and strips, images smaller than the window, channel counts, the largest sums, the sigma
cases, padded rows and misaligned bases through the C entry, batching, out=, the unchanged 3 and 5
paths, the blob fallback, the refusals, and the quality the wider windows buy."""
import functools

import numpy as np
import pytest

import blur_model as bm
import carve
import wiener_model as wm
from blur_cases import (BOX7_OVER_3, GAUSS9_OVER_3, GAUSS9_OVER_5, KS, QUALITY_SEED, QUALITY_VAR,
                        TAPS, quality_figures)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def image(shape, seed=0):
    """random bytes with a flat patch and a saturated patch (read-only)"""
    x = np.random.default_rng(seed + 7 * shape[-2]).integers(0, 256, shape, dtype=np.uint8)
    h, w = shape[-3], shape[-2]
    x[..., : h // 3, : w // 3, :] = 200
    x[..., h - h // 4:, w - w // 4:, :] = 255
    x.setflags(write=False)
    return x


def dev_of(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


@functools.lru_cache(maxsize=None)
def ref_box(shape, k, seed=0):
    return bm.blur(image(shape, seed), k)


@functools.lru_cache(maxsize=None)
def ref_gauss(shape, k, sigma=0.0, seed=0):
    return bm.gaussian_blur(image(shape, seed), k, sigma)


def check_both(shape, k):
    import idn
    xd = dev_of(image(shape))
    got = idn.blur(xd, k)
    assert got.shape == xd.shape and got.dtype == xd.dtype
    assert np.array_equal(got.cpu().numpy(), ref_box(shape, k)), ("box", shape, k)
    assert np.array_equal(idn.gaussian_blur(xd, k).cpu().numpy(), ref_gauss(shape, k)), \
        ("gaussian", shape, k)


def seam_shape():
    """three channels, one strip and three rows, one tile and a few byte columns of every wide
    kernel: idn.ops.BLUR_TILE holds (strip rows, tile byte columns) of the box kernel (128, 256)
    and of the Gaussian kernel at 3 channels (128, 252: whole groups of 4 pixels)"""
    import idn
    rows_b, cols_b = idn.ops.BLUR_TILE["box"]
    rows_g, cols_g = idn.ops.BLUR_TILE["gaussian"][3]
    h = max(rows_b, rows_g) + 3
    w = max(cols_b, cols_g) // 3 + 5
    assert h > rows_b and h > rows_g and w * 3 > cols_b and w * 3 > cols_g
    assert h * w * 3 <= 100 * 400 * 3
    return (h, w, 3)


@pytest.mark.parametrize("k", KS)
def test_every_window_on_the_seams(dev, k):
    check_both(seam_shape(), k)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 40, 3), (2, 24, 3), (5, 3, 3), (3, 4, 3)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [7, 15, 31])
def test_images_smaller_than_the_window(dev, k, shape):
    check_both(shape, k)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [7, 31])
def test_channels(dev, k, c):
    """wider than one tile at every channel count (the Gaussian tile is 256, 256, 252, 256)"""
    check_both((37, 280 // c + 3, c), k)


@pytest.mark.parametrize("kind", ["zeros", "full", "checkerboard"])
def test_extremes_at_31(dev, kind):
    import idn
    shape = (40, 90, 3)
    if kind == "checkerboard":  # the largest sums next to the smallest
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        x = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    else:
        x = np.full(shape, 0 if kind == "zeros" else 255, np.uint8)
    xd = dev_of(x)
    for k in (29, 31):
        b, g = idn.blur(xd, k).cpu().numpy(), idn.gaussian_blur(xd, k).cpu().numpy()
        assert np.array_equal(b, bm.blur(x, k)) and np.array_equal(g, bm.gaussian_blur(x, k))
        if kind != "checkerboard":
            assert np.array_equal(b, x) and np.array_equal(g, x)


@pytest.mark.parametrize("ks", sorted(TAPS), ids=str)
def test_sigma_cases(dev, ks):
    import idn
    shape = (45, 91, 3)
    k, sigma = ks
    xd = dev_of(image(shape))
    got = idn.gaussian_blur(xd, k, sigma=sigma).cpu().numpy()
    assert np.array_equal(got, ref_gauss(shape, k, sigma))
    assert idn.ops.gaussian_taps(k, sigma).tolist() == TAPS[ks]
    if ks == (3, 0.1):
        assert np.array_equal(got, image(shape))  # the tap of 256: the identity


def test_sigma_0_at_7_is_the_dyadic_kernel_not_sigma_1_4(dev):
    """0.3 * ((7 - 1) * 0.5 - 1) + 0.8 = 1.4, but sigma 0 takes OpenCV's fixed kernel"""
    import idn
    shape = (45, 91, 3)
    xd = dev_of(image(shape))
    a = idn.gaussian_blur(xd, 7).cpu().numpy()
    b = idn.gaussian_blur(xd, 7, sigma=1.4).cpu().numpy()
    assert bm.gaussian_taps(7, 1.4).tolist() != bm.gaussian_taps(7, 0.0).tolist()
    assert np.array_equal(a, ref_gauss(shape, 7)) and np.array_equal(b, ref_gauss(shape, 7, 1.4))
    assert not np.array_equal(a, b)


# ---- layouts ------------------------------------------------------------------------------------------

def _call(entry, xin, out, stride, k, sigma=None):
    import torch
    from idn import _lib
    n, h, w, c = xin.shape
    args = (k,) if sigma is None else (k, float(sigma))
    rc = getattr(_lib.load(), entry)(xin.data_ptr(), out.data_ptr(), n, h, w, c, stride, *args,
                                     torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, entry)


@pytest.mark.parametrize("k", [7, 31])
def test_padded_rows_through_the_c_entry(dev, k):
    import torch
    x = np.stack([image((33, 90, 3), s) for s in range(2)])
    rb, pad = 270, 19
    wide = torch.full((2, 33, rb + pad), 0xA5, dtype=torch.uint8, device="cuda")
    xin = wide[:, :, :rb].view(2, 33, 90, 3)
    xin.copy_(dev_of(x))
    for entry, sigma, ref in (("idn_box_blur_u8", None, bm.blur(x, k)),
                              ("idn_gaussian_blur_u8", None, bm.gaussian_blur(x, k)),
                              ("idn_gaussian_blur_sigma_u8", 2.5, bm.gaussian_blur(x, k, 2.5))):
        wide_out = torch.full_like(wide, 0x5A)
        out = wide_out[:, :, :rb].view(2, 33, 90, 3)
        _call(entry, xin, out, rb + pad, k, sigma)
        assert np.array_equal(out.cpu().numpy(), ref), entry
        assert bool((wide_out[:, :, rb:] == 0x5A).all()), entry  # the padding is not written
    assert bool((wide[:, :, rb:] == 0xA5).all())


@pytest.mark.parametrize("offset", [1, 3, 8])
def test_misaligned_bases(dev, offset):
    shape = (33, 90, 3)
    x = image(shape)
    for entry, sigma, ref in (("idn_box_blur_u8", None, ref_box(shape, 9)),
                              ("idn_gaussian_blur_u8", None, ref_gauss(shape, 9)),
                              ("idn_gaussian_blur_sigma_u8", 2.5, ref_gauss(shape, 9, 2.5))):
        buf_x, xd = carve.carve(x[None], offset)
        buf_y, yd = carve.carve_out((1,) + shape, np.uint8, offset)
        assert xd.data_ptr() % 16 == offset and yd.data_ptr() % 16 == offset
        _call(entry, xd, yd, 270, 9, sigma)
        assert np.array_equal(yd[0].cpu().numpy(), ref), entry
        carve.untouched(buf_y, offset, yd.numel())
        carve.untouched(buf_x, offset, xd.numel())
        assert np.array_equal(xd[0].cpu().numpy(), x)


def test_batch_equals_single_images(dev):
    import idn
    shape = (40, 91, 3)
    x = np.stack([image(shape, s) for s in range(3)])
    xd = dev_of(x)
    for k in (7, 21):
        b, g = idn.blur(xd, k), idn.gaussian_blur(xd, k, sigma=3.0)
        assert np.array_equal(b.cpu().numpy(), bm.blur(x, k))
        assert np.array_equal(g.cpu().numpy(), bm.gaussian_blur(x, k, 3.0))
        for i in range(3):
            assert np.array_equal(idn.blur(xd[i], k).cpu().numpy(), b[i].cpu().numpy())
            assert np.array_equal(idn.gaussian_blur(xd[i], k, sigma=3.0).cpu().numpy(),
                                  g[i].cpu().numpy())


def test_out_given_and_empty_batch(dev):
    import torch
    import idn
    shape = (33, 90, 3)
    xd = dev_of(image(shape))
    for fn, ref in ((lambda o: idn.blur(xd, 11, out=o), ref_box(shape, 11)),
                    (lambda o: idn.gaussian_blur(xd, 11, out=o), ref_gauss(shape, 11)),
                    (lambda o: idn.gaussian_blur(xd, 11, o, sigma=2.5), ref_gauss(shape, 11, 2.5))):
        out = torch.full_like(xd, 9)
        got = fn(out)
        assert got.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), ref)
    empty = torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda")
    assert idn.blur(empty, 9).shape == (0, 8, 8, 3)
    assert idn.gaussian_blur(empty, 9, sigma=2.0).shape == (0, 8, 8, 3)


# ---- what must not move -------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(33, 90, 3), (37, 72, 4), (2, 3, 3), (600, 1000, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_3_and_5_still_equal_the_oracle(dev, shape):
    import idn
    import oracle.cv
    x = image(shape)
    xd = dev_of(x)
    assert np.array_equal(idn.gaussian_blur(xd, 5).cpu().numpy(), oracle.cv.gaussian_blur(x, 5))
    assert np.array_equal(idn.gaussian_blur(xd, 3).cpu().numpy(), oracle.cv.gaussian_blur(x, 3))
    assert np.array_equal(idn.blur(xd, 3).cpu().numpy(), oracle.cv.blur(x, 3))
    if shape[0] < 100:  # and a sigma of 0 given by name is the same call
        assert np.array_equal(idn.gaussian_blur(xd, 5, sigma=0.0).cpu().numpy(),
                              oracle.cv.gaussian_blur(x, 5))
        assert np.array_equal(idn.blur(xd, 5).cpu().numpy(), oracle.cv.blur(x, 5))


def test_blob_falls_back_at_7(dev):
    import idn
    x = np.stack([image((40, 88, 3), s) for s in range(2)])
    xd = dev_of(x)
    got = idn.ops.gaussian_blob(xd, 7)
    want = idn.ops.blob(idn.gaussian_blur(xd, 7))
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    means = np.asarray(idn.ops.PIXEL_MEANS)
    ref = (bm.gaussian_blur(x, 7).astype(np.float64) - means).astype(np.float32)
    assert np.array_equal(got.cpu().numpy(), ref)


def test_refusals(dev):
    import idn
    from idn._lib import IdnError
    xd = dev_of(image((33, 90, 3)))
    for k in (1, 4, 33):
        with pytest.raises(IdnError):
            idn.blur(xd, k)
        with pytest.raises(IdnError):
            idn.gaussian_blur(xd, k)
        with pytest.raises(IdnError):
            idn.gaussian_blur(xd, k, sigma=1.0)
    for sigma in (-1.0, float("nan"), float("inf")):
        with pytest.raises(IdnError):
            idn.gaussian_blur(xd, 9, sigma=sigma)


# ---- quality --------------------------------------------------------------------------------------------

def test_quality_on_the_smooth_image(dev):
    """idn.random_noise at var = (40/255)^2 on the smooth image: the 9 Gaussian beats the 5 and the
    3, the 7 box the 3 box.  The model on this draw (tests/test_blur_model.py computes it from the
    host model of the noise stream): noisy 16.33 dB, Gaussian 3 / 5 / 9 24.31 / 26.27 / 27.76,
    box 3 / 7 24.87 / 27.04, so +1.49, +3.45 and +2.17 dB against thresholds of 1.0, 3.0, 1.5."""
    import idn
    clean = wm.smooth_image()
    c3 = np.repeat(clean[..., None], 3, axis=2)
    cd = dev_of(c3)
    nd = idn.random_noise(cd, "gaussian", var=QUALITY_VAR, seed=QUALITY_SEED, out="u8")
    p = lambda y: float(idn.psnr(cd, y))  # noqa: E731
    g = {k: p(idn.gaussian_blur(nd, k)) for k in (3, 5, 9)}
    b = {k: p(idn.blur(nd, k)) for k in (3, 7)}
    print(f"noisy {p(nd):.3f} gauss 3/5/9 {g[3]:.3f} {g[5]:.3f} {g[9]:.3f} box 3/7 {b[3]:.3f} "
          f"{b[7]:.3f}")
    assert g[9] >= g[5] + GAUSS9_OVER_5
    assert g[9] >= g[3] + GAUSS9_OVER_3
    assert b[7] >= b[3] + BOX7_OVER_3
    # the model on the device's draw gives the device's figures
    mg, mb = quality_figures(c3, nd.cpu().numpy())
    for k in g:
        assert abs(mg[k] - g[k]) < 1e-6
    for k in b:
        assert abs(mb[k] - b[k]) < 1e-6
