"""median_blur at ksize 7..31 (csrc/median_large_u8.hip) against oracle.cv.median_blur, bit for bit.

Product library, no knobs, except test_band_knob.  The kernel's constants: a wave owns MEDL_SEG =
64 output bytes of a row and marches down a band of at most MEDL_BAND_ROWS = 128 rows (a launch
that leaves most of the device idle halves its bands, down to MEDL_BAND_MIN = 32 rows).
ksize <= 15 runs the byte-bin instance, ksize >= 17 the u16-bin one.
"""
import functools

import numpy as np
import pytest

from carve import FILL
from conftest import textured

pytestmark = pytest.mark.gpu

KS = [7, 9, 11, 15, 17, 31]
SHAPES = [(2, 5, 7, 3), (1, 9, 1, 3), (1, 1, 40, 3), (1, 37, 53, 3), (2, 64, 96, 3), (1, 23, 64, 1),
          (1, 20, 70, 4), (1, 40, 129, 3), (1, 140, 129, 3)]


def _run(img, k, **kw):
    import torch
    import idn
    y = idn.median_blur(torch.from_numpy(img).cuda(), k, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _img(shape, seed):
    n, h, w, c = shape
    return textured(n, h, w, c=c, seed=seed)


@functools.lru_cache(maxsize=None)
def _ref_cached(shape, seed, k):
    import oracle
    r = oracle.cv.median_blur(_img(shape, seed), k)
    r.setflags(write=False)
    return r


def _same(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.array_equal(got, ref), (what, np.argwhere(got != ref)[:6])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("k", KS)
def test_bitexact_small(dev, k, shape):
    """images smaller than the window, h = 1, w = 1, odd row bytes, C = 1 and 4, and 140 x 129 x 3:
    387 row bytes are seven 64-byte wave segments, and 140 rows are more than one band whatever
    the band height (MEDL_BAND_ROWS = 128; this launch takes five bands of 28 rows)"""
    seed = sum(shape) + k
    _same(_run(_img(shape, seed), k), _ref_cached(shape, seed, k), (k, shape))


@pytest.mark.parametrize("k", list(range(7, 32, 2)))
def test_every_ksize(dev, k):
    shape = (1, 37, 53, 3)
    _same(_run(_img(shape, 100 + k), k), _ref_cached(shape, 100 + k, k), k)


@pytest.mark.parametrize("k", [15, 17, 31])
def test_counter_limits_constant(dev, k):
    """one bin holds the whole window: 225 (the byte bin's worst case), 289, 961"""
    import oracle
    for v in (0, 255, 128):
        img = np.full((1, 40, 70, 3), v, np.uint8)
        _same(_run(img, k), img, (k, v))
    img = np.zeros((1, 80, 70, 3), np.uint8)
    img[:, 40:] = 255  # a march down it empties bin 0 while it fills bin 255
    _same(_run(img, k), oracle.cv.median_blur(img, k), (k, "halves"))


@pytest.mark.parametrize("k", [7, 15, 31])
def test_saltpepper_extremes(dev, k):
    import oracle
    rs = np.random.RandomState(40 + k)
    img = textured(2, 60, 1000, seed=k)
    m = rs.random_sample(img.shape)
    img[m < 0.2] = 0
    img[(m >= 0.2) & (m < 0.4)] = 255
    img[0, 10:20] = 255
    _same(_run(img, k), oracle.cv.median_blur(img, k), k)


@pytest.mark.parametrize("k", [7, 15])
def test_full_size(dev, k):
    shape = (1, 600, 1000, 3)
    _same(_run(_img(shape, k), k), _ref_cached(shape, k, k), k)


@pytest.mark.parametrize("k", [7, 17])
def test_images_do_not_leak(dev, k):
    imgs = textured(3, 6, 40, seed=70 + k)
    imgs[1] = 255 - imgs[1]
    batch = _run(imgs, k)
    for i in range(3):
        _same(batch[i], _run(imgs[i], k), (k, i))
    rep = _run(np.stack([imgs[2]] * 3), k)
    assert np.array_equal(rep[0], rep[1]) and np.array_equal(rep[0], rep[2])
    _same(rep[0], batch[2], (k, "repeated"))


@pytest.mark.parametrize("shape", [(2, 23, 64, 3), (1, 23, 64, 1)], ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("k", [7, 17])
def test_layouts(dev, k, shape):
    """src and dst carved out of larger byte buffers at pointer offsets 1, 3, 5 with rows of
    w*c + 5 bytes, through the C entry point: exact bytes, and every padding and guard byte of the
    destination keeps its sentinel"""
    import torch
    from idn import _lib
    lib = _lib.load()
    n, h, w, c = shape
    seed = 7 * k + c
    img = _img(shape, seed)
    ref = _ref_cached(shape, seed, k)
    rb, rs, guard = w * c, w * c + 5, 4096
    body = n * h * rs
    for so, do in [(1, 3), (3, 5), (5, 1)]:
        sbuf = torch.full((guard + 64 + body + guard,), FILL, dtype=torch.uint8, device="cuda")
        dbuf = torch.full_like(sbuf, FILL)
        sview = sbuf[guard + so:guard + so + body].view(n, h, rs)
        sview[:, :, :rb] = torch.from_numpy(img.reshape(n, h, rb)).cuda()
        rc = lib.idn_median_blur_u8(sbuf.data_ptr() + guard + so, dbuf.data_ptr() + guard + do,
                                    n, h, w, c, rs, k, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "idn_median_blur_u8")
        torch.cuda.synchronize()
        d = dbuf.cpu().numpy()
        out = d[guard + do:guard + do + body].reshape(n, h, rs)
        _same(out[:, :, :rb].reshape(shape), ref, (k, so, do))
        assert (out[:, :, rb:] == FILL).all(), "row padding written"
        assert (d[:guard + do] == FILL).all() and (d[guard + do + body:] == FILL).all(), "guard written"
        s = sbuf.cpu().numpy()[guard + so:guard + so + body].reshape(n, h, rs)
        assert np.array_equal(s[:, :, :rb].reshape(shape), img), "the source was written"


def test_out_argument(dev):
    import torch
    import idn
    shape = (2, 23, 64, 3)
    img = _img(shape, 9)
    x = torch.from_numpy(img).cuda()
    out = torch.full_like(x, 77)
    y = idn.median_blur(x, 9, out=out)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    _same(first, _ref_cached(shape, 9, 9), "out=")
    idn.median_blur(x, 9, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)


@pytest.mark.parametrize("k", [1, 8, 33, -7])
def test_rejections(dev, k):
    import torch
    import idn
    from idn import _lib
    x = torch.from_numpy(_img((1, 12, 16, 3), 1)).cuda()
    out = torch.full_like(x, 77)
    with pytest.raises(_lib.IdnError, match="supported"):
        idn.median_blur(x, k, out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())


@pytest.mark.parametrize("k", [7, 17])
def test_band_knob(dev, k, monkeypatch):
    """tuning build, IDN_MEDIAN_LARGE_ROWS = 7: 23 rows are four bands (three bands would do)"""
    from idn import _lib
    shape = (1, 23, 64, 3)
    monkeypatch.setenv("IDN_MEDIAN_LARGE_ROWS", "7")
    with _lib.variant("tuning"):
        got = _run(_img(shape, 50 + k), k)
    _same(got, _ref_cached(shape, 50 + k, k), k)


def _quality_clean():
    y, x = np.mgrid[0:96, 0:128]
    img = np.stack([40 + x, 60 + y, 200 - (x + y) // 2], axis=-1).astype(np.int64)
    img[20:60, 30:90] += 50
    img[70:90, 10:40, 0] -= 30
    return np.clip(img, 0, 255).astype(np.uint8)


def test_quality_on_heavy_saltpepper(dev):
    """s&p at amount 0.6 on the smooth 96 x 128 x 3 image: the 9 x 9 median beats the 5 x 5 by at
    least 3 dB (scipy with numpy's s&p: 8.9 dB) and the 15 x 15 the 9 x 9 by more than 1 dB (2.8)"""
    import torch
    import idn
    clean = torch.from_numpy(_quality_clean()).cuda()
    noisy = idn.random_noise(clean, "s&p", amount=0.6, seed=11)
    p = {k: float(idn.psnr(clean, idn.median_blur(noisy, k))) for k in (5, 9, 15)}
    print("psnr", p)
    assert p[9] >= p[5] + 3.0, p
    assert p[15] > p[9] + 1.0, p
