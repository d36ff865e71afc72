"""adaptive_median (csrc/adaptive_median_u8.hip) against its definition, bit for bit, for the output
and for the ksize map.

The reference is tests/adaptive_median_model.py; for images of more than MODEL_MAX samples it is
the scipy composition of tests/adaptive_median_scipy.py, which tests/test_adaptive_median.py proves
equal to the model (the model sorts every window at every level and is too slow there).  The
kernel's constants: a workgroup stages AMED_ROWS = 32 output rows (equal bands) by AMED_SEG = 256
row bytes, and each of its four waves owns 64 of those bytes.
"""
import functools

import numpy as np
import pytest

import adaptive_median_model as model
import adaptive_median_scipy
from carve import FILL
from conftest import textured

pytestmark = pytest.mark.gpu

KS = [3, 5, 7, 9, 15, 17, 31]
SHAPES = [(2, 5, 7, 3), (1, 9, 1, 3), (1, 1, 40, 3), (1, 37, 53, 3), (2, 64, 96, 3), (1, 23, 64, 1),
          (1, 20, 70, 4), (1, 40, 129, 3), (1, 140, 129, 3)]
COVERAGE_SHAPES = [(1, 37, 53, 3), (1, 40, 129, 3), (1, 20, 70, 4)]  # every level occurs at K = 31
MODEL_MAX = 16000
_ids = dict(ids=lambda s: "%dx%dx%dx%d" % s)


def _run(img, k, **kw):
    import torch
    import idn
    x = torch.from_numpy(np.array(img)).cuda()  # a private copy: the cached inputs are read-only
    y, ks = idn.adaptive_median(x, k, return_ksize=True, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy(), ks.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _img(shape, seed, kind):
    """kind: 'pepper' (half the samples 0, 3 % 255: reaches every level), 'textured', or the s&p
    amount"""
    n, h, w, c = shape
    img = textured(n, h, w, c=c, seed=seed)
    m = np.random.RandomState(seed).random_sample(img.shape)
    if kind == "pepper":
        img[m < 0.5] = 0
        img[m > 0.97] = 255
    elif kind != "textured":
        img[m < kind / 2] = 0
        img[(m >= kind / 2) & (m < kind)] = 255
    img.setflags(write=False)
    return img


def _reference(img, k):
    if img.size <= MODEL_MAX:
        return model.adaptive_median(img, k)
    return adaptive_median_scipy.adaptive_median(img, k)


@functools.lru_cache(maxsize=None)
def _ref_cached(shape, seed, kind, k):
    out, ks = _reference(_img(shape, seed, kind), k)
    out.setflags(write=False)
    ks.setflags(write=False)
    return out, ks


def _same(got, ref, what):
    for g, r, name in zip(got, ref, ("out", "ksize")):
        assert g.shape == r.shape and g.dtype == r.dtype == np.uint8
        assert np.array_equal(g, r), (what, name, np.argwhere(g != r)[:6])


@pytest.mark.parametrize("shape", SHAPES, **_ids)
@pytest.mark.parametrize("k", KS)
def test_bitexact_every_level(dev, k, shape):
    """pepper-heavy input; images smaller than the window, h = 1, w = 1, odd row bytes, C = 1 and
    4, 387 row bytes (two segments, the second with two idle waves) and 140 rows (five bands)"""
    seed = 10  # one input per shape: the model's map at 31 then holds every level 18 times or more
    ref = _ref_cached(shape, seed, "pepper", k)
    if k == 31 and shape in COVERAGE_SHAPES:
        assert shape[1] * shape[2] * shape[3] <= MODEL_MAX  # the map below is the model's own
        counts = {v: int((ref[1] == v).sum()) for v in [0] + list(range(3, 32, 2))}
        assert min(counts.values()) >= 10, counts
    _same(_run(_img(shape, seed, "pepper"), k), ref, (k, shape))


@pytest.mark.parametrize("k", list(range(3, 32, 2)))
def test_every_max_ksize(dev, k):
    shape = (1, 37, 53, 3)
    _same(_run(_img(shape, 100 + k, "pepper"), k), _ref_cached(shape, 100 + k, "pepper", k), k)


@pytest.mark.parametrize("kind", ["textured", 0.3, 0.6])
@pytest.mark.parametrize("k", [3, 7, 15, 31])
def test_textured_and_symmetric_saltpepper(dev, k, kind):
    for shape in [(1, 37, 53, 3), (1, 20, 70, 4), (1, 23, 64, 1)]:
        seed = 7 * k + shape[3]
        _same(_run(_img(shape, seed, kind), k), _ref_cached(shape, seed, kind, k), (k, kind, shape))


@pytest.mark.parametrize("k", [15, 31])
def test_flat_inputs(dev, k):
    """a constant image comes back unchanged with ksize 0: the level loop runs to K on every lane"""
    for v in (0, 128, 255):
        img = np.full((1, 40, 70, 3), v, np.uint8)
        _same(_run(img, k), (img, np.zeros_like(img)), (k, v))
    img = np.zeros((1, 80, 70, 3), np.uint8)
    img[:, 40:] = 255
    _same(_run(img, k), adaptive_median_scipy.adaptive_median(img, k), (k, "halves"))


def test_full_size(dev):
    shape = (1, 600, 1000, 3)
    _same(_run(_img(shape, 7, 0.4), 7), _ref_cached(shape, 7, 0.4, 7), "full size")


@pytest.mark.parametrize("k", [7, 15])
def test_saltpepper_extremes(dev, k):
    rs = np.random.RandomState(40 + k)
    img = textured(2, 60, 1000, seed=k)
    m = rs.random_sample(img.shape)
    img[m < 0.2] = 0
    img[(m >= 0.2) & (m < 0.4)] = 255
    img[0, 10:20] = 255
    _same(_run(img, k), adaptive_median_scipy.adaptive_median(img, k), k)


@pytest.mark.parametrize("k", [7, 17])
def test_images_do_not_leak(dev, k):
    imgs = np.array(_img((3, 6, 40, 3), 70 + k, "pepper"))
    imgs[1] = 255 - imgs[1]
    batch = _run(imgs, k)
    _same(batch, model.adaptive_median(imgs, k), (k, "batch"))
    for i in range(3):
        _same([b[i] for b in batch], _run(imgs[i], k), (k, i))
    rep = _run(np.stack([imgs[2]] * 3), k)
    for r, b in zip(rep, batch):
        assert np.array_equal(r[0], r[1]) and np.array_equal(r[0], r[2])
        assert np.array_equal(r[0], b[2])
    again = _run(imgs, k)
    _same(again, batch, (k, "second call"))


@pytest.mark.parametrize("shape", [(2, 23, 64, 3), (1, 23, 64, 1), (1, 20, 70, 4)], **_ids)
@pytest.mark.parametrize("k", [7, 17])
def test_layouts(dev, k, shape):
    """src, dst and ksize_map carved out of larger byte buffers at pointer offsets 1, 3, 5 with rows
    of w*c + 5 bytes, through the C entry point: exact bytes, every padding and guard byte of both
    outputs keeps its sentinel, the source is untouched; and the same with ksize_map = NULL"""
    import torch
    from idn import _lib
    lib = _lib.load()
    n, h, w, c = shape
    seed = 7 * k + c
    img = np.array(_img(shape, seed, "pepper"))
    ref = _ref_cached(shape, seed, "pepper", k)
    rb, rs, guard = w * c, w * c + 5, 4096
    body = n * h * rs
    for so, do, ko, with_map in [(1, 3, 5, True), (3, 5, 1, True), (5, 1, 3, True), (1, 3, 5, False)]:
        sbuf = torch.full((guard + 64 + body + guard,), FILL, dtype=torch.uint8, device="cuda")
        dbuf = torch.full_like(sbuf, FILL)
        kbuf = torch.full_like(sbuf, FILL)
        sview = sbuf[guard + so:guard + so + body].view(n, h, rs)
        sview[:, :, :rb] = torch.from_numpy(img.reshape(n, h, rb)).cuda()
        rc = lib.idn_adaptive_median_u8(sbuf.data_ptr() + guard + so, dbuf.data_ptr() + guard + do,
                                        kbuf.data_ptr() + guard + ko if with_map else None,
                                        n, h, w, c, rs, k, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "idn_adaptive_median_u8")
        torch.cuda.synchronize()
        for buf, off, want in ((dbuf, do, ref[0]), (kbuf, ko, ref[1])):
            d = buf.cpu().numpy()
            if buf is kbuf and not with_map:
                assert (d == FILL).all(), "a null ksize_map was written"
                continue
            out = d[guard + off:guard + off + body].reshape(n, h, rs)
            got = out[:, :, :rb].reshape(shape)
            assert np.array_equal(got, want), (k, so, do, ko, np.argwhere(got != want)[:6])
            assert (out[:, :, rb:] == FILL).all(), "row padding written"
            assert (d[:guard + off] == FILL).all() and (d[guard + off + body:] == FILL).all(), \
                "guard written"
        s = sbuf.cpu().numpy()[guard + so:guard + so + body].reshape(n, h, rs)
        assert np.array_equal(s[:, :, :rb].reshape(shape), img), "the source was written"
        assert (s[:, :, rb:] == FILL).all()


def test_out_argument(dev):
    import torch
    import idn
    shape = (2, 23, 64, 3)
    x = torch.from_numpy(np.array(_img(shape, 9, "pepper"))).cuda()
    out = torch.full_like(x, 77)
    y = idn.adaptive_median(x, 9, out=out)
    assert isinstance(y, torch.Tensor) and y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    ref = _ref_cached(shape, 9, "pepper", 9)
    assert np.array_equal(first, ref[0])
    y2, ks = idn.adaptive_median(x, 9, out, return_ksize=True)
    torch.cuda.synchronize()
    assert y2.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), first)
    assert np.array_equal(ks.cpu().numpy(), ref[1])


def test_return_ksize_and_squeeze(dev):
    import torch
    import idn
    shape = (1, 23, 64, 3)
    x = torch.from_numpy(np.array(_img(shape, 4, "pepper"))).cuda()
    ref = _ref_cached(shape, 4, "pepper", 15)
    y = idn.adaptive_median(x[0])  # (H,W,C), the default max_ksize = 15
    assert isinstance(y, torch.Tensor) and y.shape == x.shape[1:] and y.dtype == torch.uint8
    y, ks = idn.adaptive_median(x[0], return_ksize=True)
    assert y.shape == ks.shape == x.shape[1:] and ks.dtype == torch.uint8 and ks.is_cuda
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), ref[0][0]) and np.array_equal(ks.cpu().numpy(), ref[1][0])
    y4, ks4 = idn.adaptive_median(x, 15, return_ksize=True)
    assert y4.shape == ks4.shape == x.shape


@pytest.mark.parametrize("k", [1, 8, 33, -7])
def test_rejections(dev, k):
    import torch
    import idn
    from idn import _lib
    x = torch.from_numpy(np.array(_img((1, 12, 16, 3), 1, "textured"))).cuda()
    out = torch.full_like(x, 77)
    with pytest.raises(_lib.IdnError, match="supported"):
        idn.adaptive_median(x, k, out=out, return_ksize=True)
    torch.cuda.synchronize()
    assert bool((out == 77).all())


def _quality_clean():
    y, x = np.mgrid[0:96, 0:128]
    img = np.stack([40 + x, 60 + y, 200 - (x + y) // 2], axis=-1).astype(np.int64)
    img[20:60, 30:90] += 50
    img[70:90, 10:40, 0] -= 30
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("amount", [0.4, 0.6])
def test_quality_beats_the_fixed_windows(dev, amount):
    """the device's own s&p draw on the smooth 96 x 128 x 3 image: max_ksize = 15 is at least 2 dB
    above the best of median_blur at 5, 9 and 15"""
    import torch
    import idn
    clean = torch.from_numpy(_quality_clean()).cuda()
    noisy = idn.random_noise(clean, "s&p", amount=amount, seed=11)
    fixed = {k: float(idn.psnr(clean, idn.median_blur(noisy, k))) for k in (5, 9, 15)}
    got = float(idn.psnr(clean, idn.adaptive_median(noisy, 15)))
    print("psnr amount", amount, "adaptive15", round(got, 2), "median_blur",
          {k: round(v, 2) for k, v in fixed.items()})
    assert got >= max(fixed.values()) + 2.0, (got, fixed)
