"""GPU: idn.wiener against the numpy definition tests/wiener_model.py, bit for bit: every window
kind, both borders, both outputs, the tile seams of the kernel, every way to give the noise, the
device-side noise estimate, the v == 0 rule, layouts and misaligned bases, and the quality it buys
on the smooth test image."""
import functools

import numpy as np
import pytest

import carve
import wiener_model as wm

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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


def check(x, ksize, noise, border="zero"):
    """both outputs and the noise used, against the model"""
    import idn
    xd = dev_of(x)
    ref, used = wm.wiener(x, ksize, noise, border=border, out="f64", return_noise=True)
    got, got_used = idn.wiener(xd, ksize, noise, border=border, out="f64", return_noise=True)
    assert got.shape == xd.shape and got_used.shape == used.shape
    assert np.array_equal(bits(got_used.cpu().numpy()), bits(used))
    assert np.array_equal(bits(got.cpu().numpy()), bits(ref))
    got8 = idn.wiener(xd, ksize, noise, border=border)
    assert got8.dtype == xd.dtype and np.array_equal(got8.cpu().numpy(), wm.to_u8(ref))


# ---- shapes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", [None, 400.0], ids=["estimated", "given"])
@pytest.mark.parametrize("ksize", [3, (7, 3), 15, 31], ids=str)
@pytest.mark.parametrize("c", [1, 3])
def test_window_larger_than_the_image(dev, c, ksize, noise):
    check(image((5, 7, c)), ksize, noise)


@pytest.mark.parametrize("border", wm.BORDERS)
@pytest.mark.parametrize("ksize", [1, 3, 5, (7, 3), (3, 9), 15, 31], ids=str)
@pytest.mark.parametrize("shape", [(33, 70, 3), (64, 97, 1)], ids=lambda s: "x".join(map(str, s)))
def test_shapes_windows_borders(dev, shape, ksize, border):
    check(image(shape), ksize, None, border)
    check(image(shape), ksize, 300.0, border)


@pytest.mark.parametrize("border", wm.BORDERS)
@pytest.mark.parametrize("c,d", [(1, 1), (1, -1), (3, 1), (3, -1)],
                         ids=["c1-over", "c1-under", "c3-over", "c3-under"])
def test_tile_seams(dev, c, d, border):
    """one more and one less than the workgroup's tile in each direction: at one channel exactly,
    at three the nearest widths on either side of the 256 byte columns"""
    import idn
    rows, cols = idn.ops.WIENER_TILE
    w = cols + d if c == 1 else (cols // 3 + (1 if d > 0 else 0))
    assert (w * c > cols) == (d > 0)
    x = image((rows + d, w, c))
    check(x, (5, 7), None, border)
    check(x, 31, 123.5, border)


def test_two_tiles_in_each_direction(dev):
    import idn
    rows, cols = idn.ops.WIENER_TILE
    check(image((2 * rows + 3, (2 * cols + 30) // 3, 3)), (9, 15), None, "reflect101")


def test_batch_equals_single_images_and_repeats(dev):
    import idn
    x = np.stack([image((40, 53, 3), s) for s in range(3)])
    xd = dev_of(x)
    for noise in (None, 250.0):
        a, na = idn.wiener(xd, 7, noise, out="f64", return_noise=True)
        b, nb = idn.wiener(xd, 7, noise, out="f64", return_noise=True)
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
        assert np.array_equal(bits(na.cpu().numpy()), bits(nb.cpu().numpy()))
        for i in range(3):
            one, n1 = idn.wiener(xd[i], 7, noise, out="f64", return_noise=True)
            assert one.shape == (40, 53, 3) and n1.shape == (3,)
            assert np.array_equal(bits(one.cpu().numpy()), bits(a[i].cpu().numpy()))
            assert np.array_equal(bits(n1.cpu().numpy()), bits(na[i].cpu().numpy()))
        assert np.array_equal(bits(a.cpu().numpy()), bits(wm.wiener(x, 7, noise, out="f64")))


def test_reflect101_refused_where_undefined(dev):
    import idn
    xd = dev_of(image((5, 7, 3)))
    check(image((5, 7, 3)), (9, 13), 100.0, "reflect101")  # 4 < 5 and 6 < 7: the largest defined
    for ksize in ((11, 3), (3, 15), 31):
        with pytest.raises(ValueError, match="reflect101"):
            idn.wiener(xd, ksize, 100.0, border="reflect101")


# ---- the noise ----------------------------------------------------------------------------------------

def test_noise_forms(dev):
    import torch
    import idn
    x = np.stack([image((33, 70, 3), s) for s in range(2)])
    xd = dev_of(x)
    per_c = [90.0, 400.5, 1234.0]
    per_nc = np.array([[50.0, 60.0, 70.0], [800.0, 0.0, 2e4]])
    cases = [(225.0, 225.0), (per_c, per_c), (tuple(per_c), per_c), (np.array(per_c), per_c),
             (torch.tensor(per_c, dtype=torch.float64, device=xd.device), per_c),
             (torch.from_numpy(per_nc).to(xd.device), per_nc)]
    for given, model_noise in cases:
        got, used = idn.wiener(xd, 5, given, out="f64", return_noise=True)
        ref, ref_used = wm.wiener(x, 5, model_noise, out="f64", return_noise=True)
        assert np.array_equal(bits(used.cpu().numpy()), bits(ref_used))
        assert np.array_equal(bits(got.cpu().numpy()), bits(ref))
    # one image with a (1, C) and a (C,) tensor
    one = idn.wiener(xd[1], 5, torch.from_numpy(per_nc[1:]).to(xd.device), out="f64")
    assert np.array_equal(bits(one.cpu().numpy()), bits(wm.wiener(x[1], 5, per_nc[1], out="f64")))


@pytest.mark.parametrize("ksize", [3, (7, 3), 31], ids=str)
def test_estimated_noise_is_the_exact_quotient(dev, ksize):
    import idn
    x = image((64, 97, 3))
    kh, kw = (ksize, ksize) if np.isscalar(ksize) else ksize
    n = kh * kw
    _, used = idn.wiener(dev_of(x), ksize, None, return_noise=True)
    for ch in range(3):
        s1, s2 = wm.window_sums(x[..., ch], ksize)
        want = np.float64(float(wm.q_sum(s1, s2, n))) / np.float64(float(n * n * 64 * 97))
        assert bits(used[ch].cpu().numpy()) == bits(want)


def test_estimate_sigma_squared_passes_straight_through(dev):
    import idn
    clean = wm.smooth_image(64, 96)
    x = np.stack([wm.noisy_image(clean, sd, s) for sd, s in ((15.0, 1), (25.0, 2))])
    xd = dev_of(x)
    var = idn.estimate_sigma(xd) ** 2
    assert var.shape == (2, 3) and var.is_cuda
    got, used = idn.wiener(xd, 5, var, border="reflect101", out="f64", return_noise=True)
    doubles = var.cpu().numpy()
    assert np.array_equal(bits(used.cpu().numpy()), bits(doubles))
    assert ((doubles > 100) & (doubles < 1000)).all()
    ref = wm.wiener(x, 5, doubles, border="reflect101", out="f64")
    assert np.array_equal(bits(got.cpu().numpy()), bits(ref))


def test_zero_noise_returns_the_input_and_huge_noise_the_mean(dev):
    import idn
    x = image((33, 70, 3))
    xd = dev_of(x)
    for border in wm.BORDERS:
        assert np.array_equal(idn.wiener(xd, 5, 0.0, border=border).cpu().numpy(), x)
        got = idn.wiener(xd, (5, 3), 1e9, border=border).cpu().numpy()
        mean = np.stack([wm.stats(x[..., ch], (5, 3), border)[0] for ch in range(3)], axis=-1)
        assert np.array_equal(got, np.rint(mean).astype(np.uint8))


# ---- v == 0 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("border", wm.BORDERS)
def test_all_zero_image_gives_zeros(dev, border):
    import idn
    xd = dev_of(np.zeros((2, 9, 11, 3), np.uint8))
    r, used = idn.wiener(xd, 3, None, border=border, out="f64", return_noise=True)
    assert not bits(r.cpu().numpy()).any() and not bits(used.cpu().numpy()).any()
    assert not idn.wiener(xd, 3, None, border=border).cpu().numpy().any()


def test_flat_half_with_zero_noise_is_finite_and_unchanged(dev):
    import idn
    x = np.random.default_rng(5).integers(0, 256, (12, 20, 1), dtype=np.uint8)
    x[:, 10:] = 255
    r = idn.wiener(dev_of(x), 5, 0.0, out="f64").cpu().numpy()
    assert np.isfinite(r).all()
    assert np.array_equal(r[2:-2, 12:-2], np.full((8, 6, 1), 255.0))
    assert np.array_equal(bits(r), bits(wm.wiener(x, 5, 0.0, out="f64")))


@pytest.mark.parametrize("noise", [None, 0.0, 225.0])
def test_constant_image_keeps_its_interior(dev, noise):
    import idn
    x = np.full((11, 13, 3), 77, np.uint8)
    got = idn.wiener(dev_of(x), (5, 3), noise).cpu().numpy()
    assert np.array_equal(got[2:-2, 1:-1], x[2:-2, 1:-1])
    assert np.array_equal(got, wm.wiener(x, (5, 3), noise))
    assert np.array_equal(idn.wiener(dev_of(x), (5, 3), noise, border="reflect101").cpu().numpy(), x)


# ---- layouts ------------------------------------------------------------------------------------------

def test_out_u8_given(dev):
    import torch
    import idn
    x = np.stack([image((33, 70, 3), s) for s in range(2)])
    xd = dev_of(x)
    out = torch.full_like(xd, 9)
    assert idn.wiener(xd, 5, 300.0, out_u8=out) is out
    assert np.array_equal(out.cpu().numpy(), wm.wiener(x, 5, 300.0))
    with pytest.raises(ValueError, match="in-place"):
        idn.wiener(xd, 5, 300.0, out_u8=xd)


@pytest.mark.parametrize("noise", [None, 300.0], ids=["estimated", "given"])
def test_padded_rows(dev, noise):
    import torch
    import idn
    x = np.stack([image((33, 70, 3), s) for s in range(2)])
    pad = 19
    wide = torch.full((2, 33, 70 * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda")
    xin = wide[:, :, :210].view(2, 33, 70, 3)
    xin.copy_(dev_of(x))
    assert not xin.is_contiguous()
    ref = wm.wiener(x, (7, 5), noise, border="reflect101")
    wide_out = torch.full_like(wide, 0x5A)
    out = wide_out[:, :, :210].view(2, 33, 70, 3)
    idn.wiener(xin, (7, 5), noise, border="reflect101", out_u8=out)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert bool((wide_out[:, :, 210:] == 0x5A).all())  # the padding is not written
    assert np.array_equal(idn.wiener(xin, (7, 5), noise, border="reflect101").cpu().numpy(), ref)
    f64 = idn.wiener(xin, (7, 5), noise, border="reflect101", out="f64")
    assert f64.is_contiguous() and np.array_equal(wm.to_u8(f64.cpu().numpy()), ref)


@pytest.mark.parametrize("offset", [1, 3, 8])
def test_misaligned_bases(dev, offset):
    import idn
    x = image((33, 70, 3))
    ref = wm.wiener(x, 5, None)
    buf_x, xd = carve.carve(x, offset)
    buf_y, yd = carve.carve_out(x.shape, np.uint8, (offset * 5) % 16 + 1)
    idn.wiener(xd, 5, None, out_u8=yd)
    assert np.array_equal(yd.cpu().numpy(), ref)
    carve.untouched(buf_y, (offset * 5) % 16 + 1, yd.numel())
    carve.untouched(buf_x, offset, xd.numel())
    assert np.array_equal(xd.cpu().numpy(), x)
    # the float64 result next to its guards (8-byte steps keep a double aligned)
    buf_n, nz = carve.carve(np.array([100.0, 200.0, 300.0]), 8)
    r = idn.wiener(xd, 5, nz, out="f64")
    assert np.array_equal(bits(r.cpu().numpy()), bits(wm.wiener(x, 5, [100.0, 200.0, 300.0],
                                                                  out="f64")))
    carve.untouched(buf_n, 8, 24)


# ---- quality --------------------------------------------------------------------------------------------

def test_quality_on_the_smooth_image(dev):
    """The model's own figures for seed 0 (computed on the CPU, tests/test_wiener.py holds them):
    noisy 24.61 dB; wiener 5x5 with noise=225: 30.95 dB under the zero border (+6.34), 32.00 dB
    under reflect101 (+7.39); the 5x5 mirror-border box filter 29.52 dB, so +1.43 dB and +2.47 dB.
    The box filter is cv2.blur(x, (5, 5)) restated on the host (rint of the reflect101 window
    mean: 25 taps cannot tie): idn.blur takes ksize 3 only.  The output is bit-equal to the model,
    so the figures are the device's too."""
    import idn
    clean = wm.smooth_image()
    c3 = np.repeat(clean[..., None], 3, axis=2)
    noisy = wm.noisy_image(clean, 15.0, 0)
    box = np.stack([np.rint(wm.stats(noisy[..., ch], 5, "reflect101")[0]) for ch in range(3)],
                   axis=-1).astype(np.uint8)
    cd, nd = dev_of(c3), dev_of(noisy)
    p_noisy = float(idn.psnr(cd, nd))
    p_box = float(idn.psnr(cd, dev_of(box)))
    p_zero = float(idn.psnr(cd, idn.wiener(nd, 5, noise=225.0)))
    p_refl = float(idn.psnr(cd, idn.wiener(nd, 5, noise=225.0, border="reflect101")))
    print(f"noisy {p_noisy:.3f} box {p_box:.3f} wiener zero {p_zero:.3f} reflect101 {p_refl:.3f}")
    assert p_zero >= p_noisy + 5.0
    assert p_zero >= p_box + 1.0
    assert p_refl >= p_zero
