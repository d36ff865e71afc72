"""GPU: idn.denoise_dct against the numpy float64 definition tests/dct_model.py.

The kernel computes in fp32, so a coefficient within rounding of its threshold can fall the other
way and move the samples of its patch by up to about 0.6.  Those samples are the model's risk mask
(margin 2e-3; at most 5 % of an image on the cases used here), and off it the float output lies
within tol = 4 x max|fp32 model - float64 model| (off the mask, on the same input) of the model:
a fast factorisation and another summation order may err a few times as much as the matrix form
of the fp32 model, while a wrong tap, count or threshold errs by 1e-2 or more.  The uint8 output
equals the model's off the mask, except where the model's value lies within tol of a rounding
tie; there it may differ by 1.  Then: the tile seams, the same bits in every batch and on every
call, every way to give sigma, the limit images, layouts and misaligned bases, what is refused,
and the quality on the smooth test image."""
import numpy as np
import pytest

import carve
import dct_model as dm
import wiener_model as wm
from dct_cases import MAX_SHARE, PARITY_SDS, PARITY_SHAPES, parity_case, parity_image, references

pytestmark = pytest.mark.gpu

OFF_LATTICE = 15.1  # a sigma whose threshold 45.3 is no multiple of 1/8 (test_tile_seams)


def dev_of(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


def bits32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def compare(got32, got8, x, r64, r32, mask, what=""):
    """the assertions of the module docstring; returns the largest deviation off the mask"""
    share = mask.mean()
    assert share <= MAX_SHARE, (what, share)
    ok = ~mask
    tol = 4.0 * np.abs(r32.astype(np.float64) - r64)[ok].max()
    assert got32.dtype == np.float32 and got32.shape == x.shape and np.isfinite(got32).all()
    dev = np.abs(got32.astype(np.float64) - r64)[ok].max()
    print(f"{what}: risk share {share:.4f} tol {tol:.3e} deviation off the mask {dev:.3e}")
    assert dev <= tol, (what, dev, tol)
    assert got8.dtype == np.uint8 and got8.shape == x.shape
    ref8 = dm.to_u8(r64)
    near_tie = np.abs(np.abs(r64 - np.floor(r64)) - 0.5) <= tol
    diff = np.abs(got8.astype(np.int16) - ref8.astype(np.int16))
    assert not diff[ok & ~near_tie].any(), what
    assert diff[ok & near_tie].max(initial=0) <= 1, what
    return dev


def check(x, sigma, color, factor=3.0, refs=None, what=""):
    import idn
    r64, r32, mask = refs if refs is not None else references(x, sigma, color, factor)
    got8, got32 = idn.denoise_dct(dev_of(x), sigma, factor=factor, color=color, out="both")
    return compare(got32.cpu().numpy(), got8.cpu().numpy(), x, r64, r32, mask,
                   what or f"{x.shape} sigma {sigma} color {color}")


# ---- parity -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sd", PARITY_SDS, ids=lambda s: f"sd{s:g}")
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity(dev, shape, sd):
    for color in ((False, True) if shape[2] == 3 else (False,)):
        x, r64, r32, mask = parity_case(shape, sd, color)
        check(x, sd, color, refs=(r64, r32, mask))


# ---- seams --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("dh,dw", [(1, 1), (1, -1), (-1, 1), (-1, -1)],
                         ids=["over-over", "over-under", "under-over", "under-under"])
def test_tile_seams(dev, dh, dw, c):
    """one row and one column more and less than one workgroup's patches cover.  OFF_LATTICE:
    on integer planes the coefficients (0,4), (4,0) and (4,4) are multiples of 1/8, and so is
    T = 3 * 15; at 3 * 15.1 = 45.3 none of them can come within the margin of the threshold,
    which keeps the risk share of these larger images below the 5 % (at 15.0 it is 4.5 to 5.3 %)"""
    import idn
    th, tw = idn.ops.DCT_TILE
    x = parity_image((th + 7 + dh, tw + 7 + dw, c), 15.0)
    check(x, OFF_LATTICE, c == 3)
    if c == 3:
        check(x, OFF_LATTICE, False)


@pytest.mark.parametrize("c", [1, 3])
def test_two_tiles_in_each_direction(dev, c):
    import idn
    th, tw = idn.ops.DCT_TILE
    check(parity_image((2 * th + 9, 2 * tw + 9, c), 40.0), 40.0, c == 3)


# ---- determinism --------------------------------------------------------------------------------------

@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_batch_equals_single_images_and_repeats(dev, color):
    import idn
    xd = dev_of(parity_image((3, 40, 75, 3), 15.0))
    a8, a32 = idn.denoise_dct(xd, 15.0, color=color, out="both")
    b8, b32 = idn.denoise_dct(xd, 15.0, color=color, out="both")
    assert np.array_equal(bits32(a32), bits32(b32)) and np.array_equal(a8.cpu().numpy(), b8.cpu().numpy())
    for i in range(3):
        o8, o32 = idn.denoise_dct(xd[i], 15.0, color=color, out="both")
        assert o8.shape == (40, 75, 3) and o32.shape == (40, 75, 3)
        assert np.array_equal(bits32(o32), bits32(a32[i]))
        assert np.array_equal(o8.cpu().numpy(), a8[i].cpu().numpy())
    assert np.array_equal(idn.denoise_dct(xd, 15.0, color=color).cpu().numpy(), a8.cpu().numpy())
    assert np.array_equal(bits32(idn.denoise_dct(xd, 15.0, color=color, out="f32")), bits32(a32))


# ---- sigma --------------------------------------------------------------------------------------------

def test_sigma_forms(dev):
    import torch
    import idn
    x = parity_image((2, 33, 70, 3), 15.0)
    xd = dev_of(x)

    def run(sigma, img=xd):
        return bits32(idn.denoise_dct(img, sigma, out="f32"))

    def t64(v):
        return torch.tensor(v, dtype=torch.float64, device=xd.device)

    want = run(15.0)
    for same in ([15.0] * 3, (15.0, 15.0, 15.0), np.full(3, 15.0), t64([15.0] * 3),
                 t64([[15.0] * 3] * 2), t64([[15.0], [15.0]])):
        assert np.array_equal(run(same), want)
    per_c = [9.0, 15.5, 31.0]
    want = run(per_c)
    assert np.array_equal(run(t64(per_c)), want) and np.array_equal(run(t64([per_c, per_c])), want)
    # another sigma per image: every image equals its own call
    per_nc = [[9.0, 15.5, 31.0], [40.0, 12.0, 20.0]]
    got = run(t64(per_nc))
    per_n = [[12.0], [33.0]]
    got1 = run(t64(per_n))
    for i in range(2):
        assert np.array_equal(got[i], run(per_nc[i], xd[i]))
        assert np.array_equal(got[i], run(t64([per_nc[i]]), xd[i]))  # (1, C) with one image
        assert np.array_equal(got1[i], run(per_n[i][0], xd[i]))
        assert np.array_equal(got1[i], run(t64([per_n[i]]), xd[i]))  # (1, 1)
    # one channel: (N, 1) is (N, C)
    x1 = xd[..., :1].contiguous()
    got = run(t64(per_n), x1)
    for i in range(2):
        assert np.array_equal(got[i], run(per_n[i][0], x1[i]))


def test_estimate_sigma_passes_straight_in(dev):
    import idn
    clean = wm.smooth_image(64, 96)
    x = np.stack([wm.noisy_image(clean, sd, s) for sd, s in ((15.0, 1), (25.0, 2))])
    xd = dev_of(x)
    sg = idn.estimate_sigma(xd)
    assert sg.shape == (2, 3) and sg.is_cuda
    got = idn.denoise_dct(xd, sg, out="f32")
    doubles = sg.cpu().numpy()
    assert ((doubles > 10) & (doubles < 35)).all()
    for i in range(2):
        one = idn.denoise_dct(xd[i], [float(v) for v in doubles[i]], out="f32")
        assert np.array_equal(bits32(got[i]), bits32(one))
        assert np.array_equal(bits32(got[i]), bits32(idn.denoise_dct(xd[i], idn.estimate_sigma(xd[i]),
                                                                      out="f32")))


def test_unequal_sigmas_are_propagated_through_the_colour_transform(dev):
    x = parity_image((33, 70, 3), 15.0)
    # thresholds 27.3, 47.1, 93.9 (and 52.85): off the 1/8 lattice, as in test_tile_seams.  The
    # other factor is a larger one: below 3 the density of noise coefficients at the threshold
    # grows and the risk share with it (10.9 % at 2.7 with the colour transform)
    check(x, [9.1, 15.7, 31.3], True)
    check(x, [9.1, 15.7, 31.3], False)
    check(x, OFF_LATTICE, True, factor=3.5)
    check(x, OFF_LATTICE, False, factor=3.5)


# ---- limit images -------------------------------------------------------------------------------------

@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_zero_sigma_returns_the_input_and_huge_sigma_the_patch_means(dev, color):
    import idn
    x = parity_image((33, 70, 3), 15.0)
    assert np.array_equal(idn.denoise_dct(dev_of(x), 0.0, color=color).cpu().numpy(), x)
    assert np.array_equal(idn.denoise_dct(dev_of(x), 15.0, factor=0.0, color=color).cpu().numpy(), x)
    check(x, 1e6, color)


@pytest.mark.parametrize("c", [1, 3])
def test_limit_images(dev, c):
    import idn
    const = np.full((19, 23, c), 77, np.uint8)
    checker = (((np.arange(19)[:, None] + np.arange(23)[None, :]) % 2) * 255).astype(np.uint8)
    checker = np.repeat(checker[..., None], c, axis=2)
    for color in ((False, True) if c == 3 else (False,)):
        got8, got32 = idn.denoise_dct(dev_of(const), 15.0, color=color, out="both")
        assert np.array_equal(got8.cpu().numpy(), const)
        assert np.abs(got32.cpu().numpy() - 77.0).max() <= 1e-4
        for x in (np.zeros_like(const), np.full_like(const, 255), checker):
            check(x, 40.0, color)


# ---- layouts ------------------------------------------------------------------------------------------

def test_out_u8_given(dev):
    import torch
    import idn
    xd = dev_of(parity_image((2, 33, 70, 3), 15.0))
    ref8, ref32 = idn.denoise_dct(xd, 15.0, out="both")
    out = torch.full_like(xd, 9)
    assert idn.denoise_dct(xd, 15.0, out_u8=out) is out
    assert np.array_equal(out.cpu().numpy(), ref8.cpu().numpy())
    out.fill_(9)
    got = idn.denoise_dct(xd, 15.0, out="both", out_u8=out)
    assert got[0] is out and np.array_equal(out.cpu().numpy(), ref8.cpu().numpy())
    assert np.array_equal(bits32(got[1]), bits32(ref32))
    with pytest.raises(ValueError, match="in-place"):
        idn.denoise_dct(xd, 15.0, out_u8=xd)


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_padded_rows(dev, color):
    import torch
    import idn
    x = parity_image((2, 33, 70, 3), 15.0)
    ref8, ref32 = idn.denoise_dct(dev_of(x), 15.0, color=color, out="both")
    pad = 19
    wide = torch.full((2, 33, 70 * 3 + pad), 0xA5, dtype=torch.uint8, device="cuda")
    xin = wide[:, :, :210].view(2, 33, 70, 3)
    xin.copy_(dev_of(x))
    assert not xin.is_contiguous()
    wide_out = torch.full_like(wide, 0x5A)
    out = wide_out[:, :, :210].view(2, 33, 70, 3)
    idn.denoise_dct(xin, 15.0, color=color, out_u8=out)
    assert np.array_equal(out.cpu().numpy(), ref8.cpu().numpy())
    assert bool((wide_out[:, :, 210:] == 0x5A).all())  # the padding is not written
    assert np.array_equal(idn.denoise_dct(xin, 15.0, color=color).cpu().numpy(), ref8.cpu().numpy())
    f32 = idn.denoise_dct(xin, 15.0, color=color, out="f32")  # read where it lies, written compact
    assert f32.is_contiguous() and np.array_equal(bits32(f32), bits32(ref32))


@pytest.mark.parametrize("offset", [1, 3, 8])
def test_misaligned_bases(dev, offset):
    import idn
    x = parity_image((33, 70, 3), 15.0)
    ref8, ref32 = idn.denoise_dct(dev_of(x), 15.0, out="both")
    buf_x, xd = carve.carve(x, offset)
    buf_y, yd = carve.carve_out(x.shape, np.uint8, (offset * 5) % 16 + 1)
    idn.denoise_dct(xd, 15.0, out_u8=yd)
    assert np.array_equal(yd.cpu().numpy(), ref8.cpu().numpy())
    carve.untouched(buf_y, (offset * 5) % 16 + 1, yd.numel())
    carve.untouched(buf_x, offset, xd.numel())
    assert np.array_equal(xd.cpu().numpy(), x)
    # sigma next to its guards (8-byte steps keep a double aligned)
    buf_s, sg = carve.carve(np.array([15.0, 15.0, 15.0]), 8)
    assert np.array_equal(bits32(idn.denoise_dct(xd, sg, out="f32")), bits32(ref32))
    carve.untouched(buf_s, 8, 24)


# ---- refusals -----------------------------------------------------------------------------------------

def test_refusals(dev):
    import idn
    for shape in ((7, 20, 3), (20, 7, 1), (2, 7, 7, 3)):
        with pytest.raises(idn.IdnError, match="unsupported"):
            idn.denoise_dct(dev_of(np.zeros(shape, np.uint8)), 15.0)
    xd = dev_of(np.zeros((16, 16, 3), np.uint8))
    for patch in (16, 4):
        with pytest.raises(idn.IdnError, match="unsupported"):
            idn.denoise_dct(xd, 15.0, patch=patch)
    assert idn.denoise_dct(dev_of(np.zeros((0, 16, 16, 3), np.uint8)), 15.0).shape == (0, 16, 16, 3)


# ---- quality ------------------------------------------------------------------------------------------

def test_quality_on_the_smooth_image(dev):
    """The model's figures (tests/test_dct_model.py: host noise, so they apply): sd 15, seed 0:
    wiener 5x5 reflect101 32.00 dB, denoise_dct per channel 35.60 (+3.60), with the colour
    transform 39.75 (+4.15, the best case: this image's channels are equal)."""
    import idn
    clean = wm.smooth_image()
    cd = dev_of(np.repeat(clean[..., None], 3, axis=2))
    nd = dev_of(wm.noisy_image(clean, 15.0, 0))
    p_w = float(idn.psnr(cd, idn.wiener(nd, 5, noise=225.0, border="reflect101")))
    p_plain = float(idn.psnr(cd, idn.denoise_dct(nd, 15.0, color=False)))
    p_color = float(idn.psnr(cd, idn.denoise_dct(nd, 15.0, color=True)))
    print(f"wiener {p_w:.3f} denoise_dct {p_plain:.3f} with the colour transform {p_color:.3f}")
    assert p_plain >= p_w + 3.0
    assert p_color >= p_plain + 3.0
