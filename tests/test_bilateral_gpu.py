"""GPU: idn.bilateral_filter / idn_bilateral_u8 against the float64 model
(tests/bilateral_model.py) at every radius, on every kernel the dispatch at the end of
csrc/bilateral_u8.hip can choose, across tile seams, with padded rows and in the persistent loop.

Which kernel a case runs (R = radius):
  C = 3, R <= 5, w >= 2   bilateral_u8_pre2_kernel<R>  (128 x 32 tiles, persistent workgroups)
  C = 3, R >= 6 or w = 1  bilateral_u8_kernel<3, R>    (64 x 16 tiles)
  C = 1                   bilateral_u8_kernel<1, R>

  test                               d              C, w          kernels
  test_every_radius                  3..17 odd      3, 129        pre2<1..5>, generic<3, 6..8>
                                     3..17 odd      1, 129        generic<1, 1..8>
  test_generic_color_small_radii     3..11 odd      3, 1          generic<3, 1..5>
  test_even_and_degenerate_d         1..17          3 and 1, 70   pre2<1..5>, generic<3, 6..8>,
                                                                  generic<1, 1..8>
  test_derived_radius                <= 0           3 and 1, 70   R = 1, 2, 4, 5, 8
  test_smaller_than_window           7, 11, 17      3 and 1, 1..5 pre2<3, 5>, generic<3, 3|5|8>
                                                                  (w = 1), generic<1, 3|5|8>
  test_persistent_loop               5, 9, 11       3, 6          pre2<2, 4, 5>, 2-3 tiles each
  test_row_padding                   5, 11, 15 / 7  3 / 1, 70     pre2<2, 5>, generic<3, 7>,
                                                                  generic<1, 3>
  test_tuning_forms                  3..11 odd      3, 129        pre2<1..5, SYM = false>,
                                                                  bilateral_u8_pre_kernel<1..5, 4>
"""
import numpy as np
import pytest

import bilateral_model as bm

pytestmark = pytest.mark.gpu


def _run(img, d, sc, ss):
    import torch
    import idn
    y = idn.bilateral_filter(torch.tensor(np.asarray(img)).cuda(), d, sc, ss)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _hold(got, pre, what):
    bad, stats = bm.rule(got, pre)
    print(f"{what}: {stats['mismatches']} of {stats['samples']} differ, "
          f"boundary dist {stats['max_boundary_dist']:.3g}")
    assert not bad, (what, bad)
    return stats


@pytest.mark.parametrize("family", bm.FAMILIES)
@pytest.mark.parametrize("params", bm.WIDE + bm.NARROW, ids=lambda p: f"d{p[0]}-{p[1]:g}-{p[2]:g}")
@pytest.mark.parametrize("shape", bm.SEAM_SHAPES, ids=lambda s: f"c{s[3]}")
def test_every_radius(dev, shape, params, family):
    """every radius 1..8 for both channel counts on an image of odd width that crosses the
    tile seams of both kernels: the rule against the model, and <= 1 LSB from the fp32 oracle"""
    import oracle
    img, pre = bm.case(family, shape, params)
    got = _run(img, *params)
    _hold(got, pre, (family, shape, params))
    ref = oracle.cv.bilateral_filter(img, *params)
    assert np.abs(got.astype(np.int32) - ref.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("params", bm.WIDE[:5], ids=lambda p: f"d{p[0]}")
def test_generic_color_small_radii(dev, params):
    """w == 1 sends C = 3 at radius 1..5 to the generic kernel; 20 rows are two of its tiles"""
    img, pre = bm.case("bytes", bm.COLUMN_SHAPE, params)
    _hold(_run(img, *params), pre, params)


@pytest.mark.parametrize("shape", bm.EVEN_SHAPES, ids=lambda s: f"c{s[3]}")
@pytest.mark.parametrize("d,same_as", bm.EVEN_D)
def test_even_and_degenerate_d(dev, shape, d, same_as):
    """radius = d // 2, at least 1: d = 1, 2 filter like 3 and an even d like d + 1"""
    assert bm.radius_of(d, bm.EVEN_SIGMAS[1]) == same_as // 2
    p, q = (d,) + bm.EVEN_SIGMAS, (same_as,) + bm.EVEN_SIGMAS
    img, pre = bm.case("bytes", shape, p)
    got = _run(img, *p)
    np.testing.assert_array_equal(got, _run(img, *q))
    _hold(got, pre, p)
    np.testing.assert_array_equal(pre, bm.bilateral(img, *q))


@pytest.mark.parametrize("shape", bm.DERIVED_SHAPES, ids=lambda s: f"c{s[3]}")
@pytest.mark.parametrize("params,radius", bm.DERIVED, ids=lambda v: str(v).replace(" ", ""))
def test_derived_radius(dev, shape, params, radius):
    """d <= 0: radius = rint(1.5 * sigma_space), half to even (4.5 -> 4, 7.5 -> 8), at least 1"""
    assert bm.radius_of(params[0], params[2]) == radius
    img, pre = bm.case("saltpepper", shape, params)
    got = _run(img, *params)
    _hold(got, pre, params)
    # and the bytes of the explicit window of that radius
    np.testing.assert_array_equal(got, _run(img, 2 * radius + 1, params[1], params[2]))


@pytest.mark.parametrize("shape", bm.DERIVED_SHAPES, ids=lambda s: f"c{s[3]}")
def test_sigma_clamps(dev, shape):
    """sigma <= 0 counts as 1"""
    img, pre = bm.case("textured", shape, (5, 1.0, 1.0))
    want = _run(img, 5, 1.0, 1.0)
    _hold(want, pre, "sigma 1")
    for p in bm.SIGMA_CLAMPS:
        np.testing.assert_array_equal(_run(img, *p), want)
        np.testing.assert_array_equal(bm.bilateral(img, *p), pre)


@pytest.mark.parametrize("c", [3, 1])
def test_smaller_than_window(dev, c):
    """images smaller than the window at radius 3, 5 and 8: nearly every tap is border.  The
    images are a few bytes each, so the mismatch cap applies to the pooled cases"""
    gots, pres = [], []
    for n, h, w in bm.TINY_SHAPES:
        for d in bm.TINY_D:
            for family in ("bytes", "saltpepper"):
                params = (d, 200.0, 100.0)
                img, pre = bm.case(family, (n, h, w, c), params)
                got = _run(img, *params)
                diff = np.abs(got.astype(np.int32) - bm.to_u8(pre).astype(np.int32))
                assert diff.max() <= 1, (family, (n, h, w), d)
                gots.append(got)
                pres.append(pre)
    _hold(gots, pres, f"pooled c={c}")


@pytest.mark.parametrize("d", bm.PERSISTENT_D)
def test_persistent_loop(dev, d):
    """more tiles than resident workgroups (2 per CU): every workgroup of the two-column kernel
    takes a second and some a third tile, with a new image base and a re-staged tile each time.
    The bytes equal the same images in calls of one tile per workgroup"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = bm.persistent_n(cus)
    params = (d, 200.0, 100.0)
    img, pre = bm.case("bytes", (n,) + bm.PERSISTENT_HW + (3,), params)
    got = _run(img, *params)
    _hold(got, pre, (n, params))
    parts = [_run(img[i:i + cus], *params) for i in range(0, n, cus)]
    np.testing.assert_array_equal(got, np.concatenate(parts))


@pytest.mark.parametrize("shape", bm.BATCH_SHAPES, ids=lambda s: f"c{s[3]}")
@pytest.mark.parametrize("d", bm.BATCH_D)
def test_batch_and_repeat(dev, shape, d):
    """an image's bytes do not depend on its place in a batch, and a call repeats"""
    params = (d, 75.0, 75.0)
    img, pre = bm.case("saltpepper", shape, params)
    got = _run(img, *params)
    _hold(got, pre, (shape, params))
    np.testing.assert_array_equal(_run(img, *params), got)
    for i in range(shape[0]):
        np.testing.assert_array_equal(_run(img[i:i + 1], *params), got[i:i + 1])


def _run_padded(img, params, pad):
    """the C ABI on rows of exactly w*c + pad bytes: an odd stride starts every other row at an
    odd address"""
    import torch
    from idn import _lib
    lib = _lib.load()
    n, h, w, c = img.shape
    rs = w * c + pad
    buf = torch.zeros((n, h, rs), dtype=torch.uint8, device="cuda")
    buf[:, :, : w * c] = torch.tensor(img.reshape(n, h, w * c)).cuda()
    out = torch.full_like(buf, 77)
    rc = lib.idn_bilateral_u8(buf.data_ptr(), out.data_ptr(), n, h, w, c, rs, *params, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out[:, :, w * c:] == 77).all())  # padding untouched
    return out[:, :, : w * c].cpu().numpy().reshape(n, h, w, c)


@pytest.mark.parametrize("pad", bm.PADS)
@pytest.mark.parametrize("c,d", bm.PAD_CASES)
def test_row_padding(dev, c, d, pad):
    """row_stride > w*c, odd strides included (the two-column kernel's byte stores instead of
    its u16 stores): the compact call's bytes, and nothing written between the rows"""
    params = (d, 200.0, 100.0)
    img, pre = bm.case("bytes", bm.PAD_SHAPE + (c,), params)
    want = _run(img, *params)
    _hold(want, pre, (c, params))
    np.testing.assert_array_equal(_run_padded(img, params, pad), want)


@pytest.mark.parametrize("d", bm.TUNING_D)
def test_tuning_forms(dev, monkeypatch, d):
    """tuning build, radius 1..5.  IDN_BL2_SYM=0 (every tap looked up, IEEE division) gives the
    product's bytes: each output's fp32 sum keeps its order.  IDN_BL2=0, the one-column kernel,
    sums in another order and is held to the rule against the model (measured on the MI355X: its
    bytes were equal to the product's too, on all 30 cases)"""
    from idn import _lib
    equal = []
    for params in bm.tuning_params(d):
        for family in bm.FAMILIES:
            img, pre = bm.case(family, bm.SEAM_SHAPES[0], params)
            want = _run(img, *params)
            with monkeypatch.context() as m:
                m.setenv("IDN_BL2_SYM", "0")
                with _lib.variant("tuning"):
                    np.testing.assert_array_equal(_run(img, *params), want)
            with monkeypatch.context() as m:
                m.setenv("IDN_BL2", "0")
                with _lib.variant("tuning"):
                    one = _run(img, *params)
            _hold(one, pre, ("one-column", family, params))
            equal.append(bool(np.array_equal(one, want)))
    print(f"one-column bytes equal to the product's: {sum(equal)} of {len(equal)} cases")


def test_errors_leave_out_untouched(dev):
    """radius 9 (d = 19, or d = 0 with sigma_space 6) is unsupported, C = 2 and 4 are invalid:
    IdnError, and nothing is written"""
    import torch
    import idn
    from idn._lib import IdnError
    assert bm.radius_of(19, 1.0) == 9 and bm.radius_of(0, 6.0) == 9
    for c, params, word in ((3, (19, 60.0, 3.0), "radius"), (1, (19, 60.0, 3.0), "radius"),
                            (3, (0, 60.0, 6.0), "radius"), (2, (9, 60.0, 3.0), "channels"),
                            (4, (9, 60.0, 3.0), "channels")):
        x = torch.from_numpy(bm.make_input("bytes", (2, 9, 12, c), 5)).cuda()
        out = torch.full_like(x, 77)
        with pytest.raises(IdnError, match=word):
            idn.bilateral_filter(x, *params, out=out)
        torch.cuda.synchronize()
        assert bool((out == 77).all())


@pytest.mark.parametrize("c", [3, 1])
def test_empty_batch(dev, c):
    """n = 0: an empty result, no error (torch gives an empty tensor a null data pointer)"""
    import torch
    import idn
    y = idn.bilateral_filter(torch.empty((0, 5, 7, c), dtype=torch.uint8, device="cuda"), 9, 20.0, 100.0)
    assert tuple(y.shape) == (0, 5, 7, c) and y.dtype == torch.uint8
