"""CPU: tests/blur_model.py, the definition of idn.blur and idn.gaussian_blur at every odd window
3..31, against the oracle (cv2's 3 and 5 Gaussians, cv2.blur at every window) and against an
independent scipy formulation; the Q8 taps, literally and through idn_gaussian_taps; the argument
checks of the C entries, which need no GPU; and the quality the wider windows buy."""
import ctypes
import functools
from pathlib import Path

import numpy as np
import pytest

import blur_model as bm
import wiener_model as wm
from blur_cases import (BOX7_OVER_3, GAUSS9_OVER_3, GAUSS9_OVER_5, KS, SHAPES, SID, TAPS,
                        device_noisy, quality_figures)


@functools.lru_cache(maxsize=None)
def image(shape, seed=0):
    x = np.random.default_rng(seed + 11 * shape[1]).integers(0, 256, shape, dtype=np.uint8)
    x.setflags(write=False)
    return x


def scipy_box(x, k):
    from scipy.ndimage import correlate1d
    a = x.astype(np.int64)
    one = np.ones(k, np.int64)
    s = correlate1d(correlate1d(a, one, axis=0, mode="mirror"), one, axis=1, mode="mirror")
    return ((2 * s + k * k) // (2 * k * k)).astype(np.uint8)


def scipy_gauss(x, taps):
    from scipy.ndimage import correlate1d
    a = x.astype(np.int64)
    t = np.asarray(taps, np.int64)
    s = correlate1d(correlate1d(a, t, axis=0, mode="mirror"), t, axis=1, mode="mirror")
    return ((s + 32768) >> 16).astype(np.uint8)


# ---- the model against the oracle and scipy ---------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_gaussian_model_is_the_oracle_at_3_and_5(shape):
    import oracle.cv
    x = image(shape)
    for k in (3, 5):
        assert np.array_equal(bm.gaussian_blur(x, k), oracle.cv.gaussian_blur(x, k)), k


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_box_model_is_the_oracle_at_every_window(shape):
    import oracle.cv
    x = image(shape)
    for k in KS:
        assert np.array_equal(bm.blur(x, k), oracle.cv.blur(x, k)), k


def test_box_model_does_not_call_the_oracle():
    """an integral image of its own: the module names neither the oracle nor scipy"""
    src = Path(bm.__file__).read_text()
    assert "import oracle" not in src and "from oracle" not in src and "scipy" not in src
    assert "cumsum" in src
    # and the integral image is the plain window sum
    x = image((9, 11, 1))[..., 0]
    e = bm.pad101(x, 2).astype(np.int64)
    want = sum(e[i:i + 9, j:j + 11] for i in range(5) for j in range(5))
    assert np.array_equal(bm.box_sum(x, 5), want)


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_both_models_equal_scipy_mirror(shape):
    x = image(shape)
    for k in KS:
        assert np.array_equal(bm.blur(x, k), np.stack(
            [scipy_box(x[..., ch], k) for ch in range(shape[2])], axis=-1)), k
    for k, sigma in [(k, 0.0) for k in KS] + [ks for ks in TAPS if ks[1] > 0]:
        t = bm.gaussian_taps(k, sigma)
        assert np.array_equal(bm.gaussian_blur(x, k, sigma), np.stack(
            [scipy_gauss(x[..., ch], t) for ch in range(shape[2])], axis=-1)), (k, sigma)


def test_reflection_repeats():
    assert bm.reflect101(np.arange(-7, 10), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1,
                                                             2, 1, 0, 1]
    assert bm.reflect101(np.arange(-3, 4), 1).tolist() == [0] * 7
    assert bm.reflect101(np.arange(-2, 4), 2).tolist() == [0, 1, 0, 1, 0, 1]


# ---- taps ----------------------------------------------------------------------------------------

def test_taps_sum_to_256_and_are_symmetric():
    for k in KS:
        for sigma in (0.0, 0.1, 0.3, 0.8, 1.0, 2.5, 12.0, 100.0):
            t = bm.gaussian_taps(k, sigma).astype(np.int64)
            assert t.sum() == 256 and t.size == k and np.array_equal(t, t[::-1]), (k, sigma)
            assert t.min() >= 0 and t.max() <= 256


@pytest.mark.parametrize("ks", sorted(TAPS), ids=str)
def test_literal_taps(ks):
    assert bm.gaussian_taps(*ks).tolist() == TAPS[ks]


def test_zero_outer_taps_at_29_and_31():
    for k in (29, 31):
        t = bm.gaussian_taps(k, 0.0)
        assert (t == 0).sum() == 4 and t[0] == t[1] == 0 and t[2] > 0


def test_chosen_taps_are_far_from_a_tie():
    """the precondition of comparing libm's exp with numpy's: every 256 v[i] of the cases checked
    through the C entry lies at least 1e-6 from k + 1/2 (the sigma-0 kernels at least 0.006)"""
    for ks in [(k, 0.0) for k in KS] + sorted(TAPS):
        v = bm.gaussian_weights(*ks)
        if v is None:
            continue
        d = np.abs(v - np.floor(v) - 0.5).min()
        assert d >= (0.006 if ks[1] == 0.0 else 1e-6), (ks, d)


def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_c_taps_equal_the_model():
    lib = _lib()
    for ks in [(k, 0.0) for k in KS] + sorted(TAPS):
        buf = (ctypes.c_uint16 * 32)(*([0xFFFF] * 32))
        assert lib.idn_gaussian_taps(ks[0], ks[1], ctypes.addressof(buf)) == 0, ks
        assert list(buf[:ks[0]]) == bm.gaussian_taps(*ks).tolist(), ks
        assert list(buf[ks[0]:]) == [0xFFFF] * (32 - ks[0]), ks
    import idn
    assert idn.ops.BLUR_MAX_KSIZE == 31 == bm.MAX_KSIZE
    t = idn.ops.gaussian_taps(15, 2.5)
    assert t.dtype == np.uint16 and t.tolist() == TAPS[(15, 2.5)]
    assert idn.ops.gaussian_taps(7).tolist() == TAPS[(7, 0.0)]


# ---- argument checks, before any HIP call ------------------------------------------------------------

def test_bad_ksize_and_sigma_are_refused_on_the_host():
    """fake pointers, never dereferenced: a refusal is -1 (IDN_EINVAL) or -2 (IDN_EUNSUPPORTED)
    with a message that names the entry"""
    lib = _lib()
    from idn import _lib as binding
    A, B = 0x10000, 0x20000
    buf = (ctypes.c_uint16 * 32)()
    T = ctypes.addressof(buf)
    shape = (1, 8, 8, 3, 24)
    for k in (1, 4, 33, 0, -3, 32):
        assert lib.idn_gaussian_blur_u8(A, B, *shape, k, None) == -2, k
        assert b"idn_gaussian_blur_u8" in lib.idn_last_error() and b"ksize" in lib.idn_last_error()
        assert lib.idn_gaussian_blur_sigma_u8(A, B, *shape, k, 1.0, None) == -2, k
        assert b"idn_gaussian_blur_sigma_u8" in lib.idn_last_error()
        assert lib.idn_box_blur_u8(A, B, *shape, k, None) == -2, k
        assert b"idn_box_blur_u8" in lib.idn_last_error() and b"ksize" in lib.idn_last_error()
        assert lib.idn_gaussian_taps(k, 0.0, T) == -2, k
        assert b"idn_gaussian_taps" in lib.idn_last_error()
    for sigma in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert lib.idn_gaussian_blur_sigma_u8(A, B, *shape, 9, sigma, None) == -1, sigma
        assert b"sigma" in lib.idn_last_error()
        assert lib.idn_gaussian_taps(9, sigma, T) == -1, sigma
        assert b"sigma" in lib.idn_last_error()
    assert lib.idn_gaussian_taps(9, 1.0, None) == -1 and b"null" in lib.idn_last_error()
    # the shared checks still come first, and an empty batch is a no-op at a legal window
    assert lib.idn_gaussian_blur_sigma_u8(None, B, *shape, 9, 1.0, None) == -1
    assert lib.idn_box_blur_u8(A, A, *shape, 7, None) == -1
    assert lib.idn_gaussian_blur_sigma_u8(A, B, 1, 8, 8, 3, 23, 9, 1.0, None) == -1
    assert lib.idn_gaussian_blur_sigma_u8(A, B, 0, 8, 8, 3, 24, 31, 2.0, None) == 0
    assert lib.idn_gaussian_blur_u8(A, B, 0, 8, 8, 3, 24, 9, None) == 0
    assert lib.idn_box_blur_u8(A, B, 0, 8, 8, 3, 24, 31, None) == 0
    with pytest.raises(binding.IdnError):
        import idn
        idn.ops.gaussian_taps(4)
    with pytest.raises(binding.IdnError):
        idn.ops.gaussian_taps(9, float("nan"))
    m = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    assert lib.idn_gaussian_blob_f32(A, B, 1, 8, 8, 3, 24, 7, m, None) == -2   # composed by the caller
    assert lib.idn_gaussian_blob_f32(A, B, 1, 8, 8, 3, 24, 4, m, None) == -1


# ---- constant images ---------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [0, 1, 77, 254, 255])
def test_constant_images_come_back_unchanged(value):
    x = np.full((5, 9, 2), value, np.uint8)
    for k in KS:
        assert np.array_equal(bm.blur(x, k), x), k
        assert np.array_equal(bm.gaussian_blur(x, k), x), k
    for ks in TAPS:
        assert np.array_equal(bm.gaussian_blur(x, *ks), x), ks


def test_identity_kernel():
    x = image((13, 17, 3))
    assert np.array_equal(bm.gaussian_blur(x, 3, 0.1), x)


# ---- quality -----------------------------------------------------------------------------------------

def test_quality_thresholds_hold_for_the_model():
    """numpy noise (wiener_model.noisy_image, sd 40): the issue's +1.4, +3.4 and +2.0 dB; and the
    device's own draw, from the host model of its stream"""
    clean = wm.smooth_image()
    c3 = np.repeat(clean[..., None], 3, axis=2)
    for name, noisy in [("numpy", wm.noisy_image(clean, 40.0, 0)), ("device", device_noisy(c3))]:
        g, b = quality_figures(c3, noisy)
        print(f"{name}: noisy {wm.psnr(c3, noisy):.2f} gauss 3/5/9 {g[3]:.2f} {g[5]:.2f} "
              f"{g[9]:.2f} box 3/7 {b[3]:.2f} {b[7]:.2f}")
        assert g[9] >= g[5] + GAUSS9_OVER_5, name
        assert g[9] >= g[3] + GAUSS9_OVER_3, name
        assert b[7] >= b[3] + BOX7_OVER_3, name
