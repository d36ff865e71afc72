"""CPU: the definition of adaptive_median (tests/adaptive_median_model.py) pinned to scipy, the
counting form of stage A that the kernel uses proven equal to it, the model's properties and
quality, and the host-side range checks of idn_adaptive_median_u8."""
import re
from pathlib import Path

import numpy as np
import pytest

import adaptive_median_model as model
import adaptive_median_scipy
from conftest import textured

ROOT = Path(__file__).resolve().parent.parent
# ORACLE_SHAPES of tests/test_median_large.py
ORACLE_SHAPES = [(2, 5, 7, 3), (1, 9, 1, 3), (1, 1, 40, 3), (2, 23, 64, 3), (1, 37, 53, 1),
                 (1, 20, 70, 4), (1, 40, 129, 3)]


def _pepper_heavy(shape, seed):
    """half the samples 0, 3 % of them 255: stage A fails up to the largest windows"""
    n, h, w, c = shape
    img = textured(n, h, w, c=c, seed=seed)
    m = np.random.RandomState(seed).random_sample(img.shape)
    img[m < 0.5] = 0
    img[m > 0.97] = 255
    return img


def _sap(img, amount, seed):
    """numpy s&p as in tests/test_median_large.py: half salt, half pepper"""
    out = img.copy()
    m = np.random.RandomState(seed).random_sample(img.shape)
    out[m < amount / 2] = 0
    out[(m >= amount / 2) & (m < amount)] = 255
    return out


@pytest.mark.parametrize("K", [3, 7, 15, 31])
def test_model_equals_scipy(K):
    for shape in ORACLE_SHAPES:
        for img in (_pepper_heavy(shape, K + sum(shape)),
                    _sap(textured(*shape[:3], c=shape[3], seed=K), 0.6, K + 1)):
            out, ks = model.adaptive_median(img, K)
            ref, rks = adaptive_median_scipy.adaptive_median(img, K)
            assert out.dtype == np.uint8 and ks.dtype == np.uint8 and out.shape == img.shape
            assert np.array_equal(out, ref), (K, shape, np.argwhere(out != ref)[:6])
            assert np.array_equal(ks, rks), (K, shape, np.argwhere(ks != rks)[:6])


def test_counting_form_of_stage_a():
    """mn < md < mx  <=>  mn != mx and count(== mn) <= (n-1)/2 and count(== mx) <= (n-1)/2, with
    n = k*k, at every level and sample; and where it fails the median is mn exactly when
    mn == mx or count(== mn) > (n-1)/2 (the kernel's fall-through), else mx"""
    seen = {True: 0, False: 0}
    for shape in ORACLE_SHAPES:
        for img in (_pepper_heavy(shape, sum(shape)),
                    _sap(textured(*shape[:3], c=shape[3], seed=5), 0.9, 6),
                    255 - _pepper_heavy(shape, 1 + sum(shape))):
            plane = img[0, :, :, 0]
            for k in range(3, 32, 2):
                mn, md, mx, s = model.levels(plane, k)
                half = (k * k - 1) // 2
                cmn = (s == mn[..., None]).sum(-1)
                cmx = (s == mx[..., None]).sum(-1)
                direct = (mn < md) & (md < mx)
                counted = (mn != mx) & (cmn <= half) & (cmx <= half)
                assert np.array_equal(direct, counted), (shape, k)
                fell = np.where((mn == mx) | (cmn > half), mn, mx)
                assert np.array_equal(fell[~direct], md[~direct]), (shape, k)
                seen[True] += int(direct.sum())
                seen[False] += int((~direct).sum())
    assert seen[True] > 1000 and seen[False] > 1000, seen


def test_constant_image_comes_back():
    for v in (0, 128, 255):
        img = np.full((1, 9, 11, 3), v, np.uint8)
        out, ks = model.adaptive_median(img, 7)
        assert np.array_equal(out, img) and not ks.any()


def test_lone_impulse_in_a_ramp():
    y, x = np.mgrid[0:20, 0:24]
    ramp = (10 + 3 * x + 4 * y).astype(np.uint8)[None, :, :, None]
    img = ramp.copy()
    img[0, 9, 11, 0] = 255
    out, ks = model.adaptive_median(img, 15)
    assert out[0, 9, 11, 0] == np.median(img[0, 8:11, 10:13, 0]) and ks[0, 9, 11, 0] == 3
    assert abs(int(out[0, 9, 11, 0]) - int(ramp[0, 9, 11, 0])) <= 3  # the next sample of the ramp
    out[0, 9, 11, 0] = ramp[0, 9, 11, 0]
    assert np.array_equal(out[0, 1:-1, 1:-1, 0], ramp[0, 1:-1, 1:-1, 0])
    assert (ks[0, 1:-1, 1:-1, 0] == 3).all()


@pytest.mark.parametrize("shape", [(1, 1, 40, 3), (1, 9, 1, 3), (1, 1, 1, 1)])
def test_single_row_and_column(shape):
    img = _pepper_heavy(shape, 3)
    out, ks = model.adaptive_median(img, 31)
    ref, rks = adaptive_median_scipy.adaptive_median(img, 31)
    assert np.array_equal(out, ref) and np.array_equal(ks, rks)


def test_squeezed_input_and_bad_ksize():
    img = _pepper_heavy((1, 12, 9, 3), 4)
    out, ks = model.adaptive_median(img[0], 9)
    ref, rks = model.adaptive_median(img, 9)
    assert np.array_equal(out, ref[0]) and np.array_equal(ks, rks[0])
    for k in (1, 8, 33, -7):
        with pytest.raises(ValueError):
            model.adaptive_median(img, k)


def _quality_clean():
    y, x = np.mgrid[0:96, 0:128]
    img = np.stack([40 + x, 60 + y, 200 - (x + y) // 2], axis=-1).astype(np.int64)
    img[20:60, 30:90] += 50
    img[70:90, 10:40, 0] -= 30
    return np.clip(img, 0, 255).astype(np.uint8)


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("amount", [0.2, 0.4, 0.6])
def test_quality_beats_the_best_fixed_window(amount):
    """numpy s&p, seed 0, on the smooth 96 x 128 x 3 image: max_ksize = 15 beats the best of the
    fixed medians 3, 5, 7, 9, 11, 15 by at least 2 dB (measured: 3.0, 3.3 and 4.8 dB)"""
    import scipy.ndimage as ndi
    clean = _quality_clean()
    noisy = _sap(clean, amount, 0)
    fixed = {k: _psnr(clean, ndi.median_filter(noisy, size=(k, k, 1), mode="nearest"))
             for k in (3, 5, 7, 9, 11, 15)}
    out, _ = model.adaptive_median(noisy, 15)
    got = _psnr(clean, out)
    print("amount", amount, "adaptive", round(got, 2), "fixed", {k: round(v, 2) for k, v in fixed.items()})
    assert got >= max(fixed.values()) + 2.0, (got, fixed)


# ---- host-side checks of the C entry and the binding --------------------------------------------

def test_max_ksize_constant():
    from idn import ops
    assert ops.ADAPTIVE_MEDIAN_MAX_KSIZE == 31


def test_exported_beside_median_blur():
    import idn
    assert idn.adaptive_median is idn.ops.adaptive_median


def test_symbol_is_bound():
    from idn import _lib
    assert "idn_adaptive_median_u8" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["idn_adaptive_median_u8"][1]) == 10
    assert hasattr(_lib.load(required=True), "idn_adaptive_median_u8")


def test_header_comment_names_the_range_and_the_fall_through():
    text = (ROOT / "include" / "idn.h").read_text()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int idn_adaptive_median_u8\(", text, flags=re.S)
    assert m, "idn_adaptive_median_u8 has no comment"
    body = m.group(1)
    assert re.search(r"\b31\b", body), body
    assert "fall-through" in body and re.search(r"no k passed", body), body
    assert re.search(r"#define IDN_ABI_VERSION 11\b", text)


@pytest.mark.parametrize("k", [33, 8, 1, -7])
def test_rejected_on_the_host(k):
    """dummy non-null pointers, never dereferenced: IDN_EUNSUPPORTED (-2) before any launch"""
    from idn import _lib
    lib = _lib.load()
    for kmap in (3, None):
        rc = lib.idn_adaptive_median_u8(1, 2, kmap, 1, 8, 8, 3, 24, k, None)
        assert rc == -2
        msg = lib.idn_last_error().decode()
        assert "supported" in msg and "3..31" in msg, msg
