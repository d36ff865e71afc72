"""CPU: the host models of the quality metrics agree with each other, and the C-ABI entry points
and the Python wrappers reject bad arguments before any device work (no GPU here).

The exact-integer form (metrics_model.ssim_int / mse_int) is what the kernels are held to on the
GPU (tests/test_metrics_gpu.py); the scipy restatement of skimage 0.14.2's float code pins it to
skimage.  Their measured difference is <= 2.3e-14 over the cases below; 1e-12 leaves room for
scipy's summation order and nothing more."""
import ctypes

import numpy as np
import pytest

import metrics_model as mm


def _lib():
    from idn import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


@pytest.mark.parametrize("family", mm.FAMILIES)
@pytest.mark.parametrize("shape,c,win", mm.CASES,
                         ids=["%dx%dx%d-c%d-w%d" % (*s, c, w) for s, c, w in mm.CASES])
def test_integer_form_matches_skimage_restatement(shape, c, win, family):
    X, Y = mm.make_pair(family, shape, c)
    for x, y in zip(X, Y):
        si, si_ch = mm.ssim_int(x, y, win)
        sf, sf_ch = mm.compare_ssim(x, y, win)
        print(f"ssim int {si!r} float {sf!r} diff {abs(si - sf):.3g}")
        assert abs(si - sf) <= 1e-12
        assert np.max(np.abs(si_ch - sf_ch)) <= 1e-12
        assert mm.mse_int(x, y) == mm.compare_mse(x, y)
        pi, pf = mm.psnr_of_mse(mm.mse_int(x, y)), mm.compare_psnr(x, y)
        assert pi == pf  # same mse bits, same expression (+inf == +inf for identical images)


def test_model_special_values():
    x = mm.make_pair("same", (1, 37, 53), 3)[0][0]
    assert mm.ssim_int(x, x, 7)[0] == 1.0
    assert np.isposinf(mm.psnr_of_mse(mm.mse_int(x, x)))
    X, Y = mm.make_pair("black_white", (1, 37, 53), 3)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    assert abs(mm.ssim_int(X[0], Y[0], 7)[0] - C1 * C2 / ((255.0 ** 2 + C1) * C2)) <= 1e-15
    assert mm.psnr_of_mse(mm.mse_int(X[0], Y[0])) == 0.0
    inv = mm.make_pair("inverted", (1, 64, 96), 3)
    assert mm.ssim_int(inv[0][0], inv[1][0], 7)[0] < -0.5  # negative covariance
    with pytest.raises(ValueError):
        mm.ssim_int(x[:5], x[:5], 7)
    with pytest.raises(ValueError):
        mm.compare_ssim(x[:5], x[:5], 7)


def test_argument_validation_without_gpu():
    """idn_mse_u8 / idn_ssim_u8 reject bad arguments on the host before any HIP call: -1
    (IDN_EINVAL) and a message; idn_metrics_workspace_size, which returns a size, gives 0 for a
    shape neither accepts"""
    lib = _lib()
    A, B, O, WS = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: validation fails first
    n, h, w, c = 1, 16, 16, 3

    def mse(a=A, b=B, o=O, c=c, sa=w * c, sb=w * c):
        return lib.idn_mse_u8(a, b, o, n, h, w, c, sa, sb, WS, 1 << 20, None)

    def ssim(a=A, b=B, o=O, c=c, sa=w * c, sb=w * c, win=7, h=h, w=w):
        return lib.idn_ssim_u8(a, b, o, None, None, n, h, w, c, sa, sb, win, WS, 1 << 20, None)

    for bad in (dict(a=None), dict(b=None), dict(o=None)):
        assert mse(**bad) == -1 and b"null" in lib.idn_last_error()
        assert ssim(**bad) == -1 and b"null" in lib.idn_last_error()
    for bad in (dict(sa=w * c - 1), dict(sb=w * c - 1)):
        assert mse(**bad) == -1 and b"row_stride" in lib.idn_last_error()
        assert ssim(**bad) == -1 and b"row_stride" in lib.idn_last_error()
    for cc in (2, 4, 0):
        assert mse(c=cc, sa=64, sb=64) == -1 and b"channels" in lib.idn_last_error()
        assert ssim(c=cc, sa=64, sb=64) == -1 and b"channels" in lib.idn_last_error()
        assert lib.idn_metrics_workspace_size(n, h, w, cc, 7) == 0
    for win in (4, 8, 1, 13, 0, -3):
        assert ssim(win=win) == -1 and b"win_size" in lib.idn_last_error()
    assert ssim(win=11, h=10, sa=64, sb=64) == -1 and b"exceeds" in lib.idn_last_error()
    assert ssim(win=11, w=10, sa=64, sb=64) == -1 and b"exceeds" in lib.idn_last_error()
    # a workspace that is missing or too small: IDN_EWORKSPACE (-4), still before any HIP call
    assert lib.idn_mse_u8(A, B, O, n, h, w, c, w * c, w * c, None, 0, None) == -4
    assert lib.idn_ssim_u8(A, B, O, None, None, n, h, w, c, w * c, w * c, 7, WS, 8, None) == -4
    assert b"workspace" in lib.idn_last_error()


def test_workspace_size():
    lib = _lib()
    for (h, w, c, win) in [(7, 7, 3, 7), (37, 53, 1, 3), (600, 1000, 3, 7), (600, 1000, 3, 11),
                           (600, 1000, 3, 0), (5, 5, 3, 7)]:
        sizes = [lib.idn_metrics_workspace_size(n, h, w, c, win) for n in (1, 2, 3, 16, 256)]
        assert sizes[0] > 0
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.idn_metrics_workspace_size(0, 16, 16, 3, 7) == 0
    assert lib.idn_metrics_workspace_size(1, 0, 16, 3, 7) == 0


def test_wrapper_rejects_before_touching_the_device():
    """dtype, shape and window errors come first, so they are raised for CPU tensors too"""
    import torch
    import idn
    x = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    for fn in (idn.mse, idn.psnr, idn.ssim):
        with pytest.raises(TypeError, match="uint8"):
            fn(x.float(), x)
        with pytest.raises(TypeError, match="uint8"):
            fn(x, x.double())
        with pytest.raises(TypeError, match="Tensor"):
            fn(x.numpy(), x)
        with pytest.raises(ValueError, match="shape mismatch"):
            fn(x, x[:, :8])
        with pytest.raises(ValueError, match="shape mismatch"):
            fn(x, x[0])
        with pytest.raises(ValueError, match="channels"):
            fn(x[..., :2], x[..., :2])
        with pytest.raises(ValueError, match="expected"):
            fn(x[0, 0], x[0, 0])
    for win in (4, 13, 1, 7.5):
        with pytest.raises(ValueError, match="win_size"):
            idn.ssim(x, x, win)
    with pytest.raises(ValueError, match="exceeds"):
        idn.ssim(x[:, :9], x[:, :9], 11)
    with pytest.raises(ValueError, match="GPU only"):  # valid arguments: the device check is last
        idn.ssim(x, x, 7)
    assert idn.ops.ssim is idn.ssim and idn.ops.mse is idn.mse and idn.ops.psnr is idn.psnr
