"""GPU: idn.mse / idn.psnr / idn.ssim against the exact-integer host model
(tests/metrics_model.py), which tests/test_metrics.py pins to skimage 0.14.2's float code.

Bounds.  mse: the sum is an integer below 2^53 and is divided once, so it is bit-equal to the
model.  psnr: <= ~100 dB and a few ulp of log10, 1e-12 absolute.  ssim: |S| <= 1 and at most
1.8e6 terms per image; even a serial float64 sum errs by at most 1.8e6 * 1.1e-16 ~ 2e-10, and the
per-window arithmetic is the model's own (two products and a division on exact integers), so 1e-9
absolute."""
import functools

import numpy as np
import pytest

import metrics_model as mm

pytestmark = pytest.mark.gpu

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
BLACK_WHITE_SSIM = C1 * C2 / ((255.0 ** 2 + C1) * C2)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(family, shape, c, win):
    """inputs and the model's values of one case, computed once and shared (treated read-only)"""
    X, Y = mm.make_pair(family, shape, c)
    ref = [mm.ssim_int(x, y, win) for x, y in zip(X, Y)]
    ssim = np.array([r[0] for r in ref])
    ssim_ch = np.stack([r[1] for r in ref])
    mse = np.array([mm.mse_int(x, y) for x, y in zip(X, Y)])
    return X, Y, ssim, ssim_ch, mse, mm.psnr_of_mse(mse)


@pytest.mark.parametrize("family", mm.FAMILIES)
@pytest.mark.parametrize("shape,c,win", mm.CASES,
                         ids=["%dx%dx%d-c%d-w%d" % (*s, c, w) for s, c, w in mm.CASES])
def test_metrics_match_host_model(dev, shape, c, win, family):
    import idn
    X, Y, ssim_ref, ch_ref, mse_ref, psnr_ref = _case(family, shape, c, win)
    x, y = _t(X), _t(Y)
    n = shape[0]

    mse = _np(idn.mse(x, y))
    psnr = _np(idn.psnr(x, y))
    ssim = _np(idn.ssim(x, y, win))
    ch, mse2 = idn.ssim(x, y, win, per_channel=True, return_mse=True)
    ch, mse2 = _np(ch), _np(mse2)
    assert mse.dtype == psnr.dtype == ssim.dtype == ch.dtype == np.float64
    assert mse.shape == psnr.shape == ssim.shape == (n,) and ch.shape == (n, c)
    print(f"ssim {ssim!r} ref {ssim_ref!r} maxdiff {np.max(np.abs(ssim - ssim_ref)):.3g} "
          f"ch maxdiff {np.max(np.abs(ch - ch_ref)):.3g} mse {mse!r} psnr {psnr!r}")

    assert np.array_equal(mse, mse_ref)
    assert np.array_equal(mse2, mse)                      # same bits from the ssim pass
    finite = np.isfinite(psnr_ref)
    assert np.array_equal(np.isposinf(psnr), ~finite)     # identical images: +inf
    assert np.all(np.abs(psnr[finite] - psnr_ref[finite]) <= 1e-12)
    assert np.all(np.abs(ssim - ssim_ref) <= 1e-9)
    assert np.all(np.abs(ch - ch_ref) <= 1e-9)
    if family == "same":
        assert np.all(ssim == 1.0) and np.all(ch == 1.0) and np.all(mse == 0.0)
        assert np.all(np.isposinf(psnr))
    if family == "black_white":
        assert np.all(psnr == 0.0)
        assert np.all(np.abs(ssim - BLACK_WHITE_SSIM) <= 1e-15)
    if family == "inverted":
        assert np.all(ssim < 0)                           # negative covariance keeps its sign

    # a second call gives the same bits
    assert np.array_equal(_np(idn.ssim(x, y, win)), ssim)
    ch3 = _np(idn.ssim(x, y, win, per_channel=True))
    assert np.array_equal(ch3, ch)
    assert np.array_equal(_np(idn.mse(x, y)), mse)


@pytest.mark.parametrize("family", ["noisy", "random"])
def test_batch_image_equals_the_pair_alone(dev, family):
    import idn
    X, Y = _case(family, (3, 64, 96), 3, 7)[:2]
    x, y = _t(X), _t(Y)
    ssim, mse = idn.ssim(x, y, return_mse=True)
    ch = _np(idn.ssim(x, y, per_channel=True))
    psnr = _np(idn.psnr(x, y))
    ssim, mse = _np(ssim), _np(mse)
    assert len(set(ssim.tolist())) == 3                   # different seeds: an index mix-up shows
    for i in range(3):
        s1, m1 = idn.ssim(x[i], y[i], return_mse=True)    # (H, W, C): 0-d results
        assert s1.shape == () and m1.shape == ()
        assert _np(s1) == ssim[i] and _np(m1) == mse[i]
        assert np.array_equal(_np(idn.ssim(x[i], y[i], per_channel=True)), ch[i])
        assert _np(idn.mse(x[i], y[i])) == mse[i]
        assert _np(idn.psnr(x[i:i + 1], y[i:i + 1]))[0] == psnr[i]


@pytest.mark.parametrize("shape,c,win", [((2, 37, 53), 3, 7), ((2, 17, 344), 3, 11),
                                         ((2, 37, 53), 1, 3)])
def test_row_strides_at_the_c_abi(dev, shape, c, win):
    """row_stride_a = w*c + 13, row_stride_b = w*c + 5, padding 0xFF: the same bits as the
    contiguous call (a read into the padding would change them)"""
    import torch
    from idn import _lib
    lib = _lib.load()
    X, Y = _case("noisy", shape, c, win)[:2]
    n, h, w = shape
    wc = w * c

    def padded(A, stride):
        buf = np.full((n, h, stride), 0xFF, np.uint8)
        buf[:, :, :wc] = A.reshape(n, h, wc)
        return _t(buf)

    sa, sb = wc + 13, wc + 5
    nbytes = lib.idn_metrics_workspace_size(n, h, w, c, win)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    for tag, (a, b, ra, rb) in {"dense": (_t(X), _t(Y), wc, wc),
                                "strided": (padded(X, sa), padded(Y, sb), sa, sb)}.items():
        out = torch.full((3, n), -7.0, dtype=torch.float64, device="cuda")
        ch = torch.full((n, c), -7.0, dtype=torch.float64, device="cuda")
        rc = lib.idn_mse_u8(a.data_ptr(), b.data_ptr(), out[0].data_ptr(), n, h, w, c, ra, rb,
                            ws.data_ptr(), nbytes, stream)
        _lib.check(rc, "idn_mse_u8")
        rc = lib.idn_ssim_u8(a.data_ptr(), b.data_ptr(), out[1].data_ptr(), ch.data_ptr(),
                             out[2].data_ptr(), n, h, w, c, ra, rb, win, ws.data_ptr(), nbytes,
                             stream)
        _lib.check(rc, "idn_ssim_u8")
        res[tag] = (_np(out), _np(ch))
    assert np.array_equal(res["dense"][0], res["strided"][0])
    assert np.array_equal(res["dense"][1], res["strided"][1])
    _, _, ssim_ref, ch_ref, mse_ref, _ = _case("noisy", shape, c, win)
    out, ch = res["strided"]
    assert np.array_equal(out[0], mse_ref) and np.array_equal(out[2], mse_ref)
    assert np.all(np.abs(out[1] - ssim_ref) <= 1e-9) and np.all(np.abs(ch - ch_ref) <= 1e-9)


def test_scoring_a_denoiser_end_to_end(dev):
    """idn.ssim(clean, denoised) and idn.ssim(clean, noisy) on device tensors the bank produced
    match the host model on the downloaded bytes (no claim about which is larger)"""
    import idn
    from conftest import textured
    clean = _t(textured(2, 64, 96, seed=41))
    noisy = idn.random_noise(clean, "gaussian", var=0.01, seed=5)
    den = idn.gaussian_blur(noisy, 5)
    c_np, n_np, d_np = _np(clean), _np(noisy), _np(den)
    for other, o_np in ((den, d_np), (noisy, n_np)):
        got = _np(idn.ssim(clean, other))
        ref = np.array([mm.ssim_int(a, b, 7)[0] for a, b in zip(c_np, o_np)])
        assert np.all(np.abs(got - ref) <= 1e-9)
        mse_ref = np.array([mm.mse_int(a, b) for a, b in zip(c_np, o_np)])
        assert np.array_equal(_np(idn.mse(clean, other)), mse_ref)
        assert np.all(np.abs(_np(idn.psnr(clean, other)) - mm.psnr_of_mse(mse_ref)) <= 1e-12)


def test_gpu_argument_errors(dev):
    import idn
    x = _t(np.zeros((1, 16, 16, 3), np.uint8))
    with pytest.raises(ValueError):
        idn.ssim(x, x.cpu())
    with pytest.raises(ValueError):
        idn.ssim(x, x, 8)
    with pytest.raises(TypeError):
        idn.mse(x, x.float())
