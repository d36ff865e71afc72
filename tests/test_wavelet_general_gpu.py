"""GPU: idn.denoise_wavelet's options against their definition, tests/wavelet_general_model.py.

Tolerance: the project's contract for the wavelet denoiser (tests/test_wavelet_gpu.py) --
|X' - model| <= 1e-5 before the U8 cast, and U8 outputs one LSB apart only where 255 X' lies
within 255e-5 of an integer.  The cases, with the conditions that make them test their options
(tests/test_wavelet_general.py asserts those from the model), are tests/wavelet_general_cases.py's.
"""
import numpy as np
import pytest

import wavelet_general_cases as wc
import wavelet_general_model as wm
from carve import carve, carve_out, untouched
from test_wavelet_gpu import TOL, check_u8

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in wc.CASES]
_REF = {}


def ref(name):
    """(input, model result) of a case, computed once and not written to"""
    if name not in _REF:
        case = wc.BY_NAME[name]
        x = wc.make_input(case)
        with np.errstate(all="ignore"):
            r = wm.denoise(x, **wc.kwargs(case))
        x.setflags(write=False)
        r.setflags(write=False)
        _REF[name] = (x, r)
    return _REF[name]


def gpu(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()


def run(x, **kw):
    import idn
    u8, f32 = idn.denoise_wavelet(gpu(x) if isinstance(x, np.ndarray) else x, out="both", **kw)
    return u8.cpu().numpy(), f32.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_the_model(dev, name):
    case = wc.BY_NAME[name]
    x, r = ref(name)
    u8, f = run(x, **wc.kwargs(case))
    assert f.shape == r.shape == x.shape and u8.dtype == np.uint8
    err = np.abs(f - r).max()
    print(f"{name}: max |f32 - model| = {err:.3e}")
    assert err <= TOL
    check_u8(u8, r, wm.to_u8(r))


def test_batch_with_sigma_per_image(dev):
    """three different images, an (N, C) sigma tensor: image i has the bits of its own call"""
    import torch
    import idn
    xs = np.stack([wc.make_u8(64, 96, 3, seed=s)[0] for s in (3, 4, 5)])
    sig = np.array([[0.02, 0.03, 0.025], [0.04, 0.015, 0.02], [0.01, 0.02, 0.03]])
    kw = dict(wavelet="sym4", levels=2, mode="hard", convert2ycbcr=False)
    u8, f = idn.denoise_wavelet(gpu(xs), out="both", sigma=torch.from_numpy(sig).cuda(), **kw)
    for i in range(3):
        u1, f1 = idn.denoise_wavelet(gpu(xs[i]), out="both", sigma=tuple(sig[i]), **kw)
        assert torch.equal(u8[i], u1) and torch.equal(f[i], f1), i
        with np.errstate(all="ignore"):
            r = wm.denoise(xs[i], sigma=sig[i], **kw)
        assert np.abs(f1.cpu().numpy() - r).max() <= TOL
    assert not torch.equal(f[0], f[1])


def test_batch_of_one_channel_images(dev):
    """four one-channel images (two pseudo-images, the second with one plane) against single calls"""
    import torch
    import idn
    xs = np.stack([wc.make_u8(37, 53, 1, seed=s)[0] for s in (3, 4, 5, 6)])
    kw = dict(wavelet="db2", convert2ycbcr=False)
    f = idn.denoise_wavelet(gpu(xs), out="f32", **kw)
    for i in range(4):
        assert torch.equal(f[i], idn.denoise_wavelet(gpu(xs[i]), out="f32", **kw)), i
    with np.errstate(all="ignore"):
        r = wm.denoise(xs[3], **kw)
    assert np.abs(f[3].cpu().numpy() - r).max() <= TOL


def test_sigma_from_estimate_sigma(dev):
    """estimate_sigma(x) / 255 as a device tensor is the call with the same numbers as floats"""
    import torch
    import idn
    x = gpu(np.stack([wc.make_u8(64, 96, 3, seed=s)[0] for s in (3, 4)]))
    s = idn.estimate_sigma(x) / 255
    assert s.is_cuda and s.dtype == torch.float64 and tuple(s.shape) == (2, 3)
    kw = dict(wavelet="db2", convert2ycbcr=False, out="f32")
    a = idn.denoise_wavelet(x, sigma=s, **kw)
    vals = s.cpu().numpy()
    for i in range(2):
        b = idn.denoise_wavelet(x[i], sigma=[float(v) for v in vals[i]], **kw)
        assert torch.equal(a[i], b)


@pytest.mark.parametrize("name,off_in,off_out", [("db2_64x96_L2_ycc_soft", 1, 3),
                                                 ("coif5_130x77_none", 3, 1),
                                                 ("db1_64x96_c1", 1, 1)])
def test_misaligned_buffers(dev, name, off_in, off_out):
    import torch
    import idn
    case = wc.BY_NAME[name]
    x, r = ref(name)
    want = idn.denoise_wavelet(gpu(x), out="u8", **wc.kwargs(case))
    bx, xv = carve(x, off_in)
    by, yv = carve_out(x.shape, np.uint8, off_out)
    got = idn.denoise_wavelet(xv, out="u8", out_u8=yv, **wc.kwargs(case))
    assert got.data_ptr() == yv.data_ptr() and torch.equal(got, want)
    untouched(bx, off_in, xv.nbytes)
    untouched(by, off_out, yv.nbytes)
    check_u8(got.cpu().numpy(), r, wm.to_u8(r))


def _general(lib, src, out8, outf, n, h, w, c, stride, wv, lv, method, mode, ycc, sigma):
    import torch
    from idn import _lib
    nbytes = lib.idn_wavelet_general_workspace_size(n, h, w, c, wv, lv)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    is64 = src.dtype == torch.float64
    rc = lib.idn_wavelet_denoise_general(
        None if is64 else src.data_ptr(), src.data_ptr() if is64 else None,
        out8.data_ptr() if out8 is not None else None, outf.data_ptr() if outf is not None else None,
        n, h, w, c, stride, wv, lv, method, mode, ycc, sigma, ws.data_ptr(), nbytes,
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "idn_wavelet_denoise_general")
    torch.cuda.synchronize()


def test_padded_row_stride(dev):
    """rows of w*c + 5 bytes in and out: the padding is not read as pixels and not written"""
    import torch
    import idn
    from idn import _lib
    case = wc.BY_NAME["sym4_64x17"]
    x, r = ref(case.name)
    h, w, c = x.shape
    stride = w * c + 5
    src = torch.full((h, stride), 0xEE, dtype=torch.uint8, device="cuda")
    src[:, :w * c] = gpu(x).view(h, w * c)
    dst = torch.full((h, stride), 0xA5, dtype=torch.uint8, device="cuda")
    sig = torch.full((1, 3), float(case.sigma), dtype=torch.float64, device="cuda")
    _general(_lib.load(), src, dst, None, 1, h, w, c, stride, idn.ops.WAVELETS["sym4"], -1, 0, 0, 0,
             sig.data_ptr())
    want = idn.denoise_wavelet(gpu(x), out="u8", **wc.kwargs(case))
    assert torch.equal(dst[:, :w * c].reshape(h, w, c), want)
    assert bool((dst[:, w * c:] == 0xA5).all())


def test_defaults_written_out_are_the_default_call(dev):
    import torch
    import idn
    x = gpu(wc.make_u8(64, 96, 3)[0])
    for wavelet in ("bior1.5", "db1"):
        a = idn.denoise_wavelet(x, wavelet, out="both")
        b = idn.denoise_wavelet(x, wavelet=wavelet, levels=None, out="both", out_u8=None,
                                ycc_keys=None, sigma=None, mode="soft", method="BayesShrink",
                                convert2ycbcr=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("wavelet", ["db1", "bior1.5"])
@pytest.mark.parametrize("f64", [False, True])
def test_general_entry_point_with_todays_options(dev, wavelet, f64):
    """the plumbing of the new entry point against the existing oracle"""
    import torch
    import idn
    from idn import _lib
    from oracle import wavelet as ow
    x = wc.make_u8(37, 53, 3)[0]
    want = ow.denoise_wavelet(x, wavelet)
    src = gpu(x).double() / 255.0 if f64 else gpu(x)
    if f64:
        want = ow.denoise_wavelet(src.cpu().numpy(), wavelet)
    h, w, c = x.shape
    out8 = torch.empty((h, w, c), dtype=torch.uint8, device="cuda")
    outf = torch.empty((h, w, c), dtype=torch.float32, device="cuda")
    _general(_lib.load(), src.contiguous(), out8, outf, 1, h, w, c, w * c, idn.ops.WAVELETS[wavelet],
             -1, 0, 0, 1, None)
    assert np.abs(outf.cpu().numpy().astype(np.float64) - want).max() <= TOL
    check_u8(out8.cpu().numpy(), want, (255 * want).astype(np.uint8))
    tuned = idn.denoise_wavelet(src, wavelet, out="f32").cpu().numpy().astype(np.float64)
    assert np.abs(tuned - outf.cpu().numpy()).max() <= 2 * TOL
