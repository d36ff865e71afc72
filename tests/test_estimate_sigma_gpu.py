"""GPU: idn.estimate_sigma against tests/sigma_model.py, bit for bit.

The expected values are the fixture's (tests/golden/sigma.npz: the real skimage's, which
tests/test_estimate_sigma.py holds equal to the model's on the same arrays), loaded once.  Every
comparison is on the float64 bits, NaN positions compared separately.  The cases cover the three
ways a plane's median is found (csrc/estimate_sigma.hip): listed by the first pass (at most 1024
keys), counting passes and then a list (64x97, 70x1100, 300x20, the 240x400 sanity image; on
64x97 and one channel of 70x1100 the two middle keys part at the second digit and are listed
apart), and all six
digits (the half-saturated 64x97 image, whose median is one of more than 1024 equal keys; the two
checkerboards, whose middle keys part at the first digit, each with more than 1024 keys behind
it, so that both ranks go on counting in histograms of their own).
"""
from pathlib import Path

import numpy as np
import pytest

import sigma_cases as sc
import sigma_model as sm
from carve import carve, carve_out, untouched

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "sigma.npz"
CASES = sc.cases()
NAMES = [name for name, _ in CASES]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as f:
        out = {k: f[k] for k in f.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def _dev(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name,x", CASES, ids=NAMES)
def test_equals_model(dev, gold, name, x):
    import idn
    import torch
    got = idn.estimate_sigma(_dev(x, dev))
    assert got.dtype == torch.float64 and got.device.type == "cuda"
    assert tuple(got.shape) == (x.shape[:-3] + (x.shape[-1],))
    assert same_bits(_np(got), gold["sig/" + name]), (name, _np(got), gold["sig/" + name])
    avg = idn.estimate_sigma(_dev(x, dev), average_sigmas=True)
    assert tuple(avg.shape) == x.shape[:-3] and avg.dtype == torch.float64
    assert same_bits(_np(avg), gold["avg/" + name]), (name, _np(avg), gold["avg/" + name])
    assert same_bits(_np(avg), sm.average(gold["sig/" + name]))


def test_random_noise_float64_output(dev):
    """the float64 batch idn.random_noise hands over, estimated where it lies"""
    import idn
    x = _dev(sc.random_bytes(33, 35, 3) // 2 + 60, dev)
    noisy = idn.random_noise(x, "gaussian", var=(15 / 255.0) ** 2, seed=11, out="f64")
    got = _np(idn.estimate_sigma(noisy))
    assert same_bits(got, sm.estimate_sigma(_np(noisy)))


def test_repeatable_and_batch_independent(dev, gold):
    import idn
    import torch
    for name in ("batch-5x24x40x3-u8", "batch-5x24x40x3-f64"):
        xb = _dev(dict(CASES)[name], dev)
        a, b = _np(idn.estimate_sigma(xb)), _np(idn.estimate_sigma(xb))
        assert same_bits(a, b) and same_bits(a, gold["sig/" + name])
        for i in (0, 2, 4):
            assert same_bits(_np(idn.estimate_sigma(xb[i])), a[i]), (name, i)
        rev = _np(idn.estimate_sigma(torch.flip(xb, dims=(0,))))
        assert same_bits(rev[::-1], a), name
    # a large plane beside small ones in one workspace, then alone
    big = _dev(dict(CASES)["two-70x1100x3-u8"], dev)
    one = _np(idn.estimate_sigma(big))
    two = _np(idn.estimate_sigma(torch.stack([big, torch.flip(big, dims=(1,))])))
    assert same_bits(two[0], one) and same_bits(one, gold["sig/two-70x1100x3-u8"])


def _call(lib, x, out, ws, nbytes):
    import torch
    from idn import _lib
    n, h, w, c = x.shape
    f64 = x.dtype == torch.float64
    rc = lib.idn_estimate_sigma(None if f64 else x.data_ptr(), x.data_ptr() if f64 else None,
                                out.data_ptr(), n, h, w, c, w * c, ws.data_ptr(), nbytes,
                                torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "idn_estimate_sigma")


@pytest.mark.parametrize("name,offsets", [("random-300x20x3-u8", (0, 1, 3, 8)),
                                          ("half-64x97x1-u8", (0, 3)),
                                          ("random-300x20x3-f64", (0, 8))])
def test_misaligned_buffers(dev, gold, name, offsets):
    """source, result and workspace carved out of guarded allocations: the aligned run's bits, and
    no byte written outside the result or the workspace"""
    from idn import _lib
    lib = _lib.load()
    x = dict(CASES)[name][None]
    n, h, w, c = x.shape
    nbytes = lib.idn_estimate_sigma_workspace_size(n, h, w, c, int(x.dtype == np.float64))
    assert nbytes > 0
    for so in offsets:
        for do in (0, 8):
            sbuf, xs = carve(x, so)
            obuf, out = carve_out((n, c), np.float64, do)
            wbuf, ws = carve_out((nbytes,), np.uint8, 8 if do else 0)
            _call(lib, xs, out, ws, nbytes)
            got = _np(out)
            untouched(obuf, do, out.numel() * 8)
            untouched(wbuf, 8 if do else 0, nbytes)
            assert np.array_equal(_np(xs), x)
            assert same_bits(got[0], gold["sig/" + name]), (name, so, do)


def test_small_sides_are_refused(dev):
    import idn
    import torch
    for shape in ((3, 8, 3), (8, 3, 1), (2, 3, 3, 3)):
        with pytest.raises(idn.IdnError, match="at least 4"):
            idn.estimate_sigma(torch.zeros(shape, dtype=torch.uint8, device=dev))
    assert tuple(idn.estimate_sigma(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=dev)).shape) == (0, 3)


def smooth(h=240, w=400):
    """a smooth colour image in 70..190: its db2 detail band is far below the noise"""
    y = np.arange(h)[:, None, None]
    x = np.arange(w)[None, :, None]
    ch = np.arange(3)[None, None, :]
    v = 130 + 50 * np.sin(2 * np.pi * x / 200 + ch) * np.cos(2 * np.pi * y / 120) + 5 * ch
    return np.rint(v).astype(np.uint8)


@pytest.mark.parametrize("sd", [10, 15, 25])
def test_estimates_the_noise_it_was_given(dev, sd):
    """sanity, not parity: Gaussian noise of a known sd on a smooth 240 x 400 x 3 image is
    estimated within 10 %.  The median of 24 000 keys has a sampling error under 1 % and the real
    skimage is 0.6 - 1.1 % off at sd 15 and 25 on a 120 x 200 plane (4 % at sd 5, where the byte
    rounding shows); Philox makes the draw, and so the figure, the same on every run."""
    import idn
    x = _dev(smooth(), dev)
    noisy = idn.random_noise(x, "gaussian", var=(sd / 255.0) ** 2, seed=2024, out="u8")
    got = _np(idn.estimate_sigma(noisy))
    print(f"sd {sd}: estimated {got}")
    assert same_bits(got, sm.estimate_sigma(_np(noisy)))
    assert np.all(np.abs(got - sd) <= 0.10 * sd), (sd, got)
    f64 = idn.random_noise(x, "gaussian", var=(sd / 255.0) ** 2, seed=2024, out="f64")
    got64 = _np(idn.estimate_sigma(f64)) * 255.0
    assert np.all(np.abs(got64 - sd) <= 0.10 * sd), (sd, got64)
