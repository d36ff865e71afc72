"""GPU: idn.nl_means against the numpy host model (tests/nlm_model.py), bit for bit.

The scheme is integer arithmetic throughout, so every case asserts np.array_equal.  So that an
identity or near-identity kernel cannot pass, each case also asserts on the model that its output
differs from its input in at least half of the bytes (0.1 for the h = 3 leg of the flat case, where
most pixels keep little but their own weight)."""
import functools

import numpy as np
import pytest

import nlm_model as nm
from conftest import textured

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _input(kind):
    x = {
        "tex": lambda: textured(2, 40, 72, seed=3),
        "tex_c1": lambda: textured(1, 40, 72, c=1, seed=4),
        "min14": lambda: textured(1, 14, 14, seed=8),
        "odd": lambda: textured(2, 75, 131, seed=6),
        "flat": lambda: nm.flat_noisy(33, 47, 3, 120, 6.0)[None],
        "steps": lambda: nm.steps(40, 72, 3, 4.0)[None],
    }[kind]()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(kind, h, t, s):
    """the model's output of one case, computed once and shared (read-only)"""
    y = nm.nl_means_batch(_input(kind), h, t, s)
    y.setflags(write=False)
    return y


CASES = [
    # kind, h, t, s, least share of bytes the model must change
    ("tex", 15.0, 7, 21, 0.5),      # 1 base case
    ("tex", 10.0, 7, 21, 0.5),      # 2 other table lengths
    ("tex", 20.0, 7, 21, 0.5),
    ("tex_c1", 15.0, 7, 21, 0.5),   # 3 C = 1
    ("tex", 15.0, 5, 11, 0.5),      # 4 other fpm (69599, and 336860 > 65535)
    ("tex", 15.0, 3, 5, 0.5),
    ("min14", 15.0, 7, 21, 0.5),    # 5 minimum size: every window is reflected
    ("odd", 15.0, 7, 21, 0.5),      # 6 odd sizes, more than one tile both ways
    ("flat", 6.0, 7, 21, 0.5),      # 7 flat + sd 6
    ("flat", 3.0, 7, 21, 0.1),      #   some pixels keep only the centre weight: wsum == fpm
    ("steps", 5.0, 7, 21, 0.5),     # 8 edges
]


@pytest.mark.parametrize("kind,h,t,s,least", CASES,
                         ids=["%s-h%g-t%d-s%d" % c[:4] for c in CASES])
def test_matches_the_model(dev, kind, h, t, s, least):
    import idn
    x, ref = _input(kind), _ref(kind, h, t, s)
    share = nm.changed_share(x, ref)
    got = _np(idn.nl_means(_t(x), h, t, s))
    print(f"model changes {share:.3f} of the bytes; kernel differs from the model in "
          f"{int(np.sum(got != ref))} bytes")
    assert share >= least
    assert got.shape == x.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref)


def test_centre_weight_only_pixels(dev):
    """the h = 3 leg of the flat case has pixels whose wsum is exactly fpm (only the zero offset
    weighs): they return their input byte, and the kernel agrees"""
    import idn
    x = _input("flat")[0]
    out, wsum = nm.nl_means(x, 3.0, return_wsum=True)
    alone = wsum == nm.params(7, 21)[0]
    assert 0 < alone.mean() < 0.2
    assert np.array_equal(out[alone], x[alone])
    got = _np(idn.nl_means(_t(x), 3.0))
    assert np.array_equal(got[alone], x[alone])


def test_constant_and_checkerboard_come_back(dev):
    import idn
    for x in (np.full((1, 40, 72, 3), 77, np.uint8), np.full((1, 20, 23, 1), 255, np.uint8),
              nm.checkerboard(40, 72, 3)[None], nm.checkerboard(21, 22, 1)[None]):
        assert np.array_equal(_np(idn.nl_means(_t(x), 15.0)), x)


def test_padded_rows(dev):
    """rows of w*c + 12 bytes for source and destination, padding 0xFF / 0xEE: the same bits, and
    the destination's padding is untouched"""
    import torch
    import idn
    x, ref = _input("tex"), _ref("tex", 15.0, 7, 21)
    n, h, w, c = x.shape
    pitch = w * c + 12
    src = np.full((n, h, pitch), 0xFF, np.uint8)
    src[:, :, :w * c] = x.reshape(n, h, w * c)
    src_d = _t(src)
    dst_d = torch.full((n, h, pitch), 0xEE, dtype=torch.uint8, device="cuda")
    xv = src_d[:, :, :w * c].unflatten(2, (w, c))
    ov = dst_d[:, :, :w * c].unflatten(2, (w, c))
    assert not xv.is_contiguous() and xv.stride() == (h * pitch, pitch, c, 1)
    res = idn.nl_means(xv, 15.0, out=ov)
    assert res.data_ptr() == ov.data_ptr()
    got = _np(dst_d)
    assert np.array_equal(got[:, :, :w * c].reshape(x.shape), ref)
    assert np.all(got[:, :, w * c:] == 0xEE)
    # a padded source alone (no out): a compact result with the same bits
    res2 = idn.nl_means(xv, 15.0)
    assert res2.is_contiguous() and np.array_equal(_np(res2), ref)
    # the C-ABI with the pitch directly
    from idn import _lib, ops
    wt = _t(ops.nl_means_weights(15.0, c)[0])
    dst2 = torch.full((n, h, pitch), 0xEE, dtype=torch.uint8, device="cuda")
    rc = _lib.load().idn_nlmeans_u8(src_d.data_ptr(), dst2.data_ptr(), n, h, w, c, pitch, 7, 21,
                                    wt.data_ptr(), wt.numel(),
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "idn_nlmeans_u8")
    assert np.array_equal(_np(dst2), got)


def test_batch_equals_one_image_launches_and_repeats(dev):
    import idn
    x, ref = _input("odd"), _ref("odd", 15.0, 7, 21)
    xd = _t(x)
    both = _np(idn.nl_means(xd, 15.0))
    assert not np.array_equal(ref[0], ref[1])            # an index mix-up would show
    for i in range(x.shape[0]):
        one = idn.nl_means(xd[i], 15.0)                  # (H, W, C) in, (H, W, C) out
        assert one.shape == x.shape[1:]
        assert np.array_equal(_np(one), both[i])
        assert np.array_equal(_np(idn.nl_means(xd[i:i + 1], 15.0))[0], both[i])
    assert np.array_equal(_np(idn.nl_means(xd, 15.0)), both)  # a second call: the same bits
    assert np.array_equal(both, ref)


def test_out_is_honoured(dev):
    import torch
    import idn
    x, ref = _input("tex"), _ref("tex", 15.0, 7, 21)
    xd = _t(x)
    out = torch.zeros_like(xd)
    res = idn.nl_means(xd, 15.0, out=out)
    assert res is out and np.array_equal(_np(out), ref)
    assert np.array_equal(_np(xd), x)                    # the source is left alone
    out1 = torch.zeros_like(xd[0])
    assert idn.nl_means(xd[0], 15.0, out=out1) is out1 and np.array_equal(_np(out1), ref[0])
    with pytest.raises(ValueError):
        idn.nl_means(xd, 15.0, out=xd)
    with pytest.raises(ValueError):
        idn.nl_means(xd, 15.0, out=out[:1])


def test_table_longer_than_the_cap(dev):
    """h = 60 at C = 3 needs 56946 weights: unsupported when that exceeds NLMEANS_MAX_WEIGHTS,
    bit-equal otherwise"""
    import idn
    x = _input("min14")
    n_weights = len(nm.weights(60.0, 3, 7, 21)[0])
    assert n_weights == 56946
    if n_weights > idn.ops.NLMEANS_MAX_WEIGHTS:
        with pytest.raises(idn.IdnError, match="unsupported"):
            idn.nl_means(_t(x), 60.0)
    else:
        assert np.array_equal(_np(idn.nl_means(_t(x), 60.0)), nm.nl_means_batch(x, 60.0))


@pytest.mark.parametrize("h,entries", [(22.0, 7656), (25.0, 9887), (39.0, 24060)])
def test_long_tables(dev, h, entries):
    """tables that fill the 64 KB of LDS every launch gets (7656 entries), need the kernel's LDS
    limit raised (9887: two workgroups per CU still fit) and leave room for one workgroup per CU
    (24060, just below the cap) run and match"""
    import idn
    x = _input("odd")[:1]
    assert len(nm.weights(h, 3, 7, 21)[0]) == entries <= idn.ops.NLMEANS_MAX_WEIGHTS
    ref = nm.nl_means_batch(x, h)
    assert nm.changed_share(x, ref) >= 0.5
    assert np.array_equal(_np(idn.nl_means(_t(x), h)), ref)


def test_scoring_example(dev):
    """the README's idn.ssim(clean, idn.nl_means(noisy, h=...)) runs on device tensors and the
    denoised batch is the model's"""
    import idn
    clean = _t(textured(1, 40, 72, seed=41))
    noisy = idn.random_noise(clean, "gaussian", var=(12.0 / 255) ** 2, seed=5)
    den = idn.nl_means(noisy, h=12.0)
    assert np.array_equal(_np(den), nm.nl_means_batch(_np(noisy), 12.0))
    s = _np(idn.ssim(clean, den))
    assert s.shape == (1,) and np.all(np.isfinite(s))
