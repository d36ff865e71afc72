"""GPU: idn.nl_means_colored and the two linear Lab conversions against the numpy host model
(tests/nlm_colored_model.py), bit for bit.

Everything is integer arithmetic, so every comparison is np.array_equal.  So that an identity leg
cannot pass, each model case also asserts, on the model, that the L plane and the (a, b) planes
each change in at least half of their bytes."""
import functools

import numpy as np
import pytest

import nlm_colored_model as cm
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
        "min14": lambda: textured(1, 14, 14, seed=8),
        "odd": lambda: textured(2, 75, 131, seed=6),
        "odd1": lambda: textured(2, 75, 131, seed=6)[:1],
        "flat": lambda: nm.flat_noisy(33, 47, 3, 120, 6.0)[None],
        "steps": lambda: nm.steps(40, 72, 3, 4.0)[None],
    }[kind]()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(kind, h, hc, t=7, s=21):
    """(output, share of L bytes changed, share of (a, b) bytes changed) of one case on the model,
    computed once and shared (read-only)"""
    outs, labs, dens = zip(*(cm.nl_means_colored(im, h, hc, t, s, return_lab=True)
                             for im in _input(kind)))
    y, lab, den = np.stack(outs), np.stack(labs), np.stack(dens)
    y.setflags(write=False)
    return (y, nm.changed_share(lab[..., 0], den[..., 0]),
            nm.changed_share(lab[..., 1:], den[..., 1:]))


def _all_colours():
    """all 2^24 byte triples as one 4096 x 4096 x 3 image"""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> s).astype(np.uint8) for s in (0, 8, 16)], -1).reshape(4096, 4096, 3)


def _chunked(fn, x, rows=256):
    return np.concatenate([fn(x[i:i + rows]) for i in range(0, x.shape[0], rows)])


def test_conversions_over_all_colours(dev):
    from idn import ops
    x = _all_colours()
    xd = _t(x)
    lab = _np(ops.cvt_color_lab(xd, True, linear=True))
    assert np.array_equal(lab, _chunked(cm.lbgr2lab, x))
    back = _np(ops.cvt_color_lab(xd, False, linear=True))
    assert np.array_equal(back, _chunked(cm.lab2lbgr, x))
    assert not np.array_equal(back, x) and not np.array_equal(lab, x)


def test_conversion_default_is_the_srgb_flavour(dev):
    from idn import ops
    from oracle import cvlab
    x = _input("tex")
    xd = _t(x)
    assert np.array_equal(_np(ops.cvt_color_lab(xd)), cvlab.bgr2lab(x))
    assert np.array_equal(_np(ops.cvt_color_lab(xd, False)), cvlab.lab2bgr(x))
    assert not np.array_equal(cvlab.bgr2lab(x), cm.lbgr2lab(x))


@pytest.mark.parametrize("fn,model", [("idn_lbgr2lab_u8", cm.lbgr2lab), ("idn_lab2lbgr_u8", cm.lab2lbgr)])
def test_conversion_padded_rows(dev, fn, model):
    import torch
    from idn import _lib
    x = _input("tex")[:1]
    n, h, w, c = x.shape
    pitch = w * c + 12
    src = np.full((n, h, pitch), 0xFF, np.uint8)
    src[:, :, :w * c] = x.reshape(n, h, w * c)
    src_d = _t(src)
    dst_d = torch.full((n, h, pitch), 0xEE, dtype=torch.uint8, device="cuda")
    rc = getattr(_lib.load(), fn)(src_d.data_ptr(), dst_d.data_ptr(), n, h, w, pitch,
                                  torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, fn)
    got = _np(dst_d)
    assert np.array_equal(got[:, :, :w * c].reshape(x.shape), model(x))
    assert np.all(got[:, :, w * c:] == 0xEE)


CASES = [
    # kind, h, h_color, t, s
    ("tex", 15.0, 15.0, 7, 21),     # base case
    ("tex", 10.0, 20.0, 7, 21),     # different strengths: a swap of the two tables would show
    ("tex", 20.0, 10.0, 7, 21),
    ("tex", 15.0, 15.0, 5, 11),     # other fpm (69599, and 336860 > 65535) and shifts
    ("tex", 15.0, 15.0, 3, 5),
    ("min14", 15.0, 15.0, 7, 21),   # minimum size: every window is reflected
    ("odd", 15.0, 15.0, 7, 21),     # 2 x 3 tiles, ragged edges
    ("flat", 6.0, 6.0, 7, 21),
    ("steps", 5.0, 10.0, 7, 21),
]


@pytest.mark.parametrize("kind,h,hc,t,s", CASES, ids=["%s-h%g-hc%g-t%d-s%d" % c for c in CASES])
def test_matches_the_model(dev, kind, h, hc, t, s):
    import idn
    x = _input(kind)
    ref, share_l, share_ab = _ref(kind, h, hc, t, s)
    got = _np(idn.nl_means_colored(_t(x), h, hc, t, s))
    print(f"model changes {share_l:.3f} of the L bytes and {share_ab:.3f} of the (a, b) bytes; "
          f"kernel differs from the model in {int(np.sum(got != ref))} bytes")
    assert share_l >= 0.5 and share_ab >= 0.5
    assert got.shape == x.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref)


def test_swapped_strengths_differ_on_the_model():
    a, b = _ref("tex", 10.0, 20.0)[0], _ref("tex", 20.0, 10.0)[0]
    assert nm.changed_share(a, b) > 0.5


def test_one_leg_idle(dev):
    """h = 3 leaves nearly every L byte alone while h_color = 10 changes most (a, b) bytes"""
    import idn
    x = _input("tex")
    ref, share_l, share_ab = _ref("tex", 3.0, 10.0)
    print(f"model changes {share_l:.4f} of the L bytes and {share_ab:.3f} of the (a, b) bytes")
    assert share_l <= 0.01 and share_ab >= 0.5
    assert np.array_equal(_np(idn.nl_means_colored(_t(x), 3.0, 10.0)), ref)


@pytest.mark.parametrize("colour", [(77, 77, 77), (200, 30, 90)])
def test_constant_images_return_the_round_trip(dev, colour):
    import idn
    x = np.empty((1, 40, 72, 3), np.uint8)
    x[:] = colour
    want = cm.lab2lbgr(cm.lbgr2lab(x))
    assert want[0, 0, 0].tolist() == {(77, 77, 77): [77, 77, 77], (200, 30, 90): [201, 30, 89]}[colour]
    assert np.array_equal(_np(idn.nl_means_colored(_t(x), 15.0, 15.0)), want)


@pytest.mark.parametrize("kind,h,hc,c,entries", [
    ("odd1", 15.0, 34.0, 2, 12191),    # above the 64 KB every launch gets
    ("min14", 15.0, 48.0, 2, 24297),   # just under the cap at C = 2
    ("min14", 68.0, 15.0, 1, 24382),   # just under the cap at C = 1
])
def test_long_tables(dev, kind, h, hc, c, entries):
    import idn
    x = _input(kind)
    assert len(nm.weights(h if c == 1 else hc, c, 7, 21)[0]) == entries <= idn.ops.NLMEANS_MAX_WEIGHTS
    ref = _ref(kind, h, hc)[0]
    assert np.array_equal(_np(idn.nl_means_colored(_t(x), h, hc)), ref)


@pytest.mark.parametrize("h,hc,c,entries", [(15.0, 49.0, 2, 25320), (69.0, 15.0, 1, 25104)])
def test_table_longer_than_the_cap(dev, h, hc, c, entries):
    import idn
    assert len(nm.weights(h if c == 1 else hc, c, 7, 21)[0]) == entries > idn.ops.NLMEANS_MAX_WEIGHTS
    with pytest.raises(idn.IdnError, match="unsupported"):
        idn.nl_means_colored(_t(_input("min14")), h, hc)


def _padded(x, fill):
    n, h, w, c = x.shape
    pitch = w * c + 12
    buf = np.full((n, h, pitch), fill, np.uint8)
    buf[:, :, :w * c] = x.reshape(n, h, w * c)
    return buf, pitch


def test_padded_rows(dev):
    """rows of 3w + 12 bytes for source and destination, padding 0xFF / 0xEE: the same bits, and
    the destination's padding is untouched"""
    import torch
    import idn
    x, ref = _input("tex"), _ref("tex", 15.0, 15.0)[0]
    n, h, w, c = x.shape
    src, pitch = _padded(x, 0xFF)
    src_d = _t(src)
    dst_d = torch.full((n, h, pitch), 0xEE, dtype=torch.uint8, device="cuda")
    xv = src_d[:, :, :w * c].unflatten(2, (w, c))
    ov = dst_d[:, :, :w * c].unflatten(2, (w, c))
    assert not xv.is_contiguous() and xv.stride() == (h * pitch, pitch, c, 1)
    # a padded source alone (no out): a compact result with the same bits
    res = idn.nl_means_colored(xv, 15.0, 15.0)
    assert res.is_contiguous() and np.array_equal(_np(res), ref)
    # padded source and destination
    res = idn.nl_means_colored(xv, 15.0, 15.0, out=ov)
    assert res.data_ptr() == ov.data_ptr()
    got = _np(dst_d)
    assert np.array_equal(got[:, :, :w * c].reshape(x.shape), ref)
    assert np.all(got[:, :, w * c:] == 0xEE)
    assert np.array_equal(_np(src_d), src)                # the source is left alone
    # the C-ABI with the pitch directly and a workspace of its own
    from idn import _lib, ops
    lib = _lib.load()
    wl, wab, _, _ = ops.nl_means_colored_weights(15.0, 15.0)
    wl_d, wab_d = _t(wl), _t(wab)
    nbytes = lib.idn_nlmeans_colored_workspace_size(n, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst2 = torch.full((n, h, pitch), 0xEE, dtype=torch.uint8, device="cuda")
    rc = lib.idn_nlmeans_colored_u8(src_d.data_ptr(), dst2.data_ptr(), n, h, w, pitch, 7, 21,
                                    wl_d.data_ptr(), wl_d.numel(), wab_d.data_ptr(), wab_d.numel(),
                                    ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "idn_nlmeans_colored_u8")
    assert np.array_equal(_np(dst2), got)
    # the workspace holds the model's L' plane, compact
    lp = np.stack([cm.nl_means_c(cm.lbgr2lab(im)[..., 0:1], 15.0)[..., 0] for im in x])
    assert np.array_equal(_np(ws)[:n * h * w].reshape(n, h, w), lp)


def test_out_is_honoured(dev):
    import torch
    import idn
    x, ref = _input("tex"), _ref("tex", 15.0, 15.0)[0]
    xd = _t(x)
    out = torch.zeros_like(xd)
    res = idn.nl_means_colored(xd, 15.0, 15.0, out=out)
    assert res is out and np.array_equal(_np(out), ref)
    assert np.array_equal(_np(xd), x)                    # the source is left alone
    out1 = torch.zeros_like(xd[0])
    assert idn.nl_means_colored(xd[0], 15.0, 15.0, out=out1) is out1
    assert np.array_equal(_np(out1), ref[0])
    with pytest.raises(ValueError):
        idn.nl_means_colored(xd, 15.0, 15.0, out=xd)      # in place
    with pytest.raises(ValueError):
        idn.nl_means_colored(xd, 15.0, 15.0, out=out[:1])  # mis-shaped


def test_batch_equals_one_image_launches_and_repeats(dev):
    import idn
    x, ref = _input("odd"), _ref("odd", 15.0, 15.0)[0]
    xd = _t(x)
    both = _np(idn.nl_means_colored(xd, 15.0, 15.0))
    assert not np.array_equal(ref[0], ref[1])            # an index mix-up would show
    for i in range(x.shape[0]):
        one = idn.nl_means_colored(xd[i], 15.0, 15.0)    # (H, W, 3) in, (H, W, 3) out
        assert one.shape == x.shape[1:]
        assert np.array_equal(_np(one), both[i])
    assert np.array_equal(_np(idn.nl_means_colored(xd, 15.0, 15.0)), both)  # the same bits again
    assert np.array_equal(both, ref)


def test_workspace_reuse_does_not_leak(dev):
    """one workspace for two different images and strengths, filled with 0xFF in between, gives
    what a fresh workspace gives: no stale L' byte reaches an output"""
    import torch
    from idn import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    xa, xb = _input("tex")[:1], _input("tex")[1:]
    n, h, w, _ = xa.shape
    nbytes = lib.idn_nlmeans_colored_workspace_size(n, h, w)
    shared = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def run(x, hl, hc, ws):
        wl, wab, _, _ = ops.nl_means_colored_weights(hl, hc)
        wl_d, wab_d, xd = _t(wl), _t(wab), _t(x)
        y = torch.empty_like(xd)
        rc = lib.idn_nlmeans_colored_u8(xd.data_ptr(), y.data_ptr(), n, h, w, 3 * w, 7, 21,
                                        wl_d.data_ptr(), wl_d.numel(), wab_d.data_ptr(),
                                        wab_d.numel(), ws.data_ptr(), nbytes, st)
        _lib.check(rc, "idn_nlmeans_colored_u8")
        return _np(y)

    first = run(xa, 15.0, 15.0, shared)
    shared.fill_(0xFF)
    second = run(xb, 10.0, 20.0, shared)
    fresh = run(xb, 10.0, 20.0, torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))
    assert np.array_equal(first, _ref("tex", 15.0, 15.0)[0][:1])
    assert np.array_equal(second, fresh)
    assert np.array_equal(second, _ref("tex", 10.0, 20.0)[0][1:])


def test_scoring_example(dev):
    """the README's idn.ssim(clean, idn.nl_means_colored(noisy, h=12, h_color=12)) runs on device
    tensors and the denoised batch is the model's"""
    import idn
    clean = _t(textured(1, 40, 72, seed=41))
    noisy = idn.random_noise(clean, "gaussian", var=(12.0 / 255) ** 2, seed=5)
    den = idn.nl_means_colored(noisy, h=12, h_color=12)
    assert np.array_equal(_np(den), cm.nl_means_colored_batch(_np(noisy), 12.0, 12.0))
    s = _np(idn.ssim(clean, den))
    assert s.shape == (1,) and np.all(np.isfinite(s))
