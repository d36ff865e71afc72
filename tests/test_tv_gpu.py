"""GPU: idn.denoise_tv_chambolle against the numpy float64 model (tests/tv_model.py).

The kernels keep the dual field in fp32, so the float result is held to 1e-5 (the project's
tolerance for a [0, 1] float result, as for the wavelets), the iteration counts to equality (the
cases of tests/tv_cases.py keep every stopping ratio 1 % away from a tie; tests/test_tv.py checks
that on the CPU), and the bytes to equality except where 255 * out lies within 255e-5 of a
half-integer, and there to 1.  Run to run, and whatever else is in the batch, results are
bit-equal."""
import numpy as np
import pytest

import tv_cases as tc
import tv_model as tm

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _run(x, **kw):
    import idn
    u8, f32, iters = idn.denoise_tv_chambolle(_t(x), out="both", return_iters=True, **kw)
    return _np(u8), _np(f32), _np(iters)


def _check(x, got, want):
    u8, f32, iters = got
    out, ref_iters, _ = want
    err = float(np.abs(f32.astype(np.float64) - out).max())
    near = tm.near_half(out)
    diff = u8.astype(np.int32) - tm.to_u8(out).astype(np.int32)
    print(f"iters {iters.tolist()} (model {ref_iters.tolist()}); max |f32 - model| {err:.3e}; "
          f"bytes off the model {int(np.count_nonzero(diff))}, near-half pixels {int(near.sum())}")
    assert u8.shape == x.shape and u8.dtype == np.uint8
    assert f32.shape == x.shape and f32.dtype == np.float32
    assert iters.shape == ref_iters.shape and iters.dtype == np.int32
    assert np.array_equal(iters, ref_iters)
    assert err <= TOL
    assert np.all(diff[~near] == 0)
    assert np.abs(diff).max() <= 1


@pytest.mark.parametrize("name", list(tc.CASES))
def test_matches_the_model(dev, name):
    x = tc.inputs(name)
    _check(x, _run(x, weight=tc.weight(name)), tc.ref(name))


@pytest.mark.parametrize("count", tc.FIXED_COUNTS)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_fixed_count_matches_the_model(dev, name, count):
    """eps = 0: the arithmetic apart from the stopping rule"""
    x = tc.inputs(name)
    _check(x, _run(x, weight=tc.weight(name), eps=0.0, n_iter_max=count), tc.ref(name, 0.0, count))


def test_padded_rows_with_out_u8(dev):
    import torch
    import idn
    name = "tex-w0.1"
    x = tc.inputs(name)
    n, h, w, c = x.shape
    pitch = w * c + 12
    src = torch.full((n, h, pitch), 0xAB, dtype=torch.uint8, device="cuda")
    dst = torch.full((n, h, pitch), 0xCD, dtype=torch.uint8, device="cuda")
    xv = src[:, :, :w * c].unflatten(2, (w, c))
    yv = dst[:, :, :w * c].unflatten(2, (w, c))
    xv.copy_(_t(x))
    res, f32, iters = idn.denoise_tv_chambolle(xv, tc.weight(name), out="both", out_u8=yv,
                                               return_iters=True)
    assert res is yv
    _check(x, (_np(yv), _np(f32), _np(iters)), tc.ref(name))
    assert np.all(_np(dst)[:, :, w * c:] == 0xCD)  # the padding is not written
    assert np.array_equal(_np(xv), x)


def test_one_iteration_returns_the_image(dev):
    x = tc.inputs("tex-c1")
    u8, f32, iters = _run(x, n_iter_max=1)
    assert np.array_equal(u8, x) and np.all(iters == 1)
    assert np.array_equal(f32, (x / 255.0).astype(np.float32))


def test_constant_image(dev):
    x = tc.constant()
    u8, f32, iters = _run(x, n_iter_max=5)
    assert np.array_equal(u8, x)
    assert np.all(iters == 5)
    assert np.array_equal(f32, (x / 255.0).astype(np.float32))


def test_mixed_batch_equals_single_launches(dev):
    """different stop counts in one batch, a constant image that never stops among them"""
    x = np.concatenate([tc.inputs("tex-w0.1"), tc.constant(), tc.inputs("tex-w0.3")])
    u8, f32, iters = _run(x, n_iter_max=40)
    assert len({tuple(r) for r in iters.tolist()}) >= 3 and np.all(iters[2] == 40)
    assert iters.min() < 40
    for i in range(len(x)):
        a8, a32, ai = _run(x[i:i + 1], n_iter_max=40)
        assert np.array_equal(ai[0], iters[i])
        assert np.array_equal(a32[0].view(np.uint32), f32[i].view(np.uint32))
        assert np.array_equal(a8[0], u8[i])
    assert np.array_equal(iters[:2], tc.ref("tex-w0.1")[1])


def test_two_runs_are_bit_equal(dev):
    x = tc.inputs("odd")
    a, b = _run(x), _run(x)
    assert np.array_equal(a[2], b[2])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[0], b[0])


def test_dirty_workspace(dev):
    """the cached workspace filled with 0xFF (NaN duals, set done flags) changes nothing"""
    from idn import ops
    x = tc.inputs("tiles")
    fresh = _run(x)
    filled = 0
    for ws in ops._WS_CACHE.values():
        ws.fill_(0xFF)
        filled += 1
    assert filled >= 1
    again = _run(x)
    assert np.array_equal(fresh[2], again[2])
    assert np.array_equal(fresh[1].view(np.uint32), again[1].view(np.uint32))
    assert np.array_equal(fresh[0], again[0])
    _check(x, again, tc.ref("tiles"))


def test_out_forms_agree(dev):
    import idn
    x = tc.inputs("tex-w0.05")
    xt = _t(x)
    kw = dict(weight=tc.weight("tex-w0.05"))
    u8, f32, iters = idn.denoise_tv_chambolle(xt, out="both", return_iters=True, **kw)
    only8 = idn.denoise_tv_chambolle(xt, **kw)
    only32, it32 = idn.denoise_tv_chambolle(xt, out="f32", return_iters=True, **kw)
    assert np.array_equal(_np(only8), _np(u8))
    assert np.array_equal(_np(only32).view(np.uint32), _np(f32).view(np.uint32))
    assert np.array_equal(_np(it32), _np(iters))
    one = idn.denoise_tv_chambolle(xt[0], out="f32", return_iters=True, **kw)
    assert tuple(one[0].shape) == x.shape[1:] and tuple(one[1].shape) == (3,)
    assert np.array_equal(_np(one[0]).view(np.uint32), _np(f32)[0].view(np.uint32))
