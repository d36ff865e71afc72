"""CPU: the host model of idn.denoise_tv_chambolle (tests/tv_model.py), the conditions that make
the GPU cases of tests/test_tv_gpu.py meaningful, and the argument checks of the C-ABI entry points
and of the wrapper, none of which needs a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import tv_cases as tc
import tv_model as tm

ROOT = Path(__file__).resolve().parent.parent


# ---- the model ------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(5, 7), (1, 6)])
def test_loop_form_equals_vectorised_form(h, w):
    x = tm.noisy(1, h, w, 3, seed=5, sd=20)
    for kw in (dict(), dict(eps=0.0, n_iter_max=6), dict(weight=0.3, eps=1e-3)):
        a, ia, ra = tm.tv_chambolle(x, **kw)
        b, ib, rb = tm.tv_chambolle(x, channel=tm.tv_channel_direct, **kw)
        assert np.array_equal(ia, ib)
        assert np.array_equal(a, b)  # bit for bit
        for i in range(3):
            assert np.array_equal(ra[0][i], rb[0][i])


@pytest.mark.parametrize("a,b,weight", [(0.2, 0.7, 0.1), (0.9, 0.1, 0.05), (0.5, 0.5, 0.3)])
def test_closed_form_of_two_pixels(a, b, weight):
    """[a, b] after one update: p = -(g/4) / (1 + |g| / (4 weight)) with g = b - a, and the second
    iteration forms out = [a - p, b + p]"""
    im = np.array([[a, b]])
    out, iters, _ = tm.tv_channel(im, weight, 0.0, 2)
    g = b - a
    p = -(g / 4) / (1 + abs(g) / (4 * weight))
    assert iters == 2
    assert np.allclose(out, [[a - p, b + p]], rtol=0, atol=1e-15)
    if g:
        assert abs(out[0, 1] - out[0, 0]) < abs(g)


def test_constant_image_returns_itself():
    x = tc.constant(6, 9)
    out, iters, r = tm.tv_chambolle(x, n_iter_max=11)
    assert np.array_equal(out, x / 255.0)
    assert np.all(iters == 11)
    assert np.array_equal(tm.to_u8(out), x)


def test_one_iteration_returns_the_image():
    x = tc.inputs("tex-c1")
    out, iters, _ = tm.tv_chambolle(x, n_iter_max=1)
    assert np.array_equal(out, x / 255.0) and np.all(iters == 1)


def test_eps_zero_runs_every_iteration():
    _, iters, _ = tm.tv_chambolle(tc.inputs("2x2"), eps=0.0, n_iter_max=9)
    assert np.all(iters == 9)


def test_break_returns_the_image_from_before_the_update():
    """a channel that stops at i returns what eps = 0 returns after i + 1 iterations: the image the
    breaking iteration formed, from the duals of iteration i - 1"""
    x = tc.inputs("1x9")
    out, iters, _ = tc.ref("1x9")
    k = int(iters[0, 0])
    assert 0 < k < tc.N_ITER_MAX
    same, _, _ = tm.tv_chambolle(x, tc.weight("1x9"), 0.0, k + 1)
    assert np.array_equal(out, same)


def test_flat_plus_noise_moves_towards_flat():
    rs = np.random.RandomState(0)
    flat = np.full((1, 32, 48, 1), 120.0)
    x = np.clip(np.rint(flat + rs.normal(0, 15, flat.shape)), 0, 255).astype(np.uint8)
    out, _, _ = tm.tv_chambolle(x)
    before = np.mean((x / 255.0 - flat / 255.0) ** 2)
    after = np.mean((out - flat / 255.0) ** 2)
    assert after < 0.5 * before


def test_larger_weight_gives_smaller_total_variation():
    x = tc.inputs("tex-c1")
    tv = [tm.total_variation(tm.tv_chambolle(x, wt)[0][0, :, :, 0]) for wt in (0.02, 0.1, 0.5)]
    assert tm.total_variation(x[0, :, :, 0] / 255.0) > tv[0] > tv[1] > tv[2]


# ---- the GPU cases mean something -----------------------------------------------------------------

@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_conditions(name):
    x = tc.inputs(name)
    out, iters, r = tc.ref(name)
    sd = tc.CASES[name][5]
    assert 12 <= sd <= 25
    assert np.all(iters < tc.N_ITER_MAX)  # a stopping case
    margin = min(np.min(np.abs(rr - 1.0)) for per_image in r for rr in per_image)
    share = np.mean(tm.to_u8(out) != x)
    near = tm.near_half(out).mean()
    print(f"{name}: iters {iters.tolist()} least |r - 1| {margin:.3f} changed {share:.3f} "
          f"near-half {near:.4f}")
    assert margin >= 0.01
    assert share >= 0.5
    assert near <= 0.02
    for k in tc.FIXED_COUNTS:
        o, it, _ = tc.ref(name, 0.0, k)
        assert np.all(it == k)
        assert np.mean(tm.to_u8(o) != x) >= 0.5


def test_cases_hold_channels_that_stop_apart():
    apart = [name for name in tc.CASES
             if any(len(set(row)) > 1 for row in tc.ref(name)[1].tolist())]
    assert "tex-w0.1" in apart and "tiles" in apart


def test_tiles_case_spans_three_tiles_each_way():
    _, h, w = tc.CASES["tiles"][:3]
    assert h > 2 * 64 and w > 2 * 256


# ---- C-ABI: arguments are checked before any device work -------------------------------------------

def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


GOOD = dict(src=0x1000, dst_u8=0x2000, dst_f32=0x3000, iters=0x4000, n=1, h=8, w=8, c=3,
            row_stride=24, weight=0.1, eps=2e-4, n_iter_max=200, ws=0x8000, ws_bytes=1 << 30)
ORDER = list(GOOD)


def _call(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.idn_tv_chambolle_u8(*[a[k] for k in ORDER], None)


BAD = [
    ("src", dict(src=None)),
    ("no destination", dict(dst_u8=None, dst_f32=None)),
    ("in place", dict(dst_u8=0x1000)),
    ("c=2", dict(c=2)),
    ("c=4", dict(c=4)),
    ("h=0", dict(h=0)),
    ("w=0", dict(w=0)),
    ("n<0", dict(n=-1)),
    ("row_stride", dict(row_stride=23)),
    ("weight=0", dict(weight=0.0)),
    ("weight<0", dict(weight=-0.1)),
    ("weight=inf", dict(weight=float("inf"))),
    ("weight=nan", dict(weight=float("nan"))),
    ("eps<0", dict(eps=-1e-9)),
    ("eps=inf", dict(eps=float("inf"))),
    ("eps=nan", dict(eps=float("nan"))),
    ("n_iter_max=0", dict(n_iter_max=0)),
    ("n_iter_max=1001", dict(n_iter_max=1001)),
    ("misaligned workspace", dict(ws=0x8004)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_abi_rejects_bad_arguments(what, kw):
    lib = _lib()
    assert _call(lib, **kw) == -1, what  # IDN_EINVAL
    assert b"idn_tv_chambolle_u8" in lib.idn_last_error()


def test_abi_workspace_is_checked():
    lib = _lib()
    need = lib.idn_tv_chambolle_workspace_size(1, 8, 8, 3)
    assert need >= 2 * 8 * 8 * 3 * 8
    assert _call(lib, ws=None) == -4  # IDN_EWORKSPACE
    assert _call(lib, ws_bytes=need - 1) == -4
    assert b"workspace" in lib.idn_last_error()
    assert _call(lib, n=0, ws=None, ws_bytes=0) == 0  # nothing to do, nothing launched


def test_abi_workspace_size():
    lib = _lib()
    size = lib.idn_tv_chambolle_workspace_size
    for bad in ((1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 2), (-1, 8, 8, 3), (0, 8, 8, 3)):
        assert size(*bad) == 0
    one, two = size(1, 600, 1000, 3), size(2, 600, 1000, 3)
    assert two == 2 * one and one % 8 == 0
    assert 48 * 600 * 1000 <= one <= 49 * 600 * 1000  # 16 bytes per pixel and channel
    assert size(256, 600, 1000, 3) < 8e9


def test_abi_10_binds_the_new_symbols():
    from idn import _lib as binding
    m = re.search(r"#define\s+IDN_ABI_VERSION\s+(\d+)", (ROOT / "include" / "idn.h").read_text())
    assert int(m.group(1)) == 11 == binding.ABI_VERSION
    lib = _lib()
    assert lib.idn_abi_version() == 11
    for name in ("idn_tv_chambolle_workspace_size", "idn_tv_chambolle_u8"):
        assert name in binding.SIGNATURES
        assert getattr(lib, name).argtypes == binding.SIGNATURES[name][1]
    assert lib.idn_tv_chambolle_workspace_size.restype is ctypes.c_size_t


# ---- the wrapper: argument errors before the device is looked at ------------------------------------

def _x(shape=(8, 8, 3), dtype="uint8"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype))


WRAPPER_BAD = [
    ("not a tensor", TypeError, lambda: (np.zeros((8, 8, 3), np.uint8),), {}),
    ("float input", TypeError, lambda: (_x(dtype="float32"),), {}),
    ("2-D", ValueError, lambda: (_x((8, 8)),), {}),
    ("two channels", ValueError, lambda: (_x((8, 8, 2)),), {}),
    ("empty image", ValueError, lambda: (_x((0, 8, 3)),), {}),
    ("weight=0", ValueError, lambda: (_x(),), dict(weight=0.0)),
    ("weight=nan", ValueError, lambda: (_x(),), dict(weight=float("nan"))),
    ("weight=inf", ValueError, lambda: (_x(),), dict(weight=float("inf"))),
    ("weight str", ValueError, lambda: (_x(),), dict(weight="0.1")),
    ("eps<0", ValueError, lambda: (_x(),), dict(eps=-1.0)),
    ("eps=inf", ValueError, lambda: (_x(),), dict(eps=float("inf"))),
    ("n_iter_max=0", ValueError, lambda: (_x(),), dict(n_iter_max=0)),
    ("n_iter_max=1001", ValueError, lambda: (_x(),), dict(n_iter_max=1001)),
    ("n_iter_max=2.5", ValueError, lambda: (_x(),), dict(n_iter_max=2.5)),
    ("out", ValueError, lambda: (_x(),), dict(out="f64")),
    ("out_u8 with f32", ValueError, lambda: (_x(),), dict(out="f32", out_u8=_x())),
    ("out_u8 shape", ValueError, lambda: (_x(),), dict(out_u8=_x((8, 9, 3)))),
    ("out_u8 dtype", ValueError, lambda: (_x(),), dict(out_u8=_x(dtype="float32"))),
]


@pytest.mark.parametrize("what,exc,args,kw", WRAPPER_BAD, ids=[b[0] for b in WRAPPER_BAD])
def test_wrapper_rejects_bad_arguments(what, exc, args, kw):
    import idn
    with pytest.raises(exc, match="denoise_tv_chambolle"):
        idn.denoise_tv_chambolle(*args(), **kw)


def test_wrapper_has_no_cpu_path():
    import idn
    with pytest.raises(ValueError, match="GPU only"):
        idn.denoise_tv_chambolle(_x())
