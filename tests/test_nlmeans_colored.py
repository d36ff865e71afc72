"""CPU: the host model of colour non-local means (tests/nlm_colored_model.py) is pinned by a
five-loop definition at C = 2, by tests/nlm_model.py at C = 1 and 3 and by facts of the 8-bit
linear Lab conversions; idn_nlmeans_colored_weights builds the model's two tables; the five new
C-ABI entry points and the Python wrapper reject bad arguments before any device work."""
import ctypes
import inspect

import numpy as np
import pytest

import nlm_colored_model as cm
import nlm_model as nm
from conftest import textured


def _lib():
    from idn import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_two_channel_model_equals_the_direct_definition():
    x = textured(1, 9, 10, c=2, seed=5)[0]      # random within +-32 of a smooth pattern
    fast = cm.nl_means_c(x, 12.0, 3, 5)
    assert np.array_equal(fast, cm.nl_means_c_direct(x, 12.0, 3, 5))
    assert nm.changed_share(x, fast) > 0.5


@pytest.mark.parametrize("c", [1, 3])
def test_model_equals_nlm_model(c):
    x = textured(1, 16, 18, c=c, seed=5)[0]
    for h, t, s in ((12.0, 3, 5), (15.0, 7, 21)):
        assert np.array_equal(cm.nl_means_c(x, h, t, s), nm.nl_means(x, h, t, s))


def test_linear_lab_facts():
    """over all 2^24 colours: the Lab ranges, the share that round-trips exactly and the largest
    round-trip error per channel; two fixed colours"""
    lo, hi = np.full(3, 255), np.zeros(3, np.int64)
    exact, worst = 0, np.zeros(3, np.int64)
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for b0 in range(0, 256, 16):
        b = np.arange(b0, b0 + 16, dtype=np.uint8)
        x = np.stack(np.broadcast_arrays(b[:, None, None], g[None], r[None]), -1)
        lab = cm.lbgr2lab(x)
        back = cm.lab2lbgr(lab)
        lo = np.minimum(lo, lab.reshape(-1, 3).min(0))
        hi = np.maximum(hi, lab.reshape(-1, 3).max(0))
        err = np.abs(back.astype(np.int64) - x).reshape(-1, 3)
        exact += int((err.sum(1) == 0).sum())
        worst = np.maximum(worst, err.max(0))
    assert lo.tolist() == [0, 42, 20] and hi.tolist() == [255, 226, 223]
    assert worst.tolist() == [4, 2, 5]
    assert 0.065 < exact / 2 ** 24 < 0.067      # the round trip is not the identity
    for colour, back in (((77, 77, 77), (77, 77, 77)), ((200, 30, 90), (201, 30, 89))):
        x = np.array(colour, np.uint8)[None]
        assert cm.lab2lbgr(cm.lbgr2lab(x)).tolist() == [list(back)]


def test_constant_image_is_the_round_trip_on_the_model():
    x = np.empty((14, 15, 3), np.uint8)
    x[:] = (200, 30, 90)
    out = cm.nl_means_colored(x, 15.0, 15.0)
    assert np.all(out == np.array((201, 30, 89), np.uint8))


def _weights(lib, h, hc, t, s, cap_l, cap_ab):
    bl = (ctypes.c_int32 * max(cap_l, 1))(*([-7] * max(cap_l, 1)))
    bab = (ctypes.c_int32 * max(cap_ab, 1))(*([-7] * max(cap_ab, 1)))
    nl, nab, shift, fpm = (ctypes.c_int(-1) for _ in range(4))
    rc = lib.idn_nlmeans_colored_weights(float(h), float(hc), t, s, bl, cap_l, ctypes.byref(nl),
                                         bab, cap_ab, ctypes.byref(nab), ctypes.byref(shift),
                                         ctypes.byref(fpm))
    return (rc, np.array(bl[:], dtype=np.int64), nl.value, np.array(bab[:], dtype=np.int64),
            nab.value, shift.value, fpm.value)


@pytest.mark.parametrize("t,s", [(7, 21), (5, 11), (3, 5)])
@pytest.mark.parametrize("h,hc", [(15, 15), (10, 20), (3, 10)])
def test_weights_equal_the_model(h, hc, t, s):
    lib = _lib()
    rl, _, shift, fpm = nm.weights(float(h), 1, t, s)
    rab = nm.weights(float(hc), 2, t, s)[0]
    rc, gl, nl, gab, nab, sh, f = _weights(lib, h, hc, t, s, len(rl) + 8, len(rab) + 8)
    assert rc == 0 and (nl, nab, sh, f) == (len(rl), len(rab), shift, fpm)
    assert np.array_equal(gl[:nl], rl) and np.array_equal(gab[:nab], rab)
    assert np.all(gl[nl:] == -7) and np.all(gab[nab:] == -7)  # nothing behind the prefixes


def test_weights_lengths_and_short_caps():
    lib = _lib()
    rl, rab = nm.weights(15.0, 1, 7, 21)[0], nm.weights(15.0, 2, 7, 21)[0]
    rc, gl, nl, gab, nab, sh, f = _weights(lib, 15, 15, 7, 21, 100, 50)
    assert rc == 0 and (nl, nab) == (len(rl), len(rab)) == (1187, 2373) and (sh, f) == (6, 19096)
    assert np.array_equal(gl, rl[:100]) and np.array_equal(gab, rab[:50])
    assert _weights(lib, 15, 15, 7, 21, 0, 0)[2::2][:2] == (1187, 2373)
    from idn import ops
    wl, wab, shift, fpm = ops.nl_means_colored_weights(15, 15)
    assert wl.dtype == wab.dtype == np.int32 and (shift, fpm) == (6, 19096)
    assert np.array_equal(wl, rl) and np.array_equal(wab, rab)
    # the lengths the GPU cases rely on, and the two just above the cap
    for h, c, n in ((34, 2, 12191), (48, 2, 24297), (68, 1, 24382), (49, 2, 25320), (69, 1, 25104)):
        assert len(nm.weights(float(h), c, 7, 21)[0]) == n
        got = _weights(lib, h if c == 1 else 15, h if c == 2 else 15, 7, 21, 0, 0)
        assert got[2 if c == 1 else 4] == n
        assert (n > ops.NLMEANS_MAX_WEIGHTS) == (h in (49, 69))


def test_weights_argument_validation():
    lib = _lib()
    ints = [ctypes.c_int() for _ in range(4)]
    nl, nab, sh, f = (ctypes.byref(v) for v in ints)
    bl, bab = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()

    def call(h=15.0, hc=15.0, t=7, s=21, wl=bl, cl=4, nl=nl, wab=bab, cab=4, nab=nab, sh=sh, f=f):
        return lib.idn_nlmeans_colored_weights(h, hc, t, s, wl, cl, nl, wab, cab, nab, sh, f)

    assert call() == 0
    for bad in (dict(wl=None), dict(wab=None), dict(nl=None), dict(nab=None), dict(sh=None),
                dict(f=None)):
        assert call(**bad) == -1 and b"null" in lib.idn_last_error()
    assert call(wl=None, cl=0, wab=None, cab=0) == 0
    for bad in (dict(cl=-1), dict(cab=-1)):
        assert call(**bad) == -1 and b"cap" in lib.idn_last_error()
    for v in (0.0, -3.0, float("nan"), float("inf")):
        assert call(h=v) == -1 and b"h must be" in lib.idn_last_error()
        assert call(hc=v) == -1 and b"h_color must be" in lib.idn_last_error()
    for t, s in ((4, 21), (1, 21), (9, 21), (7, 20), (7, 3), (7, 23)):
        assert call(t=t, s=s) == -1 and b"template_size" in lib.idn_last_error()


def test_workspace_size():
    lib = _lib()
    size = lib.idn_nlmeans_colored_workspace_size
    for n, h, w in ((1, 14, 14), (2, 75, 131), (256, 600, 1000), (3, 1, 1)):
        assert size(n, h, w) >= n * h * w
    for n, h, w in ((0, 14, 14), (-1, 14, 14), (1, 0, 14), (1, 14, 0), (1, -3, 14), (1, 14, -3)):
        assert size(n, h, w) == 0


@pytest.mark.parametrize("fn", ["idn_lbgr2lab_u8", "idn_lab2lbgr_u8"])
def test_conversion_argument_validation_without_gpu(fn):
    lib = _lib()
    call = getattr(lib, fn)
    S, D = 0x1000, 0x2000  # never dereferenced: validation fails first
    assert call(None, D, 1, 8, 8, 24, None) == -1 and b"null" in lib.idn_last_error()
    assert call(S, None, 1, 8, 8, 24, None) == -1 and b"null" in lib.idn_last_error()
    for n, h, w in ((-1, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert call(S, D, n, h, w, 24, None) == -1 and b"shape" in lib.idn_last_error()
    assert call(S, D, 1, 8, 8, 23, None) == -1 and b"row_stride" in lib.idn_last_error()
    assert fn.encode() in lib.idn_last_error()
    assert call(S, D, 0, 8, 8, 24, None) == 0       # n = 0: no launch


def test_filter_argument_validation_without_gpu():
    """idn_nlmeans_colored_u8 rejects bad arguments on the host before any HIP call"""
    lib = _lib()
    from idn import ops
    S, D, WL, WAB, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000  # never dereferenced
    h, w = 32, 40
    size = lib.idn_nlmeans_colored_workspace_size

    def call(src=S, dst=D, n=1, h=h, w=w, stride=None, t=7, s=21, wl=WL, nl=100, wab=WAB, nab=200,
             ws=WS, wsb=None):
        stride = 3 * w if stride is None else stride
        wsb = size(n, h, w) if wsb is None else wsb
        return lib.idn_nlmeans_colored_u8(src, dst, n, h, w, stride, t, s, wl, nl, wab, nab, ws,
                                          wsb, None)

    for bad in (dict(src=None), dict(dst=None), dict(wl=None), dict(wab=None)):
        assert call(**bad) == -1 and b"null" in lib.idn_last_error()
    assert call(ws=None) == -1 and b"workspace" in lib.idn_last_error()
    assert call(dst=S) == -1 and b"in-place" in lib.idn_last_error()
    assert call(stride=3 * w - 1) == -1 and b"row_stride" in lib.idn_last_error()
    for bad in (dict(n=-1), dict(h=0), dict(w=-2)):
        assert call(**bad) == -1 and b"shape" in lib.idn_last_error()
    for t, s in ((4, 21), (1, 21), (9, 21), (7, 20), (7, 3), (7, 23)):
        assert call(t=t, s=s) == -1 and b"template_size" in lib.idn_last_error()
    assert call(h=13) == -1 and b"smaller" in lib.idn_last_error()   # b + 1 = 14
    assert call(w=13) == -1 and b"smaller" in lib.idn_last_error()
    for bad in (dict(nl=0), dict(nl=-5), dict(nab=0), dict(nab=-5)):
        assert call(**bad) == -1 and b"n_weights" in lib.idn_last_error()
    assert call(wsb=size(1, h, w) - 1) == -1 and b"workspace" in lib.idn_last_error()
    assert call(wsb=h * w - 1) == -1 and b"workspace" in lib.idn_last_error()
    for bad in (dict(nl=ops.NLMEANS_MAX_WEIGHTS + 1), dict(nab=ops.NLMEANS_MAX_WEIGHTS + 1)):
        assert call(**bad) == -2                                     # IDN_EUNSUPPORTED
        assert b"IDN_NLMEANS_MAX_WEIGHTS" in lib.idn_last_error()
    assert call(n=0, nl=ops.NLMEANS_MAX_WEIGHTS, nab=ops.NLMEANS_MAX_WEIGHTS) == 0  # no launch
    assert call(n=0, h=4, w=4, t=3, s=5, ws=None, wsb=0) == 0        # b + 1 = 4
    assert call(n=0, h=3, w=4, t=3, s=5) == -1 and b"smaller" in lib.idn_last_error()


def test_wrapper_rejects_before_touching_the_device():
    import torch
    import idn
    x = torch.zeros((2, 32, 40, 3), dtype=torch.uint8)
    f = idn.nl_means_colored
    with pytest.raises(TypeError, match="uint8"):
        f(x.float())
    with pytest.raises(TypeError, match="Tensor"):
        f(x.numpy())
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="channels"):
            f(torch.zeros((2, 32, 40, c), dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected"):
        f(x[0, 0])
    for t in (4, 9, 1, 7.5):
        with pytest.raises(ValueError, match="template_window"):
            f(x, 15, 15, t)
    for s in (20, 3, 23):
        with pytest.raises(ValueError, match="search_window"):
            f(x, 15, 15, 7, s)
    for h in (0, -1.0, float("nan"), float("inf"), "3"):
        with pytest.raises(ValueError, match="h must be"):
            f(x, h, 15)
        with pytest.raises(ValueError, match="h_color must be"):
            f(x, 15, h)
    with pytest.raises(ValueError, match="smaller"):
        f(x[:, :13])
    with pytest.raises(ValueError, match="GPU only"):  # valid arguments: the device check is last
        f(x, 15.0, 15.0)
    assert idn.ops.nl_means_colored is f
    sig = inspect.signature(f)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("h", 3.0), ("h_color", 3.0), ("template_window", 7), ("search_window", 21), ("out", None)]


def test_plain_entry_points_still_reject_two_channels():
    lib = _lib()
    refs = [ctypes.byref(ctypes.c_int()) for _ in range(3)]
    assert lib.idn_nlmeans_weights(15.0, 2, 7, 21, None, 0, *refs) == -1
    assert lib.idn_nlmeans_u8(0x1000, 0x2000, 1, 32, 40, 2, 80, 7, 21, 0x3000, 100, None) == -1
    assert b"channels" in lib.idn_last_error()


def test_cvt_color_lab_default_is_unchanged():
    import torch
    from idn import ops
    sig = inspect.signature(ops.cvt_color_lab)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("to_lab", True), ("linear", False)]
    with pytest.raises(ValueError, match="GPU only"):
        ops.cvt_color_lab(torch.zeros((4, 4, 3), dtype=torch.uint8))
