"""CPU: the host model of non-local means (tests/nlm_model.py) is pinned by its own five-loop
definition and its invariants, idn_nlmeans_weights builds the model's weight table, and both C-ABI
entry points and the Python wrapper reject bad arguments before any device work (no GPU here)."""
import ctypes

import numpy as np
import pytest

import nlm_model as nm
from conftest import textured


def _lib():
    from idn import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _weights(lib, h, c, t, s, cap):
    buf = (ctypes.c_int32 * max(cap, 1))(*([-7] * max(cap, 1)))
    n, shift, fpm = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.idn_nlmeans_weights(float(h), c, t, s, buf, cap, ctypes.byref(n), ctypes.byref(shift),
                                 ctypes.byref(fpm))
    return rc, np.array(buf[:max(cap, 1)], dtype=np.int64), n.value, shift.value, fpm.value


@pytest.mark.parametrize("shape,c,t,s,h", [((16, 18), 3, 3, 5, 12.0), ((15, 15), 1, 7, 21, 15.0)])
def test_direct_definition_equals_vectorised_model(shape, c, t, s, h):
    x = textured(1, *shape, c=c, seed=5)[0]
    direct = nm.nl_means_direct(x, h, t, s)
    fast = nm.nl_means(x, h, t, s)
    assert np.array_equal(direct, fast)
    assert nm.changed_share(x, fast) > 0.5  # not an identity on this input


def test_model_constants():
    assert nm.params(7, 21) == (19096, 6, 64 / 49)
    assert nm.params(7, 11)[0] == 69599 and nm.params(7, 5)[0] == 336860
    assert nm.params(5, 11)[1:] == (5, 32 / 25) and nm.params(3, 5)[1:] == (4, 16 / 9)
    assert 21 * 21 * 19096 * 255 == 2147440680 <= nm.INT_MAX


def test_model_invariants():
    """constant and checkerboard images come back unchanged (est <= INT_MAX and wsum >= fpm are
    asserted inside the model); flat + noise at h = sd moves towards the flat image"""
    const = np.full((20, 23, 3), 77, np.uint8)
    assert np.array_equal(nm.nl_means(const, 15.0), const)
    for c in (1, 3):
        cb = nm.checkerboard(20, 22, c)
        assert np.array_equal(nm.nl_means(cb, 15.0), cb)
    white = np.full((14, 14, 3), 255, np.uint8)  # est at its largest: 441 * fpm * 255
    assert np.array_equal(nm.nl_means(white, 20.0), white)
    noisy = nm.flat_noisy(33, 47, 3, 120, 6.0)
    den = nm.nl_means(noisy, 6.0)
    mse_in = np.mean((noisy.astype(np.float64) - 120) ** 2)
    mse_out = np.mean((den.astype(np.float64) - 120) ** 2)
    print(f"mse {mse_in:.3f} -> {mse_out:.3f}")
    assert mse_out < mse_in
    with pytest.raises(ValueError):
        nm.nl_means(noisy[:13], 6.0)      # min(H, W) < b + 1
    with pytest.raises(ValueError):
        nm.nl_means(noisy, 6.0, 4, 21)


def test_reference_prefix_lengths():
    for h, n in ((1, 16), (3, 143), (10, 1582), (15, 3560), (20, 6328), (60, 56946)):
        assert len(nm.weights(float(h), 3, 7, 21)[0]) == n


@pytest.mark.parametrize("t,s", [(7, 21), (5, 11), (3, 5)])
@pytest.mark.parametrize("c", [1, 3])
def test_weights_equal_the_model(c, t, s):
    lib = _lib()
    for h in (1, 3, 6, 10, 15, 20):
        ref, _, shift, fpm = nm.weights(float(h), c, t, s)
        rc, got, n, sh, f = _weights(lib, h, c, t, s, len(ref) + 8)
        assert rc == 0
        assert (n, sh, f) == (len(ref), shift, fpm)
        assert np.array_equal(got[:n], ref)
        assert np.all(got[n:] == -7)      # nothing written behind the prefix


def test_weights_reference_prefix_lengths_from_the_library():
    lib = _lib()
    for h, n in ((1, 16), (3, 143), (10, 1582), (15, 3560), (20, 6328), (60, 56946)):
        assert _weights(lib, h, 3, 7, 21, 0)[2] == n


def test_weights_cap_below_the_prefix():
    """a cap that is too small is no error: the first cap entries and the full length"""
    lib = _lib()
    ref = nm.weights(15.0, 3, 7, 21)[0]
    rc, got, n, sh, f = _weights(lib, 15, 3, 7, 21, 100)
    assert rc == 0 and n == len(ref) == 3560 and (sh, f) == (6, 19096)
    assert np.array_equal(got, ref[:100])
    n_, s_, f_ = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = (ctypes.byref(n_), ctypes.byref(s_), ctypes.byref(f_))
    assert lib.idn_nlmeans_weights(15.0, 3, 7, 21, None, 0, *refs) == 0 and n_.value == 3560
    from idn import ops
    wt, shift, fpm = ops.nl_means_weights(15, 3)
    assert wt.dtype == np.int32 and np.array_equal(wt, ref) and (shift, fpm) == (6, 19096)


def test_weights_argument_validation():
    lib = _lib()
    n, s, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    refs = [ctypes.byref(n), ctypes.byref(s), ctypes.byref(f)]
    buf = (ctypes.c_int32 * 4)()

    def call(h=15.0, c=3, t=7, sz=21, out=buf, cap=4, refs=refs):
        return lib.idn_nlmeans_weights(h, c, t, sz, out, cap, *refs)

    assert call() == 0
    assert call(out=None) == -1 and b"null" in lib.idn_last_error()
    for i in range(3):
        bad = list(refs)
        bad[i] = None
        assert call(refs=bad) == -1 and b"null" in lib.idn_last_error()
    assert call(cap=-1) == -1 and b"cap" in lib.idn_last_error()
    for h in (0.0, -3.0, float("nan"), float("inf")):
        assert call(h=h) == -1 and b"h must be" in lib.idn_last_error()
    for c in (0, 2, 4):
        assert call(c=c) == -1 and b"channels" in lib.idn_last_error()
    for t, sz in ((4, 21), (1, 21), (9, 21), (7, 20), (7, 3), (7, 23)):
        assert call(t=t, sz=sz) == -1 and b"template_size" in lib.idn_last_error()


def test_filter_argument_validation_without_gpu():
    """idn_nlmeans_u8 rejects bad arguments on the host before any HIP call"""
    lib = _lib()
    S, D, W = 0x1000, 0x2000, 0x3000  # never dereferenced: validation fails first
    h, w, c = 32, 40, 3

    def call(src=S, dst=D, n=1, h=h, w=w, c=c, stride=None, t=7, s=21, wt=W, nw=100):
        stride = w * c if stride is None else stride
        return lib.idn_nlmeans_u8(src, dst, n, h, w, c, stride, t, s, wt, nw, None)

    for bad in (dict(src=None), dict(dst=None), dict(wt=None)):
        assert call(**bad) == -1 and b"null" in lib.idn_last_error()
    assert call(dst=S) == -1 and b"in-place" in lib.idn_last_error()
    assert call(stride=w * c - 1) == -1 and b"row_stride" in lib.idn_last_error()
    for cc in (0, 2, 4):
        assert call(c=cc, stride=4 * w) == -1 and b"channels" in lib.idn_last_error()
    for t, s in ((4, 21), (1, 21), (9, 21), (7, 20), (7, 3), (7, 23)):
        assert call(t=t, s=s) == -1 and b"template_size" in lib.idn_last_error()
    assert call(h=13) == -1 and b"smaller" in lib.idn_last_error()   # b + 1 = 14
    assert call(w=13) == -1 and b"smaller" in lib.idn_last_error()
    assert call(n=0, h=4, w=4, t=3, s=5) == 0                        # b + 1 = 4; n = 0: no launch
    assert call(n=0, h=3, w=4, t=3, s=5) == -1 and b"smaller" in lib.idn_last_error()
    for nw in (0, -5):
        assert call(nw=nw) == -1 and b"n_weights" in lib.idn_last_error()
    assert call(n=-1) == -1 and b"shape" in lib.idn_last_error()
    from idn import ops
    assert call(nw=ops.NLMEANS_MAX_WEIGHTS + 1) == -2                # IDN_EUNSUPPORTED
    assert b"IDN_NLMEANS_MAX_WEIGHTS" in lib.idn_last_error()
    assert call(n=0, nw=ops.NLMEANS_MAX_WEIGHTS) == 0


def test_max_weights_mirrors_the_header():
    import re
    from pathlib import Path
    from idn import ops
    hdr = (Path(__file__).resolve().parent.parent / "include" / "idn.h").read_text()
    m = re.search(r"#define\s+IDN_NLMEANS_MAX_WEIGHTS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == ops.NLMEANS_MAX_WEIGHTS >= 8192


def test_wrapper_rejects_before_touching_the_device():
    import torch
    import idn
    x = torch.zeros((2, 32, 40, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        idn.nl_means(x.float())
    with pytest.raises(TypeError, match="Tensor"):
        idn.nl_means(x.numpy())
    with pytest.raises(ValueError, match="channels"):
        idn.nl_means(x[..., :2])
    with pytest.raises(ValueError, match="expected"):
        idn.nl_means(x[0, 0])
    for t in (4, 9, 1, 7.5):
        with pytest.raises(ValueError, match="template_window"):
            idn.nl_means(x, 15, t)
    for s in (20, 3, 23):
        with pytest.raises(ValueError, match="search_window"):
            idn.nl_means(x, 15, 7, s)
    for h in (0, -1.0, float("nan"), "3"):
        with pytest.raises(ValueError, match="h must be"):
            idn.nl_means(x, h)
    with pytest.raises(ValueError, match="smaller"):
        idn.nl_means(x[:, :13])
    with pytest.raises(ValueError, match="GPU only"):  # valid arguments: the device check is last
        idn.nl_means(x, 15.0)
    assert idn.ops.nl_means is idn.nl_means
