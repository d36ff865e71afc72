"""CPU: the numpy definition of idn.wiener (tests/wiener_model.py) against a brute-force loop and
against the real scipy.signal.wiener (tests/golden/wiener.npz, and live where scipy imports), its
noise estimate and its v == 0 rule, and the argument checks of the C-ABI entry point and of the
wrapper, none of which needs a GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import wiener_model as wm

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "wiener.npz"
NEW = ("idn_wiener_workspace_size", "idn_wiener_u8")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the model against per-pixel loops ------------------------------------------------------------

def brute(plane, kh, kw, border, noise):
    """S1, S2 (Python ints per pixel), Q, the noise used and r, one pixel and one tap at a time"""
    h, w = plane.shape
    rh, rw = kh // 2, kw // 2
    n = kh * kw

    def idx(i, length):
        if 0 <= i < length:
            return i
        if border == "zero":
            return None
        return -i if i < 0 else 2 * length - 2 - i

    s1 = [[0] * w for _ in range(h)]
    s2 = [[0] * w for _ in range(h)]
    q = 0
    for y in range(h):
        for x in range(w):
            for dy in range(-rh, rh + 1):
                for dx in range(-rw, rw + 1):
                    yy, xx = idx(y + dy, h), idx(x + dx, w)
                    t = 0 if yy is None or xx is None else int(plane[yy, xx])
                    s1[y][x] += t
                    s2[y][x] += t * t
            q += n * s2[y][x] - s1[y][x] ** 2
    nz = np.float64(float(q)) / np.float64(float(n * n * h * w)) if noise is None \
        else np.float64(noise)
    r = np.empty((h, w), np.float64)
    for y in range(h):
        for x in range(w):
            m = np.float64(s1[y][x]) / np.float64(n)
            v = np.float64(s2[y][x]) / np.float64(n) - m * m
            if v == 0 or v < nz:
                r[y, x] = m
            else:
                r[y, x] = (np.float64(plane[y, x]) - m) * (np.float64(1.0) - nz / v) + m
    return np.array(s1, np.int64), np.array(s2, np.int64), q, nz, r


@pytest.mark.parametrize("border", wm.BORDERS)
@pytest.mark.parametrize("ksize", [(3, 3), (7, 3), (15, 15)], ids=lambda k: f"{k[0]}x{k[1]}")
@pytest.mark.parametrize("shape", [(5, 7, 1), (6, 9, 3)], ids=lambda s: "x".join(map(str, s)))
def test_model_equals_brute_force(shape, ksize, border):
    kh, kw = ksize
    h, w, c = shape
    if border == "reflect101" and (kh // 2 >= h or kw // 2 >= w):
        with pytest.raises(ValueError, match="reflect101"):
            wm.window_sums(np.zeros((h, w), np.uint8), ksize, border)
        return
    x = np.random.default_rng(h * 100 + kh).integers(0, 256, shape, dtype=np.uint8)
    x[0, 0] = 255
    x[-1, -1] = 0
    for noise in (None, 400.0, 0.0):
        got, used = wm.wiener(x, ksize, noise, border=border, out="f64", return_noise=True)
        for ch in range(c):
            p = x[..., ch]
            s1, s2, q, nz, r = brute(p, kh, kw, border, noise)
            m1, m2 = wm.window_sums(p, ksize, border)
            assert m1.dtype == np.int64 and np.array_equal(m1, s1) and np.array_equal(m2, s2)
            assert wm.q_sum(m1, m2, kh * kw) == q
            assert bits(used[ch]) == bits(nz)
            assert np.array_equal(bits(got[..., ch]), bits(r))
        u8 = wm.wiener(x, ksize, noise, border=border)
        assert u8.dtype == np.uint8 and np.array_equal(u8, np.clip(np.rint(got), 0, 255))


def test_u8_rounds_half_to_even():
    assert wm.to_u8(np.array([0.5, 1.5, 2.5, 254.5, -0.2, 255.4])).tolist() == [0, 2, 2, 254, 0, 255]


# ---- the model against the real scipy ---------------------------------------------------------------

# scipy's correlate takes its FFT path on all but the smallest cases: measured deviation <= 1.4e-12.
# 1e-9 is three orders above that and six below any algorithmic difference (the smallest nonzero
# step of v is 1/n^2 >= 1e-6).
SCIPY_ATOL = 1e-9


def fixture_cases():
    f = np.load(GOLDEN)
    for key in f.files:
        if key.startswith("r/"):
            _, plane, win, nz = key.split("/")
            yield key, plane, tuple(map(int, win.split("x"))), None if nz == "None" else float(nz)


def test_fixture_records_its_scipy_and_covers_the_cases():
    f = np.load(GOLDEN)
    assert "scipy 1.15.3" in f["versions"].tolist()
    cases = list(fixture_cases())
    assert len(cases) == 60
    assert {c[1] for c in cases} == {"rand5x7", "rand33x70", "rand96x128", "smooth96x128"}
    assert {c[2] for c in cases} == {(3, 3), (5, 5), (7, 3), (15, 15), (31, 31)}
    assert {c[3] for c in cases} == {None, 400.0, 0.0}
    assert np.array_equal(f["x/smooth96x128"], wm.smooth_image())
    assert f["at/rand5x7"].size == 35 and f["at/rand96x128"].size >= 1024


@pytest.mark.parametrize("plane", ["rand5x7", "rand33x70", "rand96x128", "smooth96x128"])
def test_model_against_scipy_fixture(plane):
    f = np.load(GOLDEN)
    x, at = f["x/" + plane], f["at/" + plane]
    seen = 0
    for key, p, ksize, noise in fixture_cases():
        if p != plane:
            continue
        ref = f[key]
        r, _ = wm.wiener_plane(x, ksize, noise)
        r = r.ravel()[at]
        ok = np.isfinite(ref)  # scipy's 0 / 0 where a window is constant and the noise 0
        assert ok.sum() >= ok.size // 2
        assert np.abs(r[ok] - ref[ok]).max() <= SCIPY_ATOL, key
        assert np.array_equal(wm.to_u8(r[ok]), wm.to_u8(ref[ok])), key
        if noise is None:
            # scipy's mean(lVar) over its FFT correlation: the FFT's error, not the definition's
            est = float(f[f"est/{p}/{ksize[0]}x{ksize[1]}"])
            assert abs(wm.estimate_noise(x, ksize) - est) <= 1e-12 * est
        seen += 1
    assert seen == 15


def test_model_against_live_scipy():
    signal = pytest.importorskip("scipy.signal")
    f = np.load(GOLDEN)
    for key, plane, ksize, noise in fixture_cases():
        x = f["x/" + plane]
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = signal.wiener(x.astype(np.float64), ksize, noise)
        r, _ = wm.wiener_plane(x, ksize, noise)
        ok = np.isfinite(ref)
        assert np.abs(r[ok] - ref[ok]).max() <= SCIPY_ATOL, key
        assert np.array_equal(wm.to_u8(r[ok]), wm.to_u8(ref[ok])), key
        # the kept samples of the fixture are what this scipy gives too (FFT: not bit for bit)
        assert np.allclose(ref.ravel()[f["at/" + plane]], f[key], rtol=0, atol=SCIPY_ATOL,
                           equal_nan=True), key


# ---- the noise estimate -------------------------------------------------------------------------------

@pytest.mark.parametrize("ksize", [3, 5, (7, 3), 15, 31], ids=str)
@pytest.mark.parametrize("shape", [(5, 7), (33, 70), (96, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_estimate_is_the_mean_local_variance(shape, ksize):
    rng = np.random.default_rng(shape[0])
    for x in (rng.integers(0, 256, shape, dtype=np.uint8), wm.smooth_image(*shape)):
        _, l_var = wm.stats(x, ksize)
        mean = np.mean(l_var)
        est = wm.estimate_noise(x, ksize)
        assert est.dtype == np.float64 and abs(est - mean) <= 1e-14 * mean
        assert bits(wm.wiener(x[..., None], ksize, None, out="f64", return_noise=True)[1][0]) \
            == bits(est)


def test_q_holds_the_largest_plane_in_64_bits():
    assert 961 ** 2 * 65025 * wm.Q_MAX_PLANE < 2 ** 64
    # the worst window: half the taps 255, half 0, at n = 961 (n*S2 - S1^2 = 255^2 * 480 * 481)
    s1, s2 = np.array([[480 * 255]], np.int64), np.array([[480 * 65025]], np.int64)
    assert wm.q_sum(s1, s2, 961) == 65025 * 480 * 481 <= 961 ** 2 * 65025 // 4 + 65025


# ---- v == 0 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("border", wm.BORDERS)
def test_all_zero_image_gives_zeros(border):
    x = np.zeros((9, 11, 3), np.uint8)
    r, used = wm.wiener(x, 3, None, border=border, out="f64", return_noise=True)
    assert np.array_equal(bits(r), bits(np.zeros_like(r))) and not used.any()
    assert not wm.wiener(x, 3, None, border=border).any()


def test_flat_half_with_zero_noise_is_finite_and_unchanged():
    x = np.random.default_rng(5).integers(0, 256, (12, 20, 1), dtype=np.uint8)
    x[:, 10:] = 255
    r = wm.wiener(x, 5, 0.0, out="f64")
    assert np.isfinite(r).all()
    assert np.array_equal(r[2:-2, 12:-2], np.full((8, 6, 1), 255.0))  # the flat interior
    assert np.array_equal(wm.wiener(x, 5, 0.0), x)  # noise 0 returns the input, flat or not
    assert np.array_equal(wm.wiener(x, 5, 0.0, border="reflect101")[:, 12:], x[:, 12:])


@pytest.mark.parametrize("noise", [None, 0.0, 225.0])
def test_constant_image_keeps_its_interior(noise):
    x = np.full((11, 13, 3), 77, np.uint8)
    assert np.array_equal(wm.wiener(x, (5, 3), noise)[2:-2, 1:-1], x[2:-2, 1:-1])
    assert np.array_equal(wm.wiener(x, (5, 3), noise, border="reflect101"), x)


# ---- the quality figures the GPU test asserts, for the model alone ------------------------------------

def test_quality_thresholds_hold_for_the_model():
    clean = wm.smooth_image()
    c3 = np.repeat(clean[..., None], 3, axis=2)
    noisy = wm.noisy_image(clean, 15.0, 0)
    p_noisy = wm.psnr(noisy, c3)
    p_zero = wm.psnr(wm.wiener(noisy, 5, 225.0), c3)
    p_refl = wm.psnr(wm.wiener(noisy, 5, 225.0, border="reflect101"), c3)
    # cv2.blur(noisy, (5, 5)): rint of the reflect101 window mean (25 taps cannot tie)
    box = np.stack([np.rint(wm.stats(noisy[..., ch], 5, "reflect101")[0]) for ch in range(3)],
                   axis=-1).astype(np.uint8)
    p_box = wm.psnr(box, c3)
    assert 24.5 <= p_noisy <= 24.7 and 29.4 <= p_box <= 29.6
    assert 30.8 <= p_zero <= 31.2 and p_zero - p_noisy >= 5.0 and p_zero - p_box >= 1.0
    assert p_refl >= p_zero
    est = wm.wiener(noisy, 5, None, return_noise=True)[1]
    assert ((est >= 585) & (est <= 605)).all()  # the mean local variance counts the signal


# ---- header and binding ---------------------------------------------------------------------------------

def test_header_history_names_the_new_entry_points():
    hdr = (ROOT / "include" / "idn.h").read_text()
    assert int(re.search(r"#define\s+IDN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11
    hist = hdr[hdr.index(" *  11  idn_quant_runs_offset"):hdr.index("#define IDN_ABI_VERSION")]
    assert hist.count("later, under the same number") == 2
    for name in NEW:
        assert name in hist, name
    body = hdr[hdr.index("/* ---- wiener"):hdr.index("/* ---- quality metrics")]
    for name in NEW:
        assert re.search(r"\b%s\(" % name, body), name
    assert "v == 0" in body and "IDN_WIENER_REFLECT101" in body
    between = hdr[hdr.index("/* ---- exposure correction"):hdr.index("/* ---- shader / bloom")]
    assert "wiener" not in between


def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_signatures_bind_the_new_entry_points():
    import ctypes
    from idn import _lib as binding
    assert binding.ABI_VERSION == 11
    for name in NEW:
        assert name in binding.SIGNATURES, name
    lib = _lib()
    assert lib.idn_abi_version() == 11
    for name in NEW:
        assert getattr(lib, name).argtypes == binding.SIGNATURES[name][1]
    assert lib.idn_wiener_workspace_size.restype is ctypes.c_size_t
    assert len(binding.SIGNATURES["idn_wiener_u8"][1]) == 17


# ---- C-ABI: arguments are checked before any device work ---------------------------------------------

SRC, DST, F64, NZ, WS, BIG = 0x10000, 0x20000, 0x40000, 0x60000, 0x80000, 1 << 30


def _call(lib, **kw):
    a = dict(src=SRC, dst_u8=DST, dst_f64=None, n=1, h=24, w=28, c=3, kh=5, kw=5, border=0,
             noise=NZ, noise_stride=0, noise_out=None, ws=WS, ws_bytes=BIG)
    a.update(kw)
    a.setdefault("row_stride", a["w"] * a["c"])
    return lib.idn_wiener_u8(a["src"], a["dst_u8"], a["dst_f64"], a["n"], a["h"], a["w"], a["c"],
                             a["row_stride"], a["kh"], a["kw"], a["border"], a["noise"],
                             a["noise_stride"], a["noise_out"], a["ws"], a["ws_bytes"], None)


BAD = [("null src", dict(src=None)), ("both destinations null", dict(dst_u8=None)),
       ("in place", dict(dst_u8=SRC)), ("n<0", dict(n=-1)), ("h=0", dict(h=0)), ("w=0", dict(w=0)),
       ("c=2", dict(c=2)), ("c=4", dict(c=4)), ("c=0", dict(c=0)),
       ("row_stride", dict(row_stride=83)),
       ("kh even", dict(kh=4)), ("kw even", dict(kw=6)), ("kh=0", dict(kh=0)),
       ("kw=-1", dict(kw=-1)), ("kh=33", dict(kh=33)), ("kw=33", dict(kw=33)),
       ("border=2", dict(border=2)), ("border=-1", dict(border=-1)),
       ("reflect101 kh//2>=h", dict(border=1, h=7, kh=15)),
       ("reflect101 kw//2>=w", dict(border=1, w=2, kw=5)),
       ("dst_f64 misaligned", dict(dst_f64=F64 + 4)), ("noise misaligned", dict(noise=NZ + 2)),
       ("noise_out misaligned", dict(noise_out=NZ + 4)),
       ("noise stride", dict(noise_stride=1)), ("noise stride<0", dict(noise_stride=-3)),
       ("workspace misaligned", dict(noise=None, ws=WS + 4))]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_abi_rejects_bad_arguments(what, kw):
    lib = _lib()
    assert _call(lib, **kw) == -1, what  # IDN_EINVAL
    assert b"idn_wiener_u8" in lib.idn_last_error()


def test_abi_workspace_and_limits():
    lib = _lib()
    size = lib.idn_wiener_workspace_size
    assert [size(0, 3), size(-1, 3), size(4, 2), size(4, 0)] == [0, 0, 0, 0]
    assert size(1, 1) == 8 and size(256, 3) == 256 * 3 * 8
    assert _call(lib, noise=None, ws=None) == -4  # IDN_EWORKSPACE
    assert _call(lib, noise=None, ws_bytes=23) == -4
    assert b"workspace" in lib.idn_last_error()
    # Q would leave 64 bits above 2^28 samples per plane; a given noise needs no Q
    assert _call(lib, noise=None, h=1 << 14, w=(1 << 14) + 1, c=1) == -2  # IDN_EUNSUPPORTED
    assert _call(lib, n=0) == 0 and _call(lib, n=0, noise=None, ws=None, ws_bytes=0) == 0
    # the zero border takes a window larger than the image
    assert _call(lib, n=0, h=5, w=7, kh=31, kw=31) == 0
    assert _call(lib, n=0, h=5, w=7, kh=31, kw=31, border=1) == -1


# ---- the wrapper: argument errors before the device is looked at ------------------------------------

def _x(shape=(24, 28, 3), dtype="uint8"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype))


def _t(vals, dtype="float64"):
    import torch
    return torch.tensor(vals, dtype=getattr(torch, dtype))


WRAPPER_BAD = [
    ("not a tensor", TypeError, lambda: (np.zeros((8, 8, 1), np.uint8),), {}),
    ("float input", TypeError, lambda: (_x(dtype="float64"),), {}),
    ("2-D", ValueError, lambda: (_x((8, 8)),), {}),
    ("5-D", ValueError, lambda: (_x((1, 1, 8, 8, 3)),), {}),
    ("two channels", ValueError, lambda: (_x((8, 8, 2)),), {}),
    ("empty image", ValueError, lambda: (_x((0, 8, 1)),), {}),
    ("even ksize", ValueError, lambda: (_x(), 4), {}),
    ("ksize 0", ValueError, lambda: (_x(), 0), {}),
    ("ksize 33", ValueError, lambda: (_x(), 33), {}),
    ("ksize 2.5", ValueError, lambda: (_x(), 2.5), {}),
    ("ksize of three", ValueError, lambda: (_x(), (3, 3, 3)), {}),
    ("ksize pair with an even side", ValueError, lambda: (_x(), (3, 8)), {}),
    ("ksize str", ValueError, lambda: (_x(), "5"), {}),
    ("negative noise", ValueError, lambda: (_x(), 3, -1.0), {}),
    ("nan noise", ValueError, lambda: (_x(), 3, float("nan")), {}),
    ("inf noise", ValueError, lambda: (_x(), 3, [1.0, float("inf"), 2.0]), {}),
    ("two noises for three channels", ValueError, lambda: (_x(), 3, [1.0, 2.0]), {}),
    ("noise str", TypeError, lambda: (_x(), 3, "225"), {}),
    ("noise of objects", TypeError, lambda: (_x(), 3, [object()] * 3), {}),
    ("float32 noise tensor", TypeError, lambda: (_x(), 3, _t([1.0, 2.0, 3.0], "float32")), {}),
    ("noise tensor shape", ValueError, lambda: (_x(), 3, _t([1.0, 2.0])), {}),
    ("noise tensor batch", ValueError, lambda: (_x((2, 8, 8, 3)), 3, _t([[1.0, 2.0, 3.0]] * 3)), {}),
    ("unknown border", ValueError, lambda: (_x(),), dict(border="replicate")),
    ("reflect101 on a small image", ValueError, lambda: (_x((5, 7, 3)), 15),
     dict(border="reflect101")),
    ("unknown out", ValueError, lambda: (_x(),), dict(out="f32")),
    ("out_u8 with f64", ValueError, lambda: (_x(),), dict(out="f64", out_u8=_x())),
    ("out_u8 shape", ValueError, lambda: (_x(),), dict(out_u8=_x((24, 28, 1)))),
    ("out_u8 dtype", ValueError, lambda: (_x(),), dict(out_u8=_x(dtype="float32"))),
]


@pytest.mark.parametrize("what,exc,args,kw", WRAPPER_BAD, ids=[b[0] for b in WRAPPER_BAD])
def test_wrapper_rejects_bad_arguments(what, exc, args, kw):
    import idn
    with pytest.raises(exc, match="wiener"):
        idn.wiener(*args(), **kw)


@pytest.mark.parametrize("kw", [{}, dict(noise=225.0, border="reflect101", out="f64"),
                                dict(noise=[1.0, 2.0, 3.0], return_noise=True)], ids=str)
def test_wrapper_has_no_cpu_path(kw):
    import idn
    assert idn.wiener is idn.ops.wiener
    with pytest.raises(ValueError, match="GPU only"):
        idn.wiener(_x(), 5, **kw)


def test_tile_is_exported():
    import idn
    rows, cols = idn.ops.WIENER_TILE
    src = (ROOT / "image-denoising_amd" / "csrc" / "wiener.hip").read_text()
    assert int(re.search(r"constexpr int WN_SR = (\d+);", src).group(1)) == rows
    assert int(re.search(r"constexpr int WN_TW = (\d+);", src).group(1)) == cols
    assert idn.ops.WIENER_BORDERS == {"zero": 0, "reflect101": 1}
