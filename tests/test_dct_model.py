"""CPU: the numpy definition of idn.denoise_dct (tests/dct_model.py) against a brute-force
per-patch scipy.fft.dctn restatement, its limits, the quality it buys on the smooth test image,
the share of samples that hang on a threshold decision (the risk mask) and the fp32 restatement
off that mask; then the header, the binding, the C-ABI's argument checks and the wrapper's, none
of which needs a GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import blur_model
import dct_model as dm
import wiener_model as wm
from dct_cases import PARITY_SDS, PARITY_SHAPES, parity_case

ROOT = Path(__file__).resolve().parent.parent
NEW = ("idn_dct_denoise_workspace_size", "idn_dct_denoise_u8")

# ---- the model against brute force -------------------------------------------------------------------

def brute(x, sigma, factor, color):
    from scipy.fft import dctn, idctn
    h, w, c = x.shape
    f = x.astype(np.float64)
    sg = np.broadcast_to(np.asarray(sigma, np.float64), (c,))
    m = np.array([[1, 1, 1], [1, 0, -1], [1, -2, 1]], np.float64)
    m /= np.sqrt((m * m).sum(1, keepdims=True))
    if color and c == 3:
        g = f @ m.T
        t = factor * np.sqrt((m * m) @ (sg * sg))
    else:
        g, t = f, factor * sg
    r = np.zeros_like(g)
    for k in range(c):
        cnt = np.zeros((h, w))
        for i in range(h - 7):
            for j in range(w - 7):
                d = dctn(g[i:i + 8, j:j + 8, k], norm="ortho")
                dc = d[0, 0]
                d[np.abs(d) < t[k]] = 0.0
                d[0, 0] = dc
                r[i:i + 8, j:j + 8, k] += idctn(d, norm="ortho")
                cnt[i:i + 8, j:j + 8] += 1
        assert np.array_equal(cnt, dm.counts(h, w))
        r[..., k] /= cnt
    return r @ m if color and c == 3 else r


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("shape", [(8, 8), (9, 13), (20, 27)], ids=lambda s: "x".join(map(str, s)))
def test_model_equals_brute_force(shape, c, color):
    pytest.importorskip("scipy.fft")
    x = wm.noisy_image(wm.smooth_image(*shape), 20.0, 3)[..., :c]
    sigma = [20.0, 12.0, 31.0][:c]
    got = dm.denoise_dct(x, sigma, factor=2.7, color=color, out="f")
    assert np.abs(got - brute(x, sigma, 2.7, color)).max() < 1e-10


def test_matrices_are_orthonormal():
    assert np.abs(dm.CM @ dm.CM.T - np.eye(8)).max() < 1e-14
    assert np.abs(dm.M3 @ dm.M3.T - np.eye(3)).max() < 1e-14


# ---- limits --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_limits(color):
    const = np.full((11, 13, 3), 77, np.uint8)
    assert np.abs(dm.denoise_dct(const, 15.0, color=color, out="f") - 77.0).max() < 1e-11
    assert np.array_equal(dm.denoise_dct(const, 15.0, color=color), const)
    x = wm.noisy_image(wm.smooth_image(20, 27), 15.0, 2)
    u8, f = dm.denoise_dct(x, 0.0, color=color, out="both")
    assert np.array_equal(u8, x) and np.abs(f - x).max() < 1e-11
    # sigma = 1e6 keeps the DC terms only: every patch becomes its mean, and a sample the mean of
    # the means of the patches that cover it
    huge = dm.denoise_dct(x, 1e6, color=color, out="f")
    h, w, _ = x.shape
    p = np.lib.stride_tricks.sliding_window_view(x.astype(np.float64), (8, 8), axis=(0, 1))
    means = p.mean(axis=(-2, -1))  # (H-7, W-7, C)
    acc = np.zeros(x.shape)
    for dy in range(8):
        for dx in range(8):
            acc[dy:dy + h - 7, dx:dx + w - 7] += means
    assert np.abs(huge - acc / dm.counts(h, w)[..., None]).max() < 1e-9


def test_sigma_forms_of_the_model():
    x = np.stack([wm.noisy_image(wm.smooth_image(16, 19), sd, s) for sd, s in ((15.0, 1), (30.0, 2))])
    per = np.array([[10.0, 20.0, 30.0], [40.0, 5.0, 15.0]])
    both = dm.denoise_dct(x, per, out="f")
    for i in range(2):
        assert np.array_equal(both[i], dm.denoise_dct(x[i], per[i], out="f"))
    one = dm.denoise_dct(x, np.array([[12.0], [33.0]]), out="f")
    assert np.array_equal(one[1], dm.denoise_dct(x[1], 33.0, out="f"))
    # the propagated thresholds: equal sigmas stay, unequal ones mix by the squared rows
    assert np.allclose(dm.thresholds([15.0] * 3, 3.0, True), 45.0, rtol=0, atol=1e-12)
    t = dm.thresholds([3.0, 6.0, 12.0], 1.0, True)
    assert np.allclose(t ** 2, [(9 + 36 + 144) / 3, (9 + 144) / 2, (9 + 4 * 36 + 144) / 6])
    assert np.array_equal(dm.thresholds([3.0, 6.0, 12.0], 2.0, False), [6.0, 12.0, 24.0])


# ---- quality -------------------------------------------------------------------------------------------

def test_quality_on_the_smooth_image():
    """measured: sd 15, seeds 0 / 1: per channel 35.60 / 35.90 dB, +3.60 / +3.69 over the Wiener
    filter (32.00 / 32.21); colour transform 39.75 / 40.13, +4.15 / +4.23 over per channel (the
    best case: the three channels of this image are equal).  sd 40, seed 0: 29.26 dB per channel,
    +1.40 over the 9x9 Gaussian (27.86)."""
    clean = wm.smooth_image()
    c3 = np.repeat(clean[..., None], 3, axis=2)
    for seed in (0, 1):
        x = wm.noisy_image(clean, 15.0, seed)
        p_w = wm.psnr(wm.wiener(x, 5, 225.0, "reflect101"), c3)
        p_plain = wm.psnr(dm.denoise_dct(x, 15.0, color=False), c3)
        p_color = wm.psnr(dm.denoise_dct(x, 15.0, color=True), c3)
        print(f"sd 15 seed {seed}: wiener {p_w:.2f} dct {p_plain:.2f} dct colour {p_color:.2f}")
        assert p_plain >= p_w + 3.0
        assert p_color >= p_plain + 3.0
    x = wm.noisy_image(clean, 40.0, 0)
    p_g = wm.psnr(blur_model.gaussian_blur(x, 9), c3)
    p_plain = wm.psnr(dm.denoise_dct(x, 40.0, color=False), c3)
    print(f"sd 40 seed 0: gaussian 9 {p_g:.2f} dct {p_plain:.2f}")
    assert p_plain >= p_g + 1.0


# ---- the risk mask and the fp32 restatement ------------------------------------------------------------

@pytest.mark.parametrize("sd", PARITY_SDS, ids=lambda s: f"sd{s:g}")
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_risk_share_and_fp32_off_the_mask(shape, sd):
    """The share of samples that hang on a decision within 2e-3 of its threshold was at most
    3.0 %; off them the fp32 restatement was within 6e-5 .. 1.1e-4 of the model.  On the mask it
    is not: integer input makes the coefficients (0,4), (4,0) and (4,4) multiples of 1/8, which
    tie with T = 45 or 120, and a flipped coefficient moved a sample by up to 0.6."""
    for color in ((False, True) if shape[2] == 3 else (False,)):
        x, r64, r32, mask = parity_case(shape, sd, color)
        share = mask.mean()
        off = np.abs(r32.astype(np.float64) - r64)[~mask].max()
        print(f"{shape} sd {sd:g} color {color}: risk share {share:.4f}, fp32 off the mask {off:.2e}")
        assert share <= 0.05
        assert off <= 1.2e-4


def test_risk_mask_marks_a_tie():
    """a patch whose (0,4) coefficient equals the threshold exactly is on the mask, whole"""
    x = np.full((8, 8, 1), 100, np.uint8)
    x[:, [0, 3, 4, 7]] = 110  # the signs of Cm[4]: only D[0,0] and D[0,4] = 40 are not zero
    d = dm.patch_dct(x[..., 0].astype(np.float64))[0, 0]
    t = abs(d[0, 4])
    assert abs(t - 40.0) < 1e-12
    assert dm.risk_mask(x, t / 3.0, color=False).all()
    assert not dm.risk_mask(x, (t + 1.0) / 3.0, color=False).any()


# ---- header and binding --------------------------------------------------------------------------------

def test_header_history_names_the_new_entry_points():
    hdr = (ROOT / "include" / "idn.h").read_text()
    assert int(re.search(r"#define\s+IDN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11
    hist = hdr[hdr.index(" *  11  idn_quant_runs_offset"):hdr.index("#define IDN_ABI_VERSION")]
    for name in NEW:
        assert name in hist, name
    body = hdr[hdr.index("/* ---- sliding DCT denoiser"):hdr.index("/* ---- quality metrics")]
    for name in NEW:
        assert re.search(r"\b%s\(" % name, body), name
    for word in ("tests/dct_model.py", "IDN_EUNSUPPORTED", "16 is not built", "unpinned"):
        assert word in body, word


def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_signatures_bind_the_new_entry_points():
    import ctypes
    from idn import _lib as binding
    for name in NEW:
        assert name in binding.SIGNATURES, name
    lib = _lib()
    for name in NEW:
        assert getattr(lib, name).argtypes == binding.SIGNATURES[name][1]
    assert lib.idn_dct_denoise_workspace_size.restype is ctypes.c_size_t
    assert len(binding.SIGNATURES["idn_dct_denoise_u8"][1]) == 16


# ---- C-ABI: arguments are checked before any device work -----------------------------------------------

SRC, DST, F32, SG, WS = 0x10000, 0x20000, 0x40000, 0x60000, 0x80000


def _call(lib, **kw):
    a = dict(src=SRC, dst_u8=DST, dst_f32=None, n=1, h=24, w=28, c=3, patch=8, color=1, sigma=SG,
             sigma_stride=0, factor=3.0, ws=None, ws_bytes=0)
    a.update(kw)
    a.setdefault("row_stride", a["w"] * a["c"])
    return lib.idn_dct_denoise_u8(a["src"], a["dst_u8"], a["dst_f32"], a["n"], a["h"], a["w"],
                                  a["c"], a["row_stride"], a["patch"], a["color"], a["sigma"],
                                  a["sigma_stride"], a["factor"], a["ws"], a["ws_bytes"], None)


BAD = [("null src", dict(src=None)), ("null sigma", dict(sigma=None)),
       ("both destinations null", dict(dst_u8=None)), ("in place", dict(dst_u8=SRC)),
       ("n<0", dict(n=-1)), ("h=0", dict(h=0)), ("w=0", dict(w=0)), ("h<0", dict(h=-8)),
       ("c=2", dict(c=2, color=0)), ("c=4", dict(c=4, color=0)), ("c=0", dict(c=0, color=0)),
       ("row_stride", dict(row_stride=83)),
       ("color=2", dict(color=2)), ("color=-1", dict(color=-1)), ("color with c=1", dict(c=1)),
       ("dst_f32 misaligned", dict(dst_f32=F32 + 2)), ("sigma misaligned", dict(sigma=SG + 4)),
       ("sigma stride", dict(sigma_stride=1)), ("sigma stride<0", dict(sigma_stride=-3)),
       ("factor<0", dict(factor=-1.0)), ("factor nan", dict(factor=float("nan"))),
       ("factor inf", dict(factor=float("inf")))]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_abi_rejects_bad_arguments(what, kw):
    lib = _lib()
    assert _call(lib, **kw) == -1, what  # IDN_EINVAL
    assert b"idn_dct_denoise_u8" in lib.idn_last_error()
    if "n" not in kw:
        assert _call(lib, n=0, **kw) == -1  # checked before the empty batch returns


UNSUPPORTED = [("patch=16", dict(patch=16)), ("patch=4", dict(patch=4)), ("patch=0", dict(patch=0)),
               ("h=7", dict(h=7)), ("w=7", dict(w=7)), ("h=1 w=1", dict(h=1, w=1))]


@pytest.mark.parametrize("what,kw", UNSUPPORTED, ids=[b[0] for b in UNSUPPORTED])
def test_abi_reports_what_is_not_built(what, kw):
    lib = _lib()
    assert _call(lib, **kw) == -2, what  # IDN_EUNSUPPORTED
    assert b"idn_dct_denoise_u8" in lib.idn_last_error()
    assert _call(lib, n=0, **kw) == -2  # checked before the empty batch returns


def test_abi_workspace_and_empty_batch():
    """the thresholds are formed in the kernel: the workspace is 0 bytes for every shape, NULL is
    accepted, and IDN_EWORKSPACE has nothing to refuse"""
    lib = _lib()
    size = lib.idn_dct_denoise_workspace_size
    assert [size(0, 8, 8, 3), size(-1, 8, 8, 3), size(4, 8, 8, 2), size(256, 600, 1000, 3)] == [0] * 4
    assert _call(lib, n=0) == 0 and _call(lib, n=0, ws=WS + 1, ws_bytes=5) == 0
    assert _call(lib, n=0, dst_u8=None, dst_f32=F32, c=1, color=0, sigma_stride=1) == 0
    assert _call(lib, n=0, h=8, w=8) == 0


# ---- the wrapper: argument errors before the device is looked at ----------------------------------------

def _x(shape=(24, 28, 3), dtype="uint8"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype))


def _t(vals, dtype="float64"):
    import torch
    return torch.tensor(vals, dtype=getattr(torch, dtype))


WRAPPER_BAD = [
    ("not a tensor", TypeError, lambda: (np.zeros((8, 8, 1), np.uint8), 15.0), {}),
    ("float input", TypeError, lambda: (_x(dtype="float64"), 15.0), {}),
    ("2-D", ValueError, lambda: (_x((8, 8)), 15.0), {}),
    ("5-D", ValueError, lambda: (_x((1, 1, 8, 8, 3)), 15.0), {}),
    ("two channels", ValueError, lambda: (_x((8, 8, 2)), 15.0), {}),
    ("four channels", ValueError, lambda: (_x((8, 8, 4)), 15.0), {}),
    ("empty image", ValueError, lambda: (_x((0, 8, 1)), 15.0), {}),
    ("negative sigma", ValueError, lambda: (_x(), -1.0), {}),
    ("nan sigma", ValueError, lambda: (_x(), float("nan")), {}),
    ("inf sigma", ValueError, lambda: (_x(), [1.0, float("inf"), 2.0]), {}),
    ("two sigmas for three channels", ValueError, lambda: (_x(), [1.0, 2.0]), {}),
    ("sigma None", TypeError, lambda: (_x(), None), {}),
    ("sigma str", TypeError, lambda: (_x(), "15"), {}),
    ("sigma of objects", TypeError, lambda: (_x(), [object()] * 3), {}),
    ("float32 sigma tensor", TypeError, lambda: (_x(), _t([1.0, 2.0, 3.0], "float32")), {}),
    ("sigma tensor shape", ValueError, lambda: (_x(), _t([1.0, 2.0])), {}),
    ("sigma tensor batch", ValueError, lambda: (_x((2, 8, 8, 3)), _t([[1.0, 2.0, 3.0]] * 3)), {}),
    ("negative factor", ValueError, lambda: (_x(), 15.0), dict(factor=-1.0)),
    ("nan factor", ValueError, lambda: (_x(), 15.0), dict(factor=float("nan"))),
    ("inf factor", ValueError, lambda: (_x(), 15.0), dict(factor=float("inf"))),
    ("factor str", ValueError, lambda: (_x(), 15.0), dict(factor="3")),
    ("color int", TypeError, lambda: (_x(), 15.0), dict(color=2)),
    ("unknown out", ValueError, lambda: (_x(), 15.0), dict(out="f64")),
    ("out_u8 with f32", ValueError, lambda: (_x(), 15.0), dict(out="f32", out_u8=_x())),
    ("out_u8 shape", ValueError, lambda: (_x(), 15.0), dict(out_u8=_x((24, 28, 1)))),
    ("out_u8 dtype", ValueError, lambda: (_x(), 15.0), dict(out_u8=_x(dtype="float32"))),
]


@pytest.mark.parametrize("what,exc,args,kw", WRAPPER_BAD, ids=[b[0] for b in WRAPPER_BAD])
def test_wrapper_rejects_bad_arguments(what, exc, args, kw):
    import idn
    with pytest.raises(exc, match="denoise_dct"):
        idn.denoise_dct(*args(), **kw)


@pytest.mark.parametrize("args,kw", [((_x, 15.0), dict(patch=16)), ((_x, 15.0), dict(patch=4)),
                                     ((lambda: _x((7, 28, 3)), 15.0), {}),
                                     ((lambda: _x((28, 7, 1)), 15.0), {})],
                         ids=["patch16", "patch4", "h7", "w7"])
def test_wrapper_reports_what_is_not_built(args, kw):
    import idn
    with pytest.raises(idn.IdnError, match="denoise_dct: unsupported"):
        idn.denoise_dct(args[0](), args[1], **kw)


def test_sigma_is_required():
    import idn
    with pytest.raises(TypeError):
        idn.denoise_dct(_x())


@pytest.mark.parametrize("kw", [{}, dict(color=False, out="f32"), dict(factor=2.5, out="both")],
                         ids=str)
def test_wrapper_has_no_cpu_path(kw):
    import idn
    assert idn.denoise_dct is idn.ops.denoise_dct
    with pytest.raises(ValueError, match="GPU only"):
        idn.denoise_dct(_x(), 15.0, **kw)
    with pytest.raises(ValueError, match="GPU only"):
        idn.denoise_dct(_x(), _t([1.0, 2.0, 3.0]), **kw)


def test_tile_is_exported():
    import idn
    rows, cols = idn.ops.DCT_TILE
    src = (ROOT / "image-denoising_amd" / "csrc" / "dct_denoise.hip").read_text()
    assert int(re.search(r"constexpr int DD_SR = (\d+);", src).group(1)) == rows
    assert int(re.search(r"constexpr int DD_TW = (\d+);", src).group(1)) == cols
    assert int(re.search(r"constexpr int DD_P = (\d+);", src).group(1)) == idn.ops.DCT_PATCH == dm.PATCH
