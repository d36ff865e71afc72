"""CPU: the numpy model of the exposure correction (tests/exposure_model.py) against the cross-check
values it was written to, the properties the GPU cases of tests/test_exposure_gpu.py rely on, and
the argument checks of the wrappers and of the C-ABI entry points, none of which needs a GPU."""
import re
import zlib
from pathlib import Path

import numpy as np
import pytest

import exposure_model as em

ROOT = Path(__file__).resolve().parent.parent
NEW = ("idn_bgr2yuv_u8", "idn_yuv2bgr_u8", "idn_equalize_hist_u8", "idn_clahe_u8",
       "idn_exposure_workspace_size", "idn_correct_exposure_u8")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.uint8).tobytes())


# ---- cross-check values: an independent writing of the same text ----------------------------------

PLANE_CRC = {(16, 16): (666349334, 3590927571), (17, 23): (779443542, 1598302282),
             (16, 21): (3328820016, 625885552), (21, 16): (92785042, 2726782454),
             (120, 68): (1813710230, 2192806565)}
PARAM_CRC = {(0.0, (4, 4)): 1899436123, (2.0, (1, 1)): 1865399569, (2.0, (3, 5)): 3302656263,
             (2.0, (8, 8)): 1451788083, (0.5, (2, 7)): 3364034396}


@pytest.mark.parametrize("shape", list(PLANE_CRC), ids=lambda s: f"{s[0]}x{s[1]}")
def test_plane_cross_checks(shape):
    p = em.plane(*shape)
    assert crc(em.clahe(p, 2.0, (4, 4))) == PLANE_CRC[shape][0]
    assert crc(em.equalize_hist(p)) == PLANE_CRC[shape][1]


@pytest.mark.parametrize("clip,grid", list(PARAM_CRC), ids=lambda v: str(v).replace(" ", ""))
def test_parameter_cross_checks(clip, grid):
    assert crc(em.clahe(em.plane(17, 23), clip, grid)) == PARAM_CRC[(clip, grid)]


def test_first_table_of_120x68():
    luts, th, tw = em.clahe_tables(em.plane(120, 68))
    assert (th, tw) == (30, 17)
    assert luts[0, 0, :8].tolist() == [1, 2, 2, 4, 5, 7, 8, 9]


def test_colour_cross_checks():
    b = em.bgr(24, 28)
    yuv = em.bgr2yuv(b)
    assert crc(yuv) == 710948763
    assert crc(em.yuv2bgr(yuv)) == 1519519735
    tone = em.exposure_tone(b)
    assert crc(tone) == 517507430
    assert round(float((yuv[..., 0] > 150).mean()), 2) == 0.51
    assert tone[0, :3].tolist() == [[8, 0, 118], [26, 0, 147], [69, 29, 200]]


def test_single_pixels():
    px = np.array([[[255, 0, 0], [0, 255, 0], [12, 200, 97], [0, 0, 255]]], np.uint8)
    assert em.bgr2yuv(px)[0].tolist() == [[29, 239, 103], [150, 54, 0], [148, 61, 83],
                                          [76, 91, 255]]  # red: V saturates
    assert em.yuv2bgr(np.array([[[120, 90, 240]]], np.uint8))[0, 0].tolist() == [43, 70, 248]


# ---- the arithmetic ---------------------------------------------------------------------------------

def test_tone_step_is_integer_for_every_byte():
    y = np.arange(256, dtype=np.uint8)
    assert np.array_equal(em.tone(y), em.tone_float(y))
    assert np.array_equal(em.tone(y)[:151], y[:151])  # strictly above 150
    assert em.tone(y)[151] == 128


def _all_colours():
    v = np.arange(0, 256, 5, dtype=np.uint8)
    v[-1] = 255
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(1, -1, 3)


def test_yuv_fixed_point_is_within_one_of_the_float_formulas():
    x = _all_colours()
    b, g, r = (x[..., k].astype(np.float64) for k in range(3))
    y = 0.114 * b + 0.587 * g + 0.299 * r
    u = (b - y) * 0.492 + 128
    v = (r - y) * 0.877 + 128
    ref = np.stack([y, u, v], axis=-1)
    got = em.bgr2yuv(x).astype(np.float64)
    inside = (ref > 0.5) & (ref < 254.5)
    assert inside.mean() > 0.9
    assert np.abs(got - ref)[inside].max() <= 1.0

    yuv = _all_colours().astype(np.float64)
    uu, vv = yuv[..., 1] - 128, yuv[..., 2] - 128
    back = np.stack([yuv[..., 0] + 2.032 * uu, yuv[..., 0] - 0.395 * uu - 0.581 * vv,
                     yuv[..., 0] + 1.140 * vv], axis=-1)
    got = em.yuv2bgr(_all_colours()).astype(np.float64)
    inside = (back > 0.5) & (back < 254.5)
    assert inside.mean() > 0.3
    assert np.abs(got - back)[inside].max() <= 1.0


def test_yuv_round_trip_is_lossy():
    b = em.bgr(24, 28)
    assert not np.array_equal(em.yuv2bgr(em.bgr2yuv(b)), b)


@pytest.mark.parametrize("value", [0, 7, 255])
def test_equalize_hist_of_a_constant_is_that_constant(value):
    x = np.full((9, 13), value, np.uint8)
    assert np.array_equal(em.equalize_hist(x), x)


def test_equalize_hist_starts_at_the_first_bin_present():
    x = np.array([[40, 40, 90, 200]], np.uint8)
    assert em.equalize_hist(x).tolist() == [[0, 0, 128, 255]]  # 255/2 = 127.5 rounds to even 128


@pytest.mark.parametrize("clip,grid", [(2.0, (4, 4)), (0.0, (4, 4)), (40.0, (4, 4)),
                                       (0.5, (2, 7)), (2.0, (8, 8))])
def test_clahe_tables_do_not_decrease(clip, grid):
    for p in (em.plane(17, 23), em.plane(120, 68)):
        luts, _, _ = em.clahe_tables(p, clip, grid)
        assert np.all(np.diff(luts.astype(np.int64), axis=-1) >= 0)
        assert luts[..., -1].min() == 255  # the clipped histogram still holds every pixel


def test_full_pad_rule():
    """either dimension failing to divide pads both: the one that divides grows by a whole count"""
    assert em.clahe_extent(16, 21, 4, 4) == (20, 24)
    assert em.clahe_extent(21, 16, 4, 4) == (24, 20)
    assert em.clahe_extent(16, 16, 4, 4) == (16, 16)
    assert em.clahe_extent(17, 23, 4, 4) == (20, 24)
    assert em.clahe_extent(5, 5, 4, 4) == (8, 8)
    assert em.clahe_tables(em.plane(16, 21))[1:] == (5, 6)


def test_residual_rule_on_a_hand_made_histogram():
    h = np.zeros(256, np.int64)
    h[10], h[20], h[30] = 100, 7, 3      # clip 5: excess 95 + 2 = 97 -> share 0, r = 97, step 2
    out = em.clip_histogram(h, 5)
    want = np.zeros(256, np.int64)
    want[10], want[20], want[30] = 5, 5, 3
    want[0:194:2] += 1                   # bins 0, 2, ..., 192: 97 of them
    assert np.array_equal(out, want) and out.sum() == h.sum()

    h = np.zeros(256, np.int64)
    h[0] = 1000                          # clip 100: excess 900 -> share 3, r = 132, step 1
    out = em.clip_histogram(h, 100)
    want = np.full(256, 3, np.int64)
    want[0] = 103
    want[:132] += 1
    assert np.array_equal(out, want) and out.sum() == 1000
    assert np.array_equal(em.clip_histogram(h, 0), h)  # clip_limit 0: no clipping


def test_round_half_even_ties_occur_at_120x68():
    """area 510, scale 0.5: every odd cumulative count is a tie, and half-up would differ"""
    p = em.plane(120, 68)
    luts, th, tw = em.clahe_tables(p)
    assert th * tw == 510 and np.float32(255.0) / np.float32(510) == 0.5
    hext, wext = em.clahe_extent(120, 68, 4, 4)
    assert (hext, wext) == (120, 68)
    ties = differ = 0
    for j in range(4):
        for i in range(4):
            tile = p[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            cum = np.cumsum(em.clip_histogram(np.bincount(tile.ravel(), minlength=256),
                                              em.clahe_clip(2.0, 510)))
            odd = cum % 2 == 1
            ties += int(odd.sum())
            differ += int((np.floor(cum * 0.5 + 0.5) != np.rint(cum * 0.5))[odd].sum())
    assert ties >= 1 and differ >= 1


def test_exposure_tone_is_the_composition():
    b = em.bgr(24, 28)
    yuv = em.bgr2yuv(b)
    y = em.clahe(em.equalize_hist(em.clahe(em.tone(yuv[..., 0]))))
    assert np.array_equal(em.exposure_tone(b), em.yuv2bgr(np.dstack([y, yuv[..., 1:]])))


# ---- header and binding -----------------------------------------------------------------------------

def test_header_history_names_the_new_entry_points():
    hdr = (ROOT / "include" / "idn.h").read_text()
    assert int(re.search(r"#define\s+IDN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 11
    hist = hdr[hdr.index(" *  11  idn_quant_runs_offset"):hdr.index("#define IDN_ABI_VERSION")]
    assert "later, under the same number" in hist
    for name in NEW:
        assert name in hist, name
    body = hdr[hdr.index("/* ---- exposure correction"):hdr.index("/* ---- shader / bloom")]
    assert "idn_nlmeans_colored_u8" in body and "unpinned" in body


def test_signatures_bind_the_new_entry_points():
    import ctypes
    from idn import _lib as binding
    assert binding.ABI_VERSION == 11
    for name in NEW:
        assert name in binding.SIGNATURES, name
    lib = _lib()
    for name in NEW:
        assert getattr(lib, name).argtypes == binding.SIGNATURES[name][1]
    assert lib.idn_exposure_workspace_size.restype is ctypes.c_size_t


# ---- C-ABI: arguments are checked before any device work -------------------------------------------

def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


SRC, DST, WS, BIG = 0x10000, 0x20000, 0x80000, 1 << 30


def _call(lib, fn, **kw):
    a = dict(src=SRC, dst=DST, n=1, h=24, w=28, clip=2.0, tx=4, ty=4, ws=WS, ws_bytes=BIG)
    c = 1 if fn in ("idn_equalize_hist_u8", "idn_clahe_u8") else 3
    a["row_stride"] = a["w"] * c
    a.update(kw)
    head = [a["src"], a["dst"], a["n"], a["h"], a["w"], a["row_stride"]]
    if fn in ("idn_bgr2yuv_u8", "idn_yuv2bgr_u8"):
        return getattr(lib, fn)(*head, None)
    mid = [a["clip"], a["tx"], a["ty"]] if fn == "idn_clahe_u8" else []
    return getattr(lib, fn)(*head, *mid, a["ws"], a["ws_bytes"], None)


COMMON_BAD = [("src", dict(src=None)), ("dst", dict(dst=None)), ("in place", dict(dst=SRC)),
              ("n<0", dict(n=-1)), ("h=0", dict(h=0)), ("w=0", dict(w=0)),
              ("row_stride", dict(row_stride=27))]
WS_BAD = [("misaligned workspace", dict(ws=WS + 4)), ("odd workspace", dict(ws=WS + 1))]
CLAHE_BAD = [("tx=0", dict(tx=0)), ("ty=17", dict(ty=17)), ("tx=17", dict(tx=17)),
             ("h<=ty", dict(h=4, ty=4)), ("w<=tx", dict(w=8, tx=8, row_stride=8)),
             ("clip<0", dict(clip=-0.5)), ("clip=inf", dict(clip=float("inf"))),
             ("clip=nan", dict(clip=float("nan")))]
BAD = ([(fn, *b) for fn in NEW if fn != "idn_exposure_workspace_size" for b in COMMON_BAD] +
       [(fn, *b) for fn in ("idn_equalize_hist_u8", "idn_clahe_u8", "idn_correct_exposure_u8")
        for b in WS_BAD] +
       [("idn_clahe_u8", *b) for b in CLAHE_BAD] +
       [("idn_correct_exposure_u8", "h=4", dict(h=4)), ("idn_correct_exposure_u8", "w=4",
                                                        dict(w=4, row_stride=12))])


@pytest.mark.parametrize("fn,what,kw", BAD, ids=[f"{b[0][4:-3]}-{b[1]}" for b in BAD])
def test_abi_rejects_bad_arguments(fn, what, kw):
    lib = _lib()
    assert _call(lib, fn, **kw) == -1, what  # IDN_EINVAL
    assert fn.encode() in lib.idn_last_error()


@pytest.mark.parametrize("fn,grid", [("idn_equalize_hist_u8", (1, 1)), ("idn_clahe_u8", (4, 4)),
                                     ("idn_correct_exposure_u8", (4, 4))])
def test_abi_workspace_is_checked(fn, grid):
    lib = _lib()
    need = lib.idn_exposure_workspace_size(1, 24, 28, *grid)
    assert need >= 24 * 28 + grid[0] * grid[1] * 256 * 5 + 256 * 5 and need % 8 == 0
    assert _call(lib, fn, ws=None) == -4  # IDN_EWORKSPACE
    assert _call(lib, fn, ws_bytes=need - 1) == -4
    assert b"workspace" in lib.idn_last_error()
    assert _call(lib, fn, n=0, ws=None, ws_bytes=0) == 0  # nothing to do, nothing launched


def test_abi_empty_batch_launches_nothing():
    lib = _lib()
    for fn in ("idn_bgr2yuv_u8", "idn_yuv2bgr_u8"):
        assert _call(lib, fn, n=0) == 0


def test_abi_workspace_size():
    lib = _lib()
    size = lib.idn_exposure_workspace_size
    for bad in ((0, 8, 8, 4, 4), (-1, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 0, 4, 4),
                (1, 8, 8, 0, 4), (1, 8, 8, 4, 17)):
        assert size(*bad) == 0
    one = size(1, 600, 1000, 4, 4)
    assert 600 * 1000 <= one <= 600 * 1000 + 32 * 1024  # one byte plane, histograms and tables
    assert size(256, 600, 1000, 4, 4) <= 256 * one
    assert size(1, 600, 1000, 16, 16) > one


# ---- the wrappers: argument errors before the device is looked at -----------------------------------

def _x(shape=(24, 28, 1), dtype="uint8"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype))


WRAPPER_BAD = [
    ("equalize_hist", "not a tensor", TypeError, lambda: (np.zeros((8, 8, 1), np.uint8),), {}),
    ("equalize_hist", "float input", TypeError, lambda: (_x(dtype="float32"),), {}),
    ("equalize_hist", "2-D", ValueError, lambda: (_x((8, 8)),), {}),
    ("equalize_hist", "three channels", ValueError, lambda: (_x((8, 8, 3)),), {}),
    ("equalize_hist", "empty image", ValueError, lambda: (_x((0, 8, 1)),), {}),
    ("clahe", "not a tensor", TypeError, lambda: ([[1]],), {}),
    ("clahe", "three channels", ValueError, lambda: (_x((8, 8, 3)),), {}),
    ("clahe", "grid of one number", ValueError, lambda: (_x(),), dict(tile_grid=4)),
    ("clahe", "grid of three", ValueError, lambda: (_x(),), dict(tile_grid=(4, 4, 4))),
    ("clahe", "tiles_x=0", ValueError, lambda: (_x(),), dict(tile_grid=(0, 4))),
    ("clahe", "tiles_y=17", ValueError, lambda: (_x(),), dict(tile_grid=(4, 17))),
    ("clahe", "tiles=2.5", ValueError, lambda: (_x(),), dict(tile_grid=(2.5, 4))),
    ("clahe", "H<=tiles_y", ValueError, lambda: (_x((4, 28, 1)),), {}),
    ("clahe", "W<=tiles_x", ValueError, lambda: (_x((24, 8, 1)),), dict(tile_grid=(8, 2))),
    ("clahe", "clip<0", ValueError, lambda: (_x(),), dict(clip_limit=-1.0)),
    ("clahe", "clip=inf", ValueError, lambda: (_x(),), dict(clip_limit=float("inf"))),
    ("clahe", "clip=nan", ValueError, lambda: (_x(),), dict(clip_limit=float("nan"))),
    ("clahe", "clip str", ValueError, lambda: (_x(),), dict(clip_limit="2")),
    ("cvt_color_yuv", "one channel", ValueError, lambda: (_x(),), {}),
    ("cvt_color_yuv", "int32 input", TypeError, lambda: (_x((8, 8, 3), "int32"),), {}),
    ("correct_exposure", "one channel", ValueError, lambda: (_x(),), {}),
    ("correct_exposure", "13 rows with denoise", ValueError, lambda: (_x((13, 28, 3)),), {}),
    ("correct_exposure", "4 columns", ValueError, lambda: (_x((24, 4, 3)),), dict(denoise=False)),
    ("correct_exposure", "5-D", ValueError, lambda: (_x((1, 1, 24, 28, 3)),), {}),
]


@pytest.mark.parametrize("op,what,exc,args,kw", WRAPPER_BAD,
                         ids=[f"{b[0]}-{b[1]}" for b in WRAPPER_BAD])
def test_wrapper_rejects_bad_arguments(op, what, exc, args, kw):
    import idn
    with pytest.raises(exc, match=op):
        getattr(idn, op)(*args(), **kw)


@pytest.mark.parametrize("op,shape,kw", [("equalize_hist", (24, 28, 1), {}),
                                         ("clahe", (24, 28, 1), {}),
                                         ("cvt_color_yuv", (24, 28, 3), {}),
                                         ("correct_exposure", (24, 28, 3), {}),
                                         ("correct_exposure", (5, 5, 3), dict(denoise=False))])
def test_wrappers_have_no_cpu_path(op, shape, kw):
    import idn
    with pytest.raises(ValueError, match="GPU only"):
        getattr(idn, op)(_x(shape), **kw)


def test_automold_drop_in_checks_its_input_on_the_host():
    import idn
    with pytest.raises(Exception, match="not a numpy array or list of numpy array"):
        idn.automold.correct_exposure("image.png")
    with pytest.raises(Exception, match="not a numpy array or list of numpy array"):
        idn.automold.correct_exposure([np.zeros((24, 28, 3), np.uint8), None])
    with pytest.raises(ValueError, match="correct_exposure"):
        idn.automold.correct_exposure(np.zeros((24, 28), np.uint8))
    assert idn.automold.correct_exposure([]) == []
