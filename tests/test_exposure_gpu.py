"""GPU: idn.equalize_hist, idn.clahe, idn.cvt_color_yuv and idn.correct_exposure against the numpy
model tests/exposure_model.py, bit for bit in every case (np.array_equal).

Shapes: 16x16 (the grid cuts the image), 17x23 (both dimensions padded), 16x21 and 21x16 (one
dimension divides and is still padded by a whole tile count), 120x68 (area 510, scale 0.5: the
rounding ties of tests/test_exposure.py), 5x5 (the smallest image a (4, 4) grid takes: 2x2 tiles,
three reflected rows and columns), 75x131 (several apply bands of 16 rows, several 32-row histogram
chunks per tile) and one 300x300 plane at grid (1, 1) whose fullest bin exceeds 65535.
"""
import functools

import numpy as np
import pytest

import exposure_model as em
from carve import carve, carve_out, untouched
from conftest import textured

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (17, 23), (16, 21), (21, 16), (120, 68), (5, 5), (75, 131)]
PARAMS = [(0.0, (4, 4)), (2.0, (1, 1)), (2.0, (3, 5)), (2.0, (8, 8)), (0.5, (2, 7)),
          (40.0, (4, 4))]
CONTENTS = ["textured", "formula", "constant", "two-levels", "first-bin-60", "dark", "bright"]


def _sid(s):
    return f"{s[0]}x{s[1]}"


@functools.lru_cache(maxsize=None)
def content(name, h, w):
    """one (h, w) uint8 plane; read-only, shared among the tests"""
    y, x = np.mgrid[0:h, 0:w]
    if name == "textured":
        p = textured(1, h, w, 1, seed=11)[0, :, :, 0]
    elif name == "formula":
        p = em.plane(h, w)
    elif name == "constant":
        p = np.full((h, w), 93)
    elif name == "two-levels":
        p = np.where((x // 3 + y // 2) % 2 == 0, 40, 200)
    elif name == "first-bin-60":
        p = 60 + em.plane(h, w) // 2            # bins 0..59 empty
    elif name == "dark":
        p = em.plane(h, w) % 151                # every value at or below 150
    elif name == "bright":
        p = 151 + em.plane(h, w) % 105          # every value above 150
    else:
        raise KeyError(name)
    p = np.ascontiguousarray(p, dtype=np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def clahe_ref(name, h, w, clip=2.0, grid=(4, 4)):
    r = em.clahe(content(name, h, w), clip, grid)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def equalize_ref(name, h, w):
    r = em.equalize_hist(content(name, h, w))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def colour(name, h, w):
    """a BGR image: the issue's formula image, or one whose luma is all dark / all bright"""
    if name == "formula":
        c = em.bgr(h, w)
    elif name == "textured":
        c = textured(1, h, w, 3, seed=5)[0]
    else:
        c = np.stack([content(name, h, w)] * 3, axis=-1)  # B = G = R: the luma is the plane
    c = np.ascontiguousarray(c)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def tone_ref(name, h, w):
    r = em.exposure_tone(colour(name, h, w))
    r.setflags(write=False)
    return r


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _changed(ref, src):
    return float(np.mean(ref != src))


# ---- clahe --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_clahe_formula_planes(dev, shape):
    import idn
    p, ref = content("formula", *shape), clahe_ref("formula", *shape)
    assert _changed(ref, p) > 0.5  # an identity cannot pass
    got = _np(idn.clahe(_dev(p[..., None], dev)))
    assert got.shape == (*shape, 1)
    assert np.array_equal(got[..., 0], ref)


@pytest.mark.parametrize("name,shape", [("formula", (17, 23)), ("textured", (75, 131))],
                         ids=lambda v: v if isinstance(v, str) else _sid(v))
@pytest.mark.parametrize("clip,grid", PARAMS, ids=lambda v: str(v).replace(" ", ""))
def test_clahe_grids_and_clip_limits(dev, name, shape, clip, grid):
    import idn
    p, ref = content(name, *shape), clahe_ref(name, *shape, clip, grid)
    assert _changed(ref, p) > 0.5
    got = _np(idn.clahe(_dev(p[..., None], dev), clip, grid))
    assert np.array_equal(got[..., 0], ref)


@pytest.mark.parametrize("shape", [(17, 23), (75, 131)], ids=_sid)
@pytest.mark.parametrize("name", CONTENTS)
def test_clahe_contents(dev, name, shape):
    import idn
    p, ref = content(name, *shape), clahe_ref(name, *shape)
    assert _changed(ref, p) > 0.5
    got = _np(idn.clahe(_dev(p[..., None], dev)))
    assert np.array_equal(got[..., 0], ref)


# ---- equalize_hist ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_equalize_hist_formula_planes(dev, shape):
    import idn
    p, ref = content("formula", *shape), equalize_ref("formula", *shape)
    assert _changed(ref, p) > 0.1  # the formula planes are close to equalised already
    got = _np(idn.equalize_hist(_dev(p[..., None], dev)))
    assert np.array_equal(got[..., 0], ref)


@pytest.mark.parametrize("name", CONTENTS)
def test_equalize_hist_contents(dev, name):
    import idn
    p, ref = content(name, 75, 131), equalize_ref(name, 75, 131)
    if name == "constant":
        assert np.array_equal(ref, p)  # cv2.equalizeHist returns a constant image as it is
    else:
        assert _changed(ref, p) > 0.1
    got = _np(idn.equalize_hist(_dev(p[..., None], dev)))
    assert np.array_equal(got[..., 0], ref)


@functools.lru_cache(maxsize=None)
def big_bin_plane():
    """300 x 300 with 70000 pixels of one value: a bin that a 16-bit counter cannot hold"""
    p = textured(1, 300, 300, 1, seed=2)[0, :, :, 0].copy()
    p.reshape(-1)[:70000] = 37
    assert np.bincount(p.ravel(), minlength=256).max() > 65535
    p.setflags(write=False)
    return p


def test_a_bin_above_65535(dev):
    import idn
    p = big_bin_plane()
    x = _dev(p[..., None], dev)
    for clip in (2.0, 0.0, 300.0):  # 300: clip 105468, above the bin, so its full count is scanned
        ref = em.clahe(p, clip, (1, 1))
        assert _changed(ref, p) > 0.5
        assert np.array_equal(_np(idn.clahe(x, clip, (1, 1)))[..., 0], ref), clip
    assert np.array_equal(_np(idn.equalize_hist(x))[..., 0], em.equalize_hist(p))


# ---- batching and layout ------------------------------------------------------------------------------

BATCH = ["formula", "textured", "two-levels"]


@pytest.mark.parametrize("shape", [(17, 23), (75, 131)], ids=_sid)
def test_batch_of_different_images(dev, shape):
    """per-image histograms do not mix, and an image gives the same bytes alone and in a batch"""
    import idn
    planes = np.stack([content(nm, *shape) for nm in BATCH])[..., None]
    x = _dev(planes, dev)
    got_c, got_e = _np(idn.clahe(x)), _np(idn.equalize_hist(x))
    assert got_c.shape == planes.shape
    for i, nm in enumerate(BATCH):
        assert np.array_equal(got_c[i, :, :, 0], clahe_ref(nm, *shape)), nm
        assert np.array_equal(got_e[i, :, :, 0], equalize_ref(nm, *shape)), nm
        assert np.array_equal(_np(idn.clahe(x[i])), got_c[i]), nm
        assert np.array_equal(_np(idn.equalize_hist(x[i])), got_e[i]), nm
    assert not np.array_equal(got_c[0], got_c[1])


def _padded(arr, pad, dev):
    """(tensor over arr with `pad` unused bytes behind each row, the buffer it is a view of)"""
    import torch
    n, h, w, c = arr.shape
    buf = torch.full((n, h, w * c + pad), 0xA5, dtype=torch.uint8, device=dev)
    view = buf.as_strided((n, h, w, c), (h * (w * c + pad), w * c + pad, c, 1))
    view.copy_(torch.from_numpy(np.array(arr)).to(dev))
    return view, buf


def test_padded_rows_and_out(dev):
    import torch
    import idn
    shape = (17, 23)
    planes = np.stack([content(nm, *shape) for nm in BATCH])[..., None]
    refs_c = np.stack([clahe_ref(nm, *shape) for nm in BATCH])[..., None]
    refs_e = np.stack([equalize_ref(nm, *shape) for nm in BATCH])[..., None]
    x, _ = _padded(planes, 9, dev)
    assert not x.is_contiguous()
    for op, ref in ((idn.clahe, refs_c), (idn.equalize_hist, refs_e)):
        assert np.array_equal(_np(op(x)), ref)               # padded in, compact out
        y, ybuf = _padded(np.zeros_like(planes), 9, dev)
        assert op(x, out=y) is y                             # padded in, padded out
        assert np.array_equal(_np(y), ref)
        assert bool((ybuf[:, :, shape[1]:] == 0xA5).all())   # the row padding is not written
        z = torch.empty(planes.shape, dtype=torch.uint8, device=dev)
        assert op(_dev(planes, dev), out=z) is z             # compact in, compact out
        assert np.array_equal(_np(z), ref)

    c = np.stack([colour(nm, 24, 28) for nm in ("formula", "textured")])
    refs = np.stack([tone_ref(nm, 24, 28) for nm in ("formula", "textured")])
    xc, _ = _padded(c, 5, dev)
    yc, ycbuf = _padded(np.zeros_like(c), 5, dev)
    assert idn.correct_exposure(xc, denoise=False, out=yc) is yc
    assert np.array_equal(_np(yc), refs)
    assert bool((ycbuf[:, :, 28 * 3:] == 0xA5).all())
    yuv = np.stack([em.bgr2yuv(im) for im in c])
    yy, _ = _padded(np.zeros_like(c), 5, dev)
    idn.cvt_color_yuv(xc, out=yy)
    assert np.array_equal(_np(yy), yuv)
    with pytest.raises(ValueError, match="in-place"):
        idn.clahe(x, out=x)


@pytest.mark.parametrize("so,do", [(1, 3), (3, 1), (0, 1), (3, 0)])
def test_offset_buffers(dev, so, do):
    """source and destination 1 and 3 bytes off an aligned base, guard bytes around both"""
    import idn
    shape = (17, 23)
    p = content("formula", *shape)[None, :, :, None]
    c = colour("formula", 24, 28)[None]
    for op, src, ref in ((idn.clahe, p, clahe_ref("formula", *shape)[None, :, :, None]),
                         (idn.equalize_hist, p, equalize_ref("formula", *shape)[None, :, :, None]),
                         (idn.cvt_color_yuv, c, em.bgr2yuv(c)),
                         (lambda x, out: idn.correct_exposure(x, denoise=False, out=out), c,
                          tone_ref("formula", 24, 28)[None])):
        xbuf, x = carve(src, so)
        ybuf, y = carve_out(src.shape, np.uint8, do)
        op(x, out=y)
        got = _np(y)
        untouched(ybuf, do, y.nbytes)
        untouched(xbuf, so, x.nbytes)
        assert np.array_equal(got, ref)


# ---- colour -------------------------------------------------------------------------------------------

def test_cvt_color_yuv_on_every_colour(dev):
    """all 2^24 colours as one 4096 x 4096 image, both ways"""
    import torch
    import idn
    v = torch.arange(1 << 24, dtype=torch.int32, device=dev)
    x = torch.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], dim=-1).to(torch.uint8)
    x = x.view(4096, 4096, 3)
    host = _np(x)
    for to_yuv, model in ((True, em.bgr2yuv), (False, em.yuv2bgr)):
        got = _np(idn.cvt_color_yuv(x, to_yuv=to_yuv))
        for r0 in range(0, 4096, 1024):  # the model in four slabs: int64 temporaries
            ref = model(host[r0:r0 + 1024])
            assert np.array_equal(got[r0:r0 + 1024], ref), (to_yuv, r0)
        assert _changed(got, host) > 0.5


# ---- the full chain -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", [("formula", (24, 28)), ("formula", (75, 131)),
                                        ("textured", (75, 131)), ("dark", (17, 23)),
                                        ("bright", (17, 23)), ("formula", (5, 5))],
                         ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_correct_exposure_tone_part(dev, name, shape):
    import idn
    c, ref = colour(name, *shape), tone_ref(name, *shape)
    assert _changed(ref, c) > 0.5
    got = _np(idn.correct_exposure(_dev(c, dev), denoise=False))
    assert np.array_equal(got, ref)


def test_correct_exposure_batch(dev):
    import idn
    names = ("formula", "textured", "bright")
    c = np.stack([colour(nm, 75, 131) for nm in names])
    got = _np(idn.correct_exposure(_dev(c, dev), denoise=False))
    for i, nm in enumerate(names):
        assert np.array_equal(got[i], tone_ref(nm, 75, 131)), nm


def test_correct_exposure_is_the_composition_of_the_public_ops(dev):
    import torch
    import idn
    x = _dev(np.stack([colour("formula", 24, 28), colour("textured", 24, 28)]), dev)
    yuv = idn.cvt_color_yuv(x)
    luma = yuv[..., :1].contiguous()
    luma = torch.where(luma > 150, (luma.to(torch.int32) * 17 // 20).to(torch.uint8), luma)
    luma = idn.clahe(idn.equalize_hist(idn.clahe(luma, 2.0, (4, 4))), 2.0, (4, 4))
    tone = idn.cvt_color_yuv(torch.cat([luma, yuv[..., 1:]], dim=-1), to_yuv=False)
    got = idn.correct_exposure(x, denoise=False)
    assert np.array_equal(_np(got), _np(tone))
    full = idn.correct_exposure(x)
    assert np.array_equal(_np(full), _np(idn.nl_means_colored(got, 3, 3, 7, 21)))
    assert not np.array_equal(_np(full), _np(got))
    out = torch.empty_like(x)
    assert idn.correct_exposure(x, out=out) is out
    assert np.array_equal(_np(out), _np(full))
    assert np.array_equal(_np(idn.correct_exposure(x[1])), _np(full)[1])


def test_automold_drop_in(dev):
    """ndarray in, ndarray out; a list keeps its order, same-shaped images share a batch"""
    import idn
    a, b, c = colour("formula", 24, 28), colour("formula", 17, 23), colour("textured", 24, 28)
    one = idn.automold.correct_exposure(np.array(a))
    assert isinstance(one, np.ndarray) and one.shape == a.shape and one.dtype == np.uint8
    assert np.array_equal(one, _np(idn.correct_exposure(_dev(a, dev))))
    many = idn.automold.correct_exposure([np.array(a), np.array(b), np.array(c)])
    assert isinstance(many, list) and [m.shape for m in many] == [a.shape, b.shape, c.shape]
    assert np.array_equal(many[0], one)
    assert np.array_equal(many[1], _np(idn.correct_exposure(_dev(b, dev))))
    assert np.array_equal(many[2], _np(idn.correct_exposure(_dev(c, dev))))
