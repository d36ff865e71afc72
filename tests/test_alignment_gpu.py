"""Every op on buffers that do not start at the base of an allocation, against the op's own oracle.

include/idn.h takes a u8 image pointer at any byte alignment and a float pointer at its natural
alignment; the launchers fork on pointer alignment in more than twenty places.  Here every op runs
with its input and its output carved out of a guarded allocation at a chosen byte offset
(tests/carve.py) -- product library, no knobs -- and must give

  * what the op's existing test asks of it (the same oracle or model, the same tolerance),
  * the bits of its own aligned run ((0, 0), the control), unless the case says why not, and
  * no byte written outside its outputs (carve.untouched on every output, and on the inputs).

Offsets are (source, destination) bytes.  Where the destination is float32 / float64 the odd
offsets are replaced by 4 / 8: a float pointer keeps its natural alignment.

Which case takes the fallback side of each alignment fork (read off the dispatch, not forced by
a knob):

  fork                                             fallback side taken by
  -----------------------------------------------  ------------------------------------------------
  stripe.hpp stripe_ok (src & 7, dst & 7)          test_filter[*-13x104 ..1400] at (4,4) (1,0) (0,1)
                                                   (3,5): stencil_u8_generic / median_u8_generic
  stencil_tile.hip tile_dma_ok (src & 15): the flat test_filter[gaussian*/box3-19x1008, 19x928] at
    tile's LDS-DMA fetch                           (8,8) (8,0): register fetch, `full` branch; the
                                                   DMA side itself at (0,0) (0,8)
  stencil_u8.hip idn_gaussian_blob_f32 (blob & 15) test_gaussian_blob[*] at (8,8) (0,8) (4,4) (0,4):
                                                   IDN_EUNSUPPORTED, ops.gaussian_blob then runs
                                                   blob(gaussian_blur(x))
  noise.hip flat (src & 15, out_u8 & 15)           test_random_noise_u8[*-8x16] at every offset but
                                                   (0,0): noise_elem16_kernel, noise_poisson_kernel
  noise_poisson.hip compact (src & 15)             test_random_noise_u8[poisson-8x16] at (8,*) (4,4)
                                                   (1,0) (3,5): unique_mask_kernel
  noise.hip ycc form (src & 1, out_f64 & 15)       test_noise_ycc_rejects_misaligned: IDN_EUNSUPPORTED
  noise_pattern.hip add_pattern / copy_slots (& 15) test_add_pattern, test_periodic_noise,
                                                   test_copy_slots at every offset but (0,0)
  quant.hip flat (src | dst | labels & 15)         test_quantize at every offset but (0,0,0)
  wavelet.hip wl_color_minmax flat (src & 3)       test_wavelet[db1-L2-12x20-u8, bior1.5-40x64-u8]
                                                   at src 1, 3: the per-pixel load
  wavelet.hip wl_haar_ok / min-max proxy (src & 3) test_wavelet[db1-L3-16x24-u8, db1-L2-12x20-u8] at
                                                   src 1, 3: the general fp64 chain;
                                                   test_wavelet[bior1.5-40x64-u8] at src 1, 3:
                                                   wl_color_minmax instead of the proxy
  wavelet_haar.hip wl_h3_synth<true> (out_u8 & 3)  test_wavelet[db1-L3-16x24-u8] out u8 at 1, 2
  wavelet_*.hip (out_u8 | row_stride) & 3 stores   test_wavelet[*] out u8 at 1, 2 (and every case of
                                                   odd row length at any offset)
  wavelet_stream.hip float out & 7 paired stores   test_wavelet[*] out f32 at 4, 12: every pair the
    (wl_synth_stream, wl_synth_final3)             aligned run stores whole is stored singly and the
                                                   other way round
  wavelet_stream.hip & 7 / & 15 in wl_dwt_stream   on a band in the workspace, not on a pointer of
                                                   the caller: the band's width decides
                                                   (test_wavelet[bior1.5-37x53-*]: 30-wide bands)
  jpeg_pixels.hip output pointer & 7, & 3          test_jpeg_decode_out at 4 (dword stores), 1 (bytes)
  bilateral_u8.hip output pointer & 1              test_bilateral at (0,1) (3,5)

Kernels that promise any alignment and had only seen aligned data: mse / ssim (test_metrics, the
inputs at 1 and 3), bilateral's dword loads at 3x - 1 (test_bilateral), the non-local-means
staging, the TV input read and the Lab converters (test_nl_means*, test_tv, test_cvt_color_lab).

A float result is compared with the control bit for bit except where the two runs go through
kernels that order their float operations differently; that is the db1 wavelet on shapes the fused
Haar path takes, whose u8 input at an odd address goes through the general fp64 chain instead
(test_wavelet says so per case and then holds the odd-address runs to each other).
"""
import ctypes
import functools
import math
import random

import numpy as np
import pytest

from carve import carve, carve_out, untouched
from conftest import textured

pytestmark = pytest.mark.gpu

OFFS = [(0, 0), (8, 8), (8, 0), (0, 8), (4, 4), (1, 0), (0, 1), (3, 5)]
MEANS = (102.9801, 115.9465, 122.7717)


def up(off, item):
    """the offset of a float output standing in for `off`: the next multiple of its item size"""
    return (off + item - 1) // item * item


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _lib():
    from idn import _lib
    return _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _rc(rc, what):
    from idn import _lib
    _lib.check(rc, what)


def _means():
    return (ctypes.c_double * 3)(*MEANS)


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error():
    """a HIP error (an illegal access shows up as one at the next synchronize) ends the session:
    no further kernel is launched on a device that has faulted"""
    yield
    import torch
    if not torch.cuda.is_available():
        return
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more runs: {e}", returncode=3)


class Carved:
    """the carved tensors of one run: every one is checked for stray writes at the end"""

    def __init__(self):
        self.items = []

    def src(self, arr, off):
        buf, v = carve(arr, off)
        self.items.append((buf, off, v.numel() * v.element_size()))
        return v

    def out(self, shape, dtype, off):
        buf, v = carve_out(shape, dtype, off)
        self.items.append((buf, off, v.numel() * v.element_size()))
        return v

    def check(self):
        for buf, off, nbytes in self.items:
            untouched(buf, off, nbytes)


# ---- Gaussian, box, median -------------------------------------------------------------------------

FILTER_SHAPES = [
    (2, 13, 104),   # rb 312 = 16 k + 8: pitched tile
    (2, 13, 112),   # rb 336: flat tile, not `full`: register fetch
    (1, 19, 1008),  # rb 3024: flat tile, `full`: LDS-DMA when the source is 16-byte aligned
    (2, 19, 928),   # rb 2784: the same, two images
    (1, 9, 504),    # rb 1512 = 24 k: the 5x5 median's 24-byte lanes
    (1, 41, 1400),  # rb 4200 > 3024: stripe form
    (2, 9, 11),     # rb 33: generic
]
FILTERS = ["gaussian3", "gaussian5", "box3", "median3", "median5"]


def _filter_fns(flt):
    import idn
    import oracle
    k = int(flt[-1])
    if flt.startswith("gaussian"):
        return idn.gaussian_blur, oracle.cv.gaussian_blur, k
    if flt.startswith("box"):
        return idn.blur, oracle.cv.blur, k
    return idn.median_blur, oracle.cv.median_blur, k


def _run_filter(flt, img):
    fn, ref_fn, k = _filter_fns(flt)
    ref = ref_fn(img, k)
    ctrl = None
    for so, do in OFFS:
        cv = Carved()
        x, y = cv.src(img, so), cv.out(img.shape, np.uint8, do)
        fn(x, k, out=y)
        got = _np(y)
        cv.check()
        assert np.array_equal(got, ref), (flt, (so, do), np.argwhere(got != ref)[:6])
        ctrl = got if ctrl is None else ctrl
        assert np.array_equal(got, ctrl), (flt, (so, do))
        assert np.array_equal(_np(x), img), "the source was written"


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("flt", FILTERS)
def test_filter(dev, flt, shape):
    """cv2's bytes at every offset pair: with the source at 8 mod 16 the fast paths stay (the
    stripe and median kernels and the pitched tile read from there; the flat tile fetches through
    registers instead of by LDS-DMA), at any offset that is not a multiple of 8 the per-pixel
    kernels take over.  19x1008 and 19x928 at (0, 0) are also the only aligned run of the flat
    tile's `full` LDS-DMA branch in the suite."""
    _run_filter(flt, textured(*shape, seed=sum(shape) + len(flt)))


@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("flt", ["box3", "median3", "median5"])
def test_filter_one_and_four_channels(dev, flt, c):
    """c = 1 and c = 4 (the per-pixel kernels whatever the alignment) on 2 x 9 x 16"""
    _run_filter(flt, textured(2, 9, 16, c=c, seed=c + len(flt)))


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("k", [3, 5])
def test_gaussian_blob(dev, k, shape):
    """float32(float64(GaussianBlur) - mean) bit for bit, fused where the layout allows (compact
    rows up to 3024 bytes, source at 0 mod 8, blob at 0 mod 16; 19x1008 / 19x928 at (0, 0): the
    `full` LDS-DMA branch under the blob epilogue) and in two steps elsewhere: both give the same
    table look-up of the same filtered bytes, so the control's bits hold everywhere."""
    import idn
    import oracle
    img = textured(*shape, seed=sum(shape) + k)
    ref = oracle.sk.blob_f32(list(oracle.cv.gaussian_blur(img, k)), MEANS)
    for so, do in OFFS:
        do = up(do, 4)
        cv = Carved()
        x, y = cv.src(img, so), cv.out(img.shape, np.float32, do)
        idn.ops.gaussian_blob(x, k, out=y)
        got = _np(y)
        cv.check()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (k, (so, do))


# ---- bilateral -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 12, 16), (1, 9, 11)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("case", [(9, 75.0, 75.0), (5, 30.0, 10.0)], ids=lambda c: "d%d" % c[0])
def test_bilateral(dev, case, shape):
    """test_bilateral_within_1lsb's rule (<= 1 LSB, only on a rounding boundary of the exact
    value) and the control's bytes: the kernel loads an unaligned dword per pixel at any base and
    stores u16 pairs only at even addresses."""
    import idn
    import oracle
    d, sc, ss = case
    img = textured(*shape, seed=d + int(sc))
    ref = oracle.cv.bilateral_filter(img, d, sc, ss)
    pre = oracle.cv.bilateral_prefilter_f32(img, d, sc, ss)
    frac = np.abs(pre - np.floor(pre) - 0.5)
    ctrl = None
    for so, do in OFFS:
        cv = Carved()
        x, y = cv.src(img, so), cv.out(img.shape, np.uint8, do)
        idn.bilateral_filter(x, d, sc, ss, out=y)
        got = _np(y)
        cv.check()
        diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
        assert diff.max() <= 1, (so, do)
        assert np.all(frac[diff > 0] < 1e-3), (so, do)
        ctrl = got if ctrl is None else ctrl
        assert np.array_equal(got, ctrl), (so, do)


# ---- random_noise ------------------------------------------------------------------------------------

SEED = 0xFFFFFFFF00000001
NOISE_LAYOUTS = {
    # shape, where the image ids come from
    "8x16": ((2, 8, 16, 3), {"offset": 2 ** 32 - 1}),           # 384 elements: flat when aligned
    "9x11": ((2, 9, 11, 3), {"image_ids": [7, 2 ** 40 + 5]}),   # 297 elements: never flat
}
NOISE_MODES = {
    "gaussian": ("gaussian", {"var": 1.0, "mean": 0.0}),
    "speckle": ("speckle", {"var": 1.0, "mean": 0.0}),
    "speckle-mean": ("speckle", {"var": 1.0, "mean": 0.1}),
    "s&p": ("s&p", {"amount": 0.4, "salt_vs_pepper": 0.3}),
    "poisson": ("poisson", {}),
}


def _noise_ids(shape, where):
    import philox_model as pm
    return pm.image_ids(shape[0], offset=where.get("offset", 0), ids=where.get("image_ids"))


@pytest.mark.parametrize("layout", list(NOISE_LAYOUTS))
@pytest.mark.parametrize("name", list(NOISE_MODES))
def test_random_noise_u8(dev, name, layout):
    """the u8 streams against tests/philox_model.py by the rules of test_noise_streams_gpu.py (s&p
    bit-equal, Poisson bit-equal but for a draw on a threshold, Gaussian / speckle a byte off by
    one only where the model's value is within rounding of an integer), and the control's bytes:
    the 16-byte form and the byte-gathering form share noise16_u8."""
    import idn
    import philox_model as pm
    import test_noise_streams_gpu as ns
    mode, kw = NOISE_MODES[name]
    shape, where = NOISE_LAYOUTS[layout]
    n = shape[0]
    imgs = ns.make_imgs(shape, 11)
    flat, ids = imgs.reshape(n, -1), _noise_ids(shape, where)
    ctrl = None
    for so, do in OFFS:
        cv = Carved()
        x, y = cv.src(imgs, so), cv.out(shape, np.uint8, do)
        idn.ops.random_noise(x, mode, seed=SEED, out="u8", out_u8=y, **where, **kw)
        got = _np(y).reshape(n, -1)
        cv.check()
        if ctrl is None:
            ctrl = got
            if mode == "s&p":
                m = pm.sap(flat, SEED, ids, kw["amount"], kw["salt_vs_pepper"])
                assert m["flip"].any() and m["salt"].any()
                assert np.array_equal(got, m["byte"])
            elif mode == "poisson":
                ns.check_poisson(f"alignment {layout}", got, None, pm.poisson(flat, SEED, ids))
            else:
                kind = pm.GAUSSIAN if mode == "gaussian" else pm.SPECKLE
                m = pm.gauss_u8(flat, SEED, ids, kind, kw["mean"], kw["var"])
                ns.check_u8(f"alignment {name} {layout}", got, m, flat, kind, kw["var"])
        # the model's rules hold for every run through the control's bytes
        assert np.array_equal(got, ctrl), (name, (so, do), np.argwhere(got != ctrl)[:6])


@pytest.mark.parametrize("layout", list(NOISE_LAYOUTS))
def test_random_noise_f64_output(dev, layout):
    """gaussian with both outputs through the C ABI, the float64 image at byte offsets 0 and 8:
    test_f64_stream_equals_model's bound against the model, the control's bits"""
    import philox_model as pm
    import test_noise_streams_gpu as ns
    shape, where = NOISE_LAYOUTS[layout]
    n, h, w, c = shape
    imgs = ns.make_imgs(shape, 12)
    flat, ids = imgs.reshape(n, -1), _noise_ids(shape, where)
    m = pm.gauss_f64(flat, SEED, ids, pm.GAUSSIAN, 0.25, 1.5)
    lib = _lib()
    ctrl = None
    for so, do, fo in [(0, 0, 0), (0, 0, 8), (1, 3, 8), (8, 8, 8), (4, 1, 0)]:
        cv = Carved()
        x, y8 = cv.src(imgs, so), cv.out(shape, np.uint8, do)
        y64 = cv.out(shape, np.float64, fo)
        idt = cv.src(np.asarray(ids, np.uint64).view(np.int64), 0)
        if "image_ids" in where:
            rc = lib.idn_noise_ids_u8(x.data_ptr(), y8.data_ptr(), y64.data_ptr(), n, h, w, c,
                                      w * c, 0, 0.25, 1.5, SEED, idt.data_ptr(), None, 0, _stream())
        else:
            rc = lib.idn_noise_u8(x.data_ptr(), y8.data_ptr(), y64.data_ptr(), n, h, w, c, w * c, 0,
                                  0.25, 1.5, SEED, where["offset"], None, None, 0, _stream())
        _rc(rc, "idn_noise_u8")
        u8, f64 = _np(y8).reshape(n, -1), _np(y64).reshape(n, -1)
        cv.check()
        ns.check_f64(f"alignment {layout} {(so, do, fo)}", u8, f64, m, flat, pm.GAUSSIAN, 1.5)
        ctrl = (u8, f64) if ctrl is None else ctrl
        assert np.array_equal(u8, ctrl[0]) and ns.bits_equal(f64, ctrl[1]), (so, do, fo)


def test_noise_ycc_rejects_misaligned(dev):
    """The fused float64 noise + colour range form needs a 2-byte aligned source and a 16-byte
    aligned float64 image (include/idn.h): elsewhere it answers IDN_EUNSUPPORTED, writes nothing,
    and ops.ycc_fusable sends the caller to random_noise + denoise_wavelet, which give the image
    the fused form gives at an aligned address.  Never a wrong result."""
    import idn
    import philox_model as pm
    import test_noise_streams_gpu as ns
    from idn._lib import IdnError
    shape = (2, 8, 16, 3)
    n, h, w, _ = shape
    imgs = ns.make_imgs(shape, 13)
    flat, ids = imgs.reshape(n, -1), pm.image_ids(n, offset=5)
    m = pm.gauss_f64(flat, SEED, ids, pm.GAUSSIAN, 0.0, 1.0)
    lib = _lib()
    ctrl = None
    for so, fo, ok in [(0, 0, True), (2, 16, True), (1, 0, False), (0, 8, False), (1, 8, False)]:
        cv = Carved()
        x, y64 = cv.src(imgs, so), cv.out(shape, np.float64, fo)
        keys = cv.out((n, 6), np.int64, 0)
        rc = lib.idn_noise_ycc_u8(x.data_ptr(), None, y64.data_ptr(), n, h, w, 0, 0.0, 1.0, SEED, 5,
                                  None, None, keys.data_ptr(), _stream())
        f64, kk = _np(y64).reshape(n, -1), _np(keys)
        cv.check()
        if not ok:
            assert rc == -2 and b"aligned" in lib.idn_last_error(), (so, fo, rc)
            assert np.all(f64.view(np.uint8) == 0xA5) and np.all(kk.view(np.uint8) == 0xA5)
            continue
        _rc(rc, "idn_noise_ycc_u8")
        ns.check_f64(f"ycc {(so, fo)}", (f64 * 255.0).astype(np.uint8), f64, m, flat, pm.GAUSSIAN, 1.0)
        ctrl = (f64, kk) if ctrl is None else ctrl
        assert ns.bits_equal(f64, ctrl[0]) and np.array_equal(kk, ctrl[1])
    # Python: an odd source address is not fusable, and the wrapper does not pretend otherwise
    cv = Carved()
    x = cv.src(imgs, 1)
    assert not idn.ops.ycc_fusable(x) and idn.ops.ycc_fusable(cv.src(imgs, 2))
    with pytest.raises(IdnError, match="aligned"):
        idn.ops.random_noise_ycc(x, "gaussian", var=1.0, seed=SEED, offset=5)
    plain = _np(idn.ops.random_noise(x, "gaussian", var=1.0, seed=SEED, offset=5, out="f64"))
    cv.check()
    assert ns.bits_equal(plain.reshape(n, -1), ctrl[0])


# ---- add_pattern, periodic_noise, copy_slots, noise_add -----------------------------------------------

def test_add_pattern(dev):
    """cv2.add(x, pattern) with the source, the pattern and the destination each off 16"""
    import idn
    import oracle
    shape = (3, 8, 16, 3)
    imgs = textured(*shape[:3], seed=21)
    pat = np.random.RandomState(22).randint(0, 256, size=shape[1:]).astype(np.uint8)
    ref = np.stack([oracle.sk.add_saturate(im, pat) for im in imgs])
    assert (ref == 255).any() and (ref < 255).any()
    for so, do in OFFS:
        for po in (0, 8, 1):
            cv = Carved()
            x, p, y = cv.src(imgs, so), cv.src(pat, po), cv.out(shape, np.uint8, do)
            idn.ops.add_pattern(x, p, out=y)
            got = _np(y)
            cv.check()
            assert np.array_equal(got, ref), (so, po, do)


def test_periodic_noise(dev):
    """add_periodic_noise: cv2.add of the cached sine pattern (test_periodic_noise_add's oracle)"""
    import idn
    import oracle
    shape = (3, 8, 16, 3)
    imgs = textured(*shape[:3], seed=23)
    pat = _np(idn.ops.periodic_pattern(8, 16, 3, 100.0))
    ref = np.stack([oracle.sk.add_saturate(im, pat) for im in imgs])
    for so, do in OFFS:
        cv = Carved()
        x, y = cv.src(imgs, so), cv.out(shape, np.uint8, do)
        idn.ops.periodic_noise(x, 100.0, out=y)
        got = _np(y)
        cv.check()
        assert np.array_equal(got, ref), (so, do)
    # the pattern itself written to an odd address: the same bytes
    for po in (1, 8):
        cv = Carved()
        p = cv.out(shape[1:], np.uint8, po)
        _rc(_lib().idn_periodic_pattern_u8(p.data_ptr(), 8, 16, 3, 100.0, _stream()), "pattern")
        got = _np(p)
        cv.check()
        assert np.array_equal(got, pat), po


def test_copy_slots(dev):
    """out[slots] = x[slots]; the other images of out keep their bytes"""
    import torch
    import idn
    shape = (3, 8, 16, 3)
    imgs = textured(*shape[:3], seed=24)
    slots = torch.tensor([2, 0], dtype=torch.int64, device="cuda")
    for so, do in OFFS:
        cv = Carved()
        x, y = cv.src(imgs, so), cv.out(shape, np.uint8, do)
        idn.ops.copy_slots(x, y, slots)
        got = _np(y)
        cv.check()
        assert np.array_equal(got[[0, 2]], imgs[[0, 2]]) and np.all(got[1] == 0xA5), (so, do)


def test_noise_add(dev):
    """the uniform additive noise against the model (bit-equal float64, test_uniform_add_equals_
    model) with its u8 cast, and Rayleigh against the control, source and u8 output off 16"""
    import idn
    import oracle
    import philox_model as pm
    import test_noise_streams_gpu as ns
    shape = (3, 8, 16, 3)
    n = shape[0]
    imgs = ns.make_imgs(shape, 25)
    m = pm.uniform_add(imgs.reshape(n, -1), SEED, pm.image_ids(n, offset=9), 1.7)
    ctrl = None
    for so, do in OFFS:
        cv = Carved()
        x, y, y2 = cv.src(imgs, so), cv.out(shape, np.uint8, do), cv.out(shape, np.uint8, do)
        _, f64 = idn.ops.noise_add(x, "uniform", 1.7, seed=SEED, offset=9, out="both", out_u8=y)
        _, r64 = idn.ops.noise_add(x, "rayleigh", 0.3, seed=SEED, offset=9, out="both", out_u8=y2)
        got, f64, ray, r64 = _np(y), _np(f64), _np(y2), _np(r64)
        cv.check()
        assert ns.bits_equal(f64.reshape(n, -1), m["f64"]), (so, do)
        assert np.array_equal(got, oracle.sk.to_u8(255 * f64)), (so, do)
        ctrl = (ray, r64) if ctrl is None else ctrl
        assert np.array_equal(ray, ctrl[0]) and ns.bits_equal(r64, ctrl[1]), (so, do)


# ---- quantize ------------------------------------------------------------------------------------------

def test_quantize(dev):
    """k = 4 on 2 x 8 x 16 through the C ABI with the input, the output and the labels each off
    16: the labels are the oracle's nearest-centre assignment for the centres the call returns and
    the output its palette (test_full_size_batch's check), and everything equals the control."""
    from oracle import cvlab
    n, h, w, k = 2, 8, 16, 4
    imgs = textured(n, h, w, seed=31)
    lib = _lib()
    nbytes = lib.idn_quant_workspace_size(n, k)
    ctrl = None
    for so, do, lo in [(s, d, 0) for s, d in OFFS] + [(0, 0, 8), (0, 0, 4), (0, 0, 1), (3, 5, 7)]:
        cv = Carved()
        x, y = cv.src(imgs, so), cv.out((n, h, w, 3), np.uint8, do)
        lab, cen = cv.out((n, h, w), np.uint8, lo), cv.out((n, k, 3), np.float64, 0)
        ws = cv.out((nbytes,), np.uint8, 0)
        rc = lib.idn_quant_u8(x.data_ptr(), y.data_ptr(), lab.data_ptr(), n, h, w, w * 3, k, 3, 10,
                              None, None, cen.data_ptr(), ws.data_ptr(), nbytes, _stream())
        _rc(rc, "idn_quant_u8")
        got, labels, centres = _np(y), _np(lab), _np(cen)
        cv.check()
        for i in range(n):
            ref, ref_labels, _ = cvlab.quantize_apply(imgs[i], centres[i])
            assert np.array_equal(labels[i], ref_labels), (so, do, lo, i)
            assert np.array_equal(got[i], ref), (so, do, lo, i)
        ctrl = (got, labels, centres) if ctrl is None else ctrl
        assert all(np.array_equal(a, b) for a, b in zip((got, labels, centres), ctrl)), (so, do, lo)


# ---- denoise_wavelet -------------------------------------------------------------------------------------

WAVELET_CASES = {
    # wavelet, levels, shape
    "db1-L3-16x24": ("db1", 3, (2, 16, 24)),    # the fused Haar-3 path (whole 8x8 blocks)
    "db1-L2-12x20": ("db1", 2, (2, 12, 20)),    # the fused Haar path, 2 levels
    "db1-L3-9x11": ("db1", 3, (1, 9, 11)),      # the general path
    "bior1.5-37x53": ("bior1.5", None, (2, 37, 53)),
    "bior1.5-40x64": ("bior1.5", None, (1, 40, 64)),
}


@functools.lru_cache(maxsize=None)
def _wavelet_case(name, f64):
    """(input, oracle result) of one case, computed once and shared (read-only)"""
    import oracle
    from test_oracle import make_img
    wavelet, levels, (n, h, w) = WAVELET_CASES[name]
    x = np.stack([make_img(h, w, 8 + i) for i in range(n)])
    if f64:
        x = np.clip(x / 255.0 + np.random.RandomState(0).normal(0, 0.2, x.shape), 0, 1)
    ref = np.stack([oracle.wavelet.denoise_wavelet(im, wavelet, levels) for im in x])
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def _wavelet_abi(x, y8, y32, wavelet, levels):
    """idn_wavelet_denoise_u8 on carved tensors (x uint8 or float64; y8 / y32 may be None)"""
    import torch
    import idn
    lib = _lib()
    n, h, w, _ = x.shape
    wv, lv = idn.ops.WAVELETS[wavelet], -1 if levels is None else levels
    nbytes = lib.idn_wavelet_workspace_size(n, h, w, wv, lv)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    u8 = x.dtype == torch.uint8
    rc = lib.idn_wavelet_denoise_u8(x.data_ptr() if u8 else None, None if u8 else x.data_ptr(),
                                    y8.data_ptr() if y8 is not None else None,
                                    y32.data_ptr() if y32 is not None else None, n, h, w, w * 3, wv,
                                    lv, ws.data_ptr(), nbytes, _stream())
    _rc(rc, "idn_wavelet_denoise_u8")


@pytest.mark.parametrize("kind", ["u8", "f64"])
@pytest.mark.parametrize("name", list(WAVELET_CASES))
def test_wavelet(dev, name, kind):
    """oracle.wavelet at 1e-5 with check_u8 for every source offset, every output form (u8, f32,
    both), the u8 output at 0, 1, 2, 4 and the float output at 0, 4, 8, 12, through the C ABI.

    Runs equal the control bit for bit with one exception: db1 on a u8 source where the fused Haar
    path applies (16x24 at 3 levels, 12x20 at 2).  That path loads dwords and needs the source at
    0 mod 4; at an odd address the image goes through the general path, whose fp64 chain orders
    its operations differently (tests/test_wavelet_gpu.py test_wavelet_haar_fused_matches_general
    holds the two to each other at 1e-5, not bit for bit).  Those runs keep the oracle's bound and
    are held to one another instead.  bior1.5 takes the same kernels at every address (its colour
    range is exact whichever kernel reduces it), and float64 input has no fork."""
    import oracle
    from test_wavelet_gpu import TOL, check_u8
    wavelet, levels, (n, h, w) = WAVELET_CASES[name]
    x, ref = _wavelet_case(name, kind == "f64")
    ref_u8 = oracle.sk.to_u8(255 * ref)
    fused = wavelet == "db1" and kind == "u8" and h % (1 << levels) == 0 and w % (1 << levels) == 0
    src_offs = [0, 8, 4, 1, 3] if kind == "u8" else [0, 8]
    ctrl = {}
    for so in src_offs:
        group = "odd" if fused and so % 4 else "ctrl"
        for o8, o32 in [(0, None), (1, None), (2, None), (4, None), (None, 0), (None, 4),
                        (None, 8), (None, 12), (0, 0), (1, 4), (2, 8), (4, 12)]:
            cv = Carved()
            xs = cv.src(x, so)
            y8 = cv.out((n, h, w, 3), np.uint8, o8) if o8 is not None else None
            y32 = cv.out((n, h, w, 3), np.float32, o32) if o32 is not None else None
            _wavelet_abi(xs, y8, y32, wavelet, levels)
            g8 = _np(y8) if y8 is not None else None
            g32 = _np(y32) if y32 is not None else None
            cv.check()
            what = (name, kind, so, o8, o32)
            if g32 is not None:
                assert np.abs(g32.astype(np.float64) - ref).max() <= TOL, what
                c = ctrl.setdefault((group, "f32"), g32)
                assert np.array_equal(g32.view(np.uint32), c.view(np.uint32)), what
            if g8 is not None:
                for i in range(n):
                    check_u8(g8[i], ref[i], ref_u8[i])
                c = ctrl.setdefault((group, "u8"), g8)
                assert np.array_equal(g8, c), what


# ---- non-local means, total variation ------------------------------------------------------------------

@pytest.mark.parametrize("c", [1, 3])
def test_nl_means(dev, c):
    """h = 10, template 7, search 21 on 2 x 24 x 40: tests/nlm_model.py bit for bit"""
    import idn
    import nlm_model as nm
    x = textured(2, 24, 40, c=c, seed=41 + c)
    ref = nm.nl_means_batch(x, 10.0, 7, 21)
    assert nm.changed_share(x, ref) > 0.5
    for so, do in OFFS:
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(x.shape, np.uint8, do)
        idn.nl_means(xs, 10.0, 7, 21, out=y)
        got = _np(y)
        cv.check()
        assert np.array_equal(got, ref), ((so, do), int(np.sum(got != ref)))


def test_nl_means_colored(dev):
    """tests/nlm_colored_model.py bit for bit on 1 x 24 x 40 (the Lab planes live in the
    workspace: only the converters touch the caller's pointers)"""
    import idn
    import nlm_colored_model as cm
    x = textured(1, 24, 40, seed=43)
    ref = cm.nl_means_colored_batch(x, 10.0, 10.0, 7, 21)
    for so, do in OFFS:
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(x.shape, np.uint8, do)
        idn.nl_means_colored(xs, 10.0, 10.0, 7, 21, out=y)
        got = _np(y)
        cv.check()
        assert np.array_equal(got, ref), ((so, do), int(np.sum(got != ref)))


def test_tv(dev):
    """eps = 0, 5 iterations on 2 x 9 x 11 x 3 through the C ABI, u8 and f32 outputs: within
    1e-5 of tests/tv_model.py, a byte off the model only where 255 * out is within rounding of a
    half (test_tv_gpu's check), 5 iterations everywhere, and the control's bits"""
    import tv_model as tm
    n, h, w, c = 2, 9, 11, 3
    x = tm.noisy(n, h, w, c, 3, 15)
    out, ref_iters, _ = tm.tv_chambolle(x, 0.1, 0.0, 5)
    assert np.all(ref_iters == 5)
    near = tm.near_half(out)
    lib = _lib()
    nbytes = lib.idn_tv_chambolle_workspace_size(n, h, w, c)
    ctrl = None
    for so, do in OFFS:
        fo = up(do, 4)
        cv = Carved()
        xs, y8 = cv.src(x, so), cv.out(x.shape, np.uint8, do)
        y32, its = cv.out(x.shape, np.float32, fo), cv.out((n, c), np.int32, 0)
        ws = cv.out((nbytes,), np.uint8, 0)
        rc = lib.idn_tv_chambolle_u8(xs.data_ptr(), y8.data_ptr(), y32.data_ptr(), its.data_ptr(),
                                     n, h, w, c, w * c, 0.1, 0.0, 5, ws.data_ptr(), nbytes, _stream())
        _rc(rc, "idn_tv_chambolle_u8")
        u8, f32, iters = _np(y8), _np(y32), _np(its)
        cv.check()
        assert np.array_equal(iters, ref_iters), (so, do)
        assert np.abs(f32.astype(np.float64) - out).max() <= 1e-5, (so, do)
        diff = u8.astype(np.int32) - tm.to_u8(out).astype(np.int32)
        assert np.all(diff[~near] == 0) and np.abs(diff).max() <= 1, (so, do)
        ctrl = (u8, f32) if ctrl is None else ctrl
        assert np.array_equal(u8, ctrl[0]), (so, do)
        assert np.array_equal(f32.view(np.uint32), ctrl[1].view(np.uint32)), (so, do)


# ---- metrics ---------------------------------------------------------------------------------------------

def test_metrics(dev):
    """mse (bit-equal to the integer model) and ssim win 7 (within 1e-9, tests/test_metrics_gpu.py's
    bound) on 2 x 17 x 24 x 3 with the two images at different offsets (1 and 3 among them: mse's
    16-byte buffer loads from an odd base), the float64 results at byte offset 0 or 8"""
    import metrics_model as mm
    n, h, w, c = 2, 17, 24, 3
    X, Y = mm.make_pair("noisy", (n, h, w), c)
    ref = [mm.ssim_int(a, b, 7) for a, b in zip(X, Y)]
    ssim_ref, ch_ref = np.array([r[0] for r in ref]), np.stack([r[1] for r in ref])
    mse_ref = np.array([mm.mse_int(a, b) for a, b in zip(X, Y)])
    lib = _lib()
    nb = max(lib.idn_metrics_workspace_size(n, h, w, c, 0), lib.idn_metrics_workspace_size(n, h, w, c, 7))
    ctrl = None
    for ao, bo, oo in [(0, 0, 0), (1, 3, 0), (3, 1, 8), (8, 8, 8), (8, 0, 0), (4, 4, 0), (0, 1, 8)]:
        cv = Carved()
        a, b = cv.src(X, ao), cv.src(Y, bo)
        m1, s, ch, m2 = (cv.out(shp, np.float64, oo) for shp in ((n,), (n,), (n, c), (n,)))
        ws = cv.out((nb,), np.uint8, 0)
        _rc(lib.idn_mse_u8(a.data_ptr(), b.data_ptr(), m1.data_ptr(), n, h, w, c, w * c, w * c,
                           ws.data_ptr(), nb, _stream()), "idn_mse_u8")
        _rc(lib.idn_ssim_u8(a.data_ptr(), b.data_ptr(), s.data_ptr(), ch.data_ptr(), m2.data_ptr(), n,
                            h, w, c, w * c, w * c, 7, ws.data_ptr(), nb, _stream()), "idn_ssim_u8")
        got = [_np(t) for t in (m1, s, ch, m2)]
        cv.check()
        assert np.array_equal(got[0], mse_ref) and np.array_equal(got[3], mse_ref), (ao, bo, oo)
        assert np.all(np.abs(got[1] - ssim_ref) <= 1e-9), (ao, bo, oo)
        assert np.all(np.abs(got[2] - ch_ref) <= 1e-9), (ao, bo, oo)
        ctrl = got if ctrl is None else ctrl
        assert all(np.array_equal(g, k) for g, k in zip(got, ctrl)), (ao, bo, oo)


# ---- Lab converters, shader, bloom, blob, resize, float64 Gaussian ---------------------------------------

@pytest.mark.parametrize("fn", ["idn_bgr2lab_u8", "idn_lab2bgr_u8", "idn_lbgr2lab_u8",
                                "idn_lab2lbgr_u8"])
def test_cvt_color_lab(dev, fn):
    """the four 8-bit Lab conversions bit for bit (oracle.cvlab, tests/nlm_colored_model.py)"""
    import nlm_colored_model as cm
    from oracle import cvlab
    model = {"idn_bgr2lab_u8": cvlab.bgr2lab, "idn_lab2bgr_u8": cvlab.lab2bgr,
             "idn_lbgr2lab_u8": cm.lbgr2lab, "idn_lab2lbgr_u8": cm.lab2lbgr}[fn]
    x = np.random.RandomState(51).randint(0, 256, size=(2, 9, 11, 3)).astype(np.uint8)
    ref = np.stack([model(im) for im in x])
    for so, do in OFFS:
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(x.shape, np.uint8, do)
        _rc(getattr(_lib(), fn)(xs.data_ptr(), y.data_ptr(), 2, 9, 11, 33, _stream()), fn)
        got = _np(y)
        cv.check()
        assert np.array_equal(got, ref), (so, do)


def test_shader(dev):
    """PIL's Brightness bit for bit (test_shader_bitexact's oracle)"""
    import oracle
    x = textured(2, 9, 11, seed=52)
    for factor in (3.0, 0.5):
        ref = np.stack([oracle.automold.shader(im, factor) for im in x])
        for so, do in OFFS:
            cv = Carved()
            xs, y = cv.src(x, so), cv.out(x.shape, np.uint8, do)
            _rc(_lib().idn_shader_u8(xs.data_ptr(), y.data_ptr(), 2, 9, 11, 3, 33, factor, _stream()),
                "idn_shader_u8")
            got = _np(y)
            cv.check()
            assert np.array_equal(got, ref), (factor, so, do)


def test_bloom(dev):
    """add_sun_flare at its smallest accepted height (300) against the sequential oracle under
    test_bloom_vs_sequential_oracle's rule, and the control's bytes"""
    import torch
    import oracle
    from idn import automold
    n, h, w = 1, 300, 64
    x = textured(n, h, w, seed=53)
    ref = np.stack([oracle.automold.add_sun_flare(im, random.Random(11)) for im in x])
    circ, wts = automold.sun_flare_circles(h, w, rng=random.Random(11), flare_center=(100, 100),
                                           angle=-math.pi / 4)
    circ, wts = np.ascontiguousarray(circ[None]), np.ascontiguousarray(wts[None])
    spans = torch.from_numpy(automold.span_table(max(int(circ[..., 2].max()), 1))).cuda()
    circ_t, wts_t = torch.from_numpy(circ).cuda(), torch.from_numpy(wts).cuda()
    ctrl = None
    for so, do in OFFS:
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(x.shape, np.uint8, do)
        _rc(_lib().idn_bloom_u8(xs.data_ptr(), y.data_ptr(), n, h, w, 3, w * 3, circ_t.data_ptr(),
                                wts_t.data_ptr(), circ.shape[1], spans.data_ptr(), _stream()),
            "idn_bloom_u8")
        got = _np(y)
        cv.check()
        d = np.abs(got.astype(int) - ref.astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 1e-4, ((so, do), d.max(), (d > 0).mean())
        ctrl = got if ctrl is None else ctrl
        assert np.array_equal(got, ctrl), (so, do)


@pytest.mark.parametrize("flip", [False, True])
def test_blob(dev, flip):
    """prep_im_for_blob + im_list_to_blob, zero padded or flipped, bit for bit (oracle.sk.blob_f32)"""
    import idn
    import oracle
    x = textured(2, 9, 11, seed=54)
    ref = oracle.sk.blob_f32(list(x), MEANS, flip=flip)
    if not flip:  # zero padding to a larger blob, as test_blob_bitexact has it
        ref, tight = np.zeros((2, 12, 16, 3), np.float32), ref
        ref[:, :9, :11] = tight
    for so, do in OFFS:
        do = up(do, 4)
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(ref.shape, np.float32, do)
        idn.ops.blob(xs, MEANS, out_hw=ref.shape[1:3], flip=flip, out=y)
        got = _np(y)
        cv.check()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (so, do)


def test_blob_from_f64(dev):
    """the float64 image's blob (test_blob_from_f64_bitexact's oracle), float64 in at 0 / 8,
    float32 out at 0, 4, 8, 12"""
    x = np.clip(textured(2, 9, 11, seed=55) / 255.0 +
                np.random.RandomState(55).normal(0, 0.3, (2, 9, 11, 3)), 0, 1) * 255.0
    ref = np.stack([_blob_ref(im) for im in x])
    for so, do in [(0, 0), (8, 4), (8, 8), (0, 12), (8, 0)]:
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(x.shape, np.float32, do)
        _rc(_lib().idn_blob_from_f64(xs.data_ptr(), y.data_ptr(), 2, 9, 11, 9, 11, _means(), 0,
                                     _stream()), "idn_blob_from_f64")
        got = _np(y)
        cv.check()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (so, do)


def _blob_ref(im):
    f = im.astype(np.float32, copy=True)
    f -= np.array([[MEANS]])[0]
    return f


def test_resize_linear(dev):
    """cv2.resize INTER_LINEAR on float32 (oracle.cvf.resize_linear_f32) bit for bit, up and down"""
    import oracle
    x = np.random.RandomState(56).uniform(-128, 128, size=(9, 11, 3)).astype(np.float32)
    for scale in (2.7, 0.5):
        ref = oracle.cvf.resize_linear_f32(x, scale, scale)
        oh, ow = ref.shape[:2]
        assert (oh, ow) == (int(round(9 * scale)), int(round(11 * scale)))
        for so, do in [(0, 0), (4, 4), (8, 12), (12, 8), (4, 0), (0, 4)]:
            cv = Carved()
            xs, y = cv.src(x[None], so), cv.out((1, oh, ow, 3), np.float32, do)
            _rc(_lib().idn_resize_linear_f32(xs.data_ptr(), y.data_ptr(), 1, 9, 11, 3, oh, ow, scale,
                                             scale, _stream()), "idn_resize_linear_f32")
            got = _np(y)[0]
            cv.check()
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (scale, so, do)


@pytest.mark.parametrize("k", [3, 5])
def test_gaussian_blur_f64(dev, k):
    """cv2.GaussianBlur on float64 (oracle.cvf.gaussian_blur_f64) bit for bit at 0 / 8"""
    import oracle
    x = np.clip(textured(2, 9, 11, seed=57) / 255.0 +
                np.random.RandomState(57).normal(0, 0.3, (2, 9, 11, 3)), 0, 1)
    ref = oracle.cvf.gaussian_blur_f64(x, k)
    for so, do in [(0, 0), (8, 8), (8, 0), (0, 8)]:
        cv = Carved()
        xs, y = cv.src(x, so), cv.out(x.shape, np.float64, do)
        _rc(_lib().idn_gaussian_blur_f64(xs.data_ptr(), y.data_ptr(), 2, 9, 11, 3, k, _stream()),
            "idn_gaussian_blur_f64")
        got = _np(y)
        cv.check()
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (k, so, do)


# ---- JPEG decode -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s420_q100_64x80.jpg", "s420_q75_odd_37x53.jpg"])
def test_jpeg_decode_out(dev, name):
    """a baseline file and one of odd width decoded into `out` at byte offsets 0, 1, 4, 8 (the
    8-byte, 4-byte and byte row stores of the colour kernel): the libjpeg 9d fixture's bytes"""
    from idn import ops
    from test_jpeg_gpu import JPEG, check_libjpeg9
    data = (JPEG / name).read_bytes()
    h, w, _ = ops.jpeg_info(data)
    for do in (0, 1, 4, 8):
        cv = Carved()
        y = cv.out((1, h, w, 3), np.uint8, do)
        ops.jpeg_decode([data], out=y)
        got = _np(y)[0]
        cv.check()
        check_libjpeg9(name, got)


# ---- position in the batch -----------------------------------------------------------------------------------

def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_batch_position_odd_image_size(dev):
    """n = 3 at 9 x 11: 297-byte images put images 1 and 2 at odd addresses inside an aligned
    batch.  Each image of the batch equals its own one-image run (a fresh, aligned tensor), for
    the ops that had no such test: wavelet, quantize, bilateral, blob, noise_add."""
    import idn
    from test_oracle import make_img
    imgs = np.stack([make_img(9, 11, 60 + i) for i in range(3)])
    x = _t(imgs)
    runs = {
        "bior1.5": lambda t, i: idn.ops.denoise_wavelet(t, "bior1.5", None, out="both"),
        "db1": lambda t, i: idn.ops.denoise_wavelet(t, "db1", 2, out="both"),
        "quantize": lambda t, i: idn.ops.quantize(t, 4, seed=3, offset=10 + i, return_labels=True,
                                                  return_centers=True),
        "bilateral": lambda t, i: idn.bilateral_filter(t, 5, 30.0, 10.0),
        "blob": lambda t, i: idn.ops.blob(t),
        "noise_add": lambda t, i: idn.ops.noise_add(t, "gamma", 0.05, seed=2, offset=7 + i,
                                                    out="both"),
    }
    for what, fn in runs.items():
        full = fn(x, 0)
        full = [_np(f) for f in (full if isinstance(full, tuple) else (full,))]
        for i in range(3):
            one = fn(_t(imgs[i:i + 1]), i)
            one = [_np(o) for o in (one if isinstance(one, tuple) else (one,))]
            for f, o in zip(full, one):
                assert np.array_equal(f[i].view(np.uint8), o[0].view(np.uint8)), (what, i)
