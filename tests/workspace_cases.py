"""One table of cases for the workspace contract of include/idn.h (tests/test_workspace_gpu.py,
tests/test_workspace_cases.py): every entry point that takes (workspace, ws_bytes), called through
idn.ops at the smallest shapes at which every region of its layout is used and its region sizes
round.  numpy and torch only; importable without a GPU.

A case names
  entry     the idn_*_workspace_size functions that size the scratch of its call
  make      its inputs, a dict of numpy arrays; keys that begin with "_" are parameters (given
            centres), the others images.  `crc` is the CRC-32 of the inputs in key order, recorded
            here: a test can tell that it rebuilt what the table was written for
  run       the call: a closure over a dict of device tensors (the same keys) that returns the
            outputs as a tuple of device tensors.  A `host` case (jpeg_decode) takes the numpy
            inputs themselves: its inputs are files in host memory
  ref       the reference of the outputs, from the inputs alone (CPU): the model, oracle or golden
            file the op's own GPU test compares with, not restated here
  check     the comparison of the op's own GPU test, at its tolerance: check(inputs, ref, outputs)
  size      size(lib, n): the entry point's workspace bytes at the case's arguments and a batch of n

The decoy of a case (decoy_of) has the shapes and types of its inputs and another reference: an
input buffer that holds it until the real input is copied over shows a read that ran too early.

Scratch is drawn from idn.ops._args._workspace by the ops; jpeg_decode allocates inside the op, so
its cases make the call at the C ABI as ops/jpeg.py does and draw from the same function.
"""
import hashlib
import json
import sys
import zlib
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
GOLD = HERE / "golden"
JPEG = GOLD / "jpeg"

SEED = 0xFFFFFFFF00000001   # the high word of the seed is live
OFFSET = 2 ** 32 - 1        # offset + i carries into the next counter word
TOL = 1e-5                  # tests/test_wavelet_gpu.py, tests/test_tv_gpu.py


def crc_of(inputs):
    c = 0
    for k in sorted(inputs):
        c = zlib.crc32(np.ascontiguousarray(inputs[k]).tobytes(), c)
    return c & 0xFFFFFFFF


def decoy_of(inputs):
    """every image mirrored in both directions and mapped to 3/4 of its range plus an offset of
    its own (so that two images of a pair do not keep their difference); parameters are kept"""
    out = {}
    for j, k in enumerate(sorted(inputs)):
        a = inputs[k]
        if k.startswith("_"):
            out[k] = a
            continue
        m = a[..., ::-1, ::-1, :]
        if a.dtype == np.uint8:
            d = (m.astype(np.int64) * 3 // 4 + 40 + 7 * j).astype(np.uint8)
        else:
            d = 0.0625 * (j + 1) + 0.75 * m
        d = np.ascontiguousarray(d)
        d.setflags(write=False)
        out[k] = d
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    """two output tuples (numpy arrays) agree in shape, type and every bit"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype
                                    and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class Case:
    def __init__(self, name, entry, make, run, ref, check, size, crc, eight=False, ring=False,
                 host=False, decoy=None, decoy_ref=None):
        self.name, self.entry = name, tuple(entry)
        self._make, self.run, self._ref, self.check, self.size = make, run, ref, check, size
        self.crc, self.eight, self.ring, self.host = crc, eight, ring, host
        self._decoy, self._decoy_ref = decoy, decoy_ref
        self._inputs = self._reference = None

    def inputs(self):
        """the inputs, made once and read-only"""
        if self._inputs is None:
            made = {k: np.ascontiguousarray(v) for k, v in self._make().items()}
            for v in made.values():
                v.setflags(write=False)
            self._inputs = made
        return self._inputs

    def reference(self):
        """the reference of the inputs, computed once and shared"""
        if self._reference is None:
            with np.errstate(all="ignore"):
                self._reference = self._ref(self.inputs())
        return self._reference

    def decoy(self):
        return self._decoy() if self._decoy else decoy_of(self.inputs())

    def decoy_reference(self):
        if self._decoy_ref:
            return self._decoy_ref()
        with np.errstate(all="ignore"):
            return self._ref(self.decoy())

    def __repr__(self):
        return self.name


CASES = []


def _add(*args, **kw):
    CASES.append(Case(*args, **kw))


def _flat(x):
    return x.reshape(x.shape[0], -1)


def _ids(n):
    import philox_model as pm
    return pm.image_ids(n, offset=OFFSET)


# ---- the tuned wavelets: idn_wavelet_denoise_u8 / _ycc ------------------------------------------------

def _check_wavelet(ref, u8, f32, to_u8):
    from test_wavelet_gpu import check_u8
    assert f32.shape == ref.shape and u8.shape == ref.shape
    err = float(np.abs(f32.astype(np.float64) - ref).max())
    assert err <= TOL, err
    for i in range(len(ref)):
        check_u8(u8[i], ref[i], to_u8(ref[i]))


def _tuned(name, wavelet, levels, n, h, w, crc, f64=False, ring=False):
    def make():
        from test_oracle import make_img
        x = np.stack([make_img(h, w, 8 + i) for i in range(n)])
        if f64:
            x = np.clip(x / 255.0 + np.random.RandomState(0).normal(0, 0.2, x.shape), 0, 1)
        return {"x": x}

    def run(t):
        import idn
        return idn.ops.denoise_wavelet(t["x"], wavelet, levels, out="both")

    def ref(inp):
        import oracle
        return np.stack([oracle.wavelet.denoise_wavelet(im, wavelet, levels) for im in inp["x"]])

    def check(inp, r, outs):
        import oracle
        _check_wavelet(r, outs[0], outs[1], lambda v: oracle.sk.to_u8(255 * v))

    def size(lib, m):
        import idn
        return lib.idn_wavelet_workspace_size(m, h, w, idn.ops.WAVELETS[wavelet],
                                              -1 if levels is None else levels)

    _add(name, ["idn_wavelet_workspace_size"], make, run, ref, check, size, crc, ring=ring)


_tuned("wavelet-bior1.5-37x53-n1", "bior1.5", None, 1, 37, 53, 0x31BFA7C9)
_tuned("wavelet-bior1.5-37x53-n3", "bior1.5", None, 3, 37, 53, 0x255B40B2, ring=True)
_tuned("wavelet-bior1.5-37x53-L2", "bior1.5", 2, 2, 37, 53, 0x77A8EB2D)
_tuned("wavelet-db1-L3-16x24", "db1", 3, 2, 16, 24, 0x4D7A009C, ring=True)   # fused, ns = 4
_tuned("wavelet-db1-L2-12x20", "db1", 2, 2, 12, 20, 0xD6D40A4D)
_tuned("wavelet-db1-L3-37x53", "db1", 3, 2, 37, 53, 0x77A8EB2D)      # general Haar path
_tuned("wavelet-bior1.5-37x53-f64", "bior1.5", None, 2, 37, 53, 0xC375E4C6, f64=True)

YCC_VAR = 0.01


def _ycc():
    h, w, n = 38, 53, 2   # an even pixel count (ycc_fusable), odd rows

    def make():
        from test_oracle import make_img
        return {"x": np.stack([make_img(h, w, 20 + i) for i in range(n)])}

    def run(t):
        import idn
        y64, keys = idn.ops.random_noise_ycc(t["x"], "gaussian", var=YCC_VAR, seed=SEED,
                                             offset=OFFSET)
        u8, f32 = idn.ops.denoise_wavelet(y64, "bior1.5", None, out="both", ycc_keys=keys)
        return y64, u8, f32

    def ref(inp):
        import oracle
        import philox_model as pm
        x = inp["x"]
        m = pm.gauss_f64(_flat(x), SEED, _ids(n), pm.GAUSSIAN, 0.0, YCC_VAR)
        noisy = m["f64"].reshape(x.shape)
        return m, np.stack([oracle.wavelet.denoise_wavelet(im, "bior1.5", None) for im in noisy])

    def check(inp, r, outs):
        import oracle
        import philox_model as pm
        import test_noise_streams_gpu as ns
        m, den = r
        y64 = _flat(outs[0])
        # the float64 image within the stream's 2-ulp bound of the model; the oracle's result on
        # the model's image moves by far less than TOL under such a change of its input
        ns.check_f64("ycc", (y64 * 255.0).astype(np.uint8), y64, m, _flat(inp["x"]), pm.GAUSSIAN,
                     YCC_VAR)
        _check_wavelet(den, outs[1], outs[2], lambda v: oracle.sk.to_u8(255 * v))

    def size(lib, m):
        return lib.idn_wavelet_workspace_size(m, h, w, 1, -1)

    _add("wavelet-ycc-bior1.5-38x53", ["idn_wavelet_workspace_size"], make, run, ref, check, size,
         0x0E5751C6, ring=True)


_ycc()


# ---- the general wavelet path -------------------------------------------------------------------------

def _general(name, crc, batch=None, ring=False):
    import wavelet_general_cases as wc
    if batch is None:
        case = wc.BY_NAME[name]
        kw, (h, w), c = wc.kwargs(case), case.shape, case.c
    else:
        kw, (h, w), c = dict(wavelet="db2", convert2ycbcr=False), (37, 53), 1

    def make():
        if batch is None:
            return {"x": wc.make_input(case)[None]}
        return {"x": np.stack([wc.make_u8(h, w, c, seed=s)[0] for s in batch])}

    def run(t):
        import idn
        return idn.denoise_wavelet(t["x"], out="both", **kw)

    def ref(inp):
        import wavelet_general_model as wm
        return np.stack([wm.denoise(im, **kw) for im in inp["x"]])

    def check(inp, r, outs):
        import wavelet_general_model as wm
        _check_wavelet(r, outs[0], outs[1], wm.to_u8)

    def size(lib, m):
        import idn
        lv = kw.get("levels")
        return lib.idn_wavelet_general_workspace_size(m, h, w, c, idn.ops.WAVELETS[kw["wavelet"]],
                                                      -1 if lv is None else lv)

    _add("general-" + name, ["idn_wavelet_general_workspace_size"], make, run, ref, check, size,
         crc, ring=ring)


_general("coif5_9x11_ycc", 0x86B17179)             # the filter is longer than the image
_general("sym4_64x17", 0x2179C40F, ring=True)
_general("db2_64x96_L3_plain_bayes", 0x8F828DAE)
_general("db2_9x11_c1", 0xC6B976C4)                # one plane, float64
_general("db2_37x53_c1_n4", 0xD9BF8CFF, batch=(3, 4, 5, 6))   # two pseudo-images, the second of one plane


# ---- quantize -----------------------------------------------------------------------------------------

def _quant(shape, k, given, crc, ring=False):
    n, h, w = shape

    def make():
        from conftest import textured
        inp = {"x": textured(n, h, w, seed=k)}
        if given:   # 8-bit Lab centres off the integer grid
            inp["_centers"] = np.round(np.random.RandomState(k).uniform(20, 235, (n, k, 3)), 3)
        return inp

    def run(t):
        import idn
        return idn.ops.quantize(t["x"], k, seed=3, offset=10, centers=t.get("_centers"),
                                return_labels=True, return_centers=True)

    def ref(inp):
        import quant_fit_model as qm
        from oracle import cvlab
        x = inp["x"]
        cen = inp["_centers"] if given else np.stack([qm.fit(x[i], k, 3, 10 + i)[0]
                                                      for i in range(n)])
        app = [cvlab.quantize_apply(x[i], cen[i]) for i in range(n)]
        return np.stack([a[0] for a in app]), np.stack([a[1] for a in app]), cen

    def check(inp, r, outs):
        from oracle import cvlab
        out, labels, cen = outs
        # the centres are the exact host model's (or the given ones), and the labels and the
        # palette the oracle's assignment for the centres the call returned
        assert same_bits((cen,), (np.asarray(r[2], np.float64),))
        for i in range(n):
            ro, rl, _ = cvlab.quantize_apply(inp["x"][i], cen[i])
            assert np.array_equal(labels[i], rl) and np.array_equal(out[i], ro), i
        assert np.array_equal(out, r[0]) and np.array_equal(labels, r[1])

    def size(lib, m):
        return lib.idn_quant_workspace_size(m, k)

    _add(f"quant-k{k}-{'centers' if given else 'fit'}-{h}x{w}", ["idn_quant_workspace_size"], make,
         run, ref, check, size, crc, ring=ring)


_quant((2, 37, 51), 3, False, 0xC07AA5DD)
_quant((2, 37, 51), 3, True, 0xE3A8B78D)
_quant((2, 37, 51), 10, False, 0x54E16547, ring=True)
_quant((2, 37, 51), 10, True, 0xE31B9453)
_quant((2, 64, 96), 3, False, 0x9C2ADC69)
_quant((2, 64, 96), 3, True, 0x3BB2ED22)
_quant((2, 64, 96), 10, False, 0xD658CF51)
_quant((2, 64, 96), 10, True, 0x8B920EFD)


# ---- nl_means_colored ---------------------------------------------------------------------------------

def _nlm_colored():
    hl, hc, t, s = 15.0, 15.0, 7, 21

    def make():
        from test_nlmeans_colored_gpu import _input
        return {"x": _input("tex")}

    def run(t_):
        import idn
        return (idn.nl_means_colored(t_["x"], hl, hc, t, s),)

    def ref(inp):
        import nlm_colored_model as cm
        return cm.nl_means_colored_batch(inp["x"], hl, hc, t, s)

    def check(inp, r, outs):
        assert np.array_equal(outs[0], r), int(np.sum(outs[0] != r))

    def size(lib, m):
        return lib.idn_nlmeans_colored_workspace_size(m, 40, 72)

    _add("nlm-colored-tex-2x40x72", ["idn_nlmeans_colored_workspace_size"], make, run, ref, check,
         size, 0x9158C3AA, ring=True)


_nlm_colored()


# ---- denoise_tv_chambolle -----------------------------------------------------------------------------

def _tv(name, crc, ring=False):
    import tv_cases as tc
    n, h, w, c = tc.CASES[name][:4]

    def make():
        return {"x": tc.inputs(name)}

    def run(t):
        import idn
        return idn.denoise_tv_chambolle(t["x"], tc.weight(name), out="both", return_iters=True)

    def ref(inp):
        import tv_model as tm
        if inp["x"] is tc.inputs(name):
            return tc.ref(name)[:2]
        return tm.tv_chambolle(inp["x"], tc.weight(name), tc.EPS, tc.N_ITER_MAX)[:2]

    def check(inp, r, outs):
        import tv_model as tm
        u8, f32, iters = outs
        out, ref_iters = r
        assert np.array_equal(iters, ref_iters), (iters.tolist(), ref_iters.tolist())
        assert float(np.abs(f32.astype(np.float64) - out).max()) <= TOL
        diff = u8.astype(np.int32) - tm.to_u8(out).astype(np.int32)
        assert np.all(diff[~tm.near_half(out)] == 0) and np.abs(diff).max() <= 1

    def size(lib, m):
        return lib.idn_tv_chambolle_workspace_size(m, h, w, c)

    _add("tv-" + name, ["idn_tv_chambolle_workspace_size"], make, run, ref, check, size, crc,
         eight=True, ring=ring)


_tv("tiles", 0xDE149076)
_tv("odd", 0x13DB4E2A, ring=True)


# ---- estimate_sigma -----------------------------------------------------------------------------------

def _sigma(name, f64, shape, crc, ring=False):
    h, w, c = shape

    def make():
        import sigma_cases as sc
        x = np.stack([sc.random_bytes(h, w, c), sc.half_saturated(h, w, c), sc.two_level(h, w, c)])
        return {"x": sc.as_f64(x) if f64 else x}

    def run(t):
        import idn
        return (idn.estimate_sigma(t["x"]),)

    def ref(inp):
        import sigma_model as sm
        return sm.estimate_sigma(inp["x"])

    def check(inp, r, outs):
        from test_estimate_sigma_gpu import same_bits as sigma_bits
        assert sigma_bits(outs[0], r), (outs[0], r)

    def size(lib, m):
        return lib.idn_estimate_sigma_workspace_size(m, h, w, c, int(f64))

    _add("sigma-" + name, ["idn_estimate_sigma_workspace_size"], make, run, ref, check, size, crc,
         eight=True, ring=ring)


_sigma("u8-3x33x35x3", False, (33, 35, 3), 0x852E1240, ring=True)   # the first pass lists the keys
_sigma("f64-3x64x97x1", True, (64, 97, 1), 0xAC1577EE)             # counting passes, then a list


# ---- wiener -------------------------------------------------------------------------------------------

def _wiener(border, crc, ring=False):
    ksize = (7, 3)

    def make():
        from test_wiener_gpu import image
        return {"x": np.stack([image((33, 70, 3), s) for s in range(2)])}

    def run(t):
        import idn
        r, used = idn.wiener(t["x"], ksize, None, border=border, out="f64", return_noise=True)
        return r, used, idn.wiener(t["x"], ksize, None, border=border)

    def ref(inp):
        import wiener_model as wm
        return wm.wiener(inp["x"], ksize, None, border=border, out="f64", return_noise=True)

    def check(inp, r, outs):
        import wiener_model as wm
        assert same_bits(outs[:2], (r[0], r[1]))
        assert np.array_equal(outs[2], wm.to_u8(r[0]))

    def size(lib, m):
        return lib.idn_wiener_workspace_size(m, 3)

    _add("wiener-7x3-" + border, ["idn_wiener_workspace_size"], make, run, ref, check, size, crc,
         eight=True, ring=ring)


_wiener("zero", 0xFF781DC2, ring=True)
_wiener("reflect101", 0xFF781DC2)


# ---- mse, ssim ----------------------------------------------------------------------------------------

def _metrics(op, crc):
    shape, c, win = (2, 37, 53), 3, 7

    def make():
        import metrics_model as mm
        X, Y = mm.make_pair("noisy", shape, c)
        return {"x": X, "y": Y}

    def run(t):
        import idn
        if op == "mse":
            return (idn.mse(t["x"], t["y"]),)
        ch, mse = idn.ssim(t["x"], t["y"], win, per_channel=True, return_mse=True)
        return idn.ssim(t["x"], t["y"], win), ch, mse

    def ref(inp):
        import metrics_model as mm
        pairs = list(zip(inp["x"], inp["y"]))
        mse = np.array([mm.mse_int(a, b) for a, b in pairs])
        if op == "mse":
            return (mse,)
        s = [mm.ssim_int(a, b, win) for a, b in pairs]
        return np.array([v[0] for v in s]), np.stack([v[1] for v in s]), mse

    def check(inp, r, outs):
        if op == "mse":
            assert np.array_equal(outs[0], r[0])
            return
        assert np.all(np.abs(outs[0] - r[0]) <= 1e-9) and np.all(np.abs(outs[1] - r[1]) <= 1e-9)
        assert np.array_equal(outs[2], r[2])

    def size(lib, m):
        return lib.idn_metrics_workspace_size(m, shape[1], shape[2], c, 0 if op == "mse" else win)

    _add(op + "-2x37x53x3", ["idn_metrics_workspace_size"], make, run, ref, check, size, crc,
         eight=True, ring=True)


_metrics("mse", 0x641EA57D)
_metrics("ssim", 0x641EA57D)


# ---- exposure -----------------------------------------------------------------------------------------

EXPOSURE_BATCH = ("formula", "textured", "two-levels")   # tests/test_exposure_gpu.py BATCH
CLAHE = (2.0, (3, 5))


def _histogram(op, shape, crc, ring=False):
    h, w = shape

    def make():
        from test_exposure_gpu import content
        return {"x": np.stack([content(nm, h, w) for nm in EXPOSURE_BATCH])[..., None]}

    def run(t):
        import idn
        return (idn.equalize_hist(t["x"]) if op == "equalize" else idn.clahe(t["x"], *CLAHE),)

    def ref(inp):
        import exposure_model as em
        fn = em.equalize_hist if op == "equalize" else (lambda p: em.clahe(p, *CLAHE))
        return np.stack([fn(np.ascontiguousarray(p[..., 0])) for p in inp["x"]])[..., None]

    def check(inp, r, outs):
        assert np.array_equal(outs[0], r)

    def size(lib, m):
        return lib.idn_exposure_workspace_size(m, h, w, *((1, 1) if op == "equalize" else CLAHE[1]))

    _add(f"{op}-{h}x{w}", ["idn_exposure_workspace_size"], make, run, ref, check, size, crc,
         eight=True, ring=ring)


_histogram("equalize", (17, 23), 0x93036EF8)
_histogram("equalize", (75, 131), 0xBFB83E35, ring=True)
_histogram("clahe", (17, 23), 0x93036EF8)
_histogram("clahe", (75, 131), 0xBFB83E35, ring=True)


def _correct_exposure(denoise, crc):
    h, w = 24, 28

    def make():
        from test_exposure_gpu import colour
        return {"x": np.stack([colour(nm, h, w) for nm in ("formula", "textured")])}

    def run(t):
        import idn
        return (idn.correct_exposure(t["x"], denoise=denoise),)

    def ref(inp):
        import exposure_model as em
        import nlm_colored_model as cm
        tone = np.stack([em.exposure_tone(im) for im in inp["x"]])
        return cm.nl_means_colored_batch(tone, 3.0, 3.0, 7, 21) if denoise else tone

    def check(inp, r, outs):
        assert np.array_equal(outs[0], r)

    def size(lib, m):
        return lib.idn_exposure_workspace_size(m, h, w, 4, 4)

    entry = ["idn_exposure_workspace_size"] + (["idn_nlmeans_colored_workspace_size"] if denoise
                                               else [])
    # with denoise the second workspace is nl_means_colored's, which promises no 8-byte form
    _add("correct-exposure-24x28" + ("-denoise" if denoise else ""), entry, make, run, ref, check,
         size, crc, eight=not denoise, ring=not denoise)


_correct_exposure(False, 0xE8B9342A)
_correct_exposure(True, 0xE8B9342A)


# ---- noise --------------------------------------------------------------------------------------------

def _poisson(shape, crc, ring=False):
    n, h, w, c = shape

    def make():
        import test_noise_streams_gpu as ns
        return {"x": ns.make_imgs(shape, 2)}

    def run(t):
        import idn
        return idn.ops.random_noise(t["x"], "poisson", seed=SEED, offset=OFFSET, out="both")

    def ref(inp):
        import philox_model as pm
        return pm.poisson(_flat(inp["x"]), SEED, _ids(n))

    def check(inp, r, outs):
        import test_noise_streams_gpu as ns
        kept = len(ns.POIS_EXCUSED)   # that module's own count of excused draws is not ours to spend
        try:
            ns.check_poisson("workspace " + "x".join(map(str, shape)), _flat(outs[0]),
                             _flat(outs[1]), r)
        finally:
            del ns.POIS_EXCUSED[kept:]

    def size(lib, m):
        return lib.idn_noise_workspace_size(3, m)

    _add(f"poisson-3x{h}x{w}", ["idn_noise_workspace_size"], make, run, ref, check, size, crc,
         ring=ring)


_poisson((3, 8, 16, 3), 0xE77D147E)      # 384 elements: the flat form
_poisson((3, 37, 53, 3), 0xBD0231DD, ring=True)

BROWNIAN_DT = 0.09


def _brownian():
    shape = (2, 37, 53, 3)

    def make():
        import test_noise_streams_gpu as ns
        return {"x": ns.make_imgs(shape, 8)}

    def run(t):
        import idn
        return idn.ops.noise_add(t["x"], "brownian", BROWNIAN_DT, seed=SEED, offset=OFFSET,
                                 out="both")

    def ref(inp):
        import philox_model as pm
        flat = _flat(inp["x"])
        m = pm.brownian_add(flat, SEED, _ids(shape[0]), BROWNIAN_DT)
        # the walk does not depend on the image, the bytes do: the model walk's own bytes, which
        # only tell two inputs apart (check_brownian forms the device's from the device's walk)
        noise = (255.0 * m["walk"]).astype(np.int64) & 0xFF
        return m, np.minimum(flat.astype(np.int64) + noise, 255).astype(np.uint8)

    def check(inp, r, outs):
        import test_noise_streams_gpu as ns
        ns.check_brownian("workspace", _flat(outs[0]), _flat(outs[1]), r[0], _flat(inp["x"]),
                          BROWNIAN_DT)

    def size(lib, m, hw=(37, 53)):
        return lib.idn_noise_add_workspace_size(7, m, hw[0], hw[1], 3)

    _add("brownian-2x37x53x3", ["idn_noise_add_workspace_size"], make, run, ref, check, size,
         0x04A12AC5, ring=True)


_brownian()

FILTER_VAR = 0.01


def _noise_filter():
    shape = (5, 96, 160)

    def make():
        from conftest import textured
        return {"x": textured(*shape, seed=9)}

    def run(t):
        import idn
        kw = dict(var=FILTER_VAR, seed=SEED, offset=OFFSET)
        return (idn.ops.noise_filter(t["x"], "gaussian", "gaus_blur", 5, form="pipelined", **kw),
                idn.ops.noise_filter(t["x"], "gaussian", "gaus_blur", 5, form="serial", **kw))

    def ref(inp):
        import oracle
        import philox_model as pm
        x = inp["x"]
        m = pm.gauss_u8(_flat(x), SEED, _ids(shape[0]), pm.GAUSSIAN, 0.0, FILTER_VAR)
        return np.stack([oracle.cv.gaussian_blur(im, 5) for im in m["byte"].reshape(x.shape)])

    def check(inp, r, outs):
        # the two forms give the same bytes.  Against the host: a byte of the u8 noise stream is
        # at most one off the model's (tests/test_noise_streams_gpu.py check_u8), and cv2's
        # fixed-point Gaussian, a monotone rounding of a convex combination, moves by at most one
        # when no input moves by more
        assert np.array_equal(outs[0], outs[1])
        assert np.abs(outs[0].astype(np.int32) - r.astype(np.int32)).max() <= 1

    _add("noise-filter-pipelined-5x96x160", [], make, run, ref, check, None, 0xE57C7D6D, ring=True)


_noise_filter()


# ---- denoise_dct --------------------------------------------------------------------------------------

def _dct():
    shape, sd = (33, 70, 3), 15.0

    def make():
        from dct_cases import parity_image
        return {"x": parity_image(shape, sd)}

    def run(t):
        import idn
        return idn.denoise_dct(t["x"], sd, color=True, out="both")

    def ref(inp):
        from dct_cases import parity_case, parity_image, references
        if inp["x"] is parity_image(shape, sd):
            return parity_case(shape, sd, True)[1:]
        return references(inp["x"], sd, True)

    def check(inp, r, outs):
        from test_dct_denoise_gpu import compare
        compare(outs[1], outs[0], inp["x"], *r, what="workspace")

    def size(lib, m):
        return lib.idn_dct_denoise_workspace_size(m, *shape)

    _add("dct-33x70x3", ["idn_dct_denoise_workspace_size"], make, run, ref, check, size, 0xB1C2A12F,
         ring=True)


_dct()


# ---- jpeg_decode, at the C ABI ------------------------------------------------------------------------

def _jpeg_damage():
    if str(GOLD) not in sys.path:
        sys.path.insert(0, str(GOLD))
    import jpeg_damage
    return jpeg_damage


def _jpeg_file(spec):
    """the bytes of a golden file, or of a damaged one: spec is a name or a case of jpeg_damage"""
    if isinstance(spec, str):
        return (JPEG / spec).read_bytes()
    return _jpeg_damage().damage((JPEG / spec[0]).read_bytes(), spec[1], spec[2])


def _jpeg_sha(spec):
    if isinstance(spec, str):
        return json.loads((GOLD / "jpeg9.json").read_text())["files"][spec]["sha256"]
    key = _jpeg_damage().key(spec)
    return json.loads((GOLD / "jpeg9_damaged.json").read_text())["cases"][key]["sha256"]


def jpeg_workspace_size(lib, files, flags=0):
    from idn.ops.jpeg import _file_ptrs
    bufs, ptrs, lens = _file_ptrs(files)
    return lib.idn_jpeg_workspace_size(ptrs, lens, len(bufs), flags)


def _jpeg(name, specs, decoys, crc, ring=False):
    def files_of(inp):
        return [inp[f"file{i}"].tobytes() for i in range(len(specs))]

    def make():
        return {f"file{i}": np.frombuffer(_jpeg_file(s), np.uint8) for i, s in enumerate(specs)}

    def run(inp):
        """ops.jpeg_decode's call with the scratch drawn from idn.ops._args._workspace"""
        import torch
        from idn import _lib, ops
        from idn.ops import _args
        from idn.ops.jpeg import _file_ptrs
        files = files_of(inp)
        h, w, _ = ops.jpeg_info(files[0])
        n = len(files)
        out = torch.full((n, h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
        lib = _lib.load()
        bufs, ptrs, lens = _file_ptrs(files)
        nbytes = lib.idn_jpeg_workspace_size(ptrs, lens, n, 0)
        assert nbytes > 0
        ws = _args._workspace(nbytes, out.device)
        rc = lib.idn_jpeg_decode_u8(ptrs, lens, n, out.data_ptr(), h, w, w * 3, 0, ws.data_ptr(),
                                    nbytes, _args._stream())
        _lib.check(rc, "idn_jpeg_decode_u8")
        del bufs
        return (out,)

    def ref(inp):
        return [_jpeg_sha(s) for s in specs]

    def check(inp, r, outs):
        from test_jpeg_gpu import check_damaged, check_libjpeg9
        for i, s in enumerate(specs):
            if isinstance(s, str):
                check_libjpeg9(s, outs[0][i])
            else:
                check_damaged(_jpeg_damage().key(s), outs[0][i])
            assert hashlib.sha256(np.ascontiguousarray(outs[0][i]).tobytes()).hexdigest() == r[i]

    def size(lib, m):
        files = [_jpeg_file(specs[i % len(specs)]) for i in range(m)]
        return jpeg_workspace_size(lib, files)

    def decoy():
        return {f"file{i}": np.frombuffer(_jpeg_file(s), np.uint8) for i, s in enumerate(decoys)}

    _add("jpeg-" + name, ["idn_jpeg_workspace_size"], make, run, ref, check, size, crc, ring=ring,
         host=True, decoy=decoy, decoy_ref=lambda: [_jpeg_sha(s) for s in decoys])


_jpeg("baseline+progressive-96x128", ["s444_q95_96x128.jpg", "prog_s444_q85_96x128.jpg"],
      ["prog_s444_q85_96x128.jpg", "s444_q95_96x128.jpg"], 0xEF946DC2, ring=True)
_jpeg("prog-s420-rst4-120x160", ["prog_s420_rst4_120x160.jpg"], ["s420_rstrow_120x160.jpg"],
      0x20A780CF)
_jpeg("arith-s444-96x128", ["arith_s444_96x128.jpg"], ["prog_s444_q85_96x128.jpg"],
      0xA8F9DF0B)
_jpeg("cut-s444-96x128", [("s444_q95_96x128.jpg", "cut", 0.3)], ["s444_q95_96x128.jpg"],
      0x62D1F5A7)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
