"""CPU: idn.estimate_sigma's definition and interface.

tests/sigma_model.py (numpy float64) is the definition of idn.estimate_sigma.  Here it is held bit
for bit to what the real skimage.restoration.estimate_sigma and pywt.dwtn gave on the inputs of
tests/sigma_cases.py (tests/golden/sigma.npz, written by tests/golden/make_sigma_fixtures.py with
skimage 0.18.3 and pywt 1.1.1), the conditions the GPU file relies on are checked on those
inputs, and the C ABI and the wrapper are checked as far as they go without a device.
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import sigma_cases as sc
import sigma_model as sm

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "sigma.npz"
CASES = sc.cases()
NAMES = [name for name, _ in CASES]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as f:
        return {k: f[k] for k in f.files}


def same_bits(a, b):
    """equal float64 bits, NaN positions compared separately"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


# ---- the model against the real libraries ---------------------------------------------------------

def test_fixture_file_covers_the_cases(gold):
    assert GOLD.stat().st_size <= 200 * 1024
    for name, x in CASES:
        assert int(gold["crc/" + name]) == sc.crc(x), f"{name}: not the array the fixture was made from"
        if x.nbytes <= sc.STORED_INPUT_BYTES:
            assert np.array_equal(gold["x/" + name], x) and gold["x/" + name].dtype == x.dtype
    assert sum(k.startswith("dd/") for k in gold) == len(sc.DD_CASES) >= 2
    shapes = {x.shape[-3:] for _, x in CASES}
    assert shapes >= set(sc.SHAPES) and any(x.ndim == 4 and x.shape[0] == 5 for _, x in CASES)
    assert {x.dtype for _, x in CASES} == {np.dtype(np.uint8), np.dtype(np.float64)}


@pytest.mark.parametrize("name,x", CASES, ids=NAMES)
def test_model_equals_skimage(gold, name, x):
    got = sm.estimate_sigma(x)
    assert got.dtype == np.float64 and same_bits(got, gold["sig/" + name]), name
    assert same_bits(sm.estimate_sigma(x, average_sigmas=True), gold["avg/" + name]), name


@pytest.mark.parametrize("name", sc.DD_CASES)
def test_model_band_equals_pywt(gold, name):
    x = dict(CASES)[name]
    ref = gold["dd/" + name]
    for ch in range(x.shape[-1]):
        dd = sm.dd_band(x[..., ch])
        assert dd.shape == ((x.shape[0] + 3) // 2, (x.shape[1] + 3) // 2)
        assert np.array_equal(dd.view(np.uint64), np.ascontiguousarray(ref[..., ch]).view(np.uint64))


def test_tap_order():
    assert sm.tap_order(5, 8) == [0, 1, 2, 3]
    assert sm.tap_order(8, 8) == [0, 1, 2, 3]
    assert sm.tap_order(9, 8) == [1, 0, 2, 3]      # even n, last output: ascending in value
    assert sm.tap_order(9, 7) == [2, 1, 0, 3]      # odd n, last output: the one that differs
    # ... and it does differ: ascending order misses pywt's bits on some odd-length column
    rs = np.random.RandomState(5)
    x = rs.randint(0, 256, (7, 64)).astype(np.float64)
    asc = sum(sm.DEC_HI[j] * x[sm._extended(9 - j, 7)] for j in range(4))
    assert np.any(asc != sm.highpass_axis0(x)[4])


def test_average_is_numpys_order():
    s = np.array([[0.1, 0.2, 0.3], [1e-30, 1.0, -1.0]])
    assert np.array_equal(sm.average(s), ((s[:, 0] + s[:, 1]) + s[:, 2]) / 3.0)
    assert np.array_equal(sm.average(s), s.mean(axis=1))
    assert np.array_equal(sm.average(s[:, :1]), s[:, 0])


# ---- what the GPU file relies on ------------------------------------------------------------------

def _planes():
    for name, x in CASES:
        xb = x if x.ndim == 4 else x[None]
        for i in range(xb.shape[0]):
            for ch in range(xb.shape[-1]):
                yield name, xb[i, :, :, ch]


def test_case_conditions():
    """counts of both parities; a median among the ~1e-31 keys of a flat region; exact zeros inside
    a nonzero image; fewer than 16 nonzero keys; a NaN channel; more keys than the kernel lists,
    with and without heavy ties on the median; an even count whose two middle keys differ in the
    first digit (the exponent) while more than 1024 keys share either one's"""
    parity, tiny, zeros_inside, few, nan, big, tied, parted = set(), 0, 0, 0, 0, 0, 0, 0
    for name, p in _planes():
        d = sm.dd_band(p).ravel()
        k = np.abs(d[d != 0.0])
        if k.size == 0:
            nan += 1
            assert np.isnan(sm.plane_sigma(p))
            continue
        parity.add(k.size % 2)
        med = np.median(k)
        tiny += 0.0 < med < 1e-25
        zeros_inside += bool(np.any(d == 0.0)) and bool(p.any())
        few += k.size < 16
        big += k.size > 1024
        ks = np.sort(k)
        tied += k.size > 1024 and np.sum(k == ks[k.size // 2]) > 1024
        ea, eb = (ks[[(k.size - 1) // 2, k.size // 2]].view(np.uint64) >> np.uint64(52)).tolist()
        digit = k.view(np.uint64) >> np.uint64(52)
        parted += ea != eb and np.sum(digit == ea) > 1024 and np.sum(digit == eb) > 1024
    assert parity == {0, 1}
    assert tiny >= 1 and zeros_inside >= 1 and few >= 1 and nan >= 1 and big >= 1 and tied >= 1
    assert parted >= 1


def test_flat_region_keys_are_not_zero():
    d = sm.dd_band(np.full((8, 8), 200, np.uint8))
    assert np.all(d != 0.0) and np.abs(d).max() < 1e-25
    assert not sm.dd_band(np.zeros((8, 8), np.uint8)).any()


def test_model_rejects_small_sides():
    for shape in ((3, 8), (8, 3)):
        with pytest.raises(ValueError):
            sm.dd_band(np.zeros(shape))


# ---- the C ABI ------------------------------------------------------------------------------------

def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


NEW = ("idn_estimate_sigma_workspace_size", "idn_estimate_sigma")


def test_abi_symbols_are_declared_exported_and_bound():
    from idn import _lib as binding
    hdr = (ROOT / "include" / "idn.h").read_text()
    m = re.search(r"#define\s+IDN_ABI_VERSION\s+(\d+)", hdr)
    assert int(m.group(1)) == 11 == binding.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib()
    assert lib.idn_abi_version() == 11
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared in idn.h"
        assert name in binding.SIGNATURES
        assert getattr(lib, name).argtypes == binding.SIGNATURES[name][1]
    assert lib.idn_estimate_sigma_workspace_size.restype is ctypes.c_size_t
    # the header's parameter lists, by count and by the kinds ctypes distinguishes
    decl = re.search(r"int\s+idn_estimate_sigma\s*\(([^)]*)\)", code).group(1).split(",")
    kinds = [ctypes.c_void_p if "*" in d else ctypes.c_int64 if "int64_t" in d
             else ctypes.c_size_t if "size_t" in d else ctypes.c_int for d in decl]
    assert kinds == binding.SIGNATURES["idn_estimate_sigma"][1]
    decl = re.search(r"size_t\s+idn_estimate_sigma_workspace_size\s*\(([^)]*)\)", code).group(1)
    assert len(decl.split(",")) == 5 == len(binding.SIGNATURES[NEW[0]][1])
    assert "idn_estimate_sigma" in hdr[hdr.index("History:"):hdr.index("#define IDN_ABI_VERSION")]


def test_abi_workspace_size():
    size = _lib().idn_estimate_sigma_workspace_size
    for bad in ((0, 8, 8, 3), (-1, 8, 8, 3), (1, 3, 8, 3), (1, 8, 3, 3), (1, 8, 8, 2), (1, 8, 8, 4),
                (1, 8, 8, 0)):
        for f64 in (0, 1):
            assert size(*bad, f64) == 0, bad
    for f64 in (0, 1):
        one = size(1, 600, 1000, 3, f64)
        assert one > 0 and one % 8 == 0
        assert size(2, 600, 1000, 3, f64) == 2 * one and size(7, 600, 1000, 3, f64) == 7 * one
        assert size(256, 600, 1000, 3, f64) < 64 << 20  # counters, not a stored band
    assert size(1, 4, 4, 1, 0) > 0


GOOD = dict(src_u8=0x1000, src_f64=None, dst=0x2000, n=1, h=8, w=8, c=3, row_stride=24, ws=0x8000,
            ws_bytes=1 << 30)
ORDER = list(GOOD)


def _call(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.idn_estimate_sigma(*[a[k] for k in ORDER], None)


BAD = [
    ("no source", -1, dict(src_u8=None)),
    ("two sources", -1, dict(src_f64=0x3000)),
    ("dst", -1, dict(dst=None)),
    ("dst misaligned", -1, dict(dst=0x2004)),
    ("src_f64 misaligned", -1, dict(src_u8=None, src_f64=0x3004)),
    ("c=2", -1, dict(c=2)),
    ("c=4", -1, dict(c=4)),
    ("h=0", -1, dict(h=0)),
    ("n<0", -1, dict(n=-1)),
    ("row_stride", -1, dict(row_stride=23)),
    ("misaligned workspace", -1, dict(ws=0x8004)),
    ("h=3", -2, dict(h=3)),
    ("w=3", -2, dict(w=3, row_stride=9)),
    ("no workspace", -4, dict(ws=None)),
    ("small workspace", -4, dict(ws_bytes=1000)),
]


@pytest.mark.parametrize("what,rc,kw", BAD, ids=[b[0] for b in BAD])
def test_abi_rejects_bad_arguments(what, rc, kw):
    """fake addresses, never dereferenced: every check runs before any HIP call"""
    lib = _lib()
    assert _call(lib, **kw) == rc, what
    assert b"idn_estimate_sigma" in lib.idn_last_error()


def test_abi_accepts_an_empty_batch():
    assert _call(_lib(), n=0, ws=None, ws_bytes=0) == 0  # nothing to do, nothing launched


# ---- the wrapper: argument errors before the device is looked at ------------------------------------

def _x(shape=(8, 8, 3), dtype="uint8"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype))


WRAPPER_BAD = [
    ("not a tensor", TypeError, lambda: np.zeros((8, 8, 3), np.uint8)),
    ("float32", TypeError, lambda: _x(dtype="float32")),
    ("int32", TypeError, lambda: _x(dtype="int32")),
    ("2-D", ValueError, lambda: _x((8, 8))),
    ("5-D", ValueError, lambda: _x((1, 1, 8, 8, 3))),
    ("two channels", ValueError, lambda: _x((8, 8, 2))),
    ("four channels f64", ValueError, lambda: _x((8, 8, 4), "float64")),
    ("cpu u8", ValueError, lambda: _x()),
    ("cpu f64", ValueError, lambda: _x(dtype="float64")),
]


@pytest.mark.parametrize("what,exc,arg", WRAPPER_BAD, ids=[b[0] for b in WRAPPER_BAD])
def test_wrapper_rejects_bad_arguments(what, exc, arg):
    import idn
    with pytest.raises(exc, match="estimate_sigma"):
        idn.estimate_sigma(arg())


def test_wrapper_is_exported():
    import idn
    assert idn.estimate_sigma is idn.ops.estimate_sigma
