"""CPU: every refusal of the noise entry points (csrc/noise.hip, noise_poisson.hip,
noise_pattern.hip, noise_add.hip), by return code and idn_last_error() text.

All argument validation of these entry points runs before the first HIP call, so the table runs
without a device: the addresses are fake and never dereferenced (as in tests/test_abi.py), and
every row is either refused or returns at once (n == 0, or a copy onto itself).  Error text is
part of the ABI's behaviour: the expected codes and messages were recorded from the library before
noise.hip was split into units, and the shape errors of idn_noise_ids_u8 / idn_noise_slots_u8 are
reported under the name idn_noise_u8 on purpose.
"""
import itertools
from pathlib import Path

import pytest

A, B, O, R, K, IDS, SL, WS = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000,
                              0x80000)
EINVAL, EUNSUPPORTED = -1, -2
GAUSSIAN, SPECKLE, SAP, POISSON, UNIFORM, GAMMA, RAYLEIGH, BROWNIAN = range(8)


def _noise(fn, **kw):
    """idn_noise_u8 / _ids_u8 / _slots_u8 and idn_noise_add_u8 / _add_ids_u8: one valid call
    (1 x 8 x 16 x 3, compact rows) with the row's overrides"""
    d = dict(src=A, u8=B, f64=None, n=1, h=8, w=16, c=3, stride=None, kind=GAUSSIAN, p0=0.0,
             p1=0.01, seed=1, offset=0, replay=None, ids=IDS, slots=SL, ws=None, ws_bytes=0)
    if fn.startswith("idn_noise_add"):
        d.update(kind=UNIFORM, p0=0.1, p1=0.0)
    d.update(kw)
    stride = d["w"] * d["c"] if d["stride"] is None else d["stride"]
    head = (d["src"], d["u8"], d["f64"], d["n"], d["h"], d["w"], d["c"], stride, d["kind"],
            d["p0"], d["p1"], d["seed"])
    tail = (d["ws"], d["ws_bytes"], None)
    if fn in ("idn_noise_u8", "idn_noise_add_u8"):
        return fn, head + (d["offset"], d["replay"]) + tail
    if fn == "idn_noise_slots_u8":
        return fn, head + (d["ids"], d["slots"]) + tail
    return fn, head + (d["ids"],) + tail


def _ycc(**kw):
    d = dict(src=A, u8=None, f64=O, n=1, h=8, w=16, kind=GAUSSIAN, p0=0.0, p1=0.01, ids=None,
             replay=None, keys=K)
    d.update(kw)
    return "idn_noise_ycc_u8", (d["src"], d["u8"], d["f64"], d["n"], d["h"], d["w"], d["kind"],
                                d["p0"], d["p1"], 1, 0, d["ids"], d["replay"], d["keys"], None)


def _pattern(by_slots=False, **kw):
    d = dict(src=A, pat=R, dst=B, n=1, h=8, w=16, c=3, stride=None, slots=SL)
    d.update(kw)
    head = (d["src"], d["pat"], d["dst"], d["n"], d["h"], d["w"], d["c"])
    if by_slots:
        return "idn_add_pattern_slots_u8", head + (d["slots"], None)
    return "idn_add_pattern_u8", head + (d["w"] * d["c"] if d["stride"] is None else d["stride"],
                                         None)


def _periodic(pattern=R, h=8, w=16, c=3):
    return "idn_periodic_pattern_u8", (pattern, h, w, c, 0.5, None)


def _copy(src=A, dst=B, n=1, per_img=384, slots=SL):
    return "idn_copy_slots_u8", (src, dst, n, per_img, slots, None)


U8, IDSF, SLOTS, ADD, ADDIDS = ("idn_noise_u8", "idn_noise_ids_u8", "idn_noise_slots_u8",
                                "idn_noise_add_u8", "idn_noise_add_ids_u8")
BIG = 131072  # BIG x BIG x 4 = 2^36 elements: 2^32 chunks of 16

# (call, return code, idn_last_error() text; None where the call is accepted)
CASES = []


def _shape_rows(fn, name, got):
    """the shared shape check, in its order, and what wins when two rules are broken"""
    lim = "%s: at most 65535 images per call%s" % (name, " (got 65536)" if got else "")
    return [
        (_noise(fn, src=None), EINVAL, name + ": null src"),
        (_noise(fn, u8=None), EINVAL, name + ": at least one of out_u8 / out_f64 is required"),
        (_noise(fn, n=-1), EINVAL, name + ": bad shape"),
        (_noise(fn, h=0), EINVAL, name + ": bad shape"),
        (_noise(fn, w=0), EINVAL, name + ": bad shape"),
        (_noise(fn, c=0), EINVAL, name + ": bad shape"),
        (_noise(fn, c=5), EINVAL, name + ": bad shape"),
        (_noise(fn, n=65536), EINVAL, lim),
        (_noise(fn, src=None, n=65536), EINVAL, name + ": null src"),
        (_noise(fn, h=-3, n=65536), EINVAL, name + ": bad shape"),
        (_noise(fn, u8=None, f64=O, n=0), 0, None),
        (_noise(fn, n=0), 0, None),
    ]


for _fn in (U8, IDSF, SLOTS):
    CASES += _shape_rows(_fn, "idn_noise_u8", True)
    CASES += [
        (_noise(_fn, kind=-1), EINVAL, "idn_noise_u8: unknown noise kind -1"),
        (_noise(_fn, kind=UNIFORM), EINVAL, "idn_noise_u8: unknown noise kind 4"),
        (_noise(_fn, kind=POISSON, u8=A, ws=WS, ws_bytes=256), EINVAL,
         "idn_noise_u8: poisson cannot run in place"),
        (_noise(_fn, h=BIG, w=BIG, c=4), EINVAL, "idn_noise_u8: image too large"),
        (_noise(_fn, p1=-0.01), EINVAL, "idn_noise_u8: var must be >= 0"),
        (_noise(_fn, kind=SPECKLE, f64=O, p1=-1e-300), EINVAL, "idn_noise_u8: var must be >= 0"),
        (_noise(_fn, kind=SAP, p0=-0.1, p1=0.5), EINVAL,
         "idn_noise_u8: amount / salt_vs_pepper must be in [0, 1]"),
        (_noise(_fn, kind=SAP, p0=1.5, p1=0.5), EINVAL,
         "idn_noise_u8: amount / salt_vs_pepper must be in [0, 1]"),
        (_noise(_fn, kind=SAP, p0=0.05, p1=-0.5), EINVAL,
         "idn_noise_u8: amount / salt_vs_pepper must be in [0, 1]"),
        (_noise(_fn, kind=SAP, p0=0.05, p1=1.0625), EINVAL,
         "idn_noise_u8: amount / salt_vs_pepper must be in [0, 1]"),
        (_noise(_fn, kind=POISSON), EINVAL,
         "idn_noise_u8: poisson needs 256 workspace bytes (got 0)"),
        (_noise(_fn, kind=POISSON, ws=WS, ws_bytes=255), EINVAL,
         "idn_noise_u8: poisson needs 256 workspace bytes (got 255)"),
        (_noise(_fn, kind=POISSON, ws=None, ws_bytes=4096), EINVAL,
         "idn_noise_u8: poisson needs 256 workspace bytes (got 4096)"),
        (_noise(_fn, kind=POISSON, n=8, ws=WS, ws_bytes=511), EINVAL,
         "idn_noise_u8: poisson needs 512 workspace bytes (got 511)"),
    ]
for _fn in (U8, IDSF):
    CASES += [
        (_noise(_fn, stride=47), EINVAL, "idn_noise_u8: row_stride < w*c"),
        (_noise(_fn, n=65536, stride=47), EINVAL,
         "idn_noise_u8: at most 65535 images per call (got 65536)"),
    ]
CASES += [
    (_noise(IDSF, ids=None), EINVAL, "idn_noise_ids_u8: null image_ids"),
    (_noise(IDSF, ids=None, src=None), EINVAL, "idn_noise_ids_u8: null image_ids"),
    (_noise(IDSF, ids=None, n=0), 0, None),
    (_noise(SLOTS, ids=None), EINVAL, "idn_noise_slots_u8: null image_ids"),
    (_noise(SLOTS, slots=None), EINVAL, "idn_noise_slots_u8: null slots"),
    (_noise(SLOTS, ids=None, slots=None, n=0), 0, None),
    (_noise(SLOTS, stride=47), EINVAL,
     "idn_noise_slots_u8: slots need compact rows (row_stride 47 != w*c)"),
    (_noise(SLOTS, stride=64), EINVAL,
     "idn_noise_slots_u8: slots need compact rows (row_stride 64 != w*c)"),
    (_noise(SLOTS, stride=64, src=None), EINVAL,
     "idn_noise_slots_u8: slots need compact rows (row_stride 64 != w*c)"),
]

_YCC_ALIGN = ("idn_noise_ycc_u8: needs an even pixel count per image, 2-byte aligned u8 and "
              "16-byte aligned float64 buffers")
CASES += [
    (_ycc(src=None), EINVAL, "idn_noise_ycc_u8: null src / out_f64 / ycc_keys"),
    (_ycc(f64=None), EINVAL, "idn_noise_ycc_u8: null src / out_f64 / ycc_keys"),
    (_ycc(keys=None), EINVAL, "idn_noise_ycc_u8: null src / out_f64 / ycc_keys"),
    (_ycc(kind=SAP), EINVAL, "idn_noise_ycc_u8: gaussian or speckle only (got 2)"),
    (_ycc(kind=-1), EINVAL, "idn_noise_ycc_u8: gaussian or speckle only (got -1)"),
    (_ycc(n=-1), EINVAL, "idn_noise_ycc_u8: bad shape"),
    (_ycc(h=0), EINVAL, "idn_noise_ycc_u8: bad shape"),
    (_ycc(w=0), EINVAL, "idn_noise_ycc_u8: bad shape"),
    (_ycc(p1=-0.01), EINVAL, "idn_noise_ycc_u8: var must be >= 0"),
    (_ycc(kind=SPECKLE, p1=-0.01, src=A + 1), EINVAL, "idn_noise_ycc_u8: var must be >= 0"),
    (_ycc(n=0, src=A + 1), 0, None),
    (_ycc(h=3, w=3), EUNSUPPORTED, _YCC_ALIGN),
    (_ycc(src=A + 1), EUNSUPPORTED, _YCC_ALIGN),
    (_ycc(f64=O + 8), EUNSUPPORTED, _YCC_ALIGN),
    (_ycc(u8=B + 1), EUNSUPPORTED, _YCC_ALIGN),
    (_ycc(n=65536), EUNSUPPORTED, _YCC_ALIGN),
]

for _fn in (ADD, ADDIDS):
    CASES += _shape_rows(_fn, "idn_noise_add_u8", False)
    CASES += [
        (_noise(_fn, stride=47), EINVAL, "idn_noise_add_u8: row_stride < w*c"),
        (_noise(_fn, n=65536, stride=47), EINVAL,
         "idn_noise_add_u8: at most 65535 images per call"),
        (_noise(_fn, kind=POISSON), EINVAL, "idn_noise_add_u8: unknown kind 3"),
        (_noise(_fn, kind=8), EINVAL, "idn_noise_add_u8: unknown kind 8"),
        (_noise(_fn, kind=UNIFORM, p0=-0.5), EINVAL,
         "idn_noise_add_u8: uniform high must be >= 0"),
        (_noise(_fn, kind=GAMMA, p0=0.0, p1=0.1), EINVAL,
         "idn_noise_add_u8: gamma shape must be > 0, scale >= 0"),
        (_noise(_fn, kind=GAMMA, p0=1.99, p1=-0.1), EINVAL,
         "idn_noise_add_u8: gamma shape must be > 0, scale >= 0"),
        (_noise(_fn, kind=RAYLEIGH, p0=-0.5), EINVAL,
         "idn_noise_add_u8: rayleigh scale must be >= 0"),
        (_noise(_fn, kind=BROWNIAN, p0=-0.5, ws=WS, ws_bytes=64), EINVAL,
         "idn_noise_add_u8: brownian dt must be >= 0"),
        (_noise(_fn, kind=BROWNIAN, p0=0.01), EINVAL,
         "idn_noise_add_u8: brownian needs 8 workspace bytes (got 0)"),
        (_noise(_fn, kind=BROWNIAN, p0=0.01, ws=WS, ws_bytes=7), EINVAL,
         "idn_noise_add_u8: brownian needs 8 workspace bytes (got 7)"),
        (_noise(_fn, kind=BROWNIAN, p0=0.01, ws=None, ws_bytes=64), EINVAL,
         "idn_noise_add_u8: brownian needs 8 workspace bytes (got 64)"),
        (_noise(_fn, kind=BROWNIAN, p0=0.01, n=3, h=64, w=64, c=1, ws=WS, ws_bytes=16), EINVAL,
         "idn_noise_add_u8: brownian needs 24 workspace bytes (got 16)"),
    ]
CASES += [
    (_noise(ADDIDS, ids=None), EINVAL, "idn_noise_add_ids_u8: null image_ids"),
    (_noise(ADDIDS, ids=None, src=None), EINVAL, "idn_noise_add_ids_u8: null image_ids"),
    (_noise(ADDIDS, ids=None, n=0), 0, None),
]

CASES += [
    (_periodic(pattern=None), EINVAL, "idn_periodic_pattern_u8: null pattern"),
    (_periodic(h=0), EINVAL, "idn_periodic_pattern_u8: bad shape"),
    (_periodic(w=-1), EINVAL, "idn_periodic_pattern_u8: bad shape"),
    (_periodic(c=0), EINVAL, "idn_periodic_pattern_u8: bad shape"),
]
for _by in (False, True):
    CASES += [
        (_pattern(_by, src=None), EINVAL, "idn_add_pattern_u8: null pointer"),
        (_pattern(_by, pat=None), EINVAL, "idn_add_pattern_u8: null pointer"),
        (_pattern(_by, dst=None), EINVAL, "idn_add_pattern_u8: null pointer"),
        (_pattern(_by, n=-1), EINVAL, "idn_add_pattern_u8: bad shape"),
        (_pattern(_by, h=0), EINVAL, "idn_add_pattern_u8: bad shape"),
        (_pattern(_by, w=0), EINVAL, "idn_add_pattern_u8: bad shape"),
        (_pattern(_by, c=0), EINVAL, "idn_add_pattern_u8: bad shape"),
        (_pattern(_by, n=0), 0, None),
    ]
CASES += [
    (_pattern(stride=47), EINVAL, "idn_add_pattern_u8: row_stride < w*c"),
    (_pattern(True, slots=None), EINVAL, "idn_add_pattern_slots_u8: null slots"),
    (_pattern(True, slots=None, src=None), EINVAL, "idn_add_pattern_slots_u8: null slots"),
    (_pattern(True, slots=None, n=0), 0, None),
    (_copy(src=None), EINVAL, "idn_copy_slots_u8: null pointer"),
    (_copy(dst=None), EINVAL, "idn_copy_slots_u8: null pointer"),
    (_copy(slots=None), EINVAL, "idn_copy_slots_u8: null pointer"),
    (_copy(n=-1), EINVAL, "idn_copy_slots_u8: bad shape"),
    (_copy(n=65536), EINVAL, "idn_copy_slots_u8: bad shape"),
    (_copy(per_img=0), EINVAL, "idn_copy_slots_u8: bad shape"),
    (_copy(n=0, slots=None), 0, None),
    (_copy(dst=A), 0, None),
    (("idn_poisson_levels", (None, K, None)), EINVAL, "idn_poisson_levels: null pointer"),
    (("idn_poisson_levels", (K, None, None)), EINVAL, "idn_poisson_levels: null pointer"),
]

ENTRY_POINTS = {U8, IDSF, SLOTS, "idn_noise_ycc_u8", ADD, ADDIDS, "idn_periodic_pattern_u8",
                "idn_add_pattern_u8", "idn_add_pattern_slots_u8", "idn_copy_slots_u8",
                "idn_poisson_levels"}


def _lib():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def run_cases(lib):
    """[(function, arguments, return code, message or None)] of CASES on `lib`"""
    got = []
    for (fn, args), _, _ in CASES:
        rc = getattr(lib, fn)(*args)
        got.append((fn, args, rc, lib.idn_last_error().decode() if rc != 0 else None))
    return got


def test_the_table_names_every_entry_point_and_no_accepted_launch():
    assert {fn for (fn, _), _, _ in CASES} == ENTRY_POINTS
    for (fn, args), rc, msg in CASES:  # a row that is accepted must have nothing to launch
        assert rc in (EINVAL, EUNSUPPORTED) and msg or rc == 0 and msg is None, (fn, args)
        if rc == 0:
            n = args[2] if fn == "idn_copy_slots_u8" else args[3]
            assert n == 0 or (fn == "idn_copy_slots_u8" and args[0] == args[1]), (fn, args)


def test_every_refusal_keeps_its_code_and_text():
    lib = _lib()
    want = [(fn, args, rc, msg) for (fn, args), rc, msg in CASES]
    got = run_cases(lib)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, "\n".join(f"{g[0]}{g[1]}: got {g[2:]}, expected {w[2:]}" for g, w in bad)


def test_workspace_sizes():
    """idn_noise_workspace_size: 8 mask words and vals per image, rounded up to 256 bytes, for
    Poisson alone; idn_noise_add_workspace_size: one float64 per 4096-element block and image,
    for brownian alone"""
    lib = _lib()
    for kind, n in itertools.product(range(-1, 9), (-1, 0, 1, 7, 8, 255, 256, 65535, 65536)):
        want = (n * 36 + 255) // 256 * 256 if kind == POISSON and n > 0 else 0
        assert lib.idn_noise_workspace_size(kind, n) == want, (kind, n)
    for kind, n, h, w, c in itertools.product(range(3, 9), (-1, 0, 1, 3), (0, 1, 64, 100),
                                              (-1, 1, 41, 64), (0, 1, 3, 4)):
        ok = kind == BROWNIAN and n > 0 and h > 0 and w > 0 and c > 0
        want = (h * w * c + 4095) // 4096 * n * 8 if ok else 0
        assert lib.idn_noise_add_workspace_size(kind, n, h, w, c) == want, (kind, n, h, w, c)
