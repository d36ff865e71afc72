"""CPU: every refusal of the stencil entry points (csrc/stencil_u8.hip), by return code and
idn_last_error() text.

All argument validation of these entry points runs before the first HIP call, so the table runs
without a device: the addresses are fake and never dereferenced (as in tests/test_noise_args.py),
and every row is either refused or returns at once (n == 0).  Error text is part of the ABI's
behaviour: tests/golden/stencil_args.json holds the code and message of every row as the library
gave them before stencil_u8.hip was split into units.

    python tests/test_stencil_args.py --record PACKAGE_ROOT

writes the fixture from the library built under PACKAGE_ROOT/idn (a checkout's
image-denoising_amd); on an unchanged library it reproduces the file byte for byte.
"""
import ctypes
import json
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
FIXTURE = HERE / "golden" / "stencil_args.json"

A, B = 0x10000, 0x20000  # 16-byte aligned; + 8 is 8-byte aligned
U8 = ("idn_gaussian_blur_u8", "idn_gaussian_blur_sigma_u8", "idn_box_blur_u8")
F64 = ("idn_gaussian_blur_f64", "idn_box_blur_f64")
BLOB = "idn_gaussian_blob_f32"
ENTRY_POINTS = set(U8) | set(F64) | {BLOB}
NAN = float("nan")

_SHAPE = [dict(src=None), dict(dst=None), dict(src=None, dst=None), dict(dst=A), dict(n=-1),
          dict(h=0), dict(w=0), dict(c=0), dict(c=5), dict(n=0), dict(n=0, src=None),
          dict(n=0, h=0)]
_STRIDE = [dict(stride=47), dict(stride=0), dict(stride=47, n=0), dict(stride=47, c=5)]

# (entry point, overrides of one valid call: 1 x 8 x 16 x 3, compact rows, ksize 3)
ROWS = []
for _fn in U8:
    ROWS += [(_fn, kw) for kw in _SHAPE + _STRIDE]
    ROWS += [(_fn, dict(ksize=k)) for k in (0, 1, 2, 4, 32, 33, -3)]
    ROWS += [(_fn, dict(ksize=4, n=0)), (_fn, dict(ksize=33, src=None)), (_fn, dict(ksize=7, n=0)),
             (_fn, dict(src=A + 8, dst=B + 8, n=0))]
ROWS += [(U8[1], dict(sigma=s, ksize=k)) for s in (-1.0, -1e-300, NAN) for k in (3, 5, 9)]
ROWS += [(U8[1], dict(sigma=NAN, ksize=4)), (U8[1], dict(sigma=-1.0, n=0)),
         (U8[1], dict(sigma=1.5, n=0)), (U8[1], dict(sigma=-1.0, src=None))]
for _fn in F64:
    ROWS += [(_fn, kw) for kw in _SHAPE]
    ROWS += [(_fn, dict(ksize=k)) for k in (0, 1, 4, 7, 33)]
    ROWS += [(_fn, dict(ksize=7, n=0)), (_fn, dict(ksize=7, src=None))]
ROWS += [(F64[1], dict(ksize=5))]
ROWS += [(BLOB, kw) for kw in _SHAPE + _STRIDE]
ROWS += [(BLOB, kw) for kw in (
    dict(mean=False), dict(mean=False, dst=None), dict(mean=False, n=0), dict(mean=False, src=None),
    dict(ksize=7), dict(ksize=31), dict(ksize=7, n=0), dict(ksize=7, c=1), dict(ksize=4),
    dict(ksize=33), dict(ksize=0), dict(ksize=1), dict(ksize=4, c=1),
    # layouts the fused kernels do not take
    dict(c=1), dict(c=4, w=758), dict(stride=56), dict(w=1016), dict(h=3), dict(h=5, ksize=5),
    dict(h=4, ksize=5), dict(dst=B + 8), dict(dst=B + 8, w=24), dict(src=A + 4), dict(w=15),
    dict(w=8))]


def row_id(fn, kw):
    return "%s(%s)" % (fn, ", ".join(f"{k}={kw[k]!r}" for k in sorted(kw)))


def call(lib, fn, kw):
    """the row's call on `lib` -> [return code, idn_last_error() text or None]"""
    d = dict(src=A, dst=B, n=1, h=8, w=16, c=3, stride=None, ksize=3, sigma=0.0, mean=True)
    d.update(kw)
    stride = d["w"] * d["c"] if d["stride"] is None else d["stride"]
    shape = (d["n"], d["h"], d["w"], d["c"])
    if fn in F64:
        args = (d["src"], d["dst"]) + shape + (d["ksize"], None)
    elif fn == BLOB:
        mean = (ctypes.c_double * 3)(102.9801, 115.9465, 122.7717) if d["mean"] else None
        args = (d["src"], d["dst"]) + shape + (stride, d["ksize"], mean, None)
    elif fn == U8[1]:
        args = (d["src"], d["dst"]) + shape + (stride, d["ksize"], d["sigma"], None)
    else:
        args = (d["src"], d["dst"]) + shape + (stride, d["ksize"], None)
    rc = getattr(lib, fn)(*args)
    return [rc, lib.idn_last_error().decode() if rc != 0 else None]


def dump(lib):
    """the fixture's text for `lib`: one row per line"""
    rows = ",\n".join(f"{json.dumps(row_id(fn, kw))}: {json.dumps(call(lib, fn, kw))}"
                      for fn, kw in ROWS)
    return "{\n" + rows + "\n}\n"


def test_the_table_names_every_entry_point_and_no_row_launches():
    assert {fn for fn, _ in ROWS} == ENTRY_POINTS
    want = json.loads(FIXTURE.read_text())
    ids = [row_id(fn, kw) for fn, kw in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(want)
    for fn, kw in ROWS:  # a row that is accepted must have nothing to launch
        rc, msg = want[row_id(fn, kw)]
        assert rc in (-1, -2) and msg or rc == 0 and msg is None and kw.get("n") == 0, (fn, kw)


def test_every_refusal_keeps_its_code_and_text():
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    want = json.loads(FIXTURE.read_text())
    bad = []
    for fn, kw in ROWS:
        got = call(lib, fn, kw)
        if got != want[row_id(fn, kw)]:
            bad.append(f"{row_id(fn, kw)}: got {got}, expected {want[row_id(fn, kw)]}")
    assert not bad, "\n".join(bad)
    assert dump(lib) == FIXTURE.read_text()


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    sys.path.insert(0, str(Path(sys.argv[2]).resolve()))
    from idn import _lib
    assert Path(_lib.__file__).resolve().is_relative_to(Path(sys.argv[2]).resolve()), _lib.__file__
    FIXTURE.write_text(dump(_lib.load()))
    print(f"recorded {len(ROWS)} rows from {_lib.LIB_PATH}")
