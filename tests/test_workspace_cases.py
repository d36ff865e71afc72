"""CPU: the case table of the workspace contract (tests/workspace_cases.py) is complete and means
something, and the size functions it goes by behave as include/idn.h says.

  * every idn_*_workspace_size of the header has a case, and every idn.ops module that draws
    scratch is one the GPU file plants its allocator in;
  * every input recipe reproduces (its CRC), and every decoy changes the case's reference;
  * the size functions with a batch argument do not shrink as the batch grows,
    idn_estimate_sigma_workspace_size is additive, idn_noise_add_workspace_size (brownian) grows
    with the image as well, and idn_jpeg_workspace_size grows with the file list.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import workspace_cases as wc

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "idn.h"
NAMES = [c.name for c in wc.CASES]

# the idn.ops modules that hold a `_workspace`: _args defines it, the others import it
WORKSPACE_MODULES = {"_args", "color", "exposure", "metrics", "nlmeans", "noise", "restoration",
                     "wavelet"}


def workspace_modules():
    """{name: module} of the idn.ops submodules that have a `_workspace` attribute"""
    import importlib
    import pkgutil
    import idn.ops
    found = {}
    for info in pkgutil.iter_modules(idn.ops.__path__):
        mod = importlib.import_module(f"idn.ops.{info.name}")
        if hasattr(mod, "_workspace"):
            found[info.name] = mod
    return found


def header_size_functions():
    text = HEADER.read_text()
    return sorted(set(re.findall(r"\bsize_t\s+(idn_\w+_workspace_size)\s*\(", text)))


def _lib():
    from idn import _lib
    return _lib.load()


def test_every_size_function_of_the_header_has_a_case():
    names = header_size_functions()
    assert len(names) >= 13 and "idn_jpeg_workspace_size" in names
    covered = {e for c in wc.CASES for e in c.entry}
    assert covered == set(names), (sorted(set(names) - covered), sorted(covered - set(names)))
    for c in wc.CASES:   # a case without a size function says why: its scratch is the image's size
        assert c.entry or c.name.startswith("noise-filter-pipelined"), c.name


def test_the_modules_that_draw_scratch():
    found = workspace_modules()
    assert set(found) == WORKSPACE_MODULES, sorted(found)
    from idn.ops import _args
    assert all(m._workspace is _args._workspace for m in found.values())


def test_the_ring_and_the_eight_byte_cases():
    """one ring case per entry point family, and the eight ops that promise an 8-byte workspace"""
    ring = {e for c in wc.CASES if c.ring for e in c.entry}
    assert ring == set(header_size_functions())
    eight = {c.name.split("-")[0] for c in wc.CASES if c.eight}
    assert eight == {"mse", "ssim", "tv", "sigma", "equalize", "clahe", "correct", "wiener"}


@pytest.mark.parametrize("name", NAMES)
def test_input_recipe_reproduces(name):
    case = wc.BY_NAME[name]
    assert wc.crc_of(case.inputs()) == case.crc, hex(wc.crc_of(case.inputs()))


def _differs(a, b):
    if isinstance(a, dict):
        return any(_differs(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))
    if isinstance(a, (tuple, list)):
        return len(a) != len(b) or any(_differs(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a != b


@pytest.mark.parametrize("name", NAMES)
def test_decoy_changes_the_reference(name):
    case = wc.BY_NAME[name]
    real, decoy = case.inputs(), case.decoy()
    assert sorted(real) == sorted(decoy)
    if not case.host:   # the same buffers hold either
        for k in real:
            assert real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype, k
    assert _differs(case.reference(), case.decoy_reference())


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("fill", [0x00, 0xFF, None], ids=["0x00", "0xFF", "random"])
def test_the_planted_allocator_and_its_guard_check(fill, offset):
    """tests/test_workspace_gpu.py's allocator on the CPU: a request gets exactly its bytes, at
    the offset, holding the fill; a byte inside leaves the check quiet, and one byte written just
    past the end, just before the start, or at the far end of a guard fails it"""
    from test_workspace_gpu import GUARD, Planted
    nbytes = 1173
    planted = Planted(fill, offset)
    ws = planted(nbytes, "cpu")
    buf = planted.carves[0][0]
    assert planted.requests == [nbytes] and ws.numel() == nbytes and ws.is_contiguous()
    assert ws.data_ptr() == buf.data_ptr() + GUARD + offset and buf.data_ptr() % 16 == 0
    if fill is not None:
        assert bool((ws == fill).all())
    else:
        assert len(np.unique(ws.numpy())) > 200
    ws[0] = ws[nbytes - 1] = 0x5C
    planted.check()
    lo = GUARD + offset
    for at in (lo + nbytes, lo - 1, 0, buf.numel() - 1):
        kept = int(buf[at])
        buf[at] = kept ^ 1
        with pytest.raises(AssertionError, match="bytes written"):
            planted.check()
        buf[at] = kept
    planted.check()
    assert planted(0, "cpu").numel() == 0   # a request for nothing is a request for nothing
    planted.check()


SIZED = [c.name for c in wc.CASES if c.size is not None]


@pytest.mark.parametrize("name", SIZED)
def test_size_does_not_shrink_with_the_batch(name):
    """at the case's other arguments, n = 1, 2, 3 (for jpeg_decode: the case's files repeated to
    that length); a function that sizes anything is positive from n = 1 on"""
    case = wc.BY_NAME[name]
    lib = _lib()
    s = [int(case.size(lib, n)) for n in (1, 2, 3)]
    assert s[0] <= s[1] <= s[2], s
    if "idn_dct_denoise_workspace_size" in case.entry:
        assert s == [0, 0, 0]   # the header: it needs none
    else:
        assert s[0] > 0, s


@pytest.mark.parametrize("name", [n for n in SIZED if n.startswith("sigma-")])
def test_estimate_sigma_size_is_additive(name):
    case = wc.BY_NAME[name]
    lib = _lib()
    one = int(case.size(lib, 1))
    assert [int(case.size(lib, n)) for n in (2, 3, 7)] == [2 * one, 3 * one, 7 * one]


def test_brownian_size_grows_with_the_image():
    """idn_noise_add_workspace_size(brownian) is sized by n and by the image: it does not shrink
    in either, from 9 x 11 over the case's 37 x 53 to an image of several scan blocks"""
    case = wc.BY_NAME["brownian-2x37x53x3"]
    lib = _lib()
    shapes = [(9, 11), (8, 16), (37, 53), (64, 97), (130, 200)]   # h * w grows
    assert all(a[0] * a[1] < b[0] * b[1] for a, b in zip(shapes, shapes[1:]))
    for n in (1, 2, 3):
        s = [int(case.size(lib, n, hw)) for hw in shapes]
        assert s[0] > 0 and all(a <= b for a, b in zip(s, s[1:])), (n, s)
    for hw in shapes:
        s = [int(case.size(lib, n, hw)) for n in (1, 2, 3)]
        assert all(a <= b for a, b in zip(s, s[1:])), (hw, s)
