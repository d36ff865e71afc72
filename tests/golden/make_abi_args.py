"""tests/golden/abi_args.json: what the C entry points refuse before their first HIP call (return
code and idn_last_error() text per row of tests/test_abi_args.py) and every workspace size and
offset over that module's grids, as the library built under PACKAGE_ROOT/idn gives them.

    python tests/golden/make_abi_args.py PACKAGE_ROOT      (a checkout's image-denoising_amd)

Run it without a device: a row the library accepted would launch on the table's fake addresses.
The committed file was recorded from the library before the entry points shared csrc/abi_args.hpp;
on an unchanged library the recorder reproduces it byte for byte.
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = Path(sys.argv[1]).resolve()
    sys.path[:0] = [str(root), str(HERE.parent)]
    import test_abi_args as t
    from idn import _lib
    assert Path(_lib.__file__).resolve().is_relative_to(root), _lib.__file__
    t.FIXTURE.write_text(t.dump(_lib.load()))
    print(f"recorded {len(t.ROWS)} rows and "
          f"{sum(len(t.sizes(_lib.load(), fn, g)) for fn, g in t.SIZES)} sizes from {_lib.LIB_PATH}")
