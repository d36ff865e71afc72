"""tests/golden/wiener.npz: what the real scipy.signal.wiener gives on the fixture planes (the
fixture that pins tests/wiener_model.py to the library).

Needs scipy (written with 1.15.3, recorded in the file); the test suite does not.  Planes: random
bytes of 5x7, 33x70 and 96x128 and the smooth 96x128 image of wiener_model.smooth_image();
windows 3, 5, (7, 3), 15, 31; noise None, 400.0 and 0.0: the full product, 60 cases.

  versions           the libraries' versions
  x/<plane>          the uint8 plane
  at/<plane>         int64 flat positions of the samples kept: all of a plane of at most
                     MAX_KEPT samples, else MAX_KEPT drawn without replacement plus the corners
  r/<plane>/<kh>x<kw>/<noise>   float64: scipy.signal.wiener(x.astype(float64), (kh, kw), noise)
                     at those positions (NaN where scipy divides 0 by 0)
  est/<plane>/<kh>x<kw>         float64 0-d: the noise scipy estimates, mean(lVar), restated with
                     scipy's own correlate as scipy.signal.wiener computes it

  python tests/golden/make_wiener_fixtures.py      (writes tests/golden/wiener.npz)
"""
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

MAX_KEPT = 1024
WINDOWS = (3, 5, (7, 3), 15, 31)
NOISES = (None, 400.0, 0.0)


def planes():
    import wiener_model as wm
    rng = np.random.default_rng(20240521)
    out = {f"rand{h}x{w}": rng.integers(0, 256, (h, w), dtype=np.uint8)
           for h, w in ((5, 7), (33, 70), (96, 128))}
    out["smooth96x128"] = wm.smooth_image()
    return out


def kept(shape, seed):
    size = shape[0] * shape[1]
    if size <= MAX_KEPT:
        return np.arange(size, dtype=np.int64)
    at = np.random.default_rng(seed).choice(size, MAX_KEPT, replace=False)
    corners = [0, shape[1] - 1, size - shape[1], size - 1]
    return np.unique(np.concatenate([at, corners])).astype(np.int64)


def wname(k):
    kh, kw = (k, k) if np.isscalar(k) else k
    return f"{kh}x{kw}"


def main():
    import scipy
    from scipy.signal import correlate, wiener

    out = {"versions": np.array([f"scipy {scipy.__version__}", f"numpy {np.__version__}"])}
    for i, (pname, x) in enumerate(planes().items()):
        at = kept(x.shape, i)
        out["x/" + pname] = x
        out["at/" + pname] = at
        im = x.astype(np.float64)
        for k in WINDOWS:
            kh, kw = (k, k) if np.isscalar(k) else k
            ones = np.ones((kh, kw))
            l_mean = correlate(im, ones, "same") / (kh * kw)
            l_var = correlate(im ** 2, ones, "same") / (kh * kw) - l_mean ** 2
            out[f"est/{pname}/{wname(k)}"] = np.float64(np.mean(np.ravel(l_var), axis=0))
            for nz in NOISES:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # 0 / 0 where a window is constant
                    r = wiener(im, (kh, kw), nz)
                out[f"r/{pname}/{wname(k)}/{nz}"] = np.asarray(r, np.float64).ravel()[at]
    path = HERE / "wiener.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
