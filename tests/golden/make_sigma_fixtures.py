"""tests/golden/sigma.npz: what the real skimage.restoration.estimate_sigma and pywt.dwtn give on
the inputs of tests/sigma_cases.py (the fixtures that pin tests/sigma_model.py to the libraries).

Needs scikit-image (0.14.2 .. 0.18.3: estimate_sigma is unchanged between them) and PyWavelets;
the test suite needs neither.  Per case `name` of sigma_cases.cases():

  sig/<name>   float64 (C,) or (N, C): estimate_sigma(x[i], multichannel=True,
               average_sigmas=False) of the real skimage
  avg/<name>   float64 0-d or (N,): the same with average_sigmas=True
  crc/<name>   CRC-32 of the input's bytes (a test rebuilds the input and compares)
  x/<name>     the input itself where it is at most sigma_cases.STORED_INPUT_BYTES
  dd/<name>    for sigma_cases.DD_CASES: pywt.dwtn(x[..., c], 'db2')['dd'] per channel, stacked
               on the last axis

  python tests/golden/make_sigma_fixtures.py      (writes tests/golden/sigma.npz)
"""
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))


def main():
    import pywt
    import skimage
    from skimage.restoration import estimate_sigma

    import sigma_cases as sc

    out = {"versions": np.array([f"skimage {skimage.__version__}", f"pywt {pywt.__version__}",
                                 f"numpy {np.__version__}"])}
    for name, x in sc.cases():
        xb = x if x.ndim == 4 else x[None]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the mean of an empty slice: the NaN channel
            sig = np.array([estimate_sigma(im, multichannel=True, average_sigmas=False)
                            for im in xb], dtype=np.float64)
            avg = np.array([estimate_sigma(im, multichannel=True, average_sigmas=True)
                            for im in xb], dtype=np.float64)
        out["sig/" + name] = sig if x.ndim == 4 else sig[0]
        out["avg/" + name] = avg if x.ndim == 4 else avg[0]
        out["crc/" + name] = np.uint32(sc.crc(x))
        if x.nbytes <= sc.STORED_INPUT_BYTES:
            out["x/" + name] = x
        if name in sc.DD_CASES:
            out["dd/" + name] = np.stack([pywt.dwtn(x[..., c], "db2")["dd"]
                                          for c in range(x.shape[-1])], axis=-1)
    path = HERE / "sigma.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
