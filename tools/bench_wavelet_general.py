#!/usr/bin/env python
"""Time idn.denoise_wavelet's general path on the workload batch (600 x 1000 x 3 uint8 textured
images with idn.random_noise Gaussian noise of standard deviation 15), one JSON line per leg:

  bior15_default       wavelet='bior1.5', every option at its default: the tuned kernels, for
                       scale (what leaving them costs)
  db2_bayes_soft_ycc   wavelet='db2', BayesShrink, soft, YCbCr, sigma estimated
  db2_bayes_soft_plain the same with convert2ycbcr=False
  coif5_plain          wavelet='coif5', BayesShrink, soft, convert2ycbcr=False
  bior15_visu          wavelet='bior1.5', VisuShrink (sigma estimated): the general path on the
                       tuned path's wavelet
  db2_plain_sigma      db2 plain with sigma = idn.estimate_sigma(x) / 255 as a device tensor: the
                       median does not run

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events; the line has the median, the minimum and `iters`.  bench.py stays the project's yardstick;
this script only measures the general wavelet path.

    python tools/bench_wavelet_general.py [--n 256] [--iters 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "image-denoising_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--sd", type=float, default=15.0, help="noise standard deviation, 0..255 scale")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_wavelet_general: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_nlmeans import textured_device
    from bench_tv import time_leg

    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=(a.sd / 255.0) ** 2, seed=7)
    del clean
    y = torch.empty_like(x)
    sig = idn.estimate_sigma(x) / 255
    legs = [
        ("bior15_default", dict(wavelet="bior1.5")),
        ("db2_bayes_soft_ycc", dict(wavelet="db2")),
        ("db2_bayes_soft_plain", dict(wavelet="db2", convert2ycbcr=False)),
        ("coif5_plain", dict(wavelet="coif5", convert2ycbcr=False)),
        ("bior15_visu", dict(wavelet="bior1.5", method="VisuShrink")),
        ("db2_plain_sigma", dict(wavelet="db2", convert2ycbcr=False, sigma=sig)),
    ]
    for name, kw in legs:
        med, lo = time_leg(lambda: idn.denoise_wavelet(x, out_u8=y, **kw), a.warmup, a.iters, a.settle)
        row = {"leg": name, "n": a.n, "h": a.h, "w": a.w, "c": 3, "sd": a.sd,
               "options": {k: v for k, v in kw.items() if k != "sigma"},
               "sigma": "device tensor" if "sigma" in kw else None,
               "ms_median": round(med, 3), "ms_min": round(lo, 3), "iters": a.iters,
               "ms_per_image": round(med / a.n, 4),
               "changed_fraction": round(float((y != x).float().mean()), 4)}
        line = json.dumps(row)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
