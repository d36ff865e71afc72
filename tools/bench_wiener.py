#!/usr/bin/env python
"""Time idn.wiener on the workload batch (600 x 1000 x 3 textured images with idn.random_noise
Gaussian noise of standard deviation 15), one JSON line per leg:

  wiener        idn.wiener(x, k, noise, out=...)  the hand-written kernel (csrc/wiener.hip) for the
                windows 3, 5, 7, 15 and 31, the noise given (sd ** 2) and estimated (None), and the
                outputs "u8" and "f64"
  torch_wiener  the same filter from torch ops on the --torch-n sub-batch: float64 planes, the
                window sums as avg_pool2d with zero padding times n (rounded back to the integers
                they are), scipy's arithmetic after them; its bytes are checked equal to the
                kernel's on that sub-batch
  copy          idn.ops.copy_flat over the uint8 batch: the same run's copy rate

Every wiener line carries the copy-rate time of its algorithmic bytes (1 read per sample, plus 1
or 8 written) over the measured time, the last line the t(31) / t(3) ratios (the claim that the
cost does not grow with the window's area).  Each leg: warm-up calls, a synchronise and a short
settle, then every timed call between two HIP events; the line has the median, the minimum and
`iters`.  bench.py stays the project's yardstick; this script only measures the Wiener filter.

    python tools/bench_wiener.py [--n 256] [--torch-n 16] [--out profiles/wiener/bench_wiener.jsonl]
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

WINDOWS = (3, 5, 7, 15, 31)


def torch_wiener(x, k, noise):
    """scipy.signal.wiener per channel plane from torch ops (zero border), uint8 result"""
    import torch
    import torch.nn.functional as F
    n, h, w, c = x.shape
    cnt = torch.full((), float(k * k), dtype=torch.float64, device=x.device)
    p = x.permute(0, 3, 1, 2).reshape(n * c, 1, h, w).to(torch.float64)
    s1 = torch.round(F.avg_pool2d(p, k, 1, k // 2, count_include_pad=True) * cnt)
    s2 = torch.round(F.avg_pool2d(p * p, k, 1, k // 2, count_include_pad=True) * cnt)
    m = s1 / cnt
    v = s2 / cnt - m * m
    if noise is None:
        q = (cnt * s2 - s1 * s1).to(torch.int64).sum(dim=(1, 2, 3), keepdim=True)
        nz = q.to(torch.float64) / float(k * k * k * k * h * w)
    else:
        nz = torch.full((), float(noise), dtype=torch.float64, device=x.device)
    r = (p - m) * (1.0 - nz / v) + m
    r = torch.where((v == 0) | (v < nz), m, r)
    y = torch.round(r).clamp_(0, 255).to(torch.uint8)
    return y.view(n, c, h, w).permute(0, 2, 3, 1).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--torch-n", type=int, default=16, help="sub-batch of the torch leg")
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--sd", type=float, default=15.0, help="noise standard deviation, 0..255 scale")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_wiener: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_nlmeans import textured_device
    from bench_tv import time_leg

    given = a.sd * a.sd
    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=(a.sd / 255.0) ** 2, seed=7)
    k16 = min(a.n, a.torch_n)
    xs = x[:k16]
    y = torch.empty_like(x)

    rows = []

    def emit(r):
        rows.append(r)
        line = json.dumps(r)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def leg(name, n, fn, iters, warmup, **extra):
        med, lo = time_leg(fn, warmup, iters, a.settle)
        r = {"leg": name, "n": n, "h": a.h, "w": a.w, "c": 3, "sd": a.sd,
             "ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": iters,
             "ms_per_image": round(med / n, 5)}
        r.update(extra)
        return r

    cp = leg("copy", a.n, lambda: idn.ops.copy_flat(x.reshape(-1), y.reshape(-1), 1), a.iters,
             a.warmup)
    copy_gbps = 2 * x.numel() / (cp["ms_median"] * 1e6)  # read + write
    cp["GBps"] = round(copy_gbps, 1)
    emit(cp)

    med = {}
    for out in ("u8", "f64"):
        for noise in (given, None):
            for k in WINDOWS:
                r = leg("wiener", a.n, lambda: idn.wiener(x, k, noise, out=out), a.iters, a.warmup,
                        ksize=k, noise="given" if noise is not None else "estimated", out=out)
                alg_bytes = x.numel() * (1 + (1 if out == "u8" else 8))
                at_copy = alg_bytes / (copy_gbps * 1e6)
                r["algorithmic_bytes_at_copy_rate_ms"] = round(at_copy, 4)
                r["fraction_of_copy_rate"] = round(at_copy / r["ms_median"], 4)
                med[(out, r["noise"], k)] = r["ms_median"]
                emit(r)

    for noise in (given, None):
        for k in WINDOWS:
            got = idn.wiener(xs, k, noise)
            equal = bool(torch.equal(got, torch_wiener(xs, k, noise)))
            kern = leg("wiener", k16, lambda: idn.wiener(xs, k, noise), a.iters, a.warmup, ksize=k,
                       noise="given" if noise is not None else "estimated", out="u8")
            tor = leg("torch_wiener", k16, lambda: torch_wiener(xs, k, noise), a.torch_iters, 1,
                      ksize=k, noise=kern["noise"], out="u8", bytes_equal_to_kernel=equal)
            tor["torch_min_over_kernel_median"] = round(tor["ms_min"] / kern["ms_median"], 2)
            emit(kern)
            emit(tor)

    emit({"leg": "summary", "n": a.n,
          "t31_over_t3": {f"{o}/{nz}": round(med[(o, nz, 31)] / med[(o, nz, 3)], 3)
                          for o in ("u8", "f64") for nz in ("given", "estimated")},
          "copy_GBps": cp["GBps"]})
    return 0


if __name__ == "__main__":
    sys.exit(main())
