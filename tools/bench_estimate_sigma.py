#!/usr/bin/env python
"""Time idn.estimate_sigma on the workload batch (600 x 1000 x 3 textured images with
idn.random_noise Gaussian noise of standard deviation 15), one JSON line per leg:

  sigma        idn.estimate_sigma(x)  the hand-written kernels (csrc/estimate_sigma.hip): on the
                                      whole uint8 batch, on the torch leg's uint8 sub-batch, and on
                                      the float64 form (random_noise's float64 output) of --f64-n
                                      images
  torch_sigma  the same algorithm from torch ops on the sub-batch: fp64 planes, two strided fp64
               conv2d over the symmetric extension, zeros masked to +inf, a sort, the two middle
               keys
  copy         idn.ops.copy_flat over the uint8 batch: the same run's copy rate, from which the
               time of ONE read of the batch (the algorithmic 1 byte per sample) is implied

The sigma lines carry the number of image passes that find work (counted on the sub-batch by
replaying the digit selection on torch's keys; six are launched, finished planes leave at once),
the copy-rate time of one read of the batch over the measured time, and how far the sub-batch's
values are from the torch leg's.  Each leg: warm-up calls, a synchronise and a short settle, then
every timed call between two HIP events; the line has the median, the minimum and `iters`.
bench.py stays the project's yardstick; this script only measures the noise estimate.

    python tools/bench_estimate_sigma.py [--n 256] [--torch-n 16] [--f64-n 64] [--out FILE]
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

DEC_HI = (-0.48296291314453416, 0.8365163037378079, -0.2241438680420134, -0.12940952255126037)
PPF75 = 0.6744897501960817
CAP, DIGITS = 1024, ((52, 11), (41, 11), (30, 11), (19, 11), (8, 11), (0, 8))


def _highpass(p, dim):
    """decimating db2 high-pass along dim 2 or 3 of (P, 1, H, W): symmetric extension by 2 and 3"""
    import torch
    import torch.nn.functional as F
    n = p.shape[dim]
    idx = torch.tensor([1, 0] + list(range(n)) + [n - 1, n - 2, n - 3], device=p.device)
    ext = p.index_select(dim, idx)
    k = torch.tensor(DEC_HI[::-1], dtype=torch.float64, device=p.device)
    if dim == 2:
        return F.conv2d(ext, k.view(1, 1, 4, 1), stride=(2, 1))
    return F.conv2d(ext, k.view(1, 1, 1, 4), stride=(1, 2))


def torch_keys(x):
    """|dd| per plane, (N*C, K) float64, zeros included"""
    import torch
    n, h, w, c = x.shape
    p = x.permute(0, 3, 1, 2).reshape(n * c, 1, h, w).to(torch.float64)
    return _highpass(_highpass(p, 2), 3).abs().reshape(n * c, -1)


def torch_sigma(x):
    import torch
    n, c = x.shape[0], x.shape[3]
    k = torch_keys(x)
    m = (k != 0).sum(dim=1, keepdim=True)
    s = torch.sort(torch.where(k != 0, k, torch.full_like(k, float("inf"))), dim=1).values
    lo = s.gather(1, ((m - 1) // 2).clamp_(min=0))
    hi = s.gather(1, (m // 2).clamp_(max=k.shape[1] - 1))
    sig = (lo + hi) / 2.0 / PPF75
    return torch.where(m > 0, sig, torch.full_like(sig, float("nan"))).view(n, c)


def passes_with_work(keys):
    """image passes the kernel's digit selection needs for the lower median rank of each plane"""
    import torch
    out = []
    for k in keys:
        bits = k[k != 0].view(torch.int64)
        rank = (bits.numel() - 1) // 2
        cnt = keys.shape[1]  # the bound the first pass starts from
        passes = 0
        for shift, width in DIGITS:
            passes += 1
            if cnt <= CAP or bits.numel() == 0:  # this pass lists the keys: finished
                break
            digit = (bits >> shift) & ((1 << width) - 1)
            hist = torch.bincount(digit, minlength=1 << width).cumsum(0)
            b = int(torch.searchsorted(hist, torch.tensor(rank, device=hist.device), right=True))
            rank -= int(hist[b - 1]) if b else 0
            bits = bits[digit == b]
            cnt = bits.numel()
        out.append(passes)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--torch-n", type=int, default=16, help="sub-batch of the torch leg")
    ap.add_argument("--f64-n", type=int, default=64, help="images of the float64 leg")
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--sd", type=float, default=15.0, help="noise standard deviation, 0..255 scale")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_estimate_sigma: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_nlmeans import textured_device
    from bench_tv import time_leg

    var = (a.sd / 255.0) ** 2
    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=var, seed=7)
    k = min(a.n, a.torch_n)
    kf = min(a.n, a.f64_n)
    xs = x[:k]
    xf = idn.random_noise(clean[:kf], "gaussian", var=var, seed=7, out="f64")
    y = torch.empty_like(x)

    est = idn.estimate_sigma(x)
    ref = torch_sigma(xs)
    rel = float(((est[:k] - ref).abs() / ref).max())
    passes = passes_with_work(torch_keys(xs))
    estf = idn.estimate_sigma(xf) * 255.0

    legs = [
        ("sigma", "u8", a.n, lambda: idn.estimate_sigma(x), a.iters),
        ("sigma", "u8", k, lambda: idn.estimate_sigma(xs), a.iters),
        ("sigma", "f64", kf, lambda: idn.estimate_sigma(xf), a.iters),
        ("torch_sigma", "u8", k, lambda: torch_sigma(xs), a.torch_iters),
        ("copy", "u8", a.n, lambda: idn.ops.copy_flat(x.reshape(-1), y.reshape(-1), 1), a.iters),
    ]
    rows = []
    for name, dt, n, fn, iters in legs:
        med, lo = time_leg(fn, a.warmup if name != "torch_sigma" else 1, iters, a.settle)
        rows.append({"leg": name, "dtype": dt, "n": n, "h": a.h, "w": a.w, "c": 3, "sd": a.sd,
                     "ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": iters,
                     "ms_per_image": round(med / n, 5)})
    big, sub, f64, tor, cp = rows
    copy_gbps = 2 * x.numel() / (cp["ms_median"] * 1e6)  # read + write
    cp["GBps"] = round(copy_gbps, 1)
    for r, samples, width in ((big, x.numel(), 1), (sub, xs.numel(), 1), (f64, xf.numel(), 8)):
        one_read_ms = samples * width / (copy_gbps * 1e6)
        r["one_read_at_copy_rate_ms"] = round(one_read_ms, 4)
        r["fraction_of_copy_rate_for_one_read"] = round(one_read_ms / r["ms_median"], 4)
        r["image_passes_launched"] = 6
        r["image_passes_with_work_min_max_on_sub_batch"] = [min(passes), max(passes)]
    big["sigma_mean"] = round(float(est.mean()), 4)
    big["sigma_min"] = round(float(est.min()), 4)
    big["sigma_max"] = round(float(est.max()), 4)
    f64["sigma_times_255_mean"] = round(float(estf.mean()), 4)
    sub["torch_min_over_kernel_median"] = round(tor["ms_min"] / sub["ms_median"], 2)
    sub["kernel_median_below_torch_min"] = sub["ms_median"] < tor["ms_min"]
    sub["max_rel_diff_to_torch"] = rel
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
