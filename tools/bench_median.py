#!/usr/bin/env python
"""Time idn.median_blur per window size on the workload batch (600 x 1000 x 3 uint8 textured
images), one JSON line per leg:

  median        idn.median_blur(x, k) for every k of --ks on the textured batch and again on that
                batch after idn.random_noise('s&p', amount=0.4): the content-dependence check (the
                histogram kernel's cost is meant not to depend on the data), and on the torch
                leg's sub-batch of the s&p batch
  torch_median  the same filter from torch ops on the sub-batch: replicate pad (index gather),
                unfold over the window, kthvalue of rank k*k // 2 + 1; 16 images for k <= 9, fewer
                above so that the k*k expansion fits in memory
  copy          idn.ops.copy_flat over the batch: the same-run ceiling

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events on the launch stream; the line carries the median, the minimum and its `n`.  The kernel's
line on the sub-batch also says whether its bytes equal the torch leg's and whether its median
lies below the torch leg's minimum.  bench.py stays the project's yardstick; this script only
measures the median filter.

    python tools/bench_median.py [--n 256] [--ks 3,5,7,...] [--no-torch] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "image-denoising_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

KS = (3, 5, 7, 9, 11, 15, 17, 21, 31)


def torch_sub_n(k, cap):
    return min(cap, 16 if k <= 9 else 4 if k <= 15 else 2 if k <= 21 else 1)


def torch_median(x, k):
    """cv2.medianBlur(x, k) of a (N,H,W,C) uint8 batch from torch ops"""
    import torch
    n, h, w, c = x.shape
    r = k // 2
    iy = torch.arange(-r, h + r, device=x.device).clamp_(0, h - 1)
    ix = torch.arange(-r, w + r, device=x.device).clamp_(0, w - 1)
    xp = x[:, iy][:, :, ix]                                      # BORDER_REPLICATE
    win = xp.unfold(1, k, 1).unfold(2, k, 1).reshape(n, h, w, c, k * k)
    return torch.kthvalue(win, k * k // 2 + 1, dim=-1).values


def time_leg(fn, warmup, iters, settle):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    time.sleep(settle)
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--torch-n", type=int, default=16, help="largest sub-batch of the torch leg")
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--ks", type=str, default=",".join(map(str, KS)))
    ap.add_argument("--amount", type=float, default=0.4, help="s&p amount of the second batch")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch leg and its sub-batch")
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_median: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_nlmeans import textured_device

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    ks = [int(s) for s in a.ks.split(",") if s]
    clean = textured_device(a.n, a.h, a.w, 3)
    sap = idn.random_noise(clean, "s&p", amount=a.amount, seed=7)
    y = torch.empty_like(clean)
    shape = {"h": a.h, "w": a.w, "c": 3}

    for k in ks:
        per_batch = {}
        for name, x in (("textured", clean), ("sap%g" % a.amount, sap)):
            med, lo = time_leg(lambda: idn.median_blur(x, k, out=y), a.warmup, a.iters, a.settle)
            per_batch[name] = (med, lo)
            row = {"leg": "median", "k": k, "batch": name, "n": a.n, **shape,
                   "ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": a.iters,
                   "ns_per_output_byte": round(med * 1e6 / x.numel(), 5)}
            if name != "textured":
                t_med, t_lo = per_batch["textured"]
                row["over_textured"] = round(med / t_med, 4)
                # run-to-run spread: the minimum-to-median gap of the same leg
                row["spread"] = round(max(med - lo, t_med - t_lo) / t_med, 4)
            emit(row)
        if a.no_torch:
            continue
        m = torch_sub_n(k, min(a.n, a.torch_n))
        xs = sap[:m].contiguous()
        ys = torch.empty_like(xs)
        equal = bool(torch.equal(idn.median_blur(xs, k), torch_median(xs, k)))
        med, lo = time_leg(lambda: idn.median_blur(xs, k, out=ys), a.warmup, a.iters, a.settle)
        t_med, t_lo = time_leg(lambda: torch_median(xs, k), 1, a.torch_iters, a.settle)
        emit({"leg": "median", "k": k, "batch": "sap%g" % a.amount, "n": m, **shape,
              "ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": a.iters,
              "bytes_equal_to_torch": equal, "kernel_median_below_torch_min": med < t_lo,
              "torch_min_over_kernel_median": round(t_lo / med, 1)})
        emit({"leg": "torch_median", "k": k, "batch": "sap%g" % a.amount, "n": m, **shape,
              "ms_median": round(t_med, 4), "ms_min": round(t_lo, 4), "iters": a.torch_iters})

    med, lo = time_leg(lambda: idn.ops.copy_flat(clean.reshape(-1), y.reshape(-1), 1), a.warmup,
                       a.iters, a.settle)
    emit({"leg": "copy", "n": a.n, **shape, "ms_median": round(med, 4), "ms_min": round(lo, 4),
          "iters": a.iters, "GBps": round(2 * clean.numel() / (med * 1e6), 1)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
