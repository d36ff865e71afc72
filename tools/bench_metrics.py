#!/usr/bin/env python
"""Time the quality metrics on the workload batch (256 x 600 x 1000 x 3 uint8 pairs), one JSON
line per leg:

  ssim        idn.ssim(x, y, win)            the hand-written kernel (csrc/metrics.hip)
  mse         idn.mse(x, y)
  torch_ssim  the same SSIM composed from torch ops on the device: float64 avg_pool2d of the five
              moment planes, then skimage's formula (run over the batch in chunks to bound memory)
  copy        idn.ops.copy_flat over the same bytes the metrics read (both batches, 921.6 MB):
              the same-run read ceiling

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events on the launch stream; the line carries the median and the minimum.  bench.py stays the
project's yardstick; this script only measures the metrics.

    python tools/bench_metrics.py [--n 256] [--win 7] [--iters 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "image-denoising_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def torch_ssim(x, y, win, chunk):
    """compare_ssim(multichannel=True, uniform window, sample covariance) from torch ops"""
    import torch
    import torch.nn.functional as F
    NP = win * win
    cov_norm = NP / (NP - 1)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    out = []
    for i in range(0, x.shape[0], chunk):
        X = x[i:i + chunk].permute(0, 3, 1, 2).double()
        Y = y[i:i + chunk].permute(0, 3, 1, 2).double()
        ux, uy = F.avg_pool2d(X, win, 1), F.avg_pool2d(Y, win, 1)
        uxx, uyy, uxy = F.avg_pool2d(X * X, win, 1), F.avg_pool2d(Y * Y, win, 1), F.avg_pool2d(X * Y, win, 1)
        vx = cov_norm * (uxx - ux * ux)
        vy = cov_norm * (uyy - uy * uy)
        vxy = cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        out.append(S.mean(dim=(2, 3)).mean(dim=1))
    return torch.cat(out)


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
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--win", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=16)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_metrics: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn

    g = torch.Generator(device="cuda").manual_seed(11)
    shape = (a.n, a.h, a.w, 3)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    d = torch.randint(-24, 25, shape, dtype=torch.int16, device="cuda", generator=g)
    y = (x.to(torch.int16) + d).clamp_(0, 255).to(torch.uint8)
    del d
    both = torch.cat([x.reshape(-1), y.reshape(-1)])
    dst = torch.empty_like(both)
    nbytes = both.numel()

    # the two SSIM legs compute the same thing: say how far apart they are
    k = min(a.n, a.torch_chunk)
    diff = float((idn.ssim(x[:k], y[:k], a.win) - torch_ssim(x[:k], y[:k], a.win, k)).abs().max())

    legs = [
        ("ssim", lambda: idn.ssim(x, y, a.win), a.iters, nbytes, 0),
        ("mse", lambda: idn.mse(x, y), a.iters, nbytes, 0),
        ("torch_ssim", lambda: torch_ssim(x, y, a.win, a.torch_chunk), a.torch_iters, nbytes, 0),
        ("copy", lambda: idn.ops.copy_flat(both, dst, 1), a.iters, nbytes, nbytes),
    ]
    rows = []
    for name, fn, iters, rd, wr in legs:
        med, lo = time_leg(fn, a.warmup, iters, a.settle)
        rows.append({"leg": name, "n": a.n, "h": a.h, "w": a.w, "c": 3, "win": a.win,
                     "ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": iters,
                     "bytes_read": rd, "bytes_written": wr,
                     "read_GBps": round(rd / med * 1e-6, 1)})
    by = {r["leg"]: r for r in rows}
    for r in rows:
        r["time_over_copy"] = round(r["ms_median"] / by["copy"]["ms_median"], 3)
    by["ssim"]["torch_over_ssim"] = round(by["torch_ssim"]["ms_median"] / by["ssim"]["ms_median"], 2)
    by["ssim"]["max_abs_diff_vs_torch"] = diff
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
