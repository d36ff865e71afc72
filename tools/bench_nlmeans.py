#!/usr/bin/env python
"""Time non-local means on the workload batch (600 x 1000 x 3 uint8, template 7, search 21,
h 15, textured images), one JSON line per leg:

  nlmeans        idn.nl_means(x, h, t, s)      the hand-written kernel (csrc/nlmeans.hip), on the
                                               whole batch and on the torch leg's sub-batch
  torch_nlmeans  the same algorithm composed from torch ops on the device, on a sub-batch: per
                 offset a shifted difference, the t x t box sum (avg_pool2d with divisor 1 on
                 float32: the sums stay below 2^24, so it is exact), a shift, a gather from the
                 weight table and the accumulation; s*s passes over full-size planes
  copy           idn.ops.copy_flat over the bytes the filter reads and writes: the same-run ceiling

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events on the launch stream; the line carries the median, the minimum and its `n`.  The kernel's
line on the sub-batch also says whether its median lies below the torch leg's minimum and whether
the two outputs are equal.  bench.py stays the project's yardstick; this script only measures
non-local means.

    python tools/bench_nlmeans.py [--n 256] [--torch-n 16] [--iters 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "image-denoising_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def textured_device(n, h, w, c, seed=3):
    """tests/conftest.py's textured pattern, generated on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.arange(h, device="cuda", dtype=torch.float32)[:, None, None]
    x = torch.arange(w, device="cuda", dtype=torch.float32)[None, :, None]
    base = 128 + 64 * torch.sin(2 * math.pi * x / 97) * torch.cos(2 * math.pi * y / 61)
    out = torch.empty((n, h, w, c), dtype=torch.uint8, device="cuda")
    for i in range(n):
        u = torch.rand((h, w, c), device="cuda", generator=g) * 64 - 32
        out[i] = (base + u).clamp_(0, 255).to(torch.uint8)
    return out


def _reflect_index(length, b, device):
    import torch
    i = torch.arange(-b, length + b, device=device)
    i = i.abs()
    return torch.where(i >= length, 2 * length - 2 - i, i)


def torch_nlmeans(x, h, t, s):
    """OpenCV's integer scheme from torch ops; x (N, H, W, C) uint8 on the device"""
    import torch
    import torch.nn.functional as F
    import idn
    n, H, W, C = x.shape
    tr, sr = t // 2, s // 2
    b = tr + sr
    host, shift, fpm = idn.ops.nl_means_weights(h, C, t, s)
    length = int(255 * 255 * C / ((1 << shift) / (t * t)) + 1)
    table = torch.zeros(length, dtype=torch.int64, device=x.device)
    table[:host.size] = torch.from_numpy(host).to(x.device)
    E = x.permute(0, 3, 1, 2)[:, :, _reflect_index(H, b, x.device)][:, :, :, _reflect_index(W, b, x.device)]
    E = E.to(torch.int32).contiguous()
    A = E[:, :, sr:sr + H + 2 * tr, sr:sr + W + 2 * tr]
    est = torch.zeros((n, C, H, W), dtype=torch.int64, device=x.device)
    wsum = torch.zeros((n, 1, H, W), dtype=torch.int64, device=x.device)
    for dy in range(-sr, sr + 1):
        for dx in range(-sr, sr + 1):
            d = A - E[:, :, sr + dy:sr + dy + H + 2 * tr, sr + dx:sr + dx + W + 2 * tr]
            d2 = (d * d).sum(dim=1, keepdim=True).to(torch.float32)
            ssd = F.avg_pool2d(d2, t, 1, divisor_override=1).to(torch.int64)
            wgt = table[ssd >> shift]
            wsum += wgt
            est += wgt * E[:, :, b + dy:b + dy + H, b + dx:b + dx + W]
    out = ((est + wsum // 2) // wsum).clamp_(max=255).to(torch.uint8)
    return out.permute(0, 2, 3, 1).contiguous()


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
    ap.add_argument("--torch-n", type=int, default=16, help="sub-batch of the torch leg")
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--strength", type=float, default=15.0, help="the filter's h")
    ap.add_argument("--template", type=int, default=7)
    ap.add_argument("--search", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_nlmeans: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn

    t, s, hh = a.template, a.search, a.strength
    x = textured_device(a.n, a.h, a.w, 3)
    k = min(a.n, a.torch_n)
    xs = x[:k]
    y = torch.empty_like(x)
    ys = torch.empty_like(xs)
    equal = bool(torch.equal(idn.nl_means(xs, hh, t, s), torch_nlmeans(xs, hh, t, s)))
    changed = float((idn.nl_means(xs, hh, t, s) != xs).float().mean())

    def nbytes(v):
        return v.numel()

    legs = [
        ("nlmeans", a.n, lambda: idn.nl_means(x, hh, t, s, out=y), a.iters, nbytes(x)),
        ("nlmeans", k, lambda: idn.nl_means(xs, hh, t, s, out=ys), a.iters, nbytes(xs)),
        ("torch_nlmeans", k, lambda: torch_nlmeans(xs, hh, t, s), a.torch_iters, nbytes(xs)),
        ("copy", a.n, lambda: idn.ops.copy_flat(x.reshape(-1), y.reshape(-1), 1), a.iters, nbytes(x)),
    ]
    rows = []
    for name, n, fn, iters, nb in legs:
        med, lo = time_leg(fn, a.warmup if name != "torch_nlmeans" else 1, iters, a.settle)
        rows.append({"leg": name, "n": n, "h": a.h, "w": a.w, "c": 3, "template": t, "search": s,
                     "strength": hh, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                     "iters": iters, "bytes_read": nb, "bytes_written": nb,
                     "ms_per_image": round(med / n, 5),
                     "ns_per_pixel_offset": round(med * 1e6 / (n * a.h * a.w * s * s), 6)})
    big, sub, tor, cp = rows
    big["time_over_copy"] = round(big["ms_median"] / cp["ms_median"], 1)
    sub["torch_min_over_kernel_median"] = round(tor["ms_min"] / sub["ms_median"], 2)
    sub["kernel_median_below_torch_min"] = sub["ms_median"] < tor["ms_min"]
    sub["equal_to_torch"] = equal
    sub["share_of_bytes_changed"] = round(changed, 4)
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
