#!/usr/bin/env python
"""Time idn.adaptive_median on the workload batch (600 x 1000 x 3 uint8 textured images), one JSON
line per leg:

  adaptive        idn.adaptive_median(x, K) for every K of --ks on five inputs: the textured
                  batch, that batch after idn.random_noise('s&p') at every amount of --amounts,
                  and a constant batch (every lane walks the level loop to K: its worst case)
  median          idn.median_blur(x, k) for every k of --median-ks on the s&p batches, same run
  copy            idn.ops.copy_flat over the batch: the same-run ceiling
  torch_adaptive  the same filter from torch ops on a sub-batch of the s&p 0.4 batch: replicate
                  pad (index gather), unfold over the window, amin / amax / kthvalue per level,
                  masked select; its bytes must equal the kernel's
  summary         each adaptive time over the same run's median_blur at the fixed window that is
                  best for that amount (0.2: 5, 0.4: 9, 0.6: 15), the torch leg's minimum over the
                  kernel's median, and the constant batch's time

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events on the launch stream; the line carries the median, the minimum and its `n`.  bench.py stays
the project's yardstick; this script only measures the adaptive median filter.

    python tools/bench_adaptive_median.py [--n 256] [--ks 7,15,31] [--no-torch]
        [--out profiles/adaptive_median/bench_adaptive_median.jsonl]
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

BEST_FIXED = {0.2: 5, 0.4: 9, 0.6: 15}  # README "Adaptive median": the best fixed window per amount


def torch_adaptive(x, K):
    """idn.adaptive_median(x, K, return_ksize=True) of a (N,H,W,C) uint8 batch from torch ops"""
    import torch
    n, h, w, c = x.shape
    out = x.clone()
    ksize = torch.zeros_like(x)
    undecided = torch.ones_like(x, dtype=torch.bool)
    md = x
    for k in range(3, K + 1, 2):
        r = k // 2
        iy = torch.arange(-r, h + r, device=x.device).clamp_(0, h - 1)
        ix = torch.arange(-r, w + r, device=x.device).clamp_(0, w - 1)
        xp = x[:, iy][:, :, ix]                                      # BORDER_REPLICATE
        win = xp.unfold(1, k, 1).unfold(2, k, 1).reshape(n, h, w, c, k * k)
        mn, mx = win.amin(-1), win.amax(-1)
        md = torch.kthvalue(win, k * k // 2 + 1, dim=-1).values
        del win
        a = undecided & (mn < md) & (md < mx)
        keep = (mn < x) & (x < mx)
        out = torch.where(a, torch.where(keep, x, md), out)
        ksize = torch.where(a, torch.full_like(x, k), ksize)
        undecided &= ~a
        if not bool(undecided.any()):
            break
    return torch.where(undecided, md, out), ksize


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--torch-n", type=int, default=16, help="sub-batch of the torch leg")
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--ks", type=str, default="7,15,31")
    ap.add_argument("--median-ks", type=str, default="3,5,9,15")
    ap.add_argument("--torch-ks", type=str, default="7,15", help="max_ksize values of the torch leg")
    ap.add_argument("--amounts", type=str, default="0.2,0.4,0.6")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch leg and its sub-batch")
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_adaptive_median: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_median import time_leg
    from bench_nlmeans import textured_device

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    ks = [int(s) for s in a.ks.split(",") if s]
    amounts = [float(s) for s in a.amounts.split(",") if s]
    shape = {"h": a.h, "w": a.w, "c": 3}
    clean = textured_device(a.n, a.h, a.w, 3)
    batches = [("textured", None, clean)]
    for am in amounts:
        batches.append(("sap%g" % am, am, idn.random_noise(clean, "s&p", amount=am, seed=7)))
    batches.append(("constant", None, torch.full_like(clean, 128)))
    y = torch.empty_like(clean)

    def leg(fn, iters=None, warmup=None):
        med, lo = time_leg(fn, a.warmup if warmup is None else warmup, iters or a.iters, a.settle)
        return {"ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": iters or a.iters}

    median_ms = {}
    for name, am, x in batches:
        if am is None:
            continue
        for k in [int(s) for s in a.median_ks.split(",") if s]:
            t = leg(lambda: idn.median_blur(x, k, out=y))
            median_ms[(name, k)] = t["ms_median"]
            emit({"leg": "median", "k": k, "batch": name, "n": a.n, **shape, **t})

    adaptive_ms = {}
    for name, am, x in batches:
        for K in ks:
            t = leg(lambda: idn.adaptive_median(x, K, out=y))
            adaptive_ms[(name, K)] = t["ms_median"]
            _, km = idn.adaptive_median(x[:4], K, return_ksize=True)
            hist = torch.bincount(km.reshape(-1).to(torch.int64), minlength=32).cpu().tolist()
            share = {str(v): round(hist[v] / km.numel(), 5) for v in [0] + list(range(3, K + 1, 2))
                     if hist[v]}
            emit({"leg": "adaptive", "max_ksize": K, "batch": name, "n": a.n, **shape, **t,
                  "ns_per_output_byte": round(t["ms_median"] * 1e6 / x.numel(), 5),
                  "ksize_share_first_4_images": share})

    t = leg(lambda: idn.ops.copy_flat(clean.reshape(-1), y.reshape(-1), 1))
    emit({"leg": "copy", "n": a.n, **shape, **t,
          "GBps": round(2 * clean.numel() / (t["ms_median"] * 1e6), 1)})

    torch_rows = {}
    if not a.no_torch:
        m = min(a.n, a.torch_n)
        xs = dict((nm, x) for nm, _, x in batches)["sap0.4" if 0.4 in amounts else batches[1][0]]
        xs = xs[:m].contiguous()
        ys = torch.empty_like(xs)
        for K in [int(s) for s in a.torch_ks.split(",") if s]:
            got = idn.adaptive_median(xs, K, return_ksize=True)
            ref = torch_adaptive(xs, K)
            equal = bool(torch.equal(got[0], ref[0])) and bool(torch.equal(got[1], ref[1]))
            del got, ref
            tk = leg(lambda: idn.adaptive_median(xs, K, out=ys))
            tt = leg(lambda: torch_adaptive(xs, K), iters=a.torch_iters, warmup=1)
            torch_rows[K] = round(tt["ms_min"] / tk["ms_median"], 1)
            emit({"leg": "adaptive", "max_ksize": K, "batch": "sap0.4", "n": m, **shape, **tk,
                  "bytes_equal_to_torch": equal, "torch_min_over_kernel_median": torch_rows[K]})
            emit({"leg": "torch_adaptive", "max_ksize": K, "batch": "sap0.4", "n": m, **shape, **tt})

    ratios = {}
    for name, am, _ in batches:
        if am in BEST_FIXED and (name, BEST_FIXED[am]) in median_ms:
            for K in ks:
                ratios["%s/K%d_over_median%d" % (name, K, BEST_FIXED[am])] = round(
                    adaptive_ms[(name, K)] / median_ms[(name, BEST_FIXED[am])], 3)
    emit({"leg": "summary", "n": a.n, **shape, "adaptive_over_best_fixed_median": ratios,
          "torch_min_over_kernel_median": {str(k): v for k, v in torch_rows.items()},
          "constant_ms": {str(K): adaptive_ms[("constant", K)] for K in ks}})
    return 0


if __name__ == "__main__":
    sys.exit(main())
