#!/usr/bin/env python
"""Time total-variation denoising on the workload batch (600 x 1000 x 3 uint8 textured images with
idn.random_noise Gaussian noise of standard deviation 15, default arguments), one JSON line per leg:

  tv        idn.denoise_tv_chambolle(x)   the hand-written kernels (csrc/tv.hip): on the whole
                                          batch, on the whole batch with n_iter_max set to the
                                          batch's largest iters + 1 (what the idle launches past
                                          convergence cost is the difference), and on the torch
                                          leg's sub-batch
  torch_tv  the same algorithm composed from torch ops on the device, on a sub-batch: fp32 planes,
            per-(image, channel) masks, float64 energies, and one host synchronisation per
            iteration to leave the loop when every plane has stopped
  copy      idn.ops.copy_flat over the batch: the same-run ceiling, and the rate from which the
            bytes a pixel moves per iteration are implied

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events on the launch stream; the line carries the median, the minimum and its `n`.  The kernel's
line on the sub-batch also says whether its median lies below the torch leg's minimum, whether the
iteration counts are equal and how far the float outputs are apart.  bench.py stays the project's
yardstick; this script only measures total-variation denoising.

    python tools/bench_tv.py [--n 256] [--torch-n 16] [--iters 10] [--out FILE]
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


def torch_tv(x, weight=0.1, eps=2e-4, n_iter_max=200):
    """(out float32 (N,H,W,C), iters int32 (N,C)) of the model's algorithm from torch ops"""
    import torch
    n, H, W, C = x.shape
    im = (x.permute(0, 3, 1, 2).to(torch.float64) / 255.0).to(torch.float32).contiguous()
    p0 = torch.zeros_like(im)
    p1 = torch.zeros_like(im)
    d = torch.zeros_like(im)
    out = im.clone()
    active = torch.ones((n, C, 1, 1), dtype=torch.bool, device=x.device)
    iters = torch.full((n, C, 1, 1), n_iter_max, dtype=torch.int32, device=x.device)
    e_init = e_prev = None
    q = 0.25 / weight
    for i in range(n_iter_max):
        if i > 0:
            d = -(p0 + p1)
            d[:, :, 1:, :] += p0[:, :, :-1, :]
            d[:, :, :, 1:] += p1[:, :, :, :-1]
            cur = im + d
        else:
            cur = im
        e = (d.to(torch.float64) ** 2).sum(dim=(2, 3), keepdim=True)
        g0 = torch.zeros_like(im)
        g1 = torch.zeros_like(im)
        g0[:, :, :-1, :] = cur[:, :, 1:, :] - cur[:, :, :-1, :]
        g1[:, :, :, :-1] = cur[:, :, :, 1:] - cur[:, :, :, :-1]
        norm = torch.sqrt(g0 * g0 + g1 * g1)
        e = (e + weight * norm.to(torch.float64).sum(dim=(2, 3), keepdim=True)) / float(H * W)
        den = norm * q + 1.0
        out = torch.where(active, cur, out)
        if i == 0:
            e_init = e_prev = e
        else:
            brk = active & ((e_prev - e).abs() < eps * e_init)
            iters = torch.where(brk, torch.full_like(iters, i), iters)
            active = active & ~brk
            e_prev = torch.where(active, e, e_prev)
            if not bool(active.any()):
                break
        p0 = torch.where(active, (p0 - 0.25 * g0) / den, p0)
        p1 = torch.where(active, (p1 - 0.25 * g1) / den, p1)
    return out.permute(0, 2, 3, 1).contiguous(), iters.view(n, C)


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
    ap.add_argument("--sd", type=float, default=15.0, help="noise standard deviation, 0..255 scale")
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--eps", type=float, default=2e-4)
    ap.add_argument("--n-iter-max", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_tv: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_nlmeans import textured_device

    kw = dict(weight=a.weight, eps=a.eps)
    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=(a.sd / 255.0) ** 2, seed=7)
    k = min(a.n, a.torch_n)
    xs = x[:k]
    y = torch.empty_like(x)
    ys = torch.empty_like(xs)

    _, its = idn.denoise_tv_chambolle(x, n_iter_max=a.n_iter_max, out_u8=y, return_iters=True, **kw)
    its = its.cpu().numpy()
    # iterations a plane runs: 0 .. iters on a break, n_iter_max on exhaustion
    run = (its + (its < a.n_iter_max)).astype("int64")
    tight = int(its.max()) + 1 if its.max() < a.n_iter_max else a.n_iter_max
    f32s, its_s = idn.denoise_tv_chambolle(xs, n_iter_max=a.n_iter_max, out="f32",
                                           return_iters=True, **kw)
    t32, tits = torch_tv(xs, a.weight, a.eps, a.n_iter_max)
    iters_equal = bool(torch.equal(its_s, tits))
    max_diff = float((f32s - t32).abs().max())
    changed = float((y[:k] != xs).float().mean())
    ssim_noisy = float(idn.ssim(x[:k], clean[:k]).mean())
    ssim_tv = float(idn.ssim(y[:k], clean[:k]).mean())

    legs = [
        ("tv", a.n, a.n_iter_max,
         lambda: idn.denoise_tv_chambolle(x, n_iter_max=a.n_iter_max, out_u8=y, **kw), a.iters),
        ("tv", a.n, tight,
         lambda: idn.denoise_tv_chambolle(x, n_iter_max=tight, out_u8=y, **kw), a.iters),
        ("tv", k, a.n_iter_max,
         lambda: idn.denoise_tv_chambolle(xs, n_iter_max=a.n_iter_max, out_u8=ys, **kw), a.iters),
        ("torch_tv", k, a.n_iter_max, lambda: torch_tv(xs, a.weight, a.eps, a.n_iter_max),
         a.torch_iters),
        ("copy", a.n, 0, lambda: idn.ops.copy_flat(x.reshape(-1), y.reshape(-1), 1), a.iters),
    ]
    rows = []
    for name, n, nmax, fn, iters in legs:
        med, lo = time_leg(fn, a.warmup if name != "torch_tv" else 1, iters, a.settle)
        rows.append({"leg": name, "n": n, "h": a.h, "w": a.w, "c": 3, "sd": a.sd,
                     "weight": a.weight, "eps": a.eps, "n_iter_max": nmax,
                     "ms_median": round(med, 4), "ms_min": round(lo, 4), "iters": iters,
                     "ms_per_image": round(med / n, 5)})
    big, tgt, sub, tor, cp = rows
    copy_gbps = 2 * x.numel() / (cp["ms_median"] * 1e6)  # read + write
    cp["GBps"] = round(copy_gbps, 1)
    plane_px_iters = float(run.sum()) * a.h * a.w
    for r, rr in ((big, run), (tgt, run)):
        r["stop_iters_min"] = int(its.min())
        r["stop_iters_median"] = float(statistics.median(its.reshape(-1).tolist()))
        r["stop_iters_max"] = int(its.max())
        r["iterations_run_mean"] = round(float(rr.mean()), 2)
        r["ms_per_iteration"] = round(r["ms_median"] / float(rr.max()), 4)
        r["ns_per_pixel_iteration"] = round(r["ms_median"] * 1e6 / plane_px_iters, 6)
        r["bytes_per_pixel_iteration_at_copy_rate"] = round(
            r["ms_median"] * 1e6 * copy_gbps / plane_px_iters, 2)
    big["time_over_copy"] = round(big["ms_median"] / cp["ms_median"], 1)
    big["idle_launch_ms"] = round(big["ms_median"] - tgt["ms_median"], 4)
    big["idle_launches"] = a.n_iter_max - tight
    sub["torch_min_over_kernel_median"] = round(tor["ms_min"] / sub["ms_median"], 2)
    sub["kernel_median_below_torch_min"] = sub["ms_median"] < tor["ms_min"]
    sub["iters_equal_to_torch"] = iters_equal
    sub["max_abs_diff_to_torch"] = max_diff
    sub["within_1e-5_of_torch"] = max_diff <= 1e-5
    sub["share_of_bytes_changed"] = round(changed, 4)
    sub["ssim_noisy_vs_clean"] = round(ssim_noisy, 4)
    sub["ssim_tv_vs_clean"] = round(ssim_tv, 4)
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
