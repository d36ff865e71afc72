#!/usr/bin/env python
"""Time idn.denoise_dct on the workload batch (600 x 1000 x 3 textured images with
idn.random_noise Gaussian noise of standard deviation 15), one JSON line per leg:

  dct        idn.denoise_dct(x, sd, color=..., out=...)  the hand-written kernel
             (csrc/dct_denoise.hip), colour transform on and off, outputs "u8" and "f32"; every
             line carries the issue-rate model of the kernel next to the measured time
  copy       idn.ops.copy_flat over the uint8 batch: the same run's copy rate
  wiener, tv, nl_means
             idn.wiener(x, 5, sd^2), idn.denoise_tv_chambolle(x) and idn.nl_means(x, 15) in the
             same run: the neighbours of the bank
  torch_dct  the same filter from torch ops on the --torch-n sub-batch, image by image (unfold,
             a 64 x 64 matmul each way, fold), with the kernel's time on that sub-batch, the share
             of equal bytes and the largest difference of the float results

The model: patches x VALU slots / issue rate.  A lane runs one patch per row step; the kernel's
row step holds VALU_PER_PATCH vector instructions (read from the ISA: DESIGN.md section 3), of
which PACKED are two-wide fp32 and count twice, and a wave64 instruction takes 2 cycles on a
SIMD that has two waves to choose from.  Lanes whose patch column or row lies in a workgroup's
halo are counted: the model is of the work launched, not of the work needed.

Each leg: warm-up calls, a synchronise and a short settle, then every timed call between two HIP
events; the line has the median, the minimum and `iters`.  bench.py stays the project's yardstick;
this script only measures the DCT denoiser.

    python tools/bench_dct.py [--n 256] [--torch-n 16] [--out profiles/dct_denoise/bench_dct.jsonl]
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

VALU_PER_PATCH = 590   # vector instructions of one row step of dct_denoise_kernel<3, true>
PACKED = 320           # of them v_pk_*_f32
CYCLES_PER_SLOT = 2    # a wave64 fp32 instruction on a SIMD with two waves resident
SIMDS_PER_CU = 4


def torch_dct(x, sd, color, factor=3.0):
    """tests/dct_model.py from torch ops in fp32, one image at a time; (uint8, float32)"""
    import math
    import torch
    import torch.nn.functional as F
    n, h, w, c = x.shape
    dev = x.device
    k = torch.arange(8, dtype=torch.float64, device=dev)
    cm = 0.5 * torch.cos(math.pi * (2 * k[None, :] + 1) * k[:, None] / 16)
    cm[0, :] = math.sqrt(1.0 / 8)
    kron = torch.kron(cm, cm).float()                      # (u, v) <- (y, x), 64 x 64
    m3 = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, -1.0], [1.0, -2.0, 1.0]], dtype=torch.float64,
                      device=dev)
    m3 = (m3 / m3.pow(2).sum(1, keepdim=True).sqrt()).float()
    use = color and c == 3
    thr = torch.full((c, 1, 1), factor * sd, dtype=torch.float32, device=dev)  # equal sigmas
    cnt = F.fold(torch.ones((1, 64, (h - 7) * (w - 7)), device=dev), (h, w), 8)
    out8 = torch.empty_like(x)
    out32 = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
    for i in range(n):
        p = x[i].permute(2, 0, 1).float()                  # (c, h, w)
        if use:
            p = torch.einsum("kj,jhw->khw", m3, p)
        d = kron @ F.unfold(p[:, None], 8)                 # (c, 64, L)
        keep = d.abs() >= thr
        keep[:, 0, :] = True
        r = F.fold(kron.t() @ (d * keep), (h, w), 8)[:, 0] / cnt[0]
        if use:
            r = torch.einsum("kj,khw->jhw", m3, r)
        r = r.permute(1, 2, 0)
        out32[i] = r
        out8[i] = torch.round(r).clamp_(0, 255).to(torch.uint8)
    return out8, out32


def model_ms(n, h, w, c, tile, cus, mhz):
    """(ms of the issue-rate model, patch lanes launched, patches needed)"""
    th, tw = tile
    strips, tiles = -(-h // th), -(-w // tw)
    rows = sum(min((s + 1) * th, h) - max(s * th - 7, 0) for s in range(strips))  # row steps
    lanes = n * c * tiles * 64 * rows
    slots = VALU_PER_PATCH + PACKED
    wave_steps = lanes / 64
    ms = wave_steps * slots * CYCLES_PER_SLOT / (cus * SIMDS_PER_CU * mhz * 1e3)
    return ms, lanes, n * c * (h - 7) * (w - 7)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--torch-n", type=int, default=16, help="sub-batch of the torch leg")
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--sd", type=float, default=15.0, help="noise standard deviation, 0..255 scale")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_dct: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from bench_nlmeans import textured_device
    from bench_tv import time_leg

    props = torch.cuda.get_device_properties(0)
    cus, mhz = props.multi_processor_count, getattr(props, "clock_rate", 2400000) / 1000.0
    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=(a.sd / 255.0) ** 2, seed=7)
    k16 = min(a.n, a.torch_n)
    xs = x[:k16]
    y = torch.empty_like(x)

    def emit(r):
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
    cp["GBps"] = round(2 * x.numel() / (cp["ms_median"] * 1e6), 1)
    emit(cp)

    mod, lanes, patches = model_ms(a.n, a.h, a.w, 3, idn.ops.DCT_TILE, cus, mhz)
    med = {}
    for color in (True, False):
        for out in ("u8", "f32"):
            r = leg("dct", a.n, lambda: idn.denoise_dct(x, a.sd, color=color, out=out), a.iters,
                    a.warmup, color=color, out=out, model_ms=round(mod, 3), patch_lanes=lanes,
                    patches=patches, cus=cus, mhz=mhz)
            r["model_over_measured"] = round(mod / r["ms_median"], 3)
            med[(color, out)] = r["ms_median"]
            emit(r)

    others = {}
    for name, fn in (("wiener", lambda: idn.wiener(x, 5, a.sd * a.sd)),
                     ("tv", lambda: idn.denoise_tv_chambolle(x)),
                     ("nl_means", lambda: idn.nl_means(x, 15.0))):
        r = leg(name, a.n, fn, a.iters, a.warmup)
        others[name] = r["ms_median"]
        emit(r)

    for color in (True, False):
        got8, got32 = idn.denoise_dct(xs, a.sd, color=color, out="both")
        ref8, ref32 = torch_dct(xs, a.sd, color)
        equal = float((got8 == ref8).float().mean())
        worst = float((got32 - ref32).abs().max())
        kern = leg("dct", k16, lambda: idn.denoise_dct(xs, a.sd, color=color), a.iters, a.warmup,
                   color=color, out="u8")
        tor = leg("torch_dct", k16, lambda: torch_dct(xs, a.sd, color), a.torch_iters, 1,
                  color=color, out="u8+f32", bytes_equal_to_kernel=round(equal, 6),
                  max_abs_diff_f32=worst)
        tor["torch_min_over_kernel_median"] = round(tor["ms_min"] / kern["ms_median"], 2)
        emit(kern)
        emit(tor)

    emit({"leg": "summary", "n": a.n, "dct_u8_color_ms": med[(True, "u8")],
          "dct_u8_plain_ms": med[(False, "u8")], "wiener5_ms": others["wiener"],
          "tv_ms": others["tv"], "nl_means_ms": others["nl_means"],
          "below_nl_means": med[(True, "u8")] < others["nl_means"], "copy_GBps": cp["GBps"]})
    return 0


if __name__ == "__main__":
    sys.exit(main())
