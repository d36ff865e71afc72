#!/usr/bin/env python
"""Time the exposure correction on the workload batch (256 images of 600 x 1000 x 3 uint8,
textured), one JSON line per leg:

  equalize_hist          idn.equalize_hist on the batch's first channel, (n, h, w, 1)
  clahe                  idn.clahe(., 2.0, (4, 4)) on the same planes
  correct_exposure_tone  idn.correct_exposure(x, denoise=False): the seven launches of
                         csrc/exposure.hip
  correct_exposure       idn.correct_exposure(x): the tone part and nl_means_colored(3, 3, 7, 21)
  copy_planes / copy     idn.ops.copy_flat over the planes / over the batch, in the same run

A leg's algorithmic bytes are what any implementation must move: its input read once and its output
written once (2 bytes per pixel for the plane ops, 6 for the colour ops).  `of_copy_rate` is those
bytes per second over the bytes per second of the same run's copy of the same tensor, i.e. the
copy's time over the leg's time.  The protocol is tools/bench_nlmeans.py's: warm-up calls, a
synchronise and a short settle, then every timed call between two HIP events on the launch stream.
bench.py stays the project's yardstick; this script only measures the exposure ops.

    python tools/bench_exposure.py [--n 256] [--iters 20] [--out profiles/exposure/bench_exposure.jsonl]
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

from bench_nlmeans import textured_device, time_leg  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--full-iters", type=int, default=5, help="timed calls of the whole op")
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("bench_exposure: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn

    x = textured_device(a.n, a.h, a.w, 3)
    y = torch.empty_like(x)
    p = x[..., :1].contiguous()
    q = torch.empty_like(p)
    tone = idn.correct_exposure(x, denoise=False)
    changed = float((tone != x).float().mean())

    legs = [
        ("equalize_hist", lambda: idn.equalize_hist(p, out=q), a.iters, 1),
        ("clahe", lambda: idn.clahe(p, 2.0, (4, 4), out=q), a.iters, 1),
        ("correct_exposure_tone", lambda: idn.correct_exposure(x, denoise=False, out=y), a.iters, 3),
        ("correct_exposure", lambda: idn.correct_exposure(x, out=y), a.full_iters, 3),
        ("nlmeans_colored_3_3_7_21", lambda: idn.nl_means_colored(tone, 3, 3, 7, 21, out=y),
         a.full_iters, 3),
        ("copy_planes", lambda: idn.ops.copy_flat(p.reshape(-1), q.reshape(-1), 1), a.iters, 1),
        ("copy", lambda: idn.ops.copy_flat(x.reshape(-1), y.reshape(-1), 1), a.iters, 3),
    ]
    rows = []
    for name, fn, iters, c in legs:
        med, lo = time_leg(fn, a.warmup, iters, a.settle)
        nb = a.n * a.h * a.w * c
        rows.append({"leg": name, "n": a.n, "h": a.h, "w": a.w, "c": c, "ms_median": round(med, 4),
                     "ms_min": round(lo, 4), "iters": iters, "bytes_read": nb, "bytes_written": nb,
                     "algorithmic_GBps": round(2 * nb / med / 1e6, 1),
                     "ms_per_image": round(med / a.n, 5)})
    by = {r["leg"]: r for r in rows}
    for r in rows:
        cp = by["copy_planes" if r["c"] == 1 else "copy"]
        r["of_copy_rate"] = round(cp["ms_median"] / r["ms_median"], 4)
    by["correct_exposure_tone"]["share_of_bytes_changed"] = round(changed, 4)
    by["correct_exposure"]["nlmeans_share_of_time"] = round(
        by["nlmeans_colored_3_3_7_21"]["ms_median"] / by["correct_exposure"]["ms_median"], 4)
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
