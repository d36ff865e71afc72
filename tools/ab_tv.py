#!/usr/bin/env python
"""A/B the rows a workgroup of the total-variation kernel walks (IDN_TV_ROWS, a knob of the
tools-only tuning build; the product's value is the compile-time default of csrc/tv.hip).

The arms run interleaved in one process, round after round, each call between two HIP events; one
JSON line per arm with the median and the minimum, and whether iters and the float output equal
the default arm's (the tile height changes the order the energy partials are added in, so the
energies may differ in their last bits; the dual update itself does not depend on it).

    python tools/ab_tv.py [--n 64] [--rows 32,64,128] [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "image-denoising_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--rows", default="32,64,128")
    ap.add_argument("--default-rows", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("ab_tv: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from idn import _lib
    from bench_nlmeans import textured_device

    arms = [int(r) for r in a.rows.split(",")]
    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=(15.0 / 255.0) ** 2, seed=7)
    y = torch.empty_like(x)
    ms = {r: [] for r in arms}
    res = {}
    with _lib.variant("tuning"):
        for r in [a.default_rows] + arms:  # warm-up, and the outputs to compare
            os.environ["IDN_TV_ROWS"] = str(r)
            res[r] = idn.denoise_tv_chambolle(x, out="f32", return_iters=True)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for r in arms:
                os.environ["IDN_TV_ROWS"] = str(r)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                idn.denoise_tv_chambolle(x, out_u8=y)
                e1.record()
                e1.synchronize()
                ms[r].append(e0.elapsed_time(e1))
        os.environ.pop("IDN_TV_ROWS", None)
    base = res[a.default_rows]
    for r in arms:
        row = {"ab": "tv_rows", "rows": r, "n": a.n, "h": a.h, "w": a.w, "c": 3,
               "ms_median": round(statistics.median(ms[r]), 4), "ms_min": round(min(ms[r]), 4),
               "rounds": a.rounds,
               "iters_equal_to_default": bool(torch.equal(res[r][1], base[1])),
               "f32_equal_to_default": bool(torch.equal(res[r][0], base[0]))}
        line = json.dumps(row)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
