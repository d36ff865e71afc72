#!/usr/bin/env python
"""A/B the output rows a workgroup of the wiener kernel walks (IDN_WN_SR, a knob of the tools-only
tuning build; the product's value is the compile-time default of csrc/wiener.hip, exported as
idn.ops.WIENER_TILE).  A taller strip re-reads fewer halo rows (kh - 1 per strip), a shorter one
gives a small batch more workgroups.  --two crosses the arms with the narrowest window whose
horizontal sum takes two levels (IDN_WN_TWO; 99 turns the second level off).

The arms run interleaved in one process, round after round, each call between two HIP events; one
JSON line per arm and window with the median and the minimum, and whether the result equals the
default arm's byte for byte (it must: the sums do not depend on the strip).

    python tools/ab_wiener.py [--n 256] [--sr 32,64,128,256] [--ksize 3,31] [--two 13,99] [--rounds 7]
                           [--out FILE]
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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--h", type=int, default=600)
    ap.add_argument("--w", type=int, default=1000)
    ap.add_argument("--sr", default="32,64,128,256")
    ap.add_argument("--ksize", default="3,31")
    ap.add_argument("--two", default="", help="IDN_WN_TWO values, crossed with the other arms")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        print("ab_wiener: no GPU; nothing is measured without one", file=sys.stderr)
        return 2
    import idn
    from idn import _lib
    from bench_nlmeans import textured_device

    default = idn.ops.WIENER_TILE[0]
    twos = [int(v) for v in a.two.split(",")] if a.two else [None]
    arms = [(int(s), int(k), two) for k in a.ksize.split(",") for two in twos
            for s in a.sr.split(",")]

    def setenv(s, two):
        os.environ["IDN_WN_SR"] = str(s)
        if two is None:
            os.environ.pop("IDN_WN_TWO", None)
        else:
            os.environ["IDN_WN_TWO"] = str(two)

    clean = textured_device(a.n, a.h, a.w, 3)
    x = idn.random_noise(clean, "gaussian", var=(15.0 / 255.0) ** 2, seed=7)
    ms = {arm: [] for arm in arms}
    equal = {}
    with _lib.variant("tuning"):
        for s, k, two in arms:  # warm-up, and the results to compare
            setenv(default, None)
            base = idn.wiener(x, k, 225.0)
            setenv(s, two)
            equal[(s, k, two)] = bool(torch.equal(idn.wiener(x, k, 225.0), base))
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for s, k, two in arms:
                setenv(s, two)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                idn.wiener(x, k, 225.0)
                e1.record()
                e1.synchronize()
                ms[(s, k, two)].append(e0.elapsed_time(e1))
        os.environ.pop("IDN_WN_SR", None)
        os.environ.pop("IDN_WN_TWO", None)
    for s, k, two in arms:
        row = {"ab": "wiener_rows_per_workgroup", "rows_per_workgroup": s, "ksize": k,
               "two_level_from": two, "n": a.n, "h": a.h, "w": a.w, "c": 3,
               "ms_median": round(statistics.median(ms[(s, k, two)]), 4),
               "ms_min": round(min(ms[(s, k, two)]), 4), "rounds": a.rounds,
               "equal_to_default": equal[(s, k, two)]}
        line = json.dumps(row)
        print(line, flush=True)
        if a.out is not None:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
