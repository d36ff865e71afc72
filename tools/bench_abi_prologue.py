"""Host cost of the short ops' C entry points: microseconds per call of each op on a tiny batch
(2 x 64 x 96), where the launch and the host-side prologue dominate, not the kernel.

  python tools/bench_abi_prologue.py --tree NAME [--calls 20000]
  python tools/bench_abi_prologue.py --libs parent=ab/parent.so new=ab/new.so [--rounds 7]

One JSON line per op and library: {"tree", "op", "us_per_call", "calls"}: wall clock over `calls`
back-to-back calls on one stream with one synchronize at the end, after 2000 warm-up calls.  With
--libs the builds are loaded side by side in one process (idn._lib.variant) and take turns, block
by block, `rounds` times: "us_per_call" is the median block and "blocks" lists them all, so the two
builds see the same clocks and the same interpreter.
"""
import argparse
import contextlib
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "image-denoising_amd"), str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="this")
    ap.add_argument("--libs", nargs="*", default=[], metavar="NAME=PATH")
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    import idn
    from idn import _lib, ops
    libs = dict(s.split("=", 1) for s in a.libs)
    for name, path in libs.items():
        _lib.VARIANTS[name] = Path(path).resolve()
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (2, 64, 96, 3), dtype=torch.uint8, generator=g).cuda()
    y = torch.randint(0, 256, (2, 64, 96, 3), dtype=torch.uint8, generator=g).cuda()
    out = torch.empty_like(x)
    cases = {
        "box3": lambda: idn.blur(x, 3, out=out),
        "gauss3": lambda: idn.gaussian_blur(x, 3, out=out),
        "gauss5": lambda: idn.gaussian_blur(x, 5, out=out),
        "median3": lambda: idn.median_blur(x, 3, out=out),
        "bgr2lab": lambda: ops.color.cvt_color_lab(x, True),
        "lab2bgr": lambda: ops.color.cvt_color_lab(x, False),
        "bgr2yuv": lambda: ops.exposure.cvt_color_yuv(x, True),
        "yuv2bgr": lambda: ops.exposure.cvt_color_yuv(x, False),
        "mse": lambda: ops.metrics.mse(x, y),
    }

    def block(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e6

    for op, fn in cases.items():
        trees = list(libs) or [a.tree]
        got = {t: [] for t in trees}
        for r in range(a.rounds if libs else 1):
            for t in trees:
                with (_lib.variant(t) if libs else contextlib.nullcontext()):
                    if r == 0:
                        block(fn, 2000)
                    got[t].append(round(block(fn, a.calls), 3))
        for t in trees:
            print(json.dumps({"tree": t, "op": op, "us_per_call": statistics.median(got[t]),
                              "calls": a.calls, "blocks": got[t]}), flush=True)


if __name__ == "__main__":
    main()
