"""GPU: bench.py's plain run, --dump-outputs and --full as command lines (small batches).

A plain run times its steps and prints the line without the legs that take runs of their own;
--dump-outputs writes what the last timed step computed, the same from run to run; --full adds
the copy ceiling and the per-launch event-pair median (the CPU baseline leg is skipped here with
--no-cpu: it samples for 12 s).
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_output(dev, tmp_path):
    import torch
    import idn
    import oracle
    sys.path.insert(0, str(ROOT))
    import bench
    rec = _bench("--steps", "3", "--warmup", "1", "--batch", "2", "--settle-s", "0",
                 "--dump-outputs", str(tmp_path / "d"))
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["unit"] == "Mpix/s"
    assert rec["cpu_baseline"] is None and "copy_ceiling" not in rec
    assert rec["roofline"]["kernel_ms_median_event_pairs"] is None
    assert rec["roofline"]["kernel_ms_avg"] > 0
    files = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert files == ["out.npy"]
    out = np.load(tmp_path / "d" / "out.npy")
    assert out.dtype == np.float32 and out.shape == (2, bench.H, bench.W, bench.C)
    # the same seeded batch, filtered here: the dump is the op's output, bit for bit
    x = bench.synth_batch(torch, 2, dev, seed=3)
    ref = oracle.cv.gaussian_blur(x.cpu().numpy(), 5)
    assert np.array_equal(out, ref.astype(np.float32))
    assert np.array_equal(idn.gaussian_blur(x, 5).cpu().numpy(), ref)


def test_full_run_adds_copy_ceiling_and_event_pairs(dev):
    rec = _bench("--steps", "3", "--warmup", "1", "--batch", "2", "--settle-s", "0", "--full",
                 "--no-cpu")
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["copy_ceiling"]["copy_ceiling_GBps"] > 0
    assert set(rec["copy_ceiling"]["by_policy"]) == {"default", "nontemporal"}
    assert rec["roofline"]["kernel_ms_median_event_pairs"] > 0
    assert rec["roofline"]["frac_of_copy_ceiling"] > 0
    assert rec["cpu_baseline"] is None
