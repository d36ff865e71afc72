"""The inputs of the total-variation GPU cases and their model results, shared by tests/test_tv.py
(which checks on the CPU that each case means something) and tests/test_tv_gpu.py.

An input is conftest.textured plus rounded Gaussian noise (tv_model.noisy).  The seeds were
searched: a case is kept only if, on the float64 model with the default eps and n_iter_max, every
stopping ratio r_i of every channel is at least 0.01 away from 1 (about a third of the seeds
qualify for three channels), so that a kernel within 1e-5 of the model cannot stop elsewhere for a
rounding's sake.  The kernel's tile is 256 columns x 64 rows: `tiles` is three tiles each way."""
import functools

import numpy as np

import tv_model as tm

EPS = 2e-4
N_ITER_MAX = 200

CASES = {
    # name: (n, h, w, c, weight, noise sd, seed)
    "tex-w0.1": (2, 40, 72, 3, 0.1, 15, 2),
    "tex-w0.05": (2, 40, 72, 3, 0.05, 15, 6),
    "tex-w0.3": (2, 40, 72, 3, 0.3, 15, 1),
    "tex-c1": (1, 40, 72, 1, 0.1, 20, 1),
    "odd": (2, 75, 131, 3, 0.1, 12, 1),
    "tiles": (1, 131, 515, 3, 0.1, 25, 1),
    "2x2": (1, 2, 2, 3, 0.1, 20, 2),
    "1x9": (1, 1, 9, 1, 0.1, 20, 1),
    "9x1": (1, 9, 1, 1, 0.1, 20, 1),
}
FIXED_COUNTS = (2, 7)  # n_iter_max of the eps = 0 legs


def weight(name):
    return CASES[name][4]


@functools.lru_cache(maxsize=None)
def inputs(name):
    n, h, w, c, _, sd, seed = CASES[name]
    x = tm.noisy(n, h, w, c, seed, sd)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref(name, eps=EPS, n_iter_max=N_ITER_MAX):
    """(out float64, iters, r) of the model for one case, computed once and shared (read-only)"""
    out, iters, r = tm.tv_chambolle(inputs(name), weight(name), eps, n_iter_max)
    out.setflags(write=False)
    iters.setflags(write=False)
    return out, iters, r


def constant(h=40, w=72, c=3, values=(7, 128, 250)):
    x = np.empty((1, h, w, c), dtype=np.uint8)
    x[...] = np.array(values[:c], dtype=np.uint8)
    return x
