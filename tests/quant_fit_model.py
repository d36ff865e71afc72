"""Exact host model of the quant k-means fit (csrc/quant.hip, quant_fit_kernel / quant_select_kernel).

numpy only: the definition of the device fit restated from its documented scheme, so a test can
ask "equal to the model, draw for draw and bit for bit" instead of "about as good as sklearn".
The build compiles with -ffp-contract=off, the seeding is integer arithmetic, and the Lloyd loop
is fp32 in a fixed operation order over exact integer sums with one fp64 divide per centre, so
every number below is reproducible on the host.

    fit(img_bgr_u8, k, seed, image_id) -> (centres (k, 3) float64, runs)

`runs` is a list of NINIT dicts, one per restart:
    centres   (k, 3) float64   a nonempty cluster's exact mean sum / N; an empty cluster's fp32
                               centre widened
    inertia   float64          over the samples, in the kernel's reduction order
    iters     int              Lloyd iterations executed, the one that changed nothing included
    nonempty  int              clusters with at least one sample after the last assignment
    ctrs      list of int      the Philox counters the seeding consumed, in order
    cen32     (k, 3) float32   the Lloyd loop's centres at exit
    counts    (k,) int64       cluster sizes of the last assignment

The scheme
    key       seed ^ 0xA0761D6478BD642F; a 64-bit draw is x << 32 | y of
              philox4x32((ctr, tag, lo32(id), hi32(id)), key)
    samples   S = min(h w, 8192).  h w > 8192: sample i is pixel draw(ctr=i, tag=0x51) % (h w) in
              row-major order; else sample i is pixel i.  Samples are 8-bit Lab (oracle.cvlab).
    seeding   greedy k-means++ with ntrials = 2 + int(ln k) candidates per new centre.  Restart r
              starts its counter at r (1 + (k - 1) ntrials), tag 0x52.  First centre:
              pts[draw % S].  Potentials are integer squared distances.  The cumulative order is
              the kernel's: slot 16 t + j holds sample 16 t + ((j + t) & 15) (t < 512, j < 16),
              slots at or beyond S carry 0.  Each candidate draws target = draw % pot and is the
              first slot whose running sum exceeds target; with pot == 0 no draw is consumed and
              the candidate is sample 0.  The trial with the strictly lowest new potential wins
              (the earliest on ties).
    Lloyd     at most MAX_ITER iterations on fp32 centres: distance (d0 d0 + d1 d1) + d2 d2 in
              fp32, the first strict minimum over c < k takes the sample, exact integer sums, a
              nonempty cluster moves to float32(float64(sum) / N), an empty one stays; the loop
              ends with the first iteration that changes no centre.
    result    fp64 centres as above; inertia in fp64 against them, same operation order; thread t
              adds its samples t + 512 j in j order, each wave of 64 folds by halves (32, 16, ...,
              1) and the 8 wave totals are added in order from 0.0.
    choice    a later restart wins only with a strictly lower inertia.

`_mutate` (tests only) breaks one rule at a time, to show that the test cases can tell:
    "norot"       cumulative order without the (j + t) & 15 rotation
    "last_trial"  always the last seeding trial
    "le"          `<=` for `<` in the assignment (the last minimum takes the sample)
    "ctr0"        every restart's counter starts at 0
    "lo_id"       the image id's high word dropped
"""
import math

import numpy as np

from oracle import cvlab
from philox_model import philox4x32

QUANT_TAG = 0xA0761D6478BD642F
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1
THREADS, PER_THREAD = 512, 16
SAMPLES = THREADS * PER_THREAD  # 8192
MAX_ITER = 100
NINIT = 3
KMAX = 16
TAG_SAMPLE, TAG_SEED = 0x51, 0x52
MUTATIONS = ("norot", "last_trial", "le", "ctr0", "lo_id")


def key(seed):
    return (int(seed) & MASK64) ^ QUANT_TAG


def draws(ctr, tag, image_id, k64):
    """64-bit draws x << 32 | y at the counters ctr (array or int), as Python ints in a list"""
    ctr = np.atleast_1d(np.asarray(ctr, np.uint64))
    gid = int(image_id) & MASK64
    x, y, _, _ = philox4x32((ctr, np.uint64(tag), np.uint64(gid & MASK32), np.uint64(gid >> 32)),
                            k64)
    return [(int(a) << 32) | int(b) for a, b in zip(x.tolist(), y.tolist())]


def ntrials(k):
    return 2 + int(math.log(k))


def run_first_ctr(run, k):
    return run * (1 + (k - 1) * ntrials(k))


def samples(img, seed, image_id):
    """(S, 3) int64 Lab samples of one (h, w, 3) uint8 BGR image"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w = img.shape[:2]
    npix = h * w
    flat = img.reshape(npix, 3)
    if npix > SAMPLES:
        d = draws(np.arange(SAMPLES), TAG_SAMPLE, image_id, key(seed))
        flat = flat[np.array([v % npix for v in d], dtype=np.int64)]
    return cvlab.bgr2lab(flat[None])[0].astype(np.int64)


def slot_samples(rotate=True):
    """sample index held by each of the 8192 slots of the seeding's cumulative order"""
    t = np.arange(THREADS)[:, None]
    j = np.arange(PER_THREAD)[None, :]
    return (PER_THREAD * t + (((j + t) & (PER_THREAD - 1)) if rotate else j)).reshape(-1)


def _dist2(pts, c):
    d = pts - c[None, :]
    return (d * d).sum(1)


def seed_centres(pts, k, ctr, image_id, k64, _mutate=None):
    """greedy k-means++ -> ((k, 3) int64 centres, the counters consumed)"""
    S = len(pts)
    used = []

    def draw():
        nonlocal ctr
        used.append(ctr)
        v = draws(ctr & MASK32, TAG_SEED, image_id, k64)[0]
        ctr += 1
        return v

    slots = slot_samples(rotate=_mutate != "norot")
    valid = slots < S
    sl = np.where(valid, slots, 0)
    nt = ntrials(k)
    cen = [pts[draw() % S]]
    D = _dist2(pts, cen[0])
    for _ in range(1, k):
        cums = np.cumsum(np.where(valid, D[sl], 0))
        pot = int(cums[-1])
        cands = []
        for _tr in range(nt):
            if pot == 0:
                cands.append(0)
            else:
                target = draw() % pot
                cands.append(int(slots[np.searchsorted(cums, target, side="right")]))
        best, best_pot, best_D = 0, None, None
        for tr, s in enumerate(cands):
            nd = np.minimum(D, _dist2(pts, pts[s]))
            p = int(nd.sum())
            if best_pot is None or p < best_pot or _mutate == "last_trial":
                best, best_pot, best_D = tr, p, nd
        cen.append(pts[cands[best]])
        D = best_D
    return np.array(cen, dtype=np.int64), used


def assign32(p32, cen32, last=False):
    """nearest centre under the kernel's fp32 rule: (d0 d0 + d1 d1) + d2 d2, first strict minimum"""
    d = p32[:, None, :] - cen32[None, :, :]
    d = d * d
    d = (d[..., 0] + d[..., 1]) + d[..., 2]
    assert d.dtype == np.float32
    if last:
        return d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
    return np.argmin(d, axis=1)


def cluster_sums(pts, lab, k):
    sums = np.zeros((k, 3), np.int64)
    np.add.at(sums, lab, pts)
    return sums, np.bincount(lab, minlength=k).astype(np.int64)


def lloyd(pts, cen0, _mutate=None):
    """-> (cen32, sums, counts, iters)"""
    k = len(cen0)
    cen = np.asarray(cen0).astype(np.float32)
    p32 = pts.astype(np.float32)
    iters = 0
    for _ in range(MAX_ITER):
        iters += 1
        lab = assign32(p32, cen, last=_mutate == "le")
        sums, counts = cluster_sums(pts, lab, k)
        new = cen.copy()
        ne = counts > 0
        new[ne] = (sums[ne].astype(np.float64) / counts[ne, None].astype(np.float64)).astype(np.float32)
        changed = bool((new != cen).any())
        cen = new
        if not changed:
            break
    return cen, sums, counts, iters


def inertia_device_order(pts, cen64):
    """fp64 sample inertia, reduced as the 512-thread workgroup reduces it"""
    p = pts.astype(np.float64)
    bd = np.full(len(p), 1e300)
    for c in cen64:
        d0, d1, d2 = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        bd = np.minimum(bd, (d0 * d0 + d1 * d1) + d2 * d2)
    per = np.zeros(SAMPLES)
    per[:len(p)] = bd
    per = per.reshape(PER_THREAD, THREADS)     # [j][t]: sample t + 512 j
    acc = np.zeros(THREADS)
    for j in range(PER_THREAD):
        acc = acc + per[j]
    v = acc.reshape(THREADS // 64, 64)
    o = 32
    while o:
        v = v[:, :o] + v[:, o:2 * o]
        o >>= 1
    tot = np.float64(0.0)
    for wv in v[:, 0]:
        tot = tot + wv
    return float(tot)


def fit_run(pts, k, run, seed, image_id, _mutate=None):
    gid = int(image_id) & (MASK32 if _mutate == "lo_id" else MASK64)
    ctr0 = 0 if _mutate == "ctr0" else run_first_ctr(run, k)
    cen0, used = seed_centres(pts, k, ctr0, gid, key(seed), _mutate)
    cen32, sums, counts, iters = lloyd(pts, cen0, _mutate)
    cen64 = cen32.astype(np.float64)
    ne = counts > 0
    cen64[ne] = sums[ne].astype(np.float64) / counts[ne, None].astype(np.float64)
    return dict(centres=cen64, inertia=inertia_device_order(pts, cen64), iters=iters,
                nonempty=int(ne.sum()), ctrs=used, cen32=cen32, counts=counts, seeds=cen0)


def select(runs):
    best = 0
    for r in range(1, len(runs)):
        if runs[r]["inertia"] < runs[best]["inertia"]:
            best = r
    return best


def fit(img, k, seed=0, image_id=0, _mutate=None):
    k = int(k)
    img = np.asarray(img)
    assert 1 <= k <= KMAX and img.shape[0] * img.shape[1] >= k
    gid = int(image_id) & (MASK32 if _mutate == "lo_id" else MASK64)
    pts = samples(img, seed, gid)
    runs = [fit_run(pts, k, r, seed, image_id, _mutate) for r in range(NINIT)]
    return runs[select(runs)]["centres"].copy(), runs
