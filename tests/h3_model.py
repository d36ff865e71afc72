"""Test helper: integer numpy restatement of the Haar L = 3 sigma selection (csrc/haar3.hpp) and
the input families that drive it onto each of its branches.

The model states, for a u8 H x W x 3 image (both sides multiples of 8) and each YCbCr channel:

  * T = w_c . D of every level-1 2x2 group (D = x00 - x01 - x10 + x11 per byte plane, w_c the
    rgb2ycbcr row x 1000 applied to bytes 0, 1, 2) and the equal-triple test (h3_eqtrip);
  * wl_h3_window's sample (level-1 rows 0, 16, 32, .., every column): n, nres, rho, m, the sample
    ranks klo / khi, their log-linear bins (6 mantissa bits) and the window (lo, hi);
  * wl_h3_stats' counters over the whole image: n_t, n_lo, n_c and the residue candidates;
  * wl_h3_sigma's decision (haar3.hpp: `klo >= base && khi < base + n_c`) given the number of
    residues whose fp64 dd is nonzero, and the window path's median.

Nothing here reads the kernels' results: the model is checked against the fp64 oracle by
tests/test_h3_model.py and the kernels against the model by tests/test_haar3_window_gpu.py.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

YCC_W = np.array([[65481, 128553, 24966], [-37797, -74203, 112000], [112000, -93786, -18214]],
                 np.int64)
MB = 6                 # mantissa bits of the window histogram
MM = (1 << MB) - 1
SAMPLE = 16            # every 16th level-1 row
MIN_N = 512            # fewer nonzero sample T: the window stays full
FULL = (1, 0xFFFFFFFF)


# ---- the integers ---------------------------------------------------------------------------------
def finest_T(img):
    """(T, eq): T[i, j, c] of level-1 group (i, j), int64; eq[i, j] the equal-triple pairs"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    assert img.shape[0] % 8 == 0 and img.shape[1] % 8 == 0
    x = img.astype(np.int64)
    x00, x01, x10, x11 = x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]
    D = x00 - x01 - x10 + x11
    T = D @ YCC_W.T

    def trip(a):
        return a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16)
    t00, t01, t10, t11 = trip(x00), trip(x01), trip(x10), trip(x11)
    eq = ((t00 == t01) & (t10 == t11)) | ((t00 == t10) & (t01 == t11))
    return T, eq


def h3_bin(a):
    """bin of |T| = a >= 1 (array or scalar): floor(log2 a) and the next MB bits"""
    a = np.asarray(a, np.int64)
    assert np.all(a >= 1) and np.all(a < (1 << 31))
    e = np.frexp(a.astype(np.float64))[1].astype(np.int64) - 1  # exact below 2^53
    m = np.where(e >= MB, a >> np.maximum(e - MB, 0), a << np.maximum(MB - e, 0)) & MM
    return (e << MB) + m


def h3_bin_lo(b):
    """the smallest |T| of bin b; 1 for the bins below 2^MB"""
    e = b >> MB
    return ((1 << MB) + (b & MM)) << (e - MB) if e >= MB else 1


def h3_bin_hi(b):
    """the largest |T| whose bin is <= b"""
    n = b + 1
    e = n >> MB
    if e >= 31:
        return 0xFFFFFFFF
    if e >= MB:
        return (((1 << MB) + (n & MM)) << (e - MB)) - 1
    hi = 0
    for a in range(1, 1 << MB):
        if int(h3_bin(a)) <= b:
            hi = a
    return hi


# ---- per channel ----------------------------------------------------------------------------------
@dataclass
class Channel:
    # the sample (wl_h3_window)
    n: int            # nonzero T in the sample
    nres: int         # T = 0, not an equal-triple pair, in the sample
    rho: float
    m: float
    s_klo: int        # sample ranks whose bins bound the window
    s_khi: int
    narrowed: bool    # n >= MIN_N
    lo: int
    hi: int
    # the whole image (wl_h3_stats)
    P: int            # level-1 positions
    n_t: int          # T != 0
    n_lo: int         # |T| < lo, zeros included
    n_c: int          # lo <= |T| <= hi
    n_res: int        # T = 0, not an equal-triple pair
    absT: np.ndarray  # sorted nonzero |T|

    def decide(self, nrnz):
        """wl_h3_sigma's ranks and branch given nrnz residues with a nonzero fp64 dd.  Returns a
        dict: N, klo, khi, base, fb (0 window / 1 fallback) and side: 'none' (no nonzero dd),
        'inside', 'above' (a median rank past the window's last |T|) or 'below'."""
        N = self.n_t + nrnz
        out = dict(N=N, klo=None, khi=None, base=None, fb=0, side="none")
        if N == 0:
            return out
        klo, khi = (N - 1) // 2, N // 2
        below = self.n_lo - (self.P - self.n_t)  # 0 < |T| < lo
        base = nrnz + below
        out.update(klo=klo, khi=khi, base=base)
        if klo >= base and khi < base + self.n_c:
            out["side"] = "inside"
        else:
            out["fb"] = 1
            out["side"] = "below" if klo < base else "above"
        return out

    def window_median(self, nrnz, rng):
        """the window path's sigma median: 0.5 (|T|_klo + |T|_khi) / 2 / (255000 range), formed as
        the kernel does; residues rank below every T != 0"""
        d = self.decide(nrnz)
        assert d["side"] == "inside"
        sc = 0.5 / (255000.0 * rng)
        tlo, thi = self.absT[d["klo"] - nrnz], self.absT[d["khi"] - nrnz]
        return (float(tlo) * sc + float(thi) * sc) / 2.0

    def candidates(self):
        """the |T| the window holds, sorted"""
        a = self.absT
        return a[(a >= self.lo) & (a <= self.hi)]

    def candidate_median(self, rng):
        """what a selection confined to the window's candidates would make of a fallback image:
        the median of the candidates alone, in the window path's units"""
        c = self.candidates()
        assert len(c)
        sc = 0.5 / (255000.0 * rng)
        return (float(c[(len(c) - 1) // 2]) * sc + float(c[len(c) // 2]) * sc) / 2.0


@dataclass
class Model:
    ch: list          # three Channel
    n_r: int          # residue positions of the image: some channel has T = 0, not an equal triple


def model(img):
    T, eq = finest_T(img)
    H1, W1 = eq.shape
    P = H1 * W1
    rows = np.arange(0, H1, SAMPLE)
    chans = []
    for c in range(3):
        Tc = T[..., c]
        a = np.abs(Tc)
        s = a[rows]
        seq = eq[rows]
        n = int((s != 0).sum())
        nres = int(((s == 0) & ~seq).sum())
        lo, hi = FULL
        rho = m = float("nan")
        s_klo = s_khi = -1
        if n >= MIN_N:
            rho = min(nres / n, 1.0)
            m = 2.0 / np.sqrt(float(n)) + 0.003
            qlo, qhi = 0.5 - 0.5 * rho - m, 0.5 + m
            s_klo, s_khi = int(np.floor(qlo * n)), int(np.ceil(qhi * n))
            bins = np.sort(h3_bin(s[s != 0]))
            if s_klo > 0:
                lo = h3_bin_lo(int(bins[s_klo]))
            if s_khi < n - 1:
                hi = h3_bin_hi(int(bins[s_khi]))
        nzT = a[a != 0]
        chans.append(Channel(
            n=n, nres=nres, rho=rho, m=m, s_klo=s_klo, s_khi=s_khi, narrowed=n >= MIN_N,
            lo=lo, hi=hi, P=P, n_t=int(len(nzT)), n_lo=int((a < lo).sum()),
            n_c=int(((a >= lo) & (a <= hi)).sum()), n_res=int(((a == 0) & ~eq).sum()),
            absT=np.sort(nzT)))
    n_r = int(((np.abs(T).min(axis=2) == 0) & ~eq).sum())
    return Model(chans, n_r)


# ---- the fp64 reference -----------------------------------------------------------------------------
@dataclass
class Reference:
    rng: np.ndarray     # YCbCr max - min per channel (fp64, the oracle's)
    count: np.ndarray   # nonzero finest dd per channel
    median: np.ndarray  # np.median(|nonzero dd|), NaN where there is none
    nrnz: np.ndarray    # nonzero dd among the positions with T = 0 (the residues that count)


def reference(img):
    """the oracle's finest dd of each normalised YCbCr channel (skimage's chain in fp64)"""
    import oracle
    from oracle.cv import matmul3_fma
    from oracle.wavelet import YCBCR_FROM_RGB, YCBCR_OFFSET
    T, _ = finest_T(img)
    ycc = matmul3_fma(img.astype(np.float64) * (1.0 / 255.0), YCBCR_FROM_RGB, post=YCBCR_OFFSET)
    rng, cnt, med, nrnz = np.zeros(3), np.zeros(3, np.int64), np.full(3, np.nan), np.zeros(3, np.int64)
    for c in range(3):
        mn, mx = ycc[..., c].min(), ycc[..., c].max()
        rng[c] = mx - mn
        with np.errstate(divide="ignore", invalid="ignore"):
            dd = oracle.wavelet.dwtn((ycc[..., c] - mn) / (mx - mn), "db1")["dd"]
        nz = dd != 0  # (NaN, a constant channel: counted as the kernels' keys count it)
        cnt[c] = int(nz.sum())
        nrnz[c] = int((nz & (T[..., c] == 0)).sum())
        if cnt[c]:
            med[c] = np.median(np.abs(dd[nz]))
    return Reference(rng, cnt, med, nrnz)


def bound(rng):
    """|window median - reference median| (haar3.hpp's header: the reference's dd is 0.5 T /
    (255000 range) within 2e-12 / range, the median's own rounding on top)"""
    return 2.1e-12 / rng


# ---- input families -------------------------------------------------------------------------------
SHAPES = [(256, 256), (136, 520)]
THRESHOLD_SHAPE = (128, 256)   # exactly 512 sample positions
FAMILIES = ["plain", "clipped", "quant", "quiet-sample", "loud-sample", "flat-sample", "gray",
            "plain-parity", "loud-sample-parity"]
WINDOW_FAMILIES = ["plain", "clipped", "quant", "flat-sample", "plain-parity"]
FALLBACK_FAMILIES = {"quiet-sample": "above", "loud-sample": "below", "loud-sample-parity": "below"}
CASES = ([(f, s) for f in FAMILIES for s in SHAPES] +
         [("threshold-512", THRESHOLD_SHAPE), ("threshold-511", THRESHOLD_SHAPE)])


def _pattern(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return (128 + 64 * np.sin(2 * np.pi * x / 97) * np.cos(2 * np.pi * y / 61))[..., None]


def _rows_sd(h, sampled, rest):
    """per-row noise sigma: `sampled` on the image rows the window kernel reads (32k, 32k + 1)"""
    sd = np.full(h, float(rest))
    sd[0::32] = sampled
    sd[1::32] = sampled
    return sd[:, None, None]


def _u8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def _one_value_group(img):
    """the top-left 2x2 group set to its first pixel: one T != 0 fewer per channel"""
    img = img.copy()
    img[0:2, 0:2] = img[0, 0]
    return img


@functools.lru_cache(maxsize=None)
def family(name, shape):
    """the u8 image of a family at a shape (fixed seeds; read-only)"""
    h, w = shape
    if name.endswith("-parity"):
        img = _one_value_group(family(name[:-len("-parity")], shape))
    elif name == "threshold-511":
        img = family("threshold-512", shape).copy()
        img[32:34, 8:10] = img[32, 8]  # one sampled group (level-1 row 16) flattened
    else:
        key = ["plain", "clipped", "quant", "quiet-sample", "loud-sample", "flat-sample", "gray",
               "threshold-512"].index(name)
        # (quant: seeds at which every channel's median rank sits in a run of > 200 equal |T| and
        # some channel's N is even, so the upper-middle tie test runs; test_h3_model.py checks)
        seed = {("quant", 256): 6457, ("quant", 136): 6341}.get((name, h), 6000 + 100 * key + h)
        rs = np.random.RandomState(seed)
        base = _pattern(h, w)
        if name in ("plain", "threshold-512"):
            img = _u8(base + rs.normal(0, 1, (h, w, 3)) * 20)
        elif name == "clipped":
            img = _u8(128 + rs.normal(0, 255, (h, w, 3)))
        elif name == "quant":
            img = _u8(base + rs.normal(0, 1, (h, w, 3)) * 30) & 0xE0
        elif name == "quiet-sample":
            img = _u8(base + rs.normal(0, 1, (h, w, 3)) * _rows_sd(h, 3, 40))
        elif name == "loud-sample":
            img = _u8(base + rs.normal(0, 1, (h, w, 3)) * _rows_sd(h, 40, 3))
        elif name == "flat-sample":
            img = _u8(base + rs.normal(0, 1, (h, w, 3)) * _rows_sd(h, 0, 40))
        else:  # gray: B = G = R, so Cb's and Cr's T is 0 everywhere
            img = np.repeat(_u8(base + rs.normal(0, 1, (h, w, 1)) * 20), 3, axis=2)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """(image, Model, Reference) of a family at a shape, computed once and shared"""
    img = family(name, shape)
    return img, model(img), reference(img)
