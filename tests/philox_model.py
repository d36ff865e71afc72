"""Exact host model of the Philox noise streams (csrc/noise.hip, noise_poisson.hip, noise_apply.hpp,
noise_add.hip).

numpy only: the definition of the streams restated from the documented counter layout, keys and
integer mappings, so a test can ask "equal to the reference, draw for draw" instead of "has the
right law".  Everything is vectorised over elements; images are the leading axis.

    philox4x32(ctr4, key, rounds)            the block function (Random123's Philox4x32)
    key(seed, kind), add_key(seed, kind)     stream keys of random_noise / noise_add
    image_ids(n, offset, ids)                offset + i (mod 2^64) or the explicit list
    ctr_*(...)                               the counters of each stream
    gauss_u8 / sap / poisson / gauss_f64     skimage.util.random_noise modes on the two streams
    uniform_add / rayleigh_add               the additive noises that are one block's transform
    gamma_add / brownian_add                 the rejection loop and the four-normal walk

Images are passed as uint8 arrays of shape (n, elems): the flat (y, x, channel) element order of
each image.  Kinds are idn_noise_kind's numbers.
"""
import numpy as np

GAUSSIAN, SPECKLE, SAP, POISSON, UNIFORM, GAMMA, RAYLEIGH, BROWNIAN = range(8)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
KIND_TAG = 0x9E3779B97F4A7C15
ADD_TAG = 0xD1B54A32D192ED03
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1

TAG_U8, TAG_SAP, TAG_F64, TAG_REFINE = 0, 1, 2, 3
POIS_FLAG = 0x80000000
POIS_KMAX = 512
POIS_NV = 9


def philox4x32(ctr4, key, rounds=10):
    """ctr4: four uint32-valued arrays (broadcast together); key: a 64-bit int or a (k0, k1)
    pair.  Returns the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in np.broadcast_arrays(*ctr4)]
    if isinstance(key, (tuple, list)):
        k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    else:
        k0, k1 = int(key) & MASK32, (int(key) >> 32) & MASK32
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32,
             (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def key(seed, kind):
    return (int(seed) & MASK64) ^ ((KIND_TAG * (int(kind) + 1)) & MASK64)


def add_key(seed, kind):
    return (int(seed) & MASK64) ^ ((ADD_TAG * (int(kind) + 1)) & MASK64)


def image_ids(n, offset=0, ids=None):
    if ids is not None:
        out = [int(i) & MASK64 for i in ids]
        assert len(out) == n
    else:
        out = [(int(offset) + i) & MASK64 for i in range(n)]
    return np.array(out, dtype=np.uint64)


def _lo(x):
    return np.asarray(x, np.uint64) & np.uint64(MASK32)


def _hi(x):
    return np.asarray(x, np.uint64) >> np.uint64(32)


def _ctr(c0, c1, ids):
    """(n, m) counter words from per-block words c0, c1 (m,) and image ids (n,)"""
    ids = np.asarray(ids, np.uint64).reshape(-1, 1)
    c0 = np.asarray(c0, np.uint64).reshape(1, -1)
    c1 = np.broadcast_to(np.asarray(c1, np.uint64), c0.shape[1:]).reshape(1, -1)
    return c0, c1, _lo(ids), _hi(ids)


def ctr_u8(elems, ids, tag=TAG_U8):
    """u8 Gaussian / speckle: one block per 8 elements, (q, 0, id); refinement blocks (q, 3, id)"""
    q = np.arange((elems + 7) // 8, dtype=np.uint64)
    return _ctr(q, tag, ids)


def ctr_sap(elems, ids):
    q = np.arange((elems + 3) // 4, dtype=np.uint64)
    return _ctr(q, TAG_SAP, ids)


def ctr_poisson(elems, ids):
    q = np.arange((elems + 3) // 4, dtype=np.uint64)
    return _ctr(_lo(q), _hi(q) ^ np.uint64(POIS_FLAG), ids)


def ctr_f64(elems, ids):
    pr = np.arange((elems + 1) // 2, dtype=np.uint64)
    return _ctr(_lo(pr), np.uint64(TAG_F64) ^ (_lo(_hi(pr) << np.uint64(8))), ids)


def _elems(elems, elems_at=None):
    """the element indices a model is evaluated on: 0..elems-1, or the chosen ones"""
    if elems_at is None:
        return np.arange(elems, dtype=np.uint64)
    return np.asarray(elems_at, np.uint64).ravel()


def ctr_add(elems, ids, elems_at=None):
    e = _elems(elems, elems_at)
    return _ctr(_lo(e), _hi(e), ids)


GAMMA_BOOST = 0xFF      # the attempt number of the boost block (shape < 1)
GAMMA_ATTEMPTS = 64     # the kernel's attempt cap: attempts 0..63 never reach the boost block


def _gamma_c01(e, att):
    """counter words 0, 1 of element e's attempt att: (e_lo, (e_hi << 8) | att)"""
    e = np.asarray(e, np.uint64)
    return _lo(e), _lo(_hi(e) << np.uint64(8)) | np.uint64(att)


def ctr_gamma(elems, ids, att, elems_at=None):
    """gamma: one block per element and attempt; att = GAMMA_BOOST is the boost block"""
    c0, c1 = _gamma_c01(_elems(elems, elems_at), att)
    return _ctr(c0, c1, ids)


def _brownian_block(e):
    """the block whose four normals elements 4q..4q+3 take: q = e // 4"""
    return np.asarray(e, np.uint64) >> np.uint64(2)


def ctr_brownian(elems, ids):
    q = _brownian_block(np.arange(0, elems, 4, dtype=np.uint64))
    return _ctr(_lo(q), _hi(q), ids)


def _words(blocks, elems):
    """(n, nblocks) x 4 words -> (n, elems): element e takes word e % 4 of block e // 4"""
    w = np.stack(blocks, axis=-1)
    return w.reshape(w.shape[0], -1)[:, :elems]


def _sd(var):
    return float(var) ** 0.5  # random_noise: var ** 0.5


def _x(v):
    """img_as_float of a byte: v * (1 / 255) in float64"""
    return np.asarray(v, np.float64) * (1.0 / 255.0)


# ---- u8 Gaussian / speckle --------------------------------------------------------------------
def gauss_u8(v, seed, ids, kind, mean, var):
    """v: (n, elems) uint8.  Returns dict(z, pre, byte, refined): the float64 normals, the value
    before the floor on the 0..255 scale, the byte floor(clip(pre, 0, 255)) and the mask of
    elements whose pair took its u1 from the refinement block."""
    v = np.asarray(v)
    n, elems = v.shape
    k = key(seed, kind)
    nb = (elems + 7) // 8
    w = np.stack(philox4x32(ctr_u8(elems, ids), k, 7), axis=-1)        # (n, nb, 4): word p
    f = np.stack(philox4x32(ctr_u8(elems, ids, TAG_REFINE), k, 7), axis=-1)
    lo16 = w & np.uint64(0xFFFF)
    refined = lo16 == 0
    u1 = (lo16.astype(np.float64) + 1.0) * 2.0 ** -16
    u1r = ((f & np.uint64(0xFFFF)).astype(np.float64) + 1.0) * 2.0 ** -32
    u1 = np.where(refined, u1r, u1)
    u2 = (w >> np.uint64(16)).astype(np.float64) * 2.0 ** -16
    rad = np.sqrt(-2.0 * np.log(u1))
    th = 2.0 * np.pi * u2
    z = np.stack([rad * np.cos(th), rad * np.sin(th)], axis=-1)        # (n, nb, 4, 2)
    z = z.reshape(n, nb * 8)[:, :elems]
    refined = np.repeat(refined.reshape(n, nb * 4), 2, axis=1)[:, :elems]
    vf = v.astype(np.float64)
    noise = float(mean) + _sd(var) * z
    pre = vf + (255.0 if kind == GAUSSIAN else vf) * noise
    byte = np.floor(np.clip(pre, 0.0, 255.0)).astype(np.uint8)
    return dict(z=z, pre=pre, byte=byte, refined=refined)


# ---- salt & pepper ----------------------------------------------------------------------------
def sap_threshold(pp):
    t = np.ceil(pp * 65536.0)
    return 0 if t <= 0.0 else 65536 if t >= 65536.0 else int(t)


def sap(v, seed, ids, amount, salt_vs_pepper):
    """Returns dict(byte, f64, flip, salt)"""
    v = np.asarray(v)
    n, elems = v.shape
    p0 = amount / (amount + (1.0 - amount))
    p1 = salt_vs_pepper / (salt_vs_pepper + (1.0 - salt_vs_pepper))
    w = _words(philox4x32(ctr_sap(elems, ids), key(seed, SAP), 7), elems)
    flip = (w & np.uint64(0xFFFF)) < np.uint64(sap_threshold(p0))
    salt = (w >> np.uint64(16)) < np.uint64(sap_threshold(p1))
    x = _x(v)
    keep = (255.0 * x).astype(np.uint8)  # trunc: v, or v - 1 where v / 255 * 255 rounds below v
    byte = np.where(flip, np.where(salt, 255, 0), keep).astype(np.uint8)
    f64 = np.where(flip, np.where(salt, 1.0, 0.0), x)
    return dict(byte=byte, f64=f64, flip=flip, salt=salt)


# ---- Poisson ----------------------------------------------------------------------------------
_POIS = {}


def poisson_cdf(vi):
    """(256, 512) float64 CDF rows of level vals = 2**vi, lambda = v * (1/255) * vals, by the
    kernel's recurrence in the kernel's op order"""
    if ("cdf", vi) not in _POIS:
        lam = _x(np.arange(256)) * float(1 << vi)
        p = np.exp(-lam)
        acc = np.zeros(256)
        cdf = np.empty((256, POIS_KMAX))
        for k in range(POIS_KMAX):
            acc = acc + p
            cdf[:, k] = 1.0 if k == POIS_KMAX - 1 else np.minimum(acc, 1.0)
            p = p * lam / float(k + 1)
        _POIS["cdf", vi] = cdf
    return _POIS["cdf", vi]


def thresholds_of(cdf):
    """t_k = ceil(cdf * 2^32 - 1/2) as int64 (exact: cdf * 2^32 - 1/2 is exact in float64 or
    rounds to a value with the same ceil); cdf[k] > (w + 1/2) 2^-32  <=>  w < t_k"""
    return np.ceil(np.asarray(cdf, np.float64) * 2.0 ** 32 - 0.5).astype(np.int64)


def poisson_thresholds(vi):
    if ("t", vi) not in _POIS:
        _POIS["t", vi] = thresholds_of(poisson_cdf(vi))
    return _POIS["t", vi]


def poisson_vals(v):
    """per image 2**ceil(log2(#distinct values)) -> the level index log2(vals)"""
    out = []
    for row in np.asarray(v):
        cnt = len(np.unique(row))
        vi = 0
        while (1 << vi) < cnt:
            vi += 1
        out.append(vi)
    return np.array(out, dtype=np.int64)


def poisson_words(elems, seed, ids):
    return _words(philox4x32(ctr_poisson(elems, ids), key(seed, POISSON), 7), elems)


def poisson(v, seed, ids):
    """Returns dict(k, byte, f64, w, vi, at_threshold): the counts, both outputs, the Philox
    words, the per-image level and the mask of draws whose word equals t_k or t_k - 1 of the
    chosen neighbourhood (the only draws a last-bit difference in exp can move, by one count)."""
    v = np.asarray(v)
    n, elems = v.shape
    w = poisson_words(elems, seed, ids).astype(np.int64)
    vi = poisson_vals(v)
    k = np.empty((n, elems), np.int64)
    at = np.zeros((n, elems), bool)
    for level in np.unique(vi):
        t = poisson_thresholds(int(level))                    # (256, 512) nondecreasing rows
        sel = vi == level
        rows = v[sel].astype(np.int64)
        ws = w[sel]
        # one sorted search for all rows: row r's thresholds live in [r 2^33, r 2^33 + 2^32]
        keys = (t + (np.arange(256, dtype=np.int64) << 33)[:, None]).ravel()
        pos = np.searchsorted(keys, ws + (rows << 33), side="right")  # thresholds <= w, all rows
        kk = pos - rows * POIS_KMAX
        k[sel] = kk
        tk = t[rows, np.minimum(kk, POIS_KMAX - 1)]           # first threshold above w
        tp = t[rows, np.maximum(kk - 1, 0)]                   # last threshold at or below w
        at[sel] = (ws == tk - 1) | ((kk > 0) & (ws == tp))
    assert k.min() >= 0 and k.max() < POIS_KMAX
    shift = vi[:, None]
    byte = np.minimum((255 * k) >> shift, 255).astype(np.uint8)
    f64 = np.minimum(k.astype(np.float64) / (1 << shift).astype(np.float64), 1.0)
    return dict(k=k, byte=byte, f64=f64, w=w, vi=vi, at_threshold=at)


# ---- float64 Gaussian / speckle ---------------------------------------------------------------
_LD = np.longdouble
EXTENDED = np.finfo(_LD).eps <= 2.0 ** -63


def _normals_from_u53(a1, b):
    """z0, z1 = sqrt(-2 ln(a1 2^-53)) (cos, sin)(2 pi b 2^-53) from the integers, evaluated in
    extended precision (80-bit long double, or mpmath where long double is only a double) and
    rounded to float64 once"""
    if EXTENDED:
        u1 = a1.astype(_LD) * _LD(2.0) ** -53              # exact: a1 <= 2^53 < 2^64
        rad = np.sqrt(_LD(-2.0) * np.log(u1))
        # angle in eighths of a turn: b 2^-53 = (oct + fr) / 8, fr in [0, 1) exact
        octant = (b >> np.uint64(50)).astype(np.int64)
        fr = (b & np.uint64((1 << 50) - 1)).astype(_LD) * _LD(2.0) ** -50
        pi4 = _LD(np.pi) + _LD(1.2246467991473532e-16)     # pi to 2^-106, rounded to long double
        ang = fr * (pi4 / _LD(4.0))
        s, c = np.sin(ang), np.cos(ang)
        r2 = np.sqrt(_LD(0.5))
        s45, c45 = (s + c) * r2, (c - s) * r2              # rotate by 45 degrees for odd octants
        odd = (octant & 1) == 1
        s1, c1 = np.where(odd, s45, s), np.where(odd, c45, c)
        quad = octant >> 1                                  # then by quarter turns
        cs = np.select([quad == 0, quad == 1, quad == 2], [c1, -s1, -c1], s1)
        sn = np.select([quad == 0, quad == 1, quad == 2], [s1, c1, -s1], -c1)
        return (rad * cs).astype(np.float64), (rad * sn).astype(np.float64)
    import mpmath
    mpmath.mp.prec = 100
    z0 = np.empty(a1.shape)
    z1 = np.empty(a1.shape)
    for i, (x, y) in enumerate(zip(a1.ravel().tolist(), b.ravel().tolist())):
        rad = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(x) / 2 ** 53))
        th = 2 * mpmath.pi * mpmath.mpf(y) / 2 ** 53
        z0.flat[i] = float(rad * mpmath.cos(th))
        z1.flat[i] = float(rad * mpmath.sin(th))
    return z0, z1


def normals_f64(elems, seed, ids, kind):
    """(n, elems) float64 standard normals of the float64 stream"""
    x, y, z, w = philox4x32(ctr_f64(elems, ids), key(seed, kind), 10)
    a = (x << np.uint64(21)) | (y >> np.uint64(11))
    b = (z << np.uint64(21)) | (w >> np.uint64(11))
    z0, z1 = _normals_from_u53(a + np.uint64(1), b)
    zz = np.stack([z0, z1], axis=-1)
    return zz.reshape(zz.shape[0], -1)[:, :elems]


def gauss_f64(v, seed, ids, kind, mean, var):
    """Returns dict(z, f64, byte): n = mean + sd z, out = clip(x + n) or clip(x + x n) in numpy's
    float64 op order, byte = trunc(255 out)"""
    v = np.asarray(v)
    z = normals_f64(v.shape[1], seed, ids, kind)
    noise = float(mean) + _sd(var) * z
    x = _x(v)
    out = np.clip(x + noise if kind == GAUSSIAN else x + x * noise, 0.0, 1.0)
    return dict(z=z, f64=out, byte=(out * 255.0).astype(np.uint8))


# ---- additive noises that are a fixed transform of one block -----------------------------------
def uniform_add(v, seed, ids, high, elems_at=None):
    """out = x + (0 + high * u), u = 53-bit random_sample of words 0 and 1.  elems_at: the element
    indices the columns of v stand for (default 0..elems-1)."""
    v = np.asarray(v)
    x, y, _, _ = philox4x32(ctr_add(v.shape[1], ids, elems_at), add_key(seed, UNIFORM), 10)
    bits = ((x >> np.uint64(5)) << np.uint64(26)) | (y >> np.uint64(6))
    u = bits.astype(np.float64) * 2.0 ** -53
    return dict(u=u, f64=_x(v) + (0.0 + float(high) * u))


def rayleigh_add(v, seed, ids, scale):
    """unit = sqrt(-2 ln u), u = fp32(fp32(w0) + 0.5) * 2^-32: the two fp32 roundings of the
    uniform are IEEE conversions and restated bit for bit, the log and the root are evaluated in
    float64 on that value.  out = x + (unit * scale + 0)."""
    v = np.asarray(v)
    x, _, _, _ = philox4x32(ctr_add(v.shape[1], ids), add_key(seed, RAYLEIGH), 10)
    uf = (x.astype(np.uint32).astype(np.float32) + np.float32(0.5)).astype(np.float64) * 2.0 ** -32
    unit = np.sqrt(-2.0 * np.log(uf))
    unit = np.where(uf >= 1.0, 0.0, unit)
    return dict(u=uf, unit=unit, f64=_x(v) + (unit * float(scale) + 0.0))


# ---- gamma: Marsaglia-Tsang on one block per attempt ---------------------------------------------
def _u24(w):
    """((float)(w >> 8) + 1) * 2^-24 and (float)(w >> 8) * 2^-24 are exact in fp32"""
    return (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def _u_tail(w):
    """fp32(fp32(w) + 0.5) * 2^-32: two IEEE roundings, then an exact scaling; in (0, 1]"""
    return (w.astype(np.uint32).astype(np.float32) + np.float32(0.5)).astype(np.float64) * 2.0 ** -32


def _pair_normals(wa, wb):
    """Box-Muller pair of two words: sqrt(-2 ln u1) (cos, sin)(2 pi u2), 24-bit u1 in (0, 1] and
    u2 in [0, 1), float64"""
    rad = np.sqrt(-2.0 * np.log(_u24(wa) + 2.0 ** -24))
    th = 2.0 * np.pi * _u24(wb)
    return rad * np.cos(th), rad * np.sin(th)


def gamma_add(v, seed, ids, scale, shape=1.99, elems_at=None, tau=4e-6):
    """The kernel's rejection loop, decision for decision, in float64 on the kernel's uniforms.
    a = fp32(shape) (+ 1 below 1, with boost = u_b^(1/a) from the boost block), d = a - 1/3,
    c = 1 / sqrt(9 d); attempt t draws z = cos-normal of words 0, 1 and u from word 2 of block
    (e_lo, (e_hi << 8) | t, id), v1 = 1 + c z, and accepts when v1 > 0 and
    margin = z^2/2 + d - d v + d ln v - ln u > 0, v = v1^3: g = d v boost.

    Returns a dict of (n, elems) arrays: g, att, z, v1 (of the accepted attempt), boost, ln_ub
    (ln of the boost uniform, 0 without boost), f64 = x + (g scale + 0), near_at and
    near = near_at <= tau, plus the scalars a (fp32(shape)), d, c.  near_at is the smallest, over
    the attempts up to the accepted one, of |v1| / (1 + c |z|) and, where v1 > 0, |margin| / S,
    S = 1 + z^2/2 + d v + |d ln v| + |ln u|: how close, relative to the size of its terms, the
    element came to another decision.  alt lists what a near element gives if one such decision
    falls the other way: rows (flat index, g, z, v1, att) for accepting a near attempt the model
    rejected, and for the next attempt the model accepts after an accepted near one."""
    v = np.asarray(v)
    n, m = v.shape
    e = _elems(m, elems_at)
    ids = np.asarray(ids, np.uint64).ravel()
    k = add_key(seed, GAMMA)
    size = n * m
    row, col = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
    ee, c2, c3 = e[col], _lo(ids)[row], _hi(ids)[row]
    a0 = float(np.float32(shape))
    a = a0
    boost, ln_ub = np.ones(size), np.zeros(size)
    if a < 1.0:
        c0, c1 = _gamma_c01(ee, GAMMA_BOOST)
        ln_ub = np.log(_u_tail(philox4x32((c0, c1, c2, c3), k, 10)[0]))
        boost = np.exp(ln_ub / a)
        a = float(np.float32(a) + np.float32(1.0))
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = {name: np.full(size, np.nan) for name in ("g", "z", "v1")}
    att_of = np.full(size, -1, np.int64)
    near_at = np.full(size, np.inf)
    waiting = np.zeros(size, bool)      # accepted at a near attempt: drawn on for alt
    alt = []
    live = np.arange(size)
    for att in range(GAMMA_ATTEMPTS):
        if live.size == 0:
            break
        c0, c1 = _gamma_c01(ee[live], att)
        w = philox4x32((c0, c1, c2[live], c3[live]), k, 10)
        z = _pair_normals(w[0], w[1])[0]
        v1 = 1.0 + c * z
        pos = v1 > 0.0
        vv = np.where(pos, v1, 1.0) ** 3
        ln_u = np.log(_u_tail(w[2]))
        margin = 0.5 * z * z + d - d * vv + d * np.log(vv) - ln_u
        s = 1.0 + 0.5 * z * z + d * vv + np.abs(d * np.log(vv)) + np.abs(ln_u)
        close = np.minimum(np.abs(v1) / (1.0 + c * np.abs(z)),
                           np.where(pos, np.abs(margin) / s, np.inf))
        acc = pos & (margin > 0.0)
        g = d * vv * boost[live]
        first = ~waiting[live]
        near_at[live[first]] = np.minimum(near_at[live[first]], close[first])
        nr = close <= tau
        for sel in (first & nr & ~acc & pos, ~first & acc):
            alt += [(int(i), float(gg), float(zz), float(vv1), att)
                    for i, gg, zz, vv1 in zip(live[sel], g[sel], z[sel], v1[sel])]
        sel = first & acc
        out["g"][live[sel]], out["z"][live[sel]], out["v1"][live[sel]] = g[sel], z[sel], v1[sel]
        att_of[live[sel]] = att
        waiting[live[sel & nr]] = True
        live = live[~acc | (sel & nr)]
    assert (att_of >= 0).all()
    shp = (n, m)
    res = {name: val.reshape(shp) for name, val in out.items()}
    res.update(att=att_of.reshape(shp), boost=boost.reshape(shp), ln_ub=ln_ub.reshape(shp),
               near_at=near_at.reshape(shp), near=(near_at <= tau).reshape(shp), alt=alt,
               a=a0, d=d, c=c)
    res["f64"] = _x(v) + (res["g"] * float(scale) + 0.0)
    return res


# ---- brownian: four normals per block, a sequential walk ------------------------------------------
def brownian_normals(elems, seed, ids):
    """(n, elems) float64: element e takes normal e % 4 of block e // 4 -- cos, sin of words 0, 1,
    then cos, sin of words 2, 3; element 0 is 0 (B_0 = 0)"""
    x, y, z, w = philox4x32(ctr_brownian(elems, ids), add_key(seed, BROWNIAN), 10)
    z0, z1 = _pair_normals(x, y)
    z2, z3 = _pair_normals(z, w)
    zz = _words([z0, z1, z2, z3], elems).copy()
    zz[:, 0] = 0.0
    return zz


def brownian_add(v, seed, ids, dt):
    """Returns dict(z, inc, walk): the normals, the increments sqrt(dt) z and their sequential
    np.cumsum.  The byte output is a function of the device's own walk (see the GPU test)."""
    v = np.asarray(v)
    z = brownian_normals(v.shape[1], seed, ids)
    inc = np.sqrt(float(dt)) * z
    return dict(z=z, inc=inc, walk=np.cumsum(inc, axis=1))
