"""Pins the host model of the Philox noise streams (tests/philox_model.py): known answers of the
block function, the model's Poisson law against scipy's exact CDF, its normals against the normal
law, and the disjointness of the streams' (counter, key) sets.  No GPU, no idn import."""
import numpy as np
import pytest

import philox_model as pm


def _h(s):
    return [int(x, 16) for x in s.split()]


# Random123's published Philox4x32-10 known answers (kat_vectors), and the 7-round outputs of the
# same function; the 10-round vectors are the authority
KAT = [
    (10, "00000000 00000000 00000000 00000000", "00000000 00000000",
     "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    (10, "ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    (10, "243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
    (7, "00000000 00000000 00000000 00000000", "00000000 00000000",
     "5f6fb709 0d893f64 4f121f81 4f730a48"),
    (7, "ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "5207ddc2 45165e59 4d8ee751 8c52f662"),
    (7, "243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "4dfccaba 190a87f0 c47362ba b6b5242a"),
]


@pytest.mark.parametrize("rounds,ctr,key,out", KAT)
def test_philox_known_answers(rounds, ctr, key, out):
    k = _h(key)
    got = pm.philox4x32([np.array([c]) for c in _h(ctr)], (k[0], k[1]), rounds)
    assert [int(g[0]) for g in got] == _h(out)
    # the 64-bit key form: low word first
    got64 = pm.philox4x32([np.array([c]) for c in _h(ctr)], k[0] | (k[1] << 32), rounds)
    assert [int(g[0]) for g in got64] == _h(out)


def test_keys_and_ids():
    assert pm.key(0, 0) == 0x9E3779B97F4A7C15
    assert pm.key(0x9E3779B97F4A7C15, 0) == 0
    assert pm.key(5, 3) == 5 ^ ((4 * 0x9E3779B97F4A7C15) % 2 ** 64)
    assert len({pm.key(1, k) for k in range(4)} | {pm.add_key(1, k) for k in range(4, 8)}) == 8
    ids = pm.image_ids(3, offset=2 ** 32 - 1)
    assert ids.tolist() == [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    assert pm.image_ids(2, offset=2 ** 64 - 1).tolist() == [2 ** 64 - 1, 0]
    assert pm.image_ids(2, ids=[2 ** 40 + 5, 3]).tolist() == [2 ** 40 + 5, 3]


def test_model_poisson_law_is_the_law():
    """The integer thresholds of the recurrence's CDF rows equal those of the exact CDF wherever
    the exact CDF lies in [2^-34, 1 - 2^-34], for all 9 x 256 (vals, v) rows."""
    from scipy.stats import poisson
    k = np.arange(pm.POIS_KMAX)
    checked = 0
    for vi in range(pm.POIS_NV):
        lam = (np.arange(256) * (1.0 / 255.0)) * float(1 << vi)
        exact = poisson.cdf(k[None, :], lam[:, None])
        exact[0] = 1.0  # lambda = 0: the point mass at 0
        t_model = pm.poisson_thresholds(vi)
        t_exact = pm.thresholds_of(exact)
        inside = (exact >= 2.0 ** -34) & (exact <= 1.0 - 2.0 ** -34)
        bad = inside & (t_model != t_exact)
        assert not bad.any(), (vi, np.argwhere(bad)[:4])
        checked += int(inside.sum())
        rows = pm.poisson_cdf(vi)
        assert (np.diff(rows, axis=1) >= 0).all() and (rows[:, -1] == 1.0).all()
    assert checked > 100000, checked


def _ks_normal(z):
    from scipy.special import ndtr
    z = np.sort(np.asarray(z, np.float64).ravel())
    n = z.size
    c = ndtr(z)
    i = np.arange(1, n + 1)
    return max(np.max(i / n - c), np.max(c - (i - 1) / n)), n


@pytest.mark.parametrize("stream", ["u8", "f64"])
def test_model_normals_are_normal(stream):
    """KS of 10^6 model normals of one image id against the normal CDF at the 99.9 % bound
    (Kolmogorov: 1.9495 / sqrt(n)).  Also the cos and the sin halves of the pairs on their own, and
    (z0 + z1) / sqrt(2) of each pair, which is N(0, 1) only if the two halves are independent (a
    cos / cos pair has perfect marginals and fails here).  This guards the model, not the kernel."""
    n = 10 ** 6
    ids = pm.image_ids(1, offset=11)
    if stream == "u8":
        v = np.zeros((1, n), np.uint8)
        z = pm.gauss_u8(v, 0x1234, ids, pm.GAUSSIAN, 0.0, 1.0)["z"][0]
    else:
        z = pm.normals_f64(n, 0x1234, ids, pm.GAUSSIAN)[0]
    d, m = _ks_normal(z)
    assert d < 1.9495 / np.sqrt(m), d
    for half in (z[0::2], z[1::2]):
        d, m = _ks_normal(half)
        assert d < 1.9495 / np.sqrt(m), d
    # z0 + z1 of a pair is N(0, 2) for an independent pair
    d, m = _ks_normal((z[0::2] + z[1::2]) / np.sqrt(2.0))
    assert d < 1.9495 / np.sqrt(m), d


# the shapes of tests/test_noise_streams_gpu.py: (images, elements per image)
SHAPES = [(3, 40 * 64 * 3), (2, 37 * 53 * 3), (2, 33 * 47 * 1), (1, 96 * 128 * 3),
          (1, 600 * 1000 * 3)]
SEEDS = [0x9E3779B97F4A7C15, 0xFFFFFFFF00000001]


def _tuples(ctr, key):
    """the (c0, c1, c2 | c3 << 32, key) columns of every block, as uint64"""
    c = [np.ascontiguousarray(x).ravel() for x in np.broadcast_arrays(*ctr)]
    return np.stack([c[0], c[1], c[2] | (c[3] << np.uint64(32)),
                     np.full(c[0].shape, key, np.uint64)])


def _pack(cols):
    """exact packing of the tuples into one uint64 each: word 0 as is, the other three columns
    (few distinct values each) by their rank among the distinct values"""
    out = cols[0].copy()
    shift = 32
    for col in cols[1:]:
        distinct = np.unique(col)
        assert distinct.size < 256
        out |= np.searchsorted(distinct, col).astype(np.uint64) << np.uint64(shift)
        shift += 8
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_streams_are_disjoint(seed):
    """No (counter, key) tuple is used twice: across the five streams (u8 normals, their
    refinement blocks, s&p, Poisson, float64 normals -- Gaussian and speckle each), across the
    additive noises, and across image ids, for every shape the GPU tests use."""
    for n, elems in SHAPES:
        for ids in (pm.image_ids(n, offset=2 ** 32 - 1),
                    pm.image_ids(n, ids=[2 ** 40 + 5, 3, 2 ** 32][:n])):
            parts = []
            for kind in (pm.GAUSSIAN, pm.SPECKLE):
                k = pm.key(seed, kind)
                parts += [_tuples(pm.ctr_u8(elems, ids), k),
                          _tuples(pm.ctr_u8(elems, ids, pm.TAG_REFINE), k),
                          _tuples(pm.ctr_f64(elems, ids), k)]
            parts.append(_tuples(pm.ctr_sap(elems, ids), pm.key(seed, pm.SAP)))
            parts.append(_tuples(pm.ctr_poisson(elems, ids), pm.key(seed, pm.POISSON)))
            for kind in (pm.UNIFORM, pm.RAYLEIGH):
                parts.append(_tuples(pm.ctr_add(elems, ids), pm.add_key(seed, kind)))
            every = _pack(np.concatenate(parts, axis=1))
            assert np.unique(every).size == every.size, (n, elems)


def test_pack_sees_a_collision():
    """the disjointness check itself: two streams on one tag and key do collide"""
    ids = pm.image_ids(2, offset=0)
    a = _tuples(pm.ctr_u8(64, ids), 5)
    b = _tuples(pm.ctr_u8(64, ids, pm.TAG_REFINE), 5)
    both = _pack(np.concatenate([a, b], axis=1))
    assert np.unique(both).size == both.size
    same = _pack(np.concatenate([a, _tuples(pm.ctr_u8(64, ids, pm.TAG_U8), 5)], axis=1))
    assert np.unique(same).size == same.size // 2


def test_model_edges():
    """the mappings at their end points: u1 never 0, the refinement cell, s&p thresholds, the
    Poisson inversion at the ends of a row"""
    assert pm.sap_threshold(0.0) == 0 and pm.sap_threshold(1.0) == 65536
    assert pm.sap_threshold(0.5) == 32768 and pm.sap_threshold(0.2) == 13108
    t = pm.poisson_thresholds(8)
    assert (t[0] == 2 ** 32).all()          # lambda = 0: every word gives k = 0
    assert (t[:, -1] == 2 ** 32).all()      # the last entry closes every row
    v = np.arange(256, dtype=np.uint8)[None].repeat(3, 1)
    p = pm.poisson(v, 1, pm.image_ids(1))
    assert p["vi"].tolist() == [8] and (p["k"][0, v[0] == 0] == 0).all()
    one = pm.poisson(np.full((1, 64), 255, np.uint8), 1, pm.image_ids(1))
    assert one["vi"].tolist() == [0] and set(np.unique(one["f64"])) <= {0.0, 1.0}
    g = pm.gauss_u8(np.zeros((1, 20), np.uint8), 3, pm.image_ids(1), pm.SPECKLE, 0.0, 1.0)
    assert (g["byte"] == 0).all() and np.isfinite(g["z"]).all()
