"""Pins the host model of the Philox noise streams (tests/philox_model.py): known answers of the
block function, the model's Poisson law against scipy's exact CDF, its normals against the normal
law, its gamma draws against scipy's gamma law, the disjointness of the streams' (counter, key)
sets, and the gamma rule of the GPU test on made-up outputs.  No GPU, no idn import."""
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
    additive noises (for gamma: attempts 0-3 and 63 and the boost block; the brownian blocks), and
    across image ids, for every shape the GPU tests use."""
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
            # gamma: the attempts of an element, its boost block, the other elements and images
            for att in (0, 1, 2, 3, pm.GAMMA_ATTEMPTS - 1, pm.GAMMA_BOOST):
                parts.append(_tuples(pm.ctr_gamma(elems, ids, att), pm.add_key(seed, pm.GAMMA)))
            parts.append(_tuples(pm.ctr_brownian(elems, ids), pm.add_key(seed, pm.BROWNIAN)))
            every = _pack(np.concatenate(parts, axis=1))
            assert np.unique(every).size == every.size, (n, elems)


def test_gamma_and_brownian_counters():
    """The attempt shares counter word 1 with the high word of the element index, the boost block
    lies past the attempt cap, and an element index above 2^32 moves word 1, not the attempt."""
    assert pm.GAMMA_ATTEMPTS <= pm.GAMMA_BOOST < 256
    ids = pm.image_ids(2, ids=[2 ** 40 + 5, 3])
    at = [0, 5, 2 ** 32 + 5, 2 ** 33 + 5]
    parts = [_tuples(pm.ctr_gamma(0, ids, att, elems_at=at), 7) for att in (0, 1, pm.GAMMA_BOOST)]
    c = np.concatenate(parts, axis=1)
    assert len({tuple(int(x) for x in col) for col in c.T}) == c.shape[1] == 24
    c0, c1, c2, c3 = pm.ctr_gamma(0, ids, 3, elems_at=at)
    assert c0.tolist() == [[0, 5, 5, 5]] and c1.tolist() == [[3, 3, 0x103, 0x203]]
    assert c2.ravel().tolist() == [5, 3] and c3.ravel().tolist() == [2 ** 8, 0]
    # an attempt block of one key is a uniform / Rayleigh block of another key only
    same = _pack(np.concatenate([_tuples(pm.ctr_gamma(64, ids, 0), 5),
                                 _tuples(pm.ctr_add(64, ids), 5)], axis=1))
    assert np.unique(same).size == same.size // 2
    # brownian: one block per four elements, elements 4q..4q+3 on block q
    c0, c1, _, _ = pm.ctr_brownian(10, ids)
    assert c0.tolist() == [[0, 1, 2]] and c1.tolist() == [[0, 0, 0]]
    assert pm._brownian_block([3, 4, 2 ** 34 + 7]).tolist() == [0, 1, 2 ** 32 + 1]


def _ks(x, cdf):
    x = np.sort(np.asarray(x, np.float64).ravel())
    n = x.size
    c = cdf(x)
    i = np.arange(1, n + 1)
    return max(np.max(i / n - c), np.max(c - (i - 1) / n)), n


@pytest.mark.parametrize("shape", [1.99, 0.5])
@pytest.mark.parametrize("seed", [0x1234, 5, SEEDS[0]])
def test_model_gamma_is_gamma(shape, seed):
    """KS of 10^6 model gamma draws of one image id against scipy's gamma(shape) at the 99.9 %
    bound; shape 0.5 goes through the boost block.  The rejection loop is alive and few draws sit
    near a decision."""
    from scipy.stats import gamma
    n = 10 ** 6
    m = pm.gamma_add(np.zeros((1, n), np.uint8), seed, pm.image_ids(1, offset=11), 1.0, shape)
    d, k = _ks(m["g"], gamma(shape).cdf)
    assert d < 1.9495 / np.sqrt(k), d
    assert np.array_equal(m["f64"], m["g"] * 1.0 + 0.0)
    rejected = (m["att"] > 0).mean()
    assert 0.01 < rejected < 0.04, rejected       # Marsaglia-Tsang: 2-3 % at a = 1.99 / 1.5
    assert m["near"].mean() < 1e-3


def test_model_brownian_normals_are_normal():
    """KS of 10^6 model brownian normals (and of each of the four lanes of a block, and of the
    pair sums, which are N(0, 2) only if cos and sin halves are independent); element 0 is 0."""
    n = 10 ** 6
    z = pm.brownian_normals(n, 0x1234, pm.image_ids(1, offset=11))[0]
    assert z[0] == 0.0
    z = z[4:]
    d, k = _ks_normal(z)
    assert d < 1.9495 / np.sqrt(k), d
    for lane in range(4):
        d, k = _ks_normal(z[lane::4])
        assert d < 1.9495 / np.sqrt(k), (lane, d)
    for a, b in ((0, 1), (2, 3), (0, 2), (1, 3)):
        d, k = _ks_normal((z[a::4] + z[b::4]) / np.sqrt(2.0))
        assert d < 1.9495 / np.sqrt(k), (a, b, d)
    m = pm.brownian_add(np.zeros((1, 64), np.uint8), 0x1234, pm.image_ids(1, offset=11), 0.09)
    assert np.array_equal(m["z"][0], pm.brownian_normals(n, 0x1234, pm.image_ids(1, offset=11))[0, :64])
    assert np.array_equal(m["inc"], 0.3 * m["z"]) and m["walk"][0, 0] == 0.0
    assert np.array_equal(m["walk"][0], np.cumsum(m["inc"][0]))


def test_gamma_model_on_the_gpu_inputs():
    """On the inputs of the GPU test: the rejection path is alive (some element goes past two
    attempts in every form), the near set at tau's cap stays below 1e-3 of the elements, and
    elems_at evaluates the same draws as the full model."""
    import test_noise_streams_gpu as gs
    assert gs.TAU <= 4e-6
    for shape, scale in gs.GAMMA_CASES:
        for form in gs.ADD_FORMS:
            n = form[1][0]
            flat = gs.make_imgs(form[1], 8).reshape(n, -1)
            m = pm.gamma_add(flat, form[2], gs.form_ids(form), scale, shape, tau=4e-6)
            assert m["att"].max() >= 2, (shape, form[0])
            assert m["near"].mean() < 1e-3, (shape, form[0], m["near"].mean())
            assert np.array_equal(m["near"], m["near_at"] <= 4e-6)
            assert all(m["near"].ravel()[r[0]] for r in m["alt"])
            at = np.arange(5, flat.shape[1], 7)
            sub = pm.gamma_add(flat[:, at], form[2], gs.form_ids(form), scale, shape, elems_at=at)
            assert np.array_equal(sub["f64"], m["f64"][:, at])
            assert np.array_equal(sub["att"], m["att"][:, at])
    form = gs.ADD_FORMS[0]
    flat = gs.make_imgs(form[1], 8).reshape(form[1][0], -1)
    # the GPU test's rule, on made-up outputs: a near element may hold its other decision's draw,
    # an element that is not near may not, and a third element on another attempt is too many
    m = pm.gamma_add(flat, form[2], gs.form_ids(form), 1.0, tau=4e-5)
    x = pm._x(flat)
    assert 3 <= len({r[0] for r in m["alt"]}) < 20
    assert gs.check_gamma("model", m["f64"], m, x, 1.0, tau=4e-5)[:3] == (0.0, 0.0, 0)
    out = m["f64"].copy()
    taken = []
    for i, g, _, _, att in m["alt"]:
        if i in taken:
            continue
        assert att != m["att"].ravel()[i] and g != m["g"].ravel()[i]
        taken.append(i)
        out.ravel()[i] = x.ravel()[i] + (g * 1.0 + 0.0)
        if len(taken) <= 2:
            _, tau_need, other, _ = gs.check_gamma("alt", out, m, x, 1.0, tau=4e-5)
            assert other == len(taken) and tau_need == m["near_at"].ravel()[taken].max()
        else:
            with pytest.raises(AssertionError):
                gs.check_gamma("three on another attempt", out, m, x, 1.0, tau=4e-5)
            break
    out = m["f64"].copy()
    out.ravel()[taken[0]] = x.ravel()[taken[0]] + m["alt"][0][1]
    with pytest.raises(AssertionError):     # the same value is no excuse at a tau below near_at
        gs.check_gamma("not near", out, m, x, 1.0, tau=0.5 * m["near_at"].ravel()[taken[0]])
    out = x + m["g"] * (1.0 + 20.0 * gs.EPS_G)
    with pytest.raises(AssertionError):
        gs.check_gamma("inaccurate", out, m, x, 1.0, tau=4e-5)
    m = pm.gamma_add(flat, form[2], gs.form_ids(form), 1.0)
    assert np.bincount(m["att"].ravel()).tolist() == [22640, 391, 8, 1]
    at = np.arange(3, flat.shape[1], 11)
    u = pm.uniform_add(flat, form[2], gs.form_ids(form), 0.7)
    usub = pm.uniform_add(flat[:, at], form[2], gs.form_ids(form), 0.7, elems_at=at)
    assert np.array_equal(usub["f64"], u["f64"][:, at])


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
