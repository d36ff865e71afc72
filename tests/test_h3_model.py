"""The integer model of the Haar L = 3 sigma selection (tests/h3_model.py) against the fp64
oracle, and the input families of tests/test_haar3_window_gpu.py pinned to the branch of
csrc/haar3.hpp each is built for.  CPU only: the kernels are compared with the model on the GPU."""
import numpy as np
import pytest

import h3_model as hm


def _decisions(name, shape):
    img, M, R = hm.case(name, shape)
    return M, R, [M.ch[c].decide(int(R.nrnz[c])) for c in range(3)]


def test_bins_are_monotone_and_invertible():
    """h3_bin is monotone in |T|, h3_bin_lo / h3_bin_hi bracket every bin (bins below 2^6 share
    lo = 1), and consecutive bins tile the integers"""
    a = np.unique(np.concatenate([np.arange(1, 5000), 2 ** np.arange(1, 31), 2 ** np.arange(1, 31) - 1,
                                  2 ** np.arange(1, 31) + 1,
                                  np.random.RandomState(0).randint(1, 2 ** 31 - 1, 4000)]))
    b = hm.h3_bin(a)
    assert np.all(np.diff(b) >= 0)
    for ai, bi in zip(a.tolist(), b.tolist()):
        assert hm.h3_bin_lo(bi) <= ai <= hm.h3_bin_hi(bi)
        if ai >= 64 and (bi + 1) >> hm.MB < 31:  # (the last bin's upper end is 0xFFFFFFFF)
            assert int(hm.h3_bin(hm.h3_bin_lo(bi))) == bi and int(hm.h3_bin(hm.h3_bin_hi(bi))) == bi
            assert hm.h3_bin_hi(bi) + 1 == hm.h3_bin_lo(bi + 1)
    assert hm.h3_bin_hi(31 * 64 - 1) == 0xFFFFFFFF
    assert [hm.h3_bin_hi(int(hm.h3_bin(v))) for v in (1, 2, 3, 5, 63)] == [1, 2, 3, 5, 63]


@pytest.mark.parametrize("name,shape", hm.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_model_counts_match_oracle(name, shape):
    """the model's population is the reference's: every T != 0 is a nonzero fp64 dd (so the count
    is n_t plus the nonzero residues), and no equal-triple pair is one"""
    img, M, R = hm.case(name, shape)
    T, eq = hm.finest_T(img)
    for c in range(3):
        ch = M.ch[c]
        assert ch.P == (shape[0] // 2) * (shape[1] // 2)
        assert R.count[c] == ch.n_t + R.nrnz[c]
        assert R.nrnz[c] <= ch.n_res <= M.n_r
        assert ch.n_lo >= ch.P - ch.n_t and ch.n_lo - (ch.P - ch.n_t) + ch.n_c <= ch.n_t
    assert M.n_r == int((((T == 0).any(axis=2)) & ~eq).sum())


@pytest.mark.parametrize("shape", hm.SHAPES, ids=str)
@pytest.mark.parametrize("name", hm.WINDOW_FAMILIES)
def test_window_families(name, shape):
    """a-c, f, h: every channel takes the window; a-c and h on a narrowed one (n >= 512), f on the
    full one although the image is large; the model's median within the analytic bound of the
    oracle's np.median(|nonzero dd|)"""
    M, R, D = _decisions(name, shape)
    for c in range(3):
        ch, d = M.ch[c], D[c]
        assert d["fb"] == 0 and d["side"] == "inside", (name, shape, c, d)
        if name == "flat-sample":
            assert ch.n < hm.MIN_N and (ch.lo, ch.hi) == hm.FULL
            assert ch.n_c == ch.n_t > 15000  # every |T| is appended: flushes inside the loop
        else:
            assert ch.narrowed and 1 < ch.lo < ch.hi < 0xFFFFFFFF
            assert ch.n_c < ch.n_t // 4  # a real window: a fraction of the image's |T|
        err = abs(ch.window_median(int(R.nrnz[c]), R.rng[c]) - R.median[c])
        assert err <= hm.bound(R.rng[c]), (name, shape, c, err, hm.bound(R.rng[c]))


@pytest.mark.parametrize("shape", hm.SHAPES, ids=str)
def test_quant_family_ties_and_residues(shape):
    """c: more than 200 equal |T| at the median rank (the upper middle is the same value: the
    `le_s > rhi` side of the tie test) and hundreds of residue candidates, whose sample share
    rho widens the window downwards"""
    M, R, D = _decisions("quant", shape)
    assert M.n_r > 200
    for c in range(3):
        ch, d = M.ch[c], D[c]
        nrnz = int(R.nrnz[c])
        tlo, thi = ch.absT[d["klo"] - nrnz], ch.absT[d["khi"] - nrnz]
        assert tlo == thi and int((ch.absT == tlo).sum()) > 200
        assert ch.nres > 0 and ch.rho > 0
        # without rho the lower sample rank, and with it the window's lower bound, lies higher
        assert ch.s_klo < int(np.floor((0.5 - ch.m) * ch.n))
    assert max(ch.n_res for ch in M.ch) > 200
    assert any(d["N"] % 2 == 0 for d in D)  # rhi != rlo: the tie test itself runs


@pytest.mark.parametrize("shape", hm.SHAPES, ids=str)
@pytest.mark.parametrize("name", sorted(hm.FALLBACK_FAMILIES))
def test_fallback_families(name, shape):
    """d, e (and e's parity twin): the sample narrows the window (n >= 512) and misplaces it, so
    all three channels take the exact path, d with the rank above the window and e below it.
    Sensitivity: a selection confined to the window's candidates would miss the oracle's median
    by more than 1000 x the window path's bound"""
    M, R, D = _decisions(name, shape)
    for c in range(3):
        ch, d = M.ch[c], D[c]
        assert ch.narrowed and ch.n_c > 0
        assert d["fb"] == 1 and d["side"] == hm.FALLBACK_FAMILIES[name], (name, shape, c, d)
        if d["side"] == "below":
            assert d["klo"] < d["base"]
        else:
            assert d["klo"] >= d["base"] and d["khi"] >= d["base"] + ch.n_c
        miss = abs(ch.candidate_median(R.rng[c]) - R.median[c])
        assert miss > 1000 * hm.bound(R.rng[c]), (name, shape, c, miss)


@pytest.mark.parametrize("shape", hm.SHAPES, ids=str)
def test_gray_family(shape):
    """g: Y takes a narrowed window; Cb and Cr have T = 0 everywhere (no candidate, a full
    window), every group is a residue candidate, and their median is a residue: the fallback"""
    M, R, D = _decisions("gray", shape)
    assert M.ch[0].narrowed and D[0]["fb"] == 0 and D[0]["side"] == "inside"
    err = abs(M.ch[0].window_median(int(R.nrnz[0]), R.rng[0]) - R.median[0])
    assert err <= hm.bound(R.rng[0])
    for c in (1, 2):
        ch = M.ch[c]
        assert ch.n == 0 and (ch.lo, ch.hi) == hm.FULL and ch.n_t == 0 and ch.n_c == 0
        assert ch.n_lo == ch.P and ch.n_res > 0.99 * ch.P
        assert R.count[c] == R.nrnz[c] > 0
        assert D[c]["fb"] == 1 and D[c]["side"] == "below"


@pytest.mark.parametrize("shape", hm.SHAPES, ids=str)
@pytest.mark.parametrize("name", ["plain", "loud-sample"])
def test_parity_families(name, shape):
    """h: the one-value group removes one nonzero dd per channel, so N is even in one twin and
    odd in the other (rhi == rlo and rhi != rlo both run), on the parent's branch"""
    _, R0, D0 = _decisions(name, shape)
    _, R1, D1 = _decisions(name + "-parity", shape)
    for c in range(3):
        assert D1[c]["N"] == D0[c]["N"] - 1
        assert D1[c]["fb"] == D0[c]["fb"] and D1[c]["side"] == D0[c]["side"]
    assert {D0[c]["N"] % 2 for c in range(3)} | {D1[c]["N"] % 2 for c in range(3)} == {0, 1}


def test_threshold_family():
    """i: 128 x 256 has exactly 512 sample positions; all nonzero narrows the window (n = 512),
    one flattened sampled group leaves n = 511 and the full window"""
    shape = hm.THRESHOLD_SHAPE
    M0, R0, D0 = _decisions("threshold-512", shape)
    M1, R1, D1 = _decisions("threshold-511", shape)
    for c in range(3):
        assert M0.ch[c].n == 512 and M0.ch[c].narrowed and (M0.ch[c].lo, M0.ch[c].hi) != hm.FULL
        assert M0.ch[c].n_c < M0.ch[c].n_t // 4
        assert M1.ch[c].n == 511 and not M1.ch[c].narrowed and (M1.ch[c].lo, M1.ch[c].hi) == hm.FULL
        assert M1.ch[c].n_c == M1.ch[c].n_t
        for M, R, D in ((M0, R0, D0), (M1, R1, D1)):
            assert D[c]["fb"] == 0 and D[c]["side"] == "inside"
            err = abs(M.ch[c].window_median(int(R.nrnz[c]), R.rng[c]) - R.median[c])
            assert err <= hm.bound(R.rng[c])


def test_decide_edges():
    """the decision's own edges on a tiny hand-made channel: no nonzero dd, the median a residue,
    the ranks on the window's first and last candidate, one past either end"""
    def ch(n_t, n_lo_nz, n_c, P=100):
        return hm.Channel(n=0, nres=0, rho=0.0, m=0.0, s_klo=-1, s_khi=-1, narrowed=True, lo=10, hi=20,
                          P=P, n_t=n_t, n_lo=n_lo_nz + (P - n_t), n_c=n_c, n_res=0,
                          absT=np.arange(1, n_t + 1))
    assert ch(0, 0, 0).decide(0)["side"] == "none" and ch(0, 0, 0).decide(0)["fb"] == 0
    assert ch(0, 0, 0).decide(3)["side"] == "below"           # only residues
    assert ch(10, 4, 2).decide(0)["side"] == "inside"          # N = 10: ranks 4, 5 = base, base + 1
    assert ch(10, 5, 2).decide(0)["side"] == "below"           # klo = 4 < base = 5
    assert ch(10, 4, 1).decide(0)["side"] == "above"           # khi = 5 >= base + n_c = 5
    assert ch(10, 4, 2).decide(1)["side"] == "inside"          # N = 11: rank 5 = base
    assert ch(10, 4, 2).decide(2)["side"] == "below"           # N = 12: klo = 5 < base = 6
    assert ch(11, 5, 1).decide(0)["side"] == "inside"          # odd N: one rank
