"""CPU: the float64 bilateral model (tests/bilateral_model.py) against the C oracle, the 1-LSB
rule on the fp32 oracle alone, and the proof that the rule notices a missing outermost tap."""
import numpy as np
import pytest

import bilateral_model as bm

RADII = tuple(range(1, bm.MAX_RADIUS + 1))
EXTRA_D = (1, 2, 4, 6, 10, 12, 16, 17)
SPECIAL = tuple(p for p, _ in bm.DERIVED) + bm.SIGMA_CLAMPS
SHAPE = (2, 21, 37)


def test_radius_of():
    for d in range(1, 20):
        assert bm.radius_of(d, 100.0) == max(d // 2, 1)
    for params, r in bm.DERIVED:
        assert bm.radius_of(params[0], params[2]) == r
    assert bm.radius_of(0, 6.0) == 9 and bm.radius_of(0, 0.0) == 2 and bm.radius_of(-3, -1.0) == 2
    assert [len(bm.taps(r)) for r in RADII] == [5, 13, 29, 49, 81, 113, 149, 197]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("params", [(2 * r + 1, 40.0, 2.5) for r in RADII]
                         + [(d, 40.0, 2.5) for d in EXTRA_D] + list(SPECIAL))
def test_model_equals_oracle_f64(c, params):
    """oracle.cv.bilateral_prefilter_f32 (fp64 sums, stored as float32) is the model's value
    rounded to float32: within half a float32 ulp at the value's magnitude, plus 1e-9 for the two
    fp64 summations"""
    import oracle
    img = bm.make_input("saltpepper", SHAPE + (c,), 11 + c)
    ref = oracle.cv.bilateral_prefilter_f32(img, *params).astype(np.float64)
    pre = bm.bilateral(img, *params)
    tol = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-9
    err = np.abs(ref - pre)
    print(f"max |oracle - model| = {err.max():.3g}")
    assert np.all(err <= tol), f"max excess {np.max(err - tol):.3g}"


@pytest.mark.parametrize("chunk", range(8))
def test_oracle_obeys_rule_on_gpu_cases(chunk):
    """oracle.cv.bilateral_filter (OpenCV's fp32 sums in OpenCV's order) obeys the 1-LSB rule
    against the model on every input the GPU file uses"""
    import oracle
    for family, shape, params in bm.all_cases()[chunk::8]:
        img, pre = bm.case(family, shape, params)
        bad, stats = bm.rule(oracle.cv.bilateral_filter(img, *params), pre)
        assert not bad, (family, shape, params, bad)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("r", RADII)
def test_rule_notices_a_dropped_outermost_tap(c, r):
    """a result that misses the tap (0, R) or (R, 0) fails the rule, while the full model's own
    bytes pass it: a kernel that drops an outermost tap cannot pass"""
    params = (2 * r + 1, 200.0, 100.0)
    img = bm.make_input("bytes", SHAPE + (c,), 50 + r)
    pre = bm.bilateral(img, *params)
    assert bm.rule(bm.to_u8(pre), pre)[0] == []
    for drop in ((0, r), (r, 0), (0, -r), (-r, 0)):
        bad, stats = bm.rule(bm.to_u8(bm.bilateral(img, *params, drop=drop)), pre)
        assert bad, (drop, stats)
        assert stats["mismatches"] >= 100, (drop, stats)


def test_rule_limits():
    """the rule's three clauses, each alone"""
    pre = np.full(4000, 10.2)
    got = np.full(4000, 10, np.uint8)
    assert bm.rule(got, pre)[0] == []
    g = got.copy()
    g[0] = 12
    assert any("more than 1" in s for s in bm.rule(g, pre)[0])
    g = got.copy()
    g[0] = 11  # a differing byte far from a boundary
    assert any("boundary" in s for s in bm.rule(g, pre)[0])
    pre2 = np.full(4000, 10.5 - 5e-4)
    g = got.copy()
    g[:4] = 11  # cap = max(2, 4) = 4
    assert bm.rule(g, pre2)[0] == []
    g[:5] = 11
    assert any("allowed" in s for s in bm.rule(g, pre2)[0])
    # pooled form
    assert bm.rule([got[:10], g[:5]], [pre[:10], pre2[:5]])[0] != []
