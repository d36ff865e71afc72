"""CPU: the exact host model of the quant k-means fit (tests/quant_fit_model.py) is a sound fit,
obeys its own scheme, and the case table tests/quant_fit_cases.py has the power to tell a fit
that breaks one rule of the scheme from one that keeps it.  tests/test_quant_fit_gpu.py holds the
kernel to this model bit for bit.

The 100-iteration cap of the Lloyd loop is restated in the model and reached by no case here (the
longest run takes 85 iterations, asserted below as < 100)."""
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import cvlab

import quant_fit_cases as qc
import quant_fit_model as qm

GOLD = Path(__file__).resolve().parent / "golden"


def test_fixture_quality_vs_sklearn():
    """the model's fit of the sklearn fixtures (seed 7, id 0): whole-image inertia within 5 % of
    MiniBatchKMeans's recorded inertia, the bound tests/test_quant_gpu.py holds the kernel to"""
    z = np.load(GOLD / "quant.npz", allow_pickle=False)
    meta = json.loads((GOLD / "quant.json").read_text())
    assert len(meta["quant"]) == 12
    ratios = []
    for q in meta["quant"]:
        img = z["in_" + q["input"]]
        cen, runs = qm.fit(img, q["k"], seed=7, image_id=0)
        r = cvlab.inertia(cvlab.bgr2lab(img), cen) / q["inertia"]
        ratios.append((q["case"], round(r, 4), [run["iters"] for run in runs]))
        assert r <= 1.05, (q["case"], r)
    print("inertia ratio model / sklearn, iterations:", ratios)


@pytest.mark.parametrize("name", list(qc.CASES))
def test_fixed_point_and_counters(name):
    img_name, k, gid = qc.CASES[name]
    cen, runs = qc.case_model(name)
    img = qc.image(img_name)
    pts = qm.samples(img, qc.SEED, gid)
    assert len(pts) == min(img.shape[0] * img.shape[1], qm.SAMPLES) and len(runs) == qm.NINIT
    nt = qm.ntrials(k)
    for r, run in enumerate(runs):
        assert run["iters"] < qm.MAX_ITER
        # the fp32 centres at exit assign every sample to the cluster whose exact mean they are
        lab = qm.assign32(pts.astype(np.float32), run["cen32"])
        sums, counts = qm.cluster_sums(pts, lab, k)
        assert np.array_equal(counts, run["counts"])
        ne = counts > 0
        assert run["nonempty"] == int(ne.sum()) >= 1
        mean = sums[ne].astype(np.float64) / counts[ne, None]
        assert np.array_equal(run["centres"][ne], mean)
        assert np.array_equal(run["cen32"][ne], mean.astype(np.float32))
        assert np.array_equal(run["centres"][~ne], run["cen32"][~ne].astype(np.float64))
        # the inertia is the plain sum up to the reduction order's rounding
        d = ((pts[:, None, :] - run["centres"][None]) ** 2).sum(-1).min(1)
        assert run["inertia"] == pytest.approx(float(d.sum()), rel=1e-12, abs=1e-9)
        # the restart's draws: consecutive counters from where the sequential form's stood
        first = r * (1 + (k - 1) * nt)
        assert run["ctrs"] == list(range(first, first + len(run["ctrs"])))
        assert 1 <= len(run["ctrs"]) <= 1 + (k - 1) * nt
        if name not in ("F", "G"):
            assert len(run["ctrs"]) == 1 + (k - 1) * nt
    best = min(range(qm.NINIT), key=lambda r: (runs[r]["inertia"], r))
    assert np.array_equal(cen, runs[best]["centres"])


def test_degenerate_cases_reach_what_they_claim():
    # F: two colours -> after the second centre the potential is 0: no further draw, sample 0
    # again and again, so duplicates and three empty clusters
    _, runs = qc.case_model("F")
    for run in runs:
        assert len(run["ctrs"]) == 1 + qm.ntrials(5) and run["nonempty"] == 2
        assert len(np.unique(run["seeds"], axis=0)) == 2
    _, runs = qc.case_model("G")
    for run in runs:
        assert len(run["ctrs"]) == 1 and run["nonempty"] == 1 and run["inertia"] == 0.0
    # K: k = S, every sample its own centre
    _, runs = qc.case_model("K")
    for run in runs:
        assert run["nonempty"] == 4 and run["inertia"] == 0.0
    # A1: the one centre is the exact Lab mean of the image
    cen, _ = qc.case_model("A1")
    lab = cvlab.bgr2lab(qc.image("16x24")).reshape(-1, 3).astype(np.int64)
    assert np.array_equal(cen[0], lab.sum(0).astype(np.float64) / len(lab))
    # C and D are sampled, B (h w = 8192) is not
    for name, sampled in (("B", False), ("C", True), ("D", True)):
        img_name, k, gid = qc.CASES[name]
        img = qc.image(img_name)
        pts = qm.samples(img, qc.SEED, gid)
        assert len(pts) == qm.SAMPLES
        same = np.array_equal(pts, cvlab.bgr2lab(img).reshape(-1, 3)[:qm.SAMPLES])
        assert same != sampled, name


def _runs_differ(a, b):
    return any(not np.array_equal(x["centres"], y["centres"]) for x, y in zip(a, b))


@pytest.mark.parametrize("mutation", qm.MUTATIONS)
def test_cases_detect_a_broken_rule(mutation):
    """a fit that breaks one rule of the scheme differs from the model in some restart's centres
    on at least one table case (so the bit-equality of the GPU tests would catch it).  The
    degenerate cases cannot stand in for the others: F and G see neither the cumulative order nor
    the choice of trial."""
    seen = {}
    for name in qc.CASES:
        if mutation == "lo_id" and name != "E":
            continue  # only E's id has a high word
        _, base = qc.case_model(name)
        _, mut = qc.case_model(name, mutate=mutation)
        seen[name] = _runs_differ(base, mut)
    print(mutation, "changes:", sorted(n for n, v in seen.items() if v))
    assert any(seen.values()), seen
    if mutation in ("norot", "last_trial"):
        assert not seen["F"] and not seen["G"]
        # every textured case with a seeding choice sees the choice of trial
        if mutation == "last_trial":
            assert all(seen[n] for n in ("A3", "B", "C", "D", "E", "I", "J")), seen
    if mutation == "ctr0":
        # restarts that share their draws are one fit three times
        _, mut = qc.case_model("D", mutate="ctr0")
        assert np.array_equal(mut[0]["centres"], mut[1]["centres"])
        _, base = qc.case_model("D")
        assert not np.array_equal(base[0]["centres"], base[1]["centres"])


def test_selection_is_strict():
    runs = [dict(inertia=2.0), dict(inertia=1.0), dict(inertia=1.0)]
    assert qm.select(runs) == 1
    assert qm.select([dict(inertia=1.0)] * 3) == 0


def test_inertia_reduction_order_is_the_workgroups():
    """the restated order against a literal walk over threads, lanes and waves"""
    rs = np.random.RandomState(5)
    pts = rs.randint(0, 256, size=(1600, 3)).astype(np.int64)
    cen = rs.uniform(0, 255, size=(5, 3))
    d = pts[:, None, :].astype(np.float64) - cen[None]
    d = d * d
    bd = ((d[..., 0] + d[..., 1]) + d[..., 2]).min(1)
    thread = [0.0] * 512
    for t in range(512):
        for j in range(16):
            if t + 512 * j < len(bd):
                thread[t] += float(bd[t + 512 * j])
    tot = 0.0
    for wv in range(8):
        v = thread[64 * wv:64 * wv + 64]
        for o in (32, 16, 8, 4, 2, 1):  # v += shuffle_xor(v, o), every lane at once
            v = [v[i] + v[i ^ o] for i in range(64)]
        assert len(set(v)) == 1
        tot += v[0]
    assert qm.inertia_device_order(pts, cen) == tot
