"""GPU: the quant k-means fit (quant_fit_kernel / quant_select_kernel of csrc/quant.hip) against
its exact host model tests/quant_fit_model.py, bit for bit: every restart's fp64 centres and
inertia (read from the workspace through idn_quant_runs_offset), the chosen centres, and the
labels and output the apply kernel makes of them.  The cases and what each reaches are listed in
tests/quant_fit_cases.py; tests/test_quant_fit_model.py shows that they tell a fit that breaks
one rule of the scheme (cumulative order, choice of trial, tie rule, restart counters, high id
word) from one that keeps it.  tests/test_quant_gpu.py remains the link to sklearn (quality only:
the reference never seeds its fit).

No case reaches the Lloyd loop's 100-iteration cap (the longest run takes 85 iterations).
"""
import numpy as np
import pytest

from oracle import cvlab

import quant_fit_cases as qc
import quant_fit_model as qm

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _equal(a, b):
    """arrays of a launch's result: floats by their bits, bytes by value"""
    return _same(a, b) if a.dtype == np.float64 else np.array_equal(a, b)


def launch(imgs, k, seed=qc.SEED, offset=0, image_ids=None, pad=0, pad_byte=0):
    """idn_quant_u8 on (n, h, w, 3) uint8 images with a workspace of its own (prefilled with
    0xFF bytes: a restart the kernel did not write reads as NaN).  pad > 0: rows of w*3 + pad
    bytes whose padding holds pad_byte in src and its complement in dst.
    Returns dict(out, labels, centres, run_cen (n, 3, k, 3), run_inert (n, 3), dst_pad)."""
    import torch
    from idn import _lib
    lib = _lib.load()
    imgs = np.ascontiguousarray(imgs)
    n, h, w, _ = imgs.shape
    stride = w * 3 + pad
    src = np.full((n, h, stride), pad_byte, np.uint8)
    src[:, :, :w * 3] = imgs.reshape(n, h, w * 3)
    dst_fill = pad_byte ^ 0xFF
    dev = torch.device("cuda:0")
    x = torch.from_numpy(src).to(dev)
    y = torch.full((n, h, stride), dst_fill, dtype=torch.uint8, device=dev)
    lab = torch.full((n, h, w), 0xEE, dtype=torch.uint8, device=dev)
    cen = torch.full((n, k, 3), float("nan"), dtype=torch.float64, device=dev)
    ws_bytes = lib.idn_quant_workspace_size(n, k)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=dev)
    ids = None
    if image_ids is not None:
        ids = torch.tensor([int(i) for i in image_ids], dtype=torch.int64, device=dev)
    rc = lib.idn_quant_u8(x.data_ptr(), y.data_ptr(), lab.data_ptr(), n, h, w, stride, k,
                          int(seed), int(offset), ids.data_ptr() if ids is not None else None,
                          None, cen.data_ptr(), ws.data_ptr(), ws_bytes,
                          torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "idn_quant_u8")
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    off = lib.idn_quant_runs_offset(n, k)
    cen_bytes = n * qm.NINIT * k * 3 * 8
    off_inert = off + (cen_bytes + 255) // 256 * 256   # include/idn.h
    assert 0 < off and off_inert + n * qm.NINIT * 8 <= ws_bytes
    run_cen = raw[off:off + cen_bytes].view(np.float64).reshape(n, qm.NINIT, k, 3)
    run_inert = raw[off_inert:off_inert + n * qm.NINIT * 8].view(np.float64).reshape(n, qm.NINIT)
    dst = y.cpu().numpy()
    return dict(out=dst[:, :, :w * 3].reshape(n, h, w, 3), labels=lab.cpu().numpy(),
                centres=cen.cpu().numpy(), run_cen=run_cen, run_inert=run_inert,
                dst_pad=dst[:, :, w * 3:], dst_fill=dst_fill)


def check_against_model(got, i, img, model, what):
    """image i of a launch: its three restarts, its centres, labels and output are the model's"""
    cen, runs = model
    for r, run in enumerate(runs):
        assert _same(got["run_cen"][i, r], run["centres"]), \
            (what, "restart", r, got["run_cen"][i, r], run["centres"])
        assert _same(got["run_inert"][i, r], run["inertia"]), \
            (what, "restart", r, repr(float(got["run_inert"][i, r])), repr(run["inertia"]))
    assert _same(got["centres"][i], cen), (what, got["centres"][i], cen)
    ref, ref_labels, _ = cvlab.quantize_apply(img, cen)
    assert np.array_equal(got["labels"][i], ref_labels), what
    assert np.array_equal(got["out"][i], ref), what


@pytest.mark.parametrize("name", list(qc.CASES))
def test_fit_equals_model(dev, name):
    img_name, k, gid = qc.CASES[name]
    img = qc.image(img_name)
    model = qc.case_model(name)
    got = launch(img[None], k, offset=gid)
    check_against_model(got, 0, img, model, name)
    if name == "E":  # the 64-bit id through the list as well
        by_list = launch(img[None], k, image_ids=[gid])
        check_against_model(by_list, 0, img, model, "E by image_ids")
    # what holds whatever the model says
    if name == "A1":
        lab = cvlab.bgr2lab(img).reshape(-1, 3).astype(np.int64)
        assert _same(got["centres"][0, 0], lab.sum(0).astype(np.float64) / len(lab))
    if name in ("F", "G"):
        assert np.array_equal(got["out"][0], cvlab.lab2bgr(cvlab.bgr2lab(img)))
        assert len(np.unique(got["labels"][0])) == (2 if name == "F" else 1)


@pytest.mark.parametrize("k", [2, 4, 5])
def test_batch_equals_model_and_single_launches(dev, k):
    """three copies of the 40x40 image in one launch (n * 3 workgroups), ids 10, 11, 12 by offset
    and by list: each image's restarts are the model's for its id and those of a launch of its
    own"""
    img = qc.image("40x40")
    batch = np.stack([img] * 3)
    ids = [10, 11, 12]
    models = [qc.model("40x40", k, gid) for gid in ids]
    for a, b in ((0, 1), (1, 2), (0, 2)):  # the ids matter: they seed different fits
        assert any(not np.array_equal(ra["centres"], rb["centres"])
                   for ra, rb in zip(models[a][1], models[b][1]))
    by_offset = launch(batch, k, offset=10)
    by_list = launch(batch, k, image_ids=ids)
    for i, gid in enumerate(ids):
        check_against_model(by_offset, i, img, models[i], ("offset", gid))
        check_against_model(by_list, i, img, models[i], ("list", gid))
        one = launch(img[None], k, image_ids=[gid])
        for key in ("run_cen", "run_inert", "centres", "labels", "out"):
            assert _equal(one[key][0], by_offset[key][i]), (key, gid)
            assert _equal(one[key][0], by_list[key][i]), (key, gid)


def test_strided_rows(dev):
    """case D with rows of w*3 + 8 bytes: the fit reads no padding (its byte occurs nowhere in
    the image, so a sample taken from it would move a sum), and dst's padding stays untouched"""
    img_name, k, gid = qc.CASES["D"]
    img = qc.image(img_name)
    absent = np.setdiff1d(np.arange(256), np.unique(img))
    assert len(absent)
    compact = launch(img[None], k, offset=gid)
    strided = launch(img[None], k, offset=gid, pad=8, pad_byte=int(absent[0]))
    for key in ("run_cen", "run_inert", "centres", "labels", "out"):
        assert _equal(strided[key], compact[key]), key
    check_against_model(strided, 0, img, qc.case_model("D"), "D strided")
    assert strided["dst_pad"].shape == (1, img.shape[0], 8)
    assert np.all(strided["dst_pad"] == strided["dst_fill"])


def test_deterministic_and_seeded(dev):
    img_name, k, gid = qc.CASES["D"]
    img = qc.image(img_name)
    a = launch(img[None], k, offset=gid)
    b = launch(img[None], k, offset=gid)
    for key in ("run_cen", "run_inert", "centres", "labels", "out"):
        assert _equal(a[key], b[key]), key
    other = launch(img[None], k, seed=qc.SEED + 1, offset=gid)
    for r in range(qm.NINIT):
        assert not np.array_equal(other["run_cen"][0, r, 0], a["run_cen"][0, r, 0]), r
    assert np.isfinite(other["run_inert"]).all()
