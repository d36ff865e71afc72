"""The Philox noise kernels against the exact host model of their streams (philox_model.py):
equal to the reference draw for draw, in every layout form, with the high words of seed and
image id live.

s&p, Poisson and uniform are integer mappings of the Philox words: bit-equal.  The float64
Gaussian / speckle stream is held to the 2-ulp bounds of its ln / radius / sincos
(test_f64_math.py): |out - model| <= sd * 2e-14 + 3e-16.  The u8 Gaussian / speckle stream uses
the fp32 hardware log / sin / cos, which cannot be restated bit for bit: a byte may differ from
the model's, by one, only where the model's pre-floor value lies within
s * EPS_Z * max(1, |z|) + 2e-5 of an integer (s = 255 sd, or v sd for speckle).
"""
import numpy as np
import pytest

import philox_model as pm

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = 0x9E3779B97F4A7C15, 0xFFFFFFFF00000001
OFFSET = 2 ** 32 - 1                    # offset + i carries into counter word 3
IDS = [7, 2 ** 40 + 5, 2 ** 32]
FLAT = (3, 40, 64, 3)                   # 7680 elements per image: 2 workgroups of the flat form

# accuracy of one fp32 Box-Muller normal on the hardware transcendentals, relative to
# max(1, |z|).  Four times the largest value any case needed on the MI355X (3.31e-9), rounded up
# to one digit (the per-case measurements are in DESIGN.md section 4); the hard cap is 2e-5,
# since one step of the 16-bit u2 grid moves z by ~1e-4 rad.
EPS_Z = 2e-8
assert EPS_Z <= 2e-5

# layout forms: (name, shape, seed, offset or None, ids or None, padded rows)
FORMS = [
    ("flat", FLAT, SEED_A, OFFSET, None, False),
    ("flat-ids", FLAT, SEED_B, None, IDS, False),
    ("elem-partial", (2, 37, 53, 3), SEED_B, OFFSET, None, False),   # 5883 elements: partial chunk
    ("elem-gray", (2, 33, 47, 1), SEED_A, None, [2 ** 40 + 5, 3], False),
    ("elem-padded", FLAT, SEED_B, OFFSET, None, True),
]


def make_imgs(shape, seed):
    """random bytes; every image holds all 256 values"""
    n, h, w, c = shape
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 256, size=(n, h * w * c)).astype(np.uint8)
    for i in range(n):
        imgs[i, rs.permutation(h * w * c)[:256]] = np.arange(256)
    return imgs.reshape(shape)


def form_ids(form):
    _, shape, _, offset, ids, _ = form
    return pm.image_ids(shape[0], offset=offset or 0, ids=ids)


def run_form(form, imgs, mode, kw, out):
    """(u8, f64) numpy outputs of idn's random_noise in this layout form, flattened per image"""
    import torch
    import idn
    from test_noise_gpu import noise_padded
    _, shape, seed, offset, ids, padded = form
    n = shape[0]
    if padded:
        assert kw.get("mean", 0.0) == 0.0 and kw.get("salt_vs_pepper", 0.5) == 0.5
        u8, f64 = noise_padded(imgs, mode, kw, seed, offset, out=out)
    else:
        x = torch.from_numpy(imgs).cuda()
        where = {"offset": offset} if ids is None else {"image_ids": ids}
        res = idn.ops.random_noise(x, mode, seed=seed, out=out, **where, **kw)
        torch.cuda.synchronize()
        u8, f64 = res if out == "both" else ((res, None) if out == "u8" else (None, res))
        u8 = u8.cpu().numpy() if u8 is not None else None
        f64 = f64.cpu().numpy() if f64 is not None else None
    return (u8.reshape(n, -1) if u8 is not None else None,
            f64.reshape(n, -1) if f64 is not None else None)


def forms_for(kw):
    plain = kw.get("mean", 0.0) == 0.0 and kw.get("salt_vs_pepper", 0.5) == 0.5
    return [f for f in FORMS if plain or not f[5]]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64),
                          np.ascontiguousarray(b, np.float64).view(np.uint64))


# ---- s&p ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("amount", [0.2, 0.4, 0.8])
@pytest.mark.parametrize("svp", [0.5, 0.3])
def test_sap_equals_model(dev, amount, svp):
    kw = {"amount": amount, "salt_vs_pepper": svp}
    for form in forms_for(kw):
        imgs = make_imgs(form[1], 1)
        m = pm.sap(imgs.reshape(form[1][0], -1), form[2], form_ids(form), amount, svp)
        assert m["flip"].any() and not m["flip"].all() and m["salt"].any()
        u8, f64 = run_form(form, imgs, "s&p", kw, "both")
        assert np.array_equal(u8, m["byte"]), form[0]
        assert bits_equal(f64, m["f64"]), form[0]
        only8, _ = run_form(form, imgs, "s&p", kw, "u8")
        assert np.array_equal(only8, m["byte"]), form[0]


# ---- Poisson ------------------------------------------------------------------------------------
POIS_EXCUSED = []   # every excused draw of this file: (test, image, element)


def check_poisson(what, u8, f64, m):
    """Bit-equal to the model, except a count off by one on a draw whose word sits on one of the
    model's thresholds (t_k or t_k - 1): a last-bit difference between the device's exp and numpy's
    can move a threshold by one.  At most 2 such draws over the whole file."""
    bad = np.zeros(m["k"].shape, bool)
    if u8 is not None:
        bad |= u8 != m["byte"]
    if f64 is not None:
        bad |= f64.view(np.uint64) != m["f64"].view(np.uint64)
    for i, e in np.argwhere(bad):
        vals = 1 << int(m["vi"][i])
        ok = bool(m["at_threshold"][i, e]) and f64 is not None
        for kg in (m["k"][i, e] - 1, m["k"][i, e] + 1):   # the only counts an excuse allows
            if ok and f64[i, e] == min(kg / vals, 1.0) and \
                    (u8 is None or u8[i, e] == min((255 * kg) >> int(m["vi"][i]), 255)):
                break
        else:
            ok = False
        assert ok, (what, "image", i, "element", e, "word", int(m["w"][i, e]),
                    "model k", int(m["k"][i, e]), "gpu", None if f64 is None else f64[i, e] * vals)
        POIS_EXCUSED.append((what, int(i), int(e)))
    print(f"poisson {what}: {int(bad.sum())} excused, {len(POIS_EXCUSED)} in the file so far")
    assert len(POIS_EXCUSED) <= 2, POIS_EXCUSED


def test_poisson_forms_equal_model(dev):
    for form in FORMS:
        imgs = make_imgs(form[1], 2)
        m = pm.poisson(imgs.reshape(form[1][0], -1), form[2], form_ids(form))
        assert (m["vi"] == 8).all()
        u8, f64 = run_form(form, imgs, "poisson", {}, "both")
        check_poisson(form[0], u8, f64, m)


def level_images():
    """For every level vi = 0..8, 256 / 2^vi images of 16x16x3, image j holding the 2^vi values
    j 2^vi .. (j+1) 2^vi - 1, so every (vals, v) row is drawn; and per level vi >= 2 one image
    with 2^vi - 1 distinct values (vals rounds up to 2^vi).  Returns (images, levels)."""
    rs = np.random.RandomState(9)
    imgs, levels = [], []
    for vi in range(pm.POIS_NV):
        sets = [np.arange(j << vi, (j + 1) << vi) for j in range(256 >> vi)]
        if vi >= 2:
            sets.append(np.arange(1, 1 << vi))
        for s in sets:
            px = np.resize(s, 768).astype(np.uint8)
            imgs.append(px[rs.permutation(768)])
            levels.append(vi)
    return np.stack(imgs), np.array(levels)


def test_poisson_every_row(dev):
    """All 9 x 256 CDF rows, drawn through the flat kernel: once as one shuffled batch (518
    images of mixed levels over fewer workgroups: the level block is re-staged between units),
    once level by level."""
    import torch
    import idn
    imgs, levels = level_images()
    order = np.random.RandomState(10).permutation(len(imgs))
    imgs, levels = imgs[order], levels[order]
    n = len(imgs)
    assert n > 500
    ids = pm.image_ids(n, offset=OFFSET - 100)
    m = pm.poisson(imgs, SEED_B, ids)
    assert np.array_equal(m["vi"], levels)
    drawn = {(int(vi), int(v)) for vi, row in zip(levels, imgs) for v in np.unique(row)}
    assert len(drawn) == pm.POIS_NV * 256
    assert (np.diff(levels) != 0).sum() > 256   # neighbouring units mostly differ in level
    x = torch.from_numpy(imgs.reshape(n, 16, 16, 3)).cuda()
    u8, f64 = idn.ops.random_noise(x, "poisson", seed=SEED_B, offset=OFFSET - 100, out="both")
    check_poisson("every row, one batch", u8.cpu().numpy().reshape(n, -1),
                  f64.cpu().numpy().reshape(n, -1), m)
    for vi in range(pm.POIS_NV):
        sel = np.flatnonzero(levels == vi)
        u8, f64 = idn.ops.random_noise(x[torch.from_numpy(sel).cuda()], "poisson", seed=SEED_B,
                                       image_ids=[int(i) for i in ids[sel]], out="both")
        sub = {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in m.items()}
        check_poisson(f"every row, level {vi}", u8.cpu().numpy().reshape(len(sel), -1),
                      f64.cpu().numpy().reshape(len(sel), -1), sub)


def test_poisson_parts(dev):
    """one image split over several work units of the flat kernel (parts > 1)"""
    form = ("parts", (1, 96, 128, 3), SEED_A, OFFSET, None, False)
    imgs = make_imgs(form[1], 3)
    m = pm.poisson(imgs.reshape(1, -1), form[2], form_ids(form))
    u8, f64 = run_form(form, imgs, "poisson", {}, "both")
    check_poisson("parts", u8, f64, m)


def test_poisson_rare_bins(dev):
    """The deep bins (u < 2^-16 or u > 1 - 2^-16: the bisection) and the lowest octaves of the
    guide, swept over v = 0..255: the model locates the draws, the image puts the bytes there."""
    form = ("rare", (1, 600, 1000, 3), SEED_B, None, [2 ** 40 + 5], False)
    imgs = make_imgs(form[1], 4).reshape(1, -1)
    w = pm.poisson_words(imgs.shape[1], form[2], form_ids(form))[0].astype(np.int64)
    rare = np.flatnonzero((w < 2 ** 20) | (w > 2 ** 32 - 2 ** 20))
    deep = (w[rare] < 2 ** 16) | (w[rare] >= 2 ** 32 - 2 ** 16)
    assert deep.sum() >= 32, int(deep.sum())
    imgs[0, rare] = np.arange(len(rare)) % 256
    assert len(np.unique(imgs[0, rare][deep])) >= 24
    m = pm.poisson(imgs, form[2], form_ids(form))
    assert m["vi"].tolist() == [8]
    u8, f64 = run_form(form, imgs.reshape(form[1]), "poisson", {}, "both")
    check_poisson("rare bins", u8, f64, m)
    only8, _ = run_form(form, imgs.reshape(form[1]), "poisson", {}, "u8")
    assert np.array_equal(only8, u8)


# ---- float64 Gaussian / speckle -----------------------------------------------------------------
F64_CASES = [("gaussian", 0.1, 0.0), ("gaussian", 1.0, 0.0), ("gaussian", 1.5, 0.25),
             ("speckle", 1.0, 0.0)]


def check_f64(what, u8, f64, m, imgs, kind, var):
    sd = float(var) ** 0.5
    tol = sd * 2e-14 + 3e-16
    if kind == pm.SPECKLE:
        tol = tol * (imgs.astype(np.float64) / 255.0)
    err = np.abs(f64 - m["f64"])
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    assert (err <= tol).all(), (what, worst, err[worst], f64[worst], m["f64"][worst])
    inside = (m["f64"] > 0.0) & (m["f64"] < 1.0)
    assert inside.mean() > 0.2, what        # the draws are visible, not clipped away
    assert np.array_equal(u8, (f64 * 255.0).astype(np.uint8)), what


@pytest.mark.parametrize("mode,var,mean", F64_CASES)
def test_f64_stream_equals_model(dev, mode, var, mean):
    import torch
    import idn
    kind = pm.GAUSSIAN if mode == "gaussian" else pm.SPECKLE
    kw = {"var": var, "mean": mean}
    for form in forms_for(kw):
        n = form[1][0]
        imgs = make_imgs(form[1], 5)
        flat = imgs.reshape(n, -1)
        m = pm.gauss_f64(flat, form[2], form_ids(form), kind, mean, var)
        u8, f64 = run_form(form, imgs, mode, {"var": var} if form[5] else kw, "both")
        check_f64(form[0], u8, f64, m, flat, kind, var)
        if form[0] in ("flat", "flat-ids"):   # the fused live-path kernel draws the same image
            where = {"offset": form[3]} if form[4] is None else {"image_ids": form[4]}
            y64, _ = idn.ops.random_noise_ycc(torch.from_numpy(imgs).cuda(), mode, mean=mean,
                                              var=var, seed=form[2], **where)
            y64 = y64.cpu().numpy().reshape(n, -1)
            check_f64(form[0] + " ycc", (y64 * 255.0).astype(np.uint8), y64, m, flat, kind, var)
            assert bits_equal(y64, f64)


# ---- u8 Gaussian / speckle ----------------------------------------------------------------------
U8_CASES = [("gaussian", 0.1, 0.0), ("gaussian", 1.0, 0.0), ("gaussian", 1.5, 0.0),
            ("gaussian", 1.0, 0.1), ("speckle", 0.5, 0.0), ("speckle", 1.0, 0.0),
            ("speckle", 2.0, 0.0), ("speckle", 1.0, 0.1)]


def check_u8(what, u8, m, imgs, kind, var, only=None):
    """rules 1-3 of the u8 stream; returns the EPS_Z the observed differences would need.
    only: restrict the comparison to a mask of elements (rule 4: the refined pairs)"""
    sd = float(var) ** 0.5
    s = (255.0 if kind == pm.GAUSSIAN else imgs.astype(np.float64)) * sd
    zmag = np.maximum(1.0, np.abs(m["z"]))
    dist = np.abs(m["pre"] - np.rint(m["pre"]))
    allowed = dist <= s * EPS_Z * zmag + 2e-5
    diff = u8.astype(np.int64) - m["byte"].astype(np.int64)
    if only is not None:
        diff = np.where(only, diff, 0)
    differs = diff != 0
    share = float(allowed.mean())
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(differs, (dist - 2e-5) / (s * zmag), 0.0)
    need_max = float(need.max())
    print(f"u8 stream {what}: {int(differs.sum())} of {differs.size} bytes differ, "
          f"eps needed {need_max:.3g}, share the rule excuses {share:.4%}")
    assert np.abs(diff).max() <= 1, (what, np.argwhere(np.abs(diff) > 1)[:4])
    wrong = differs & ~allowed
    assert not wrong.any(), (what, int(wrong.sum()), np.argwhere(wrong)[:4], need_max)
    assert share < 0.01, (what, share)
    return need_max


@pytest.mark.parametrize("mode,var,mean", U8_CASES)
def test_u8_stream_equals_model(dev, mode, var, mean):
    kind = pm.GAUSSIAN if mode == "gaussian" else pm.SPECKLE
    kw = {"var": var, "mean": mean}
    for form in forms_for(kw):
        n = form[1][0]
        imgs = make_imgs(form[1], 6)
        flat = imgs.reshape(n, -1)
        m = pm.gauss_u8(flat, form[2], form_ids(form), kind, mean, var)
        u8, _ = run_form(form, imgs, mode, {"var": var} if form[5] else kw, "u8")
        check_u8(f"{mode} var {var} mean {mean} {form[0]}", u8, m, flat, kind, var)
        inside = (m["pre"] > 0.0) & (m["pre"] < 255.0)
        assert inside.mean() > 0.2


@pytest.mark.parametrize("mode,var,mean", U8_CASES)
def test_u8_stream_refined_pairs(dev, mode, var, mean):
    """600x1000x3: at least 8 pairs take their radius from the refinement block (u1 = 2^-16 cell,
    |z| up to 6.66); the bytes under them are set so that the draw is not clipped away."""
    kind = pm.GAUSSIAN if mode == "gaussian" else pm.SPECKLE
    form = ("big", (1, 600, 1000, 3), SEED_A, None, [2 ** 40 + 5], False)
    imgs = make_imgs(form[1], 7).reshape(1, -1)
    first = pm.gauss_u8(imgs, form[2], form_ids(form), kind, mean, var)
    refined = first["refined"]
    assert refined.sum() >= 16, int(refined.sum())   # 8 pairs
    # gaussian: the byte at the far end from the draw's sign; speckle: a small byte
    imgs[refined] = np.where(first["z"][refined] > 0, 0, 255) if kind == pm.GAUSSIAN else 24
    m = pm.gauss_u8(imgs, form[2], form_ids(form), kind, mean, var)
    u8, _ = run_form(form, imgs.reshape(form[1]), mode, {"var": var, "mean": mean}, "u8")
    what = f"{mode} var {var} mean {mean} 600x1000"
    check_u8(what, u8, m, imgs, kind, var)
    check_u8(what + " refined pairs", u8, m, imgs, kind, var, only=refined)
    seen = refined & (m["pre"] > 0.0) & (m["pre"] < 255.0)
    # at var >= 1 a Gaussian draw of |z| > 1 clips whatever the byte; speckle keeps half of them
    assert seen.sum() >= (1 if kind == pm.GAUSSIAN else 8), int(seen.sum())
    assert np.abs(m["z"][refined]).max() > 4.0


# ---- uniform and Rayleigh additive noise ----------------------------------------------------------
ADD_FORMS = [FORMS[0], FORMS[1], FORMS[2], FORMS[3]]


def run_add(form, imgs, mode, level):
    import torch
    import idn
    _, shape, seed, offset, ids, _ = form
    where = {"offset": offset} if ids is None else {"image_ids": ids}
    u8, f64 = idn.ops.noise_add(torch.from_numpy(imgs).cuda(), mode, level, seed=seed, out="both",
                                **where)
    return u8.cpu().numpy().reshape(shape[0], -1), f64.cpu().numpy().reshape(shape[0], -1)


@pytest.mark.parametrize("high", [0.5, 1.7])
def test_uniform_add_equals_model(dev, high):
    for form in ADD_FORMS:
        imgs = make_imgs(form[1], 8)
        m = pm.uniform_add(imgs.reshape(form[1][0], -1), form[2], form_ids(form), high)
        _, f64 = run_add(form, imgs, "uniform", high)
        assert bits_equal(f64, m["f64"]), form[0]


@pytest.mark.parametrize("scale", [0.3, 1.0])
def test_rayleigh_add_equals_model(dev, scale):
    """within 4e-7 relative of the model's unit draw: three fp32 roundings (log, the product by
    -2 is exact, root, the conversion of the result) plus the 1-ulp log and root; the float64
    scale / add roundings of a value below 8 add at most 2e-15"""
    for form in ADD_FORMS:
        imgs = make_imgs(form[1], 8)
        m = pm.rayleigh_add(imgs.reshape(form[1][0], -1), form[2], form_ids(form), scale)
        _, f64 = run_add(form, imgs, "rayleigh", scale)
        err = np.abs(f64 - m["f64"])
        tol = 4e-7 * scale * m["unit"] + 2e-15
        rel = float((np.maximum(err - 2e-15, 0) / np.maximum(scale * m["unit"], 1e-300)).max())
        print(f"rayleigh {form[0]} scale {scale}: largest relative error of the unit draw {rel:.3g}")
        assert (err <= tol).all(), (form[0], np.argwhere(err > tol)[:4], rel)


# ---- structure --------------------------------------------------------------------------------
def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_kinds_and_images_draw_different_normals(dev):
    """Gaussian and speckle of one seed use different normals (the key carries the kind), and
    images i, i + 1 of a batch have uncorrelated noise fields: |corr| < 4 / sqrt(n)."""
    form = FORMS[0]
    n = form[1][0]
    imgs = np.full(form[1], 128, np.uint8)
    x = 128 * (1.0 / 255.0)
    kw = {"var": 0.01, "mean": 0.0}
    _, g = run_form(form, imgs, "gaussian", kw, "both")
    _, s = run_form(form, imgs, "speckle", kw, "both")
    zg, zs = (g - x) / 0.1, (s - x) / (x * 0.1)
    elems = zg.shape[1]
    bound = 4.0 / np.sqrt(elems)
    for z in (zg, zs):
        assert abs(z.std() - 1.0) < 0.05
        for i in range(n - 1):
            assert abs(_corr(z[i], z[i + 1])) < bound, ("images", i, _corr(z[i], z[i + 1]))
    for i in range(n):
        assert abs(_corr(zg[i], zs[i])) < bound, ("kinds", i, _corr(zg[i], zs[i]))
    # the model says the same of its own streams
    ids = form_ids(form)
    mg = pm.normals_f64(elems, form[2], ids, pm.GAUSSIAN)
    ms = pm.normals_f64(elems, form[2], ids, pm.SPECKLE)
    assert abs(_corr(mg[0], ms[0])) < bound and abs(_corr(mg[0], mg[1])) < bound
    assert abs(_corr(zg[0], mg[0])) > 0.999
