"""The Haar L = 3 sigma window (csrc/haar3.hpp) through the product library, no tuning knobs:
inputs that narrow the sampled window, that put the median rank above and below it (the exact
full-image fallback fired by the image itself), that leave it full, and that make the median a
rounding residue.  Every selection word is compared with the integer model (tests/h3_model.py,
itself checked against the fp64 oracle by tests/test_h3_model.py), the nonzero counts and sigma
medians with the oracle's fp64 finest dd, the outputs with the oracle's denoiser.

Sigma's median: bitwise where the exact path ran (it evaluates the reference's chain), within the
analytic bound 2.1e-12 / range (haar3.hpp's header) where the window's integer |T| gave it.
"""
import functools

import numpy as np
import pytest

import h3_model as hm
from test_wavelet_gpu import TOL, _h3_sel, _key_to_f64, check_u8

pytestmark = pytest.mark.gpu
MED = slice(35, 38)      # WlStats::median(c, 3)
CNT = slice(248, 251)    # nonzero finest dd per channel
SUMS = slice(8, 35)      # sums of squares per (channel, level, band)
KEYS = slice(200, 206)   # YCbCr min / max keys
SELW = slice(66, 78)     # H3Sel words


def _launch(imgs, out="both"):
    """idn.ops.denoise_wavelet(db1, 3) on a u8 batch: (u8, f32 or None, stats blocks)"""
    import torch
    from idn import _lib, ops
    x = torch.from_numpy(np.array(imgs)).cuda()  # (a writable copy: the families are read-only)
    r = ops.denoise_wavelet(x, "db1", 3, out=out)
    u8, f = r if out == "both" else (r, None)
    n, h, w, _ = x.shape
    off = _lib.load().idn_wavelet_stats_offset(n, h, w, ops.WAVELETS["db1"], 3)
    ws = ops._WS_CACHE[(str(x.device), torch.cuda.current_stream(x.device).cuda_stream)]
    st = ws[off:off + n * 256 * 8].view(torch.float64).view(n, 256).cpu().numpy().copy()
    return u8.cpu().numpy(), None if f is None else f.cpu().numpy(), st


def _launch_abi(imgs, pad=0, fill=0xAB, ws_fill=0):
    """the C-ABI on rows of w * 3 + pad bytes (padding bytes `fill`, the output's 77) with a
    workspace of its own, every byte `ws_fill` before the call: (u8, f32, stats blocks)"""
    import torch
    from idn import _lib, ops
    lib = _lib.load()
    n, h, w, _ = imgs.shape
    rs = w * 3 + pad
    buf = torch.full((n, h, rs), fill, dtype=torch.uint8, device="cuda")
    buf[:, :, :w * 3] = torch.from_numpy(np.array(imgs).reshape(n, h, w * 3)).cuda()
    out = torch.full_like(buf, 77)
    f32 = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    wv = ops.WAVELETS["db1"]
    nbytes = lib.idn_wavelet_workspace_size(n, h, w, wv, 3)
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device="cuda")
    rc = lib.idn_wavelet_denoise_u8(buf.data_ptr(), None, out.data_ptr(), f32.data_ptr(), n, h, w, rs,
                                    wv, 3, ws.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "idn_wavelet_denoise_u8")
    torch.cuda.synchronize()
    assert bool((out[:, :, w * 3:] == 77).all())  # padding untouched
    off = lib.idn_wavelet_stats_offset(n, h, w, wv, 3)
    st = ws[off:off + n * 256 * 8].view(torch.float64).view(n, 256).cpu().numpy().copy()
    return out[:, :, :w * 3].cpu().numpy().reshape(n, h, w, 3), f32.cpu().numpy(), st


@functools.lru_cache(maxsize=None)
def _single(name, shape):
    """the one-image launch of a family, shared by the tests that compare against it"""
    return _launch(hm.family(name, shape)[None])


def _same_stats(a, b):
    """selection words, medians, counts, colour keys and sums of two launches, bit for bit"""
    for s in (SELW, MED, CNT, KEYS, SUMS):
        np.testing.assert_array_equal(a[:, s].view(np.uint64), b[:, s].view(np.uint64))


@pytest.mark.parametrize("name,shape", hm.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_haar3_window_family(dev, name, shape):
    """one image of each family: window bounds, counters and branch equal to the integer model,
    nonzero counts and sigma medians to the oracle's fp64 dd, outputs within 1e-5 of the oracle.

    Branches by family: plain / clipped / quant / parity twins: a narrowed window, fb = 0;
    quiet-sample (rank above the window) and loud-sample (below): fb = 1 on all three channels;
    flat-sample: the full window (1, 0xFFFFFFFF) on a large image, fb = 0; gray: Y a narrowed
    window, Cb / Cr (T = 0 everywhere, the median a residue) fb = 1; threshold: narrowed at
    n = 512, full at n = 511."""
    import oracle
    img, M, R = hm.case(name, shape)
    u8, f, st = _single(name, shape)
    sel = _h3_sel(st)[0]
    rng = (_key_to_f64(st[:, 203:206].view(np.uint64)) - _key_to_f64(st[:, 200:203].view(np.uint64)))[0]
    dec = [M.ch[c].decide(int(R.nrnz[c])) for c in range(3)]
    for c in range(3):  # the figures first: (n, lo, hi, n_t, n_lo, n_c, n_r, N, fb, median)
        print(f"H3 {name} {shape} c={c} n={M.ch[c].n} lo={sel[c, 0]} hi={sel[c, 1]} n_t={sel[c, 2]} "
              f"n_lo={sel[c, 3]} n_c={sel[c, 4]} n_r={sel[c, 5]} N={int(st[0, 248 + c])} fb={sel[c, 6]} "
              f"med={st[0, 35 + c]!r} ref_med={R.median[c]!r} ref_N={R.count[c]} "
              f"model=({M.ch[c].lo},{M.ch[c].hi},{M.ch[c].n_t},{M.ch[c].n_lo},{M.ch[c].n_c},{dec[c]['fb']})")
    np.testing.assert_array_equal(rng, R.rng)
    for c in range(3):
        ch = M.ch[c]
        assert (int(sel[c, 0]), int(sel[c, 1])) == (ch.lo, ch.hi), c
        assert (int(sel[c, 2]), int(sel[c, 3]), int(sel[c, 4])) == (ch.n_t, ch.n_lo, ch.n_c), c
        assert int(sel[c, 5]) == (M.n_r if c == 0 else 0), c  # channel 0's slot counts for the image
        assert int(sel[c, 6]) == dec[c]["fb"], c
        if name in hm.FALLBACK_FAMILIES:
            assert int(sel[c, 6]) == 1
        if name in hm.WINDOW_FAMILIES or name.startswith("threshold"):
            assert int(sel[c, 6]) == 0
        assert st[0, 248 + c] == R.count[c], c
        got, ref = st[0, 35 + c], R.median[c]
        if np.isnan(ref):
            assert np.isnan(got), c
        elif sel[c, 6] == 1:
            assert np.float64(got).view(np.uint64) == np.float64(ref).view(np.uint64), (c, got, ref)
        else:
            assert abs(got - ref) <= hm.bound(R.rng[c]), (c, got, ref)
    ref = oracle.wavelet.denoise_wavelet(img, "db1", 3)
    assert np.abs(f[0].astype(np.float64) - ref).max() <= TOL
    check_u8(u8[0], ref, oracle.sk.to_u8(255 * ref))


def test_haar3_mixed_batch_equals_single_launches(dev):
    """fallback, window, full-window and residue images in one batch (per-image counters filled
    through global atomics, the statistics block cleared by the window kernel): every image as
    its own one-image launch, u8, selection words and medians bit for bit"""
    shape = (256, 256)
    names = ["quiet-sample", "plain", "loud-sample", "flat-sample", "gray", "quant"]
    u8, f, st = _launch(np.stack([hm.family(n, shape) for n in names]))
    fbs = _h3_sel(st)[:, :, 6]
    assert fbs[0].all() and fbs[2].all() and not fbs[1].any() and not fbs[3].any()  # a mixed batch
    for i, n in enumerate(names):
        u8s, fs, sts = _single(n, shape)
        np.testing.assert_array_equal(u8[i], u8s[0], err_msg=n)
        np.testing.assert_array_equal(f[i].view(np.uint32), fs[0].view(np.uint32), err_msg=n)
        _same_stats(st[i:i + 1], sts)


def test_haar3_workspace_reuse(dev):
    """a call on the cached workspace after one that left large counters behind (flat-sample:
    n_c = n_t, hundreds of residues) equals the call on a workspace that saw nothing else, zeroed
    or filled with 0xFF bytes"""
    shape = (256, 256)
    flat = np.stack([hm.family("flat-sample", shape)] * 2)
    second = np.stack([hm.family("quiet-sample", shape), hm.family("plain", shape)])
    _, _, st0 = _launch(flat)
    assert np.all(_h3_sel(st0)[:, :, 4] > 15000)  # what the next call finds in its slots
    u8, f, st = _launch(second)
    for ws_fill in (0, 0xFF):
        u8f, ff, stf = _launch_abi(second, ws_fill=ws_fill)
        np.testing.assert_array_equal(u8, u8f)
        np.testing.assert_array_equal(f.view(np.uint32), ff.view(np.uint32))
        _same_stats(st, stf)
    assert _h3_sel(st)[0, :, 6].all() and not _h3_sel(st)[1, :, 6].any()


def test_haar3_u8_only_equals_both(dev):
    """the u8-only launch (dword stores) on fallback and full-window images: the u8 + f32
    launch's bytes and selection words"""
    shape = (256, 256)
    imgs = np.stack([hm.family(n, shape) for n in ("quiet-sample", "loud-sample", "flat-sample")])
    u8b, _, stb = _launch(imgs)
    u8o, _, sto = _launch(imgs, out="u8")
    np.testing.assert_array_equal(u8o, u8b)
    _same_stats(sto, stb)
    assert _h3_sel(sto)[:2, :, 6].all() and not _h3_sel(sto)[2, :, 6].any()


@pytest.mark.parametrize("name", ["plain", "quiet-sample"])
def test_haar3_strided_rows(dev, name):
    """rows of w * 3 + 12 bytes (padding 0xAB) at 136 x 520, a window and a fallback image: outputs
    and selection words of the compact launch, bit for bit; the output's padding untouched"""
    shape = (136, 520)
    img = hm.family(name, shape)[None]
    u8c, fc, stc = _single(name, shape)
    u8s, fs, sts = _launch_abi(img, pad=12)
    np.testing.assert_array_equal(u8s, u8c)
    np.testing.assert_array_equal(fs.view(np.uint32), fc.view(np.uint32))
    _same_stats(sts, stc)
    assert int(_h3_sel(sts)[0, 0, 6]) == (1 if name == "quiet-sample" else 0)
