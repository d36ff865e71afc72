"""CPU: what the C entry points of include/idn.h refuse before their first HIP call, by return
code and idn_last_error() text, and every workspace size and offset they publish.

The table covers every entry point but the noise family (tests/test_noise_args.py) and idn_jpeg_*.
Its addresses are fake and never dereferenced, so every row is either refused or returns at once
(n == 0, a copy of 0 bytes); rows that break two rules at once pin the order of the checks, which
decides the error a caller sees.  Error text, check order and workspace sizes are part of the ABI's
behaviour: tests/golden/abi_args.json holds them as the library gave them before the entry points
shared one argument layer (csrc/abi_args.hpp), written by tests/golden/make_abi_args.py.

A row the library accepted would launch a kernel on a fake address, so the module skips itself
where a device is visible; without one such a row only returns IDN_EHIP and fails the table.
"""
import ctypes
import itertools
import json
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
FIXTURE = HERE / "golden" / "abi_args.json"

# 16-byte aligned fake addresses; + 4 breaks the 8-byte alignment
A, B, O, K, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x80000
MEAN, TAPS = "<mean>", "<taps>"  # real memory: three doubles / 32 uint16
NEED, SHORT = "<need>", "<need-1>"  # ws_bytes: what the op's size function gives / one less
HUGE = 1 << 40
IMAX = 2**31 - 1
NAN, INF = float("nan"), float("inf")


def _rows(cn):
    """compact rows of cn channels (a number, or the name of the channel argument)"""
    return lambda d: d["w"] * (d[cn] if isinstance(cn, str) else cn)


_U8 = dict(src=A, dst=B, n=1, h=8, w=16, c=3, stride=_rows("c"))
_WSP = dict(ws=WS, ws_bytes=HUGE, stream=None)
_CVT = dict(src=A, dst=B, n=1, h=8, w=16, stride=_rows(3), stream=None)

# entry point -> its arguments in order, with one valid call's values
SPECS = {
    "idn_gaussian_blur_u8": dict(_U8, ksize=3, stream=None),
    "idn_gaussian_blur_sigma_u8": dict(_U8, ksize=3, sigma=0.0, stream=None),
    "idn_gaussian_taps": dict(ksize=3, sigma=0.0, taps=TAPS),
    "idn_box_blur_u8": dict(_U8, ksize=3, stream=None),
    "idn_median_blur_u8": dict(_U8, ksize=3, stream=None),
    "idn_adaptive_median_u8": dict(src=A, dst=B, kmap=None, n=1, h=8, w=16, c=3, stride=_rows("c"),
                                   ksize=7, stream=None),
    "idn_bilateral_u8": dict(_U8, d=5, sigma_color=25.0, sigma_space=3.0, stream=None),
    "idn_gaussian_blob_f32": dict(_U8, ksize=3, mean=MEAN, stream=None),
    "idn_gaussian_blur_f64": dict(src=A, dst=B, n=1, h=8, w=16, c=3, ksize=3, stream=None),
    "idn_box_blur_f64": dict(src=A, dst=B, n=1, h=8, w=16, c=3, ksize=3, stream=None),
    "idn_quant_u8": dict(src=A, dst=B, labels=None, n=1, h=8, w=16, stride=_rows(3), k=4, seed=1,
                         offset=0, ids=None, cin=None, cout=None, **_WSP),
    "idn_bgr2lab_u8": _CVT, "idn_lab2bgr_u8": _CVT, "idn_lbgr2lab_u8": _CVT,
    "idn_lab2lbgr_u8": _CVT, "idn_bgr2yuv_u8": _CVT, "idn_yuv2bgr_u8": _CVT,
    "idn_copy_u8": dict(src=A, dst=B, nbytes=4096, policy=0, stream=None),
    "idn_wavelet_denoise_u8": dict(src=A, in64=None, out_u8=B, out_f32=None, n=1, h=8, w=16,
                                   stride=_rows(3), wavelet=0, levels=1, **_WSP),
    "idn_wavelet_denoise_ycc": dict(in64=O, keys=K, out_u8=B, out_f32=None, n=1, h=8, w=16,
                                    wavelet=0, levels=1, **_WSP),
    "idn_wavelet_denoise_general": dict(src=A, in64=None, out_u8=B, out_f32=None, n=1, h=8, w=16,
                                        c=3, stride=_rows("c"), wavelet=2, levels=1, method=0,
                                        mode=0, ycc=0, sigma_dev=None, **_WSP),
    "idn_nlmeans_weights": dict(hh=10.0, c=3, t=3, s=5, wt=WS, cap=16, n_weights=K, shift=K + 8,
                                fpm=K + 16),
    "idn_nlmeans_u8": dict(src=A, dst=B, n=1, h=32, w=32, c=3, stride=_rows("c"), t=3, s=5,
                           weights=K, n_weights=100, stream=None),
    "idn_nlmeans_colored_weights": dict(hh=10.0, h_color=10.0, t=3, s=5, wt_l=WS, cap_l=16, n_l=K,
                                        wt_ab=WS + 4096, cap_ab=16, n_ab=K + 8, shift=K + 16,
                                        fpm=K + 24),
    "idn_nlmeans_colored_u8": dict(src=A, dst=B, n=1, h=32, w=32, stride=_rows(3), t=3, s=5,
                                   wt_l=K, n_l=100, wt_ab=K + 4096, n_ab=100, **_WSP),
    "idn_tv_chambolle_u8": dict(src=A, dst_u8=B, dst_f32=None, iters=None, n=1, h=8, w=16, c=3,
                                stride=_rows("c"), weight=0.1, eps=2e-4, n_iter_max=200, **_WSP),
    "idn_estimate_sigma": dict(src_u8=A, src_f64=None, dst=O, n=1, h=8, w=16, c=3,
                               stride=_rows("c"), **_WSP),
    "idn_wiener_u8": dict(src=A, dst_u8=B, dst_f64=None, n=1, h=8, w=16, c=3, stride=_rows("c"),
                          kh=3, kw=3, border=0, noise=None, noise_image_stride=0, noise_out=None,
                          **_WSP),
    "idn_dct_denoise_u8": dict(src=A, dst_u8=B, dst_f32=None, n=1, h=8, w=16, c=3,
                               stride=_rows("c"), patch=8, color=0, sigma=K, sigma_image_stride=0,
                               factor=3.0, ws=None, ws_bytes=0, stream=None),
    "idn_mse_u8": dict(a=A, b=B, mse_out=O, n=1, h=8, w=16, c=3, stride_a=_rows("c"),
                       stride_b=_rows("c"), **_WSP),
    "idn_ssim_u8": dict(a=A, b=B, ssim_out=O, ssim_ch=None, mse_out=None, n=1, h=8, w=16, c=3,
                        stride_a=_rows("c"), stride_b=_rows("c"), win=7, **_WSP),
    "idn_equalize_hist_u8": dict(src=A, dst=B, n=1, h=8, w=16, stride=_rows(1), **_WSP),
    "idn_clahe_u8": dict(src=A, dst=B, n=1, h=8, w=16, stride=_rows(1), clip=2.0, tx=4, ty=4,
                         **_WSP),
    "idn_correct_exposure_u8": dict(src=A, dst=B, n=1, h=8, w=16, stride=_rows(3), **_WSP),
    "idn_shader_u8": dict(_U8, factor=0.5, stream=None),
    "idn_bloom_u8": dict(_U8, circles=K, weights=K + 4096, ncirc=2, spans=K + 8192, stream=None),
    "idn_blob_from_f64": dict(src=O, blob=B, n=1, h=8, w=16, out_h=8, out_w=16, mean=MEAN, flip=0,
                              stream=None),
    "idn_resize_linear_f32": dict(src=A, dst=B, n=1, h=8, w=16, c=3, out_h=16, out_w=32, fx=2.0,
                                  fy=2.0, stream=None),
    "idn_blob_f32": dict(_U8, out_h=8, out_w=16, mean=MEAN, flip=0, stream=None),
}

# ws_bytes = NEED / SHORT: the op's published size for the row's shape
_NEED = {
    "idn_quant_u8": lambda L, d: L.idn_quant_workspace_size(d["n"], d["k"]),
    "idn_wavelet_denoise_u8": lambda L, d: L.idn_wavelet_workspace_size(
        d["n"], d["h"], d["w"], d["wavelet"], d["levels"]),
    "idn_wavelet_denoise_ycc": lambda L, d: L.idn_wavelet_workspace_size(
        d["n"], d["h"], d["w"], d["wavelet"], d["levels"]),
    "idn_wavelet_denoise_general": lambda L, d: L.idn_wavelet_general_workspace_size(
        d["n"], d["h"], d["w"], d["c"], d["wavelet"], d["levels"]),
    "idn_nlmeans_colored_u8": lambda L, d: L.idn_nlmeans_colored_workspace_size(
        d["n"], d["h"], d["w"]),
    "idn_tv_chambolle_u8": lambda L, d: L.idn_tv_chambolle_workspace_size(
        d["n"], d["h"], d["w"], d["c"]),
    "idn_estimate_sigma": lambda L, d: L.idn_estimate_sigma_workspace_size(
        d["n"], d["h"], d["w"], d["c"], 0),
    "idn_wiener_u8": lambda L, d: L.idn_wiener_workspace_size(d["n"], d["c"]),
    # strided rows: the size function's own case (compact images need less); no window, no SSIM part
    "idn_mse_u8": lambda L, d: L.idn_metrics_workspace_size(d["n"], d["h"], d["w"], d["c"], 0),
    # the default image is small enough for the SSIM part to be the larger one
    "idn_ssim_u8": lambda L, d: L.idn_metrics_workspace_size(
        d["n"], d["h"], d["w"], d["c"], d["win"]),
    "idn_equalize_hist_u8": lambda L, d: L.idn_exposure_workspace_size(
        d["n"], d["h"], d["w"], 1, 1),
    "idn_clahe_u8": lambda L, d: L.idn_exposure_workspace_size(
        d["n"], d["h"], d["w"], d["tx"], d["ty"]),
    "idn_correct_exposure_u8": lambda L, d: L.idn_exposure_workspace_size(
        d["n"], d["h"], d["w"], 4, 4),
}

# (entry point, overrides of its valid call)
ROWS = []


def _add(fns, *kws):
    """rows of one or several entry points; a row that a shared list already gave is not repeated"""
    for fn in ([fns] if isinstance(fns, str) else fns):
        ROWS.extend((fn, kw) for kw in kws if (fn, kw) not in ROWS)


def _ws_rows(fn, **big):
    """the workspace rule: missing, NULL with bytes given, one byte short, enough but misaligned,
    short and misaligned (the size is reported), and not asked for at n == 0.  `big`: a shape past
    the op's launch size, alone and with a missing or misaligned workspace"""
    _add(fn, dict(ws=None, ws_bytes=0), dict(ws=None), dict(ws_bytes=SHORT), dict(ws_bytes=0),
         dict(ws=WS + 4, ws_bytes=NEED), dict(ws=WS + 4, ws_bytes=SHORT), dict(ws=WS + 4),
         dict(ws=None, ws_bytes=0, n=0), dict(ws=WS + 4, ws_bytes=0, n=0))
    if big:
        _add(fn, dict(big), dict(big, ws=None, ws_bytes=0), dict(big, ws=WS + 4), dict(big, n=0))


# ---- the u8 -> u8 filters: pointers, in place, shape, channels 1..4, stride, then the op's own
FILTERS = ("idn_gaussian_blur_u8", "idn_gaussian_blur_sigma_u8", "idn_box_blur_u8",
           "idn_median_blur_u8", "idn_adaptive_median_u8", "idn_bilateral_u8",
           "idn_gaussian_blob_f32")
_add(FILTERS, dict(src=None), dict(dst=None), dict(src=None, dst=None), dict(dst=A), dict(n=-1),
     dict(h=0), dict(w=0), dict(h=-2, w=-3), dict(c=0), dict(c=5), dict(stride=47), dict(stride=0),
     dict(stride=-1), dict(n=0), dict(n=0, h=0), dict(n=0, src=None),
     # two rules at once: null / shape, in place / shape, shape / channels, channels / stride
     dict(src=None, h=0), dict(dst=A, n=-1), dict(dst=A, src=None), dict(h=0, c=5),
     dict(c=5, stride=47), dict(w=0, stride=-1), dict(n=0, stride=47))
_add(FILTERS[:5], dict(ksize=4), dict(ksize=33), dict(ksize=1), dict(stride=47, ksize=4),
     dict(c=5, ksize=4), dict(ksize=4, n=0), dict(ksize=33, src=None))
_add(FILTERS[:3], dict(ksize=7, n=0), dict(ksize=7, w=IMAX, c=1), dict(ksize=7, n=IMAX, h=1 << 20),
     dict(ksize=31, w=IMAX, c=1, stride=0))
_add(FILTERS[1], dict(sigma=-1.0), dict(sigma=NAN, ksize=9), dict(sigma=INF, ksize=9),
     dict(sigma=-1.0, ksize=4), dict(sigma=-1.0, stride=47), dict(sigma=2.0, n=0),
     dict(ksize=7, sigma=2.0, w=IMAX, c=1))
_add("idn_gaussian_taps", dict(taps=None), dict(taps=None, ksize=4), dict(ksize=4), dict(ksize=1),
     dict(ksize=33), dict(sigma=-1.0), dict(sigma=NAN), dict(sigma=INF, ksize=31),
     dict(ksize=4, sigma=-1.0), dict(), dict(ksize=9, sigma=1.5), dict(ksize=31))
_add("idn_median_blur_u8", dict(ksize=7, n=0), dict(ksize=7, w=IMAX, c=4),
     dict(ksize=31, w=IMAX // 2, c=4))
_add("idn_adaptive_median_u8", dict(kmap=A), dict(kmap=B), dict(kmap=A, ksize=4),
     dict(kmap=A, stride=47), dict(kmap=O, n=0), dict(ksize=2), dict(w=IMAX, c=4),
     dict(w=IMAX, c=4, ksize=4), dict(n=IMAX), dict(n=IMAX, h=64))
_add("idn_bilateral_u8", dict(c=2), dict(c=4), dict(c=2, n=0), dict(c=2, stride=31), dict(c=2, d=99),
     dict(d=19), dict(d=99), dict(d=0, sigma_space=100.0), dict(d=99, n=0), dict(n=IMAX),
     dict(n=IMAX, d=99), dict(n=IMAX, h=1 << 20))
_add("idn_gaussian_blob_f32", dict(mean=None), dict(mean=None, dst=None), dict(mean=None, src=None),
     dict(mean=None, n=0), dict(ksize=7), dict(ksize=31, n=0), dict(ksize=4), dict(ksize=33),
     dict(c=1), dict(stride=56), dict(h=3), dict(dst=B + 8), dict(w=15))
for _fn in ("idn_gaussian_blur_f64", "idn_box_blur_f64"):
    _add(_fn, dict(src=None), dict(dst=None), dict(dst=A), dict(n=-1), dict(h=0), dict(w=0),
         dict(c=0), dict(c=5), dict(n=0), dict(src=None, h=0), dict(ksize=4), dict(ksize=7),
         dict(ksize=7, n=0), dict(ksize=7, src=None))
_add("idn_box_blur_f64", dict(ksize=5))

# ---- quant and the colour conversions
_add("idn_quant_u8", dict(src=None), dict(dst=None), dict(dst=A), dict(n=-1), dict(n=65536),
     dict(h=0), dict(w=0), dict(stride=47), dict(k=0), dict(k=17), dict(h=1, w=2, k=3), dict(n=0),
     dict(n=0, ws=None, ws_bytes=0), dict(src=None, h=0), dict(dst=A, h=0), dict(h=0, stride=-1),
     dict(stride=47, k=0), dict(k=17, h=1, w=2), dict(k=0, ws=None), dict(n=0, k=0),
     dict(ws=None, ws_bytes=0), dict(ws=None, ws_bytes=4096), dict(ws=None), dict(ws_bytes=SHORT),
     dict(ws_bytes=0), dict(ws_bytes=SHORT, n=3, k=16), dict(ws=WS + 4, ws_bytes=SHORT))
CVT = ("idn_bgr2lab_u8", "idn_lab2bgr_u8", "idn_lbgr2lab_u8", "idn_lab2lbgr_u8")
YUV = ("idn_bgr2yuv_u8", "idn_yuv2bgr_u8")
_add(CVT + YUV, dict(src=None), dict(dst=None), dict(n=-1), dict(h=0), dict(w=0), dict(stride=47),
     dict(stride=0), dict(n=0), dict(n=0, stride=47), dict(src=None, h=0), dict(h=0, stride=47),
     dict(dst=A, n=0), dict(dst=A, h=0), dict(dst=A, src=None))
_add(YUV, dict(dst=A), dict(dst=A, stride=47), dict(n=1 << 16, h=1 << 16),
     dict(n=1 << 16, h=1 << 16, stride=47), dict(n=IMAX, h=1, w=257))
_add("idn_copy_u8", dict(src=None), dict(dst=None), dict(nbytes=-16), dict(policy=2),
     dict(policy=-1), dict(src=A + 8), dict(dst=B + 4), dict(nbytes=8), dict(nbytes=4095),
     dict(nbytes=0), dict(nbytes=0, dst=A), dict(nbytes=1 << 62), dict(src=None, nbytes=-16),
     dict(nbytes=-16, policy=2), dict(policy=2, src=A + 8), dict(src=A + 8, nbytes=8),
     dict(nbytes=0, policy=2), dict(nbytes=0, src=A + 8))

# ---- wavelets
for _fn in ("idn_wavelet_denoise_u8", "idn_wavelet_denoise_ycc"):
    _add(_fn, dict(out_u8=None), dict(out_u8=None, out_f32=O, n=0), dict(n=-1),
         dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 16), dict(wavelet=2), dict(wavelet=-1),
         dict(n=0), dict(n=0, ws=None, ws_bytes=0), dict(n=0, levels=13), dict(levels=13),
         dict(levels=0, n=0), dict(levels=13, ws=None), dict(out_u8=None, h=0), dict(h=0, wavelet=7),
         dict(ws=None, ws_bytes=0), dict(ws=None, ws_bytes=4096), dict(ws=None),
         dict(ws_bytes=SHORT), dict(ws_bytes=0), dict(ws_bytes=SHORT, wavelet=1, levels=2, h=37),
         dict(ws=WS + 4, ws_bytes=SHORT))
_add("idn_wavelet_denoise_u8", dict(src=None), dict(src=None, in64=O, n=0), dict(stride=47),
     dict(stride=47, wavelet=7), dict(h=1 << 16, w=1 << 16, stride=0), dict(src=None, out_u8=None))
_add("idn_wavelet_denoise_ycc", dict(in64=None), dict(keys=None), dict(in64=None, keys=None),
     dict(keys=None, out_u8=None), dict(keys=None, n=0))
_add("idn_wavelet_denoise_general", dict(src=None), dict(in64=O), dict(src=None, in64=O, n=0),
     dict(out_u8=None), dict(out_u8=None, out_f32=O, n=0), dict(n=-1), dict(h=0), dict(w=0),
     dict(c=2), dict(c=0), dict(c=4), dict(wavelet=-1), dict(wavelet=5), dict(method=2),
     dict(method=-1), dict(mode=2), dict(ycc=1, c=1), dict(h=1 << 16, w=1 << 16),
     dict(n=65536, c=1), dict(n=21846), dict(stride=47), dict(n=0), dict(n=0, levels=11),
     dict(n=0, ws=None, ws_bytes=0), dict(levels=11), dict(levels=0, n=0), dict(levels=11, ws=None),
     dict(src=None, out_u8=None), dict(out_u8=None, h=0), dict(h=0, c=2), dict(c=2, wavelet=9),
     dict(wavelet=9, method=2), dict(method=2, mode=2), dict(mode=2, ycc=1, c=1),
     dict(ycc=1, c=1, h=1 << 16, w=1 << 16), dict(h=1 << 16, w=1 << 16, n=65536),
     dict(n=65536, stride=47), dict(stride=47, levels=11),
     dict(ws=None, ws_bytes=0), dict(ws=None, ws_bytes=4096), dict(ws=None), dict(ws_bytes=SHORT),
     dict(ws_bytes=0), dict(ws_bytes=SHORT, wavelet=4, levels=2, h=37, c=1),
     dict(ws=WS + 4, ws_bytes=SHORT))

# ---- non-local means
_add("idn_nlmeans_weights", dict(n_weights=None), dict(shift=None), dict(fpm=None),
     dict(wt=None), dict(wt=None, cap=-1), dict(cap=-1), dict(hh=0.0), dict(hh=-1.0), dict(hh=INF),
     dict(hh=NAN), dict(c=2), dict(c=0), dict(c=4), dict(t=4), dict(t=1), dict(t=9), dict(s=4),
     dict(s=3), dict(s=23), dict(cap=-1, hh=0.0), dict(hh=0.0, c=2), dict(c=2, t=4))
_add("idn_nlmeans_colored_weights", dict(n_l=None), dict(n_ab=None), dict(shift=None),
     dict(fpm=None), dict(wt_l=None), dict(wt_ab=None), dict(cap_l=-1), dict(cap_ab=-1),
     dict(wt_l=None, cap_l=-1), dict(hh=0.0), dict(hh=INF), dict(h_color=0.0), dict(h_color=NAN),
     dict(t=4), dict(s=23), dict(cap_l=-1, hh=0.0), dict(hh=0.0, h_color=0.0),
     dict(h_color=0.0, t=4))
_NLM = [dict(src=None), dict(dst=None), dict(dst=A), dict(n=-1), dict(h=0), dict(w=0),
        dict(stride=95), dict(stride=0), dict(t=4), dict(t=9), dict(s=4), dict(s=23), dict(h=3),
        dict(w=3, h=8), dict(t=7, s=21, h=13), dict(t=7, s=21, h=14, w=14, n=0), dict(n=0),
        dict(n=0, h=3), dict(src=None, h=0), dict(dst=A, h=0), dict(dst=A, src=None),
        dict(stride=95, t=4), dict(t=4, h=3)]
_add("idn_nlmeans_u8", *_NLM)
_add("idn_nlmeans_u8", dict(weights=None), dict(c=2), dict(c=0), dict(c=4), dict(h=0, c=2),
     dict(c=2, stride=10), dict(n_weights=0), dict(n_weights=-5), dict(n_weights=24577),
     dict(n_weights=24576, n=0), dict(h=3, n_weights=0), dict(n_weights=24577, n=0),
     dict(n=IMAX, h=1024, w=1024), dict(n=IMAX, h=1024, w=1024, n_weights=24577))
_add("idn_nlmeans_colored_u8", *_NLM)
_add("idn_nlmeans_colored_u8", dict(wt_l=None), dict(wt_ab=None), dict(n_l=0), dict(n_ab=0),
     dict(n_l=24577), dict(n_ab=24577), dict(n_ab=24577, n=0), dict(h=3, n_l=0),
     dict(n_l=24577, ws=None), dict(ws=None, ws_bytes=0), dict(ws=None), dict(ws_bytes=SHORT),
     dict(ws_bytes=0), dict(ws=WS + 4, ws_bytes=SHORT), dict(ws=None, ws_bytes=0, n=0),
     dict(ws_bytes=SHORT, n=3, h=33, w=37), dict(n=IMAX, h=1024, w=1024),
     dict(n=IMAX, h=1024, w=1024, ws=None), dict(n=IMAX, h=1024, w=1024, ws_bytes=4096),
     dict(n=IMAX, h=1024, w=1024, ws_bytes=1 << 62), dict(n=IMAX, h=1024, w=1024, ws_bytes=1 << 62, n_l=0))

# ---- total variation, wiener, DCT, estimate_sigma
_PLANES = [dict(src=None), dict(dst_u8=None), dict(dst_u8=A), dict(n=-1), dict(h=0), dict(w=0),
           dict(c=2), dict(c=0), dict(c=4), dict(stride=47), dict(stride=0), dict(n=0),
           dict(n=0, ws=None, ws_bytes=0), dict(src=None, dst_u8=None), dict(src=None, h=0),
           dict(dst_u8=None, h=0), dict(dst_u8=A, h=0), dict(h=0, c=2), dict(c=2, stride=10)]
_add("idn_tv_chambolle_u8", *_PLANES)
_add("idn_tv_chambolle_u8", dict(dst_u8=None, dst_f32=O, n=0), dict(weight=0.0), dict(weight=-1.0),
     dict(weight=NAN), dict(weight=INF), dict(eps=-1.0), dict(eps=NAN), dict(eps=INF), dict(eps=0.0, n=0),
     dict(n_iter_max=0), dict(n_iter_max=1001), dict(n_iter_max=1000, n=0),
     dict(stride=47, weight=0.0), dict(weight=0.0, eps=-1.0), dict(eps=-1.0, n_iter_max=0),
     dict(n_iter_max=0, n=0), dict(n_iter_max=0, ws=None))
_ws_rows("idn_tv_chambolle_u8", n=1 << 16, h=1 << 16, w=1)
_add("idn_tv_chambolle_u8", dict(n=1 << 16, h=1 << 16, w=1, n_iter_max=0),
     dict(n=1, h=1, w=1 << 30, c=3), dict(ws_bytes=SHORT, n=3, h=65, w=257, c=1))
_add("idn_wiener_u8", *_PLANES)
_add("idn_wiener_u8", dict(dst_u8=None, dst_f64=O, n=0), dict(kh=0), dict(kh=2), dict(kw=4),
     dict(kh=33), dict(kw=33), dict(kh=31, kw=31, n=0), dict(border=2), dict(border=-1),
     dict(border=1, kh=17), dict(border=1, kh=15, kw=31, n=0), dict(border=1, kw=33),
     dict(border=0, kh=17, n=0), dict(dst_f64=O + 4), dict(noise=K + 4), dict(noise_out=K + 4),
     dict(noise=K, noise_image_stride=2), dict(noise=K, noise_image_stride=1),
     dict(noise=K, noise_image_stride=3, n=0), dict(noise=None, noise_image_stride=2, n=0),
     dict(stride=47, kh=2), dict(kh=2, border=2), dict(border=2, dst_f64=O + 4),
     dict(dst_f64=O + 4, noise=K + 4), dict(noise=K + 4, noise_image_stride=2),
     dict(noise=K, noise_image_stride=2, n=0), dict(h=1 << 15, w=1 << 15, c=1),
     dict(h=1 << 15, w=1 << 15, c=1, ws=None), dict(h=1 << 14, w=1 << 14, c=1, ws=None),
     dict(noise=K, ws=None, ws_bytes=0, n=0), dict(noise=K, ws=None, ws_bytes=0, w=IMAX, c=1),
     dict(noise=K, ws=WS + 4, ws_bytes=0, n=IMAX, h=1 << 20))
_ws_rows("idn_wiener_u8", w=IMAX, c=1)
_add("idn_wiener_u8", dict(n=IMAX, h=1 << 20, ws=None), dict(ws_bytes=SHORT, n=5, c=1))
_add("idn_dct_denoise_u8", *_PLANES)
_add("idn_dct_denoise_u8", dict(sigma=None), dict(src=None, sigma=None), dict(sigma=None, dst_u8=None),
     dict(dst_u8=None, dst_f32=O, n=0), dict(color=2), dict(color=-1), dict(color=1, c=1),
     dict(color=1, n=0), dict(dst_f32=O + 2), dict(dst_f32=O + 4, n=0), dict(sigma=K + 4),
     dict(sigma_image_stride=2), dict(sigma_image_stride=1), dict(sigma_image_stride=3, n=0),
     dict(factor=-1.0), dict(factor=NAN), dict(factor=INF), dict(factor=0.0, n=0), dict(patch=16),
     dict(patch=4), dict(patch=16, n=0), dict(h=7), dict(w=7), dict(h=7, n=0), dict(ws=WS + 4, n=0),
     dict(stride=47, color=2), dict(color=2, dst_f32=O + 2), dict(dst_f32=O + 2, sigma=K + 4),
     dict(sigma=K + 4, sigma_image_stride=2), dict(sigma_image_stride=2, factor=-1.0),
     dict(factor=-1.0, patch=16), dict(patch=16, h=7), dict(w=IMAX, c=1),
     dict(n=IMAX, h=1 << 20), dict(w=IMAX, c=1, n=0), dict(w=IMAX, c=1, patch=16))
_add("idn_estimate_sigma", dict(src_u8=None), dict(src_f64=O), dict(src_u8=None, src_f64=O, n=0),
     dict(dst=None), dict(src_u8=None, dst=None), dict(n=-1), dict(h=0), dict(w=0), dict(c=2),
     dict(c=0), dict(c=4), dict(stride=47), dict(src_u8=None, src_f64=O + 4), dict(dst=O + 4),
     dict(h=3), dict(w=3), dict(h=3, n=0), dict(n=0), dict(n=0, ws=None, ws_bytes=0),
     dict(dst=None, h=0), dict(h=0, c=2), dict(c=2, stride=10),
     dict(stride=47, src_u8=None, src_f64=O + 4), dict(src_u8=None, src_f64=O + 4, dst=O + 4),
     dict(dst=O + 4, h=3), dict(h=3, ws=None))
_ws_rows("idn_estimate_sigma", h=(1 << 17) + 1, w=(1 << 17) + 1, c=1)
_add("idn_estimate_sigma", dict(n=IMAX, h=1024, w=1024, c=1), dict(w=1 << 30, c=3),
     dict(ws_bytes=SHORT, n=3, c=1))

# ---- metrics: the workspace is checked before the launch size
_PAIR = [dict(a=None), dict(b=None), dict(n=-1), dict(h=0), dict(w=0), dict(c=2), dict(c=0),
         dict(c=4), dict(stride_a=47), dict(stride_b=47), dict(stride_a=0, stride_b=-1), dict(n=0),
         dict(n=0, ws=None, ws_bytes=0), dict(a=None, h=0), dict(h=0, c=2), dict(c=2, stride_a=10),
         dict(b=A, n=0), dict(b=A, h=0)]
_BIGPAIR = dict(n=IMAX, h=1 << 12, w=1 << 12, ws_bytes=1 << 62)
for _fn, _out in (("idn_mse_u8", "mse_out"), ("idn_ssim_u8", "ssim_out")):
    _add(_fn, *_PAIR)
    _add(_fn, {_out: None}, {_out: None, "stride_a": 47}, {_out: None, "n": 0},
         {_out: None, "ws": None}, dict(_BIGPAIR), dict(_BIGPAIR, ws=None), dict(_BIGPAIR, ws=WS + 4),
         dict(_BIGPAIR, ws_bytes=4096), dict(_BIGPAIR, n=0))
# the mse rows of the workspace rule use strided images: the size function's case
_STRIDED = dict(stride_a=56, stride_b=64)
_add("idn_mse_u8", dict(h=1 << 16, stride_a=1 << 15), dict(h=1 << 16, stride_b=1 << 15),
     dict(h=1 << 16, stride_a=1 << 15, ws=None), dict(h=1 << 16, stride_a=1 << 15, n=0),
     dict(h=1 << 16, stride_a=1 << 15, mse_out=None),
     dict(_STRIDED, ws=None, ws_bytes=0), dict(_STRIDED, ws=None), dict(_STRIDED, ws_bytes=SHORT),
     dict(_STRIDED, ws_bytes=0), dict(_STRIDED, ws=WS + 4, ws_bytes=NEED),
     dict(_STRIDED, ws=WS + 4, ws_bytes=SHORT), dict(ws=None, ws_bytes=0), dict(ws_bytes=7),
     dict(ws=WS + 4, ws_bytes=8), dict(stride_a=3008, stride_b=3016, ws_bytes=SHORT, n=3, h=600, w=1000))
_add("idn_ssim_u8", dict(win=4), dict(win=1), dict(win=13), dict(win=0, n=0), dict(h=5),
     dict(w=6), dict(h=5, n=0), dict(win=3, h=3, w=3, n=0), dict(win=13, h=5),
     dict(ssim_out=None, win=4), dict(win=9, ws=None), dict(h=5, ws=None))
_ws_rows("idn_ssim_u8")
_add("idn_ssim_u8", dict(ws_bytes=SHORT, n=3, h=64, w=100, c=1, win=11))

# ---- exposure
EXPOSURE = ("idn_equalize_hist_u8", "idn_clahe_u8", "idn_correct_exposure_u8")
_add(EXPOSURE, dict(src=None), dict(dst=None), dict(dst=A), dict(n=-1), dict(h=0), dict(w=0),
     dict(stride=15), dict(stride=0), dict(n=0), dict(src=None, h=0), dict(dst=A, h=0),
     dict(dst=A, src=None), dict(h=0, stride=0), dict(stride=15, ws=None), dict(n=0, stride=15))
for _fn in EXPOSURE:
    _ws_rows(_fn, h=1 << 16, w=1 << 16)
    _add(_fn, dict(ws_bytes=SHORT, n=3, h=37, w=41))
_add("idn_clahe_u8", dict(tx=0), dict(ty=0), dict(tx=17), dict(ty=17), dict(tx=16, ty=16, n=0),
     dict(ty=8), dict(tx=16), dict(h=4), dict(ty=8, n=0), dict(clip=-1.0), dict(clip=NAN),
     dict(clip=INF), dict(clip=0.0, n=0), dict(stride=15, tx=0), dict(tx=0, ty=8),
     dict(ty=8, clip=-1.0), dict(clip=-1.0, ws=None), dict(tx=0, n=0),
     dict(ws_bytes=SHORT, tx=16, ty=7, h=37, w=41))
_add("idn_correct_exposure_u8", dict(h=4), dict(w=4), dict(h=4, n=0), dict(h=4, ws=None),
     dict(stride=47, h=4), dict(stride=47))

# ---- misc, blob
_add(("idn_shader_u8", "idn_bloom_u8"), dict(src=None), dict(dst=None), dict(c=1), dict(c=4),
     dict(n=-1), dict(h=0), dict(w=0), dict(stride=47), dict(n=0), dict(n=0, dst=A),
     dict(src=None, c=1), dict(c=1, h=0), dict(n=0, stride=47))
_add("idn_bloom_u8", dict(circles=None), dict(weights=None), dict(spans=None), dict(ncirc=-1),
     dict(ncirc=0, n=0), dict(spans=None, c=1))
_add("idn_blob_from_f64", dict(src=None), dict(blob=None), dict(mean=None), dict(n=-1), dict(h=0),
     dict(w=0), dict(out_h=7), dict(out_w=15), dict(n=0), dict(mean=None, h=0), dict(n=0, out_h=7))
_add("idn_resize_linear_f32", dict(src=None), dict(dst=None), dict(n=-1), dict(h=0), dict(w=0),
     dict(c=0), dict(out_h=0), dict(out_w=0), dict(fx=0.0), dict(fy=-1.0), dict(fx=NAN), dict(n=0),
     dict(src=None, h=0), dict(n=0, c=0))
_add("idn_blob_f32", dict(src=None), dict(dst=None), dict(mean=None), dict(c=1), dict(c=4),
     dict(n=-1), dict(h=0), dict(w=0), dict(out_h=7), dict(out_w=15), dict(stride=47), dict(n=0),
     dict(src=None, c=1), dict(c=1, h=0), dict(h=0, out_h=-1), dict(out_h=7, stride=47),
     dict(n=0, stride=47))

ENTRY_POINTS = set(SPECS)

# ---- the published workspace sizes and offsets: (function, one value list per argument); every
# argument varies on its own, the degenerate values that give 0 included
SIZES = [
    ("idn_quant_workspace_size", ((-1, 0, 1, 2, 3, 7, 64, 65535), (-1, 0, 1, 2, 3, 7, 8, 16, 17))),
    ("idn_quant_runs_offset", ((-1, 0, 1, 2, 3, 7, 64, 65535), (-1, 0, 1, 2, 3, 7, 8, 16, 17))),
    ("idn_nlmeans_colored_workspace_size", ((-1, 0, 1, 2, 5), (0, 1, 7, 32, 600),
                                            (-1, 1, 15, 16, 1000))),
    ("idn_wiener_workspace_size", ((-1, 0, 1, 2, 7, 65536), (0, 1, 2, 3, 4))),
    ("idn_dct_denoise_workspace_size", ((0, 1, 8), (0, 8, 600), (0, 8, 1000), (0, 1, 3))),
    ("idn_tv_chambolle_workspace_size", ((-1, 0, 1, 2, 5), (0, 1, 63, 64, 65, 600),
                                         (0, 1, 255, 256, 257, 1000), (0, 1, 2, 3, 4))),
    ("idn_estimate_sigma_workspace_size", ((-1, 0, 1, 3), (3, 4, 5, 600), (3, 4, 100, 1000),
                                           (0, 1, 2, 3, 4), (0, 1))),
    ("idn_metrics_workspace_size", ((0, 1, 3), (0, 1, 7, 8, 64, 600), (0, 1, 7, 33, 1000),
                                    (1, 2, 3), (0, 3, 4, 7, 11, 13))),
    ("idn_exposure_workspace_size", ((0, 1, 3), (0, 1, 7, 64, 600), (0, 1, 9, 1000),
                                     (0, 1, 4, 8, 16, 17), (0, 1, 3, 4, 16, 17))),
    ("idn_wavelet_workspace_size", ((0, 1, 3), (0, 1, 8, 13, 64, 600), (1, 8, 30, 1000),
                                    (-1, 0, 1, 2), (0, 1, 2, 3, 4, 13))),
    ("idn_wavelet_stats_offset", ((0, 1, 3), (0, 1, 8, 13, 64, 600), (1, 8, 30, 1000),
                                  (-1, 0, 1, 2), (0, 1, 2, 3, 4, 13))),
    ("idn_wavelet_general_workspace_size", ((0, 1, 2, 4), (0, 8, 37, 600), (8, 31, 1000),
                                            (1, 2, 3), (-1, 0, 2, 3, 4, 5), (0, 1, 3, 10, 11))),
]


def row_id(fn, kw):
    return "%s(%s)" % (fn, ", ".join(f"{k}={kw[k]!r}" for k in sorted(kw)))


def arguments(lib, fn, kw):
    """the row's argument list, and what must stay alive during the call"""
    unknown = set(kw) - set(SPECS[fn])
    assert not unknown, (fn, unknown)
    d = dict(SPECS[fn], **kw)
    for k, v in d.items():
        if callable(v):
            d[k] = v(d)
    if d.get("ws_bytes") in (NEED, SHORT):
        d["ws_bytes"] = _NEED[fn](lib, d) - (d["ws_bytes"] == SHORT)
    keep = {MEAN: (ctypes.c_double * 3)(102.9801, 115.9465, 122.7717),
            TAPS: (ctypes.c_uint16 * 32)()}
    return [keep.get(v, v) if isinstance(v, str) else v for v in d.values()], keep


def call(lib, fn, kw):
    """the row's call on `lib` -> [return code, idn_last_error() text or None]"""
    args, keep = arguments(lib, fn, kw)
    rc = getattr(lib, fn)(*args)
    return [rc, lib.idn_last_error().decode() if rc != 0 else None]


def sizes(lib, fn, grid):
    return [getattr(lib, fn)(*p) for p in itertools.product(*grid)]


def dump(lib):
    """the fixture's text for `lib`: one row, and one size function, per line"""
    rows = ",\n".join(f"{json.dumps(row_id(fn, kw))}: {json.dumps(call(lib, fn, kw))}"
                      for fn, kw in ROWS)
    size = ",\n".join(f"{json.dumps(fn)}: {json.dumps(sizes(lib, fn, grid), separators=(',', ':'))}"
                      for fn, grid in SIZES)
    return '{"rows": {\n' + rows + '\n},\n"sizes": {\n' + size + "\n}}\n"


def _lib():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is visible: a row the library accepted would launch on fake addresses")
    from idn import _lib
    if not Path(_lib.LIB_PATH).exists():
        pytest.skip("libidn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _accepted_without_launch(fn, kw):
    d = dict(SPECS[fn], **kw)
    return d.get("n") == 0 or d.get("nbytes") == 0 or fn == "idn_gaussian_taps"


def test_the_table_names_every_entry_point_and_no_row_launches():
    from idn._lib import SIGNATURES
    sized = {fn for fn, _ in SIZES}
    other = {fn for fn in SIGNATURES if fn.startswith(("idn_noise", "idn_jpeg", "idn_add_pattern"))}
    other |= {"idn_abi_version", "idn_version", "idn_last_error", "idn_poisson_levels",
              "idn_periodic_pattern_u8", "idn_copy_slots_u8"}
    assert ENTRY_POINTS | sized | other == set(SIGNATURES) and not ENTRY_POINTS & (sized | other)
    assert {fn for fn, _ in ROWS} == ENTRY_POINTS
    want = json.loads(FIXTURE.read_text())
    ids = [row_id(fn, kw) for fn, kw in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(want["rows"])
    for fn, kw in ROWS:  # a row that is accepted must have nothing to launch
        rc, msg = want["rows"][row_id(fn, kw)]
        assert rc in (-1, -2, -4) and msg or rc == 0 and msg is None and \
            _accepted_without_launch(fn, kw), (fn, kw, rc, msg)
    assert [fn for fn, _ in SIZES] == list(want["sizes"])
    for fn, grid in SIZES:
        assert len(want["sizes"][fn]) == len(list(itertools.product(*grid))), fn
        assert any(want["sizes"][fn]) or fn == "idn_dct_denoise_workspace_size", fn  # always 0


def test_every_refusal_keeps_its_code_and_text():
    lib = _lib()
    want = json.loads(FIXTURE.read_text())["rows"]
    bad = []
    for fn, kw in ROWS:
        got = call(lib, fn, kw)
        if got != want[row_id(fn, kw)]:
            bad.append(f"{row_id(fn, kw)}: got {got}, expected {want[row_id(fn, kw)]}")
    assert not bad, "\n".join(bad)


def test_every_workspace_size_and_offset():
    lib = _lib()
    want = json.loads(FIXTURE.read_text())["sizes"]
    for fn, grid in SIZES:
        got = sizes(lib, fn, grid)
        bad = [(p, g, w) for p, g, w in zip(itertools.product(*grid), got, want[fn]) if g != w]
        assert not bad, (fn, bad[:8])


def test_the_fixture_is_what_the_recorder_writes():
    assert dump(_lib()) == FIXTURE.read_text()
