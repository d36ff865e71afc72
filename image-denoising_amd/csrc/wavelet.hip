// Wavelet denoiser: skimage 0.14.2 denoise_wavelet(img, method='BayesShrink', mode='soft',
// wavelet=db1|bior1.5, multichannel=True, convert2ycbcr=True, wavelet_levels=L) followed by the
// caller's (255 * out).astype(np.uint8).
// Reference call sites: lib/model/test.py:197-201,1807-1810, lib/roi_data_layer/minibatch.py:
// 1653-1656, minibatch_before_curvelet.py:85-87.  Restated in numpy in oracle/wavelet.py (pinned
// against pywt 1.1.1 / skimage 0.18.3 fixtures).
//
// Three paths, a translation unit each (the host side at the end of this file picks one; every
// other option of denoise_wavelet has a unit and an entry point of its own, wavelet_general.hip):
//   fused Haar  db1, L <= 3, sides divisible by 2^L: every level inside a 2^L x 2^L block, two
//               passes over the image (wl_haar_*, and haar3.hpp's wl_h3_* for L = 3 on u8)
//               -- wavelet_haar.hip, which also has what the other two paths launch of it:
//               the sigma medians (wavelet_sigma.hpp: wl_median over the fp64 band,
//               wl_haar_median over dd codes) and the proxy min / max (wl_h3_stats<true>)
//   streaming   bior1.5: wl_dwt_stream / wl_synth_final3, one launch per level
//               -- wavelet_stream.hip
//   tiled       db1 otherwise: wl_dwt_rb / wl_synth / wl_synth_final, one launch per level
//               -- wavelet_tiled.hip
// This unit has what they share: the workspace layout (wl_layout), the kernels every path may
// launch (wl_init_stats, wl_color_minmax, wl_sumsq, wl_thresh), the per-level driver wl_run, and
// the entry points.  wavelet_common.hpp: constants, layout and statistics structs,
// the device helpers of more than one unit, and the host functions through which the units call
// one another (the launchers are the seams; every kernel is instantiated in one unit only).
// wavelet_sigma.hpp (included by wavelet_haar.hip alone): the sigma medians and their helpers;
// they share the radix selection, whose code comes out differently when its callers are spread
// over units, so they stay in one.
// Every path (all images of the batch in every launch) is
//   colour range  per-channel fp64 min / max of the YCbCr image (BGR data treated as RGB, as the
//                 reference does); the YCbCr planes are never stored
//   analysis      levels 1..L; level 1 normalises (x - min) / (max - min) on the fly; every level
//                 leaves per-workgroup sums of squares of its detail bands
//   sigma         median(|finest dd| != 0) / 0.6744897501960817, exact: the finest dd keeps pywt's
//                 fp64 op order (multiply then add, no FMA), so a detail of equal samples is 0
//   thresholds    BayesShrink t = var / sqrt(max(mean(d^2) - var, eps)) per band, from fp64 sums
//   synthesis     levels L..1, details soft-thresholded as they are read; level 1 is fused with
//                 clip [0, 1], de-normalisation, YCbCr -> RGB, clip and the U8 / f32 stores
// Bands that only continuous arithmetic reads are stored, and where measured faster computed, in
// fp32 (wl_fband).  DESIGN.md lists the forms of the product and of the tuning library.
#include "wavelet_common.hpp"
#include "abi_args.hpp"

namespace idn {

inline WlLayout wl_layout(int n, int h, int w, int wv, int levels) {
  WlLayout Lt;
  Lt.n = n;
  Lt.h = h;
  Lt.w = w;
  Lt.F = wl_filter_len(wv);
  if (levels <= 0) {
    const int ml = std::min(wl_max_level(h, Lt.F), wl_max_level(w, Lt.F));
    levels = std::max(ml - 3, 1);
  }
  Lt.L = levels;
  Lt.H[0] = h;
  Lt.W[0] = w;
  size_t off = (size_t)3 * h * w;
  for (int l = 1; l <= Lt.L && l <= WL_MAXL; ++l) {
    Lt.H[l] = (Lt.H[l - 1] + Lt.F - 1) / 2;
    Lt.W[l] = (Lt.W[l - 1] + Lt.F - 1) / 2;
    Lt.off_band[l] = off;
    off += (size_t)12 * Lt.H[l] * Lt.W[l];
  }
  Lt.img_floats = align_up(off, 64);
  Lt.stats_off = (size_t)n * Lt.img_floats * sizeof(wreal);
  size_t tiles_tot = 0;
  for (int l = 1; l <= Lt.L && l <= WL_MAXL; ++l) {
    if (wv == IDN_WAVELET_BIOR15) {
      // wl_dwt_stream: strips x row bands of whole WS_G-row groups (the bands' sums are exact,
      // see the kernel).  sq_grid: 2^-F with the band's total below 2^(52 - F) for any input.
      // With the filters' L1 norms Llo = 4 B1 + 4 B2 + 2 S2 (~1.967) and Lhi = 2 S2 (~1.414),
      // level-l data of a [0, 1] image lie within Llo^(2(l-1)) (the 'aa' chain) and a detail
      // coefficient within Llo * Lhi times that, so a square <= (Llo Lhi)^2 Llo^(4(l-1))
      const int groups = (Lt.H[l] + WS_G - 1) / WS_G;
      Lt.tiles_x[l] = ws_strips(Lt.W[l]);
      Lt.bands[l] = std::min(ws_bands(n, Lt.H[l], Lt.W[l], Lt.tiles_x[l], l), groups);
#ifdef IDN_TUNING_BUILD
      // a fixed band count per level (bit field: level l's count in bits 8(l-1)..)
      if (const int fb = (knob("IDN_WAVELET_BANDS", 0) >> (8 * (l - 1))) & 0xFF)
        Lt.bands[l] = std::min(fb, groups);
#endif
      Lt.tiles[l] = Lt.tiles_x[l] * Lt.bands[l];
      const double llo = 4.0 * B1 + 4.0 * B2 + 2.0 * S2, lhi = 2.0 * S2;
      const double bound = (llo * lhi) * (llo * lhi) * std::pow(llo, 4.0 * (l - 1)) *
                           (double)Lt.H[l] * (double)Lt.W[l];
      Lt.sq_grid[l] = std::ldexp(1.0, (int)std::ceil(std::log2(bound)) - 52);
    } else {
      Lt.bands[l] = 0;
      Lt.tiles_x[l] = (Lt.W[l] + RB_TX - 1) / RB_TX;  // wl_dwt_rb tiles
      Lt.tiles[l] = Lt.tiles_x[l] * ((Lt.H[l] + RB_TY - 1) / RB_TY);
    }
    Lt.part_tile0[l] = tiles_tot;
    tiles_tot += (size_t)Lt.tiles[l];
  }
  if (wv == IDN_WAVELET_DB1 && Lt.L <= 3 && h % (1 << Lt.L) == 0 && w % (1 << Lt.L) == 0) {
    // the fused Haar path's partials: one per workgroup of 128 threads and level
    const size_t ns = Lt.L == 3 ? 4 : 1;
    const size_t nwg = ((size_t)(h >> Lt.L) * (size_t)(w >> Lt.L) * ns + 127) / 128;
    tiles_tot = std::max(tiles_tot, (size_t)Lt.L * nwg);
  }
  Lt.part_per_img = 9 * tiles_tot;  // [c][b][tile]
  Lt.part_off = Lt.stats_off + (size_t)n * WL_STATS * sizeof(double);
  Lt.bytes = Lt.part_off + (size_t)n * Lt.part_per_img * sizeof(double);
  return Lt;
}

// ---- 1: colour transform + min / max -----------------------------------------------------------
// ycc_keys (nullable): the colour range already reduced by the float64 noise kernel that wrote the
// input (idn_noise_ycc_u8), per image min keys of Y Cb Cr then max keys -- copied in, and
// wl_color_minmax does not run
__global__ void wl_init_stats(double* stats, int n, const unsigned long long* ycc_keys = nullptr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * WL_STATS) return;
  const int k = i % WL_STATS, img = i / WL_STATS;
  if (k >= WlStats::MN64 && k < WlStats::MN64 + 3) {
    reinterpret_cast<unsigned long long*>(stats)[i] =
        ycc_keys ? ycc_keys[6 * img + (k - WlStats::MN64)] : ~0ull;  // min key
  } else if (k >= WlStats::MX64 && k < WlStats::MX64 + 3) {
    reinterpret_cast<unsigned long long*>(stats)[i] =
        ycc_keys ? ycc_keys[6 * img + 3 + (k - WlStats::MX64)] : 0ull;  // max key
  } else {
    stats[i] = 0.0;
  }
}

// per-channel min / max of the YCbCr image (fp64 exact); the planes themselves are never
// stored: the analysis recomputes Y/Cb/Cr while staging.  Compact u8 rows (row_stride == 3w,
// dword-aligned) take 4 pixels per thread with three dword loads and no index division.
__global__ __launch_bounds__(256) void wl_color_minmax(const uint8_t* __restrict__ src,
                                                       const double* __restrict__ in64, int h, int w,
                                                       int64_t row_stride, double* __restrict__ stats) {
  const int img = blockIdx.y;
  const int64_t np = (int64_t)h * w;
  // the dot products only: x -> round(x + k) is monotone, so the min / max of ycbcr64's rounded
  // sums is the rounded sum of the dot products' min / max -- the offsets are added once per
  // wave after the reduction (bit-identical, three fp64 adds per pixel fewer)
  double dmn[3] = {INFINITY, INFINITY, INFINITY}, dmx[3] = {-INFINITY, -INFINITY, -INFINITY};
  auto acc = [&](double v0, double v1, double v2) {
    const double yc[3] = {dot3(v0, v1, v2, 65.481, 128.553, 24.966),
                          dot3(v0, v1, v2, -37.797, -74.203, 112.0),
                          dot3(v0, v1, v2, 112.0, -93.786, -18.214)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // inputs are finite: fmin / fmax are plain selects
      dmn[c] = fmin(dmn[c], yc[c]);
      dmx[c] = fmax(dmx[c], yc[c]);
    }
  };
  const bool flat = !in64 && row_stride == (int64_t)w * 3 && (np & 3) == 0 &&
                    (((uintptr_t)src & 3) == 0);
  if (flat) {
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + (int64_t)img * h * row_stride);
    const int nq = (int)(np >> 2);  // groups of 4 pixels = 3 dwords
    const int stride = gridDim.x * blockDim.x;
    for (int q0 = blockIdx.x * blockDim.x + threadIdx.x; q0 < nq; q0 += 4 * stride) {
      uint32_t d[4][3];  // 4 groups in flight per thread
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = q0 + u * stride;
#pragma unroll
        for (int j = 0; j < 3; ++j) d[u][j] = q < nq ? s4[3 * q + j] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (q0 + u * stride >= nq) break;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          double v[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int k = 3 * p + c;
            v[c] = (double)((d[u][k >> 2] >> (8 * (k & 3))) & 0xFFu) * (1.0 / 255.0);
          }
          acc(v[0], v[1], v[2]);
        }
      }
    }
  } else {
    // pixel p = y * w + x with 32-bit index math (p < 2^31 per image: checked on the host)
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < (int)np; p += gridDim.x * blockDim.x) {
      const int y = p / w, x = p - y * w;
      double v[3];
      load_rgb64(src, in64, img, h, w, row_stride, y, x, v);
      acc(v[0], v[1], v[2]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double da = dmn[c], db = dmx[c];
    for (int o = 32; o > 0; o >>= 1) {
      da = fmin(da, __shfl_xor(da, o));
      db = fmax(db, __shfl_xor(db, o));
    }
    if ((threadIdx.x & 63) == 0 && da <= db) {
      const double off = c == 0 ? 16.0 : 128.0;  // ycbcr64's offsets
      atomicMinD(stats + (size_t)img * WL_STATS + WlStats::MN64 + c, __dadd_rn(da, off));
      atomicMaxD(stats + (size_t)img * WL_STATS + WlStats::MX64 + c, __dadd_rn(db, off));
    }
  }
}

// ---- 3: sum of squares per detail band ----------------------------------------------------------
__global__ __launch_bounds__(256) void wl_sumsq(double* __restrict__ stats,
                                                const double* __restrict__ part, WlLayout Lt) {
  // block = (img, c, l, b): add the level's tile partials in tile order (deterministic)
  int t = blockIdx.x;
  const int b = t % 3;
  t /= 3;
  const int l = t % Lt.L;
  t /= Lt.L;
  const int c = t % 3;
  const int img = t / 3;
  const int lev = l + 1;
  const double* p = part + img * Lt.part_per_img + (size_t)(c * 3 + b) * (Lt.part_per_img / 9) +
                    Lt.part_tile0[lev];
  double s = 0.0;
  for (int k = threadIdx.x; k < Lt.tiles[lev]; k += 256) s += p[k];
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    stats[(size_t)img * WL_STATS + WlStats::sumsq(c, l, b, Lt.L)] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- 4: sigma: wavelet_sigma.hpp, launched through wl_band_median / wl_code_median ---------------

// ---- 5: BayesShrink thresholds ------------------------------------------------------------------
__global__ void wl_thresh(double* __restrict__ stats, WlLayout Lt) {
  const int img = blockIdx.x;
  if (threadIdx.x != 0) return;
  double* st = stats + (size_t)img * WL_STATS;
  bool bad = false;
  for (int c = 0; c < 3; ++c) {
    double mn, mx;
    wl_minmax64(st, c, mn, mx);
    if (!(mx > mn)) bad = true;  // 0.14.2 divides by zero -> NaN everywhere -> U8 0
    const double sigma = st[WlStats::median(c, Lt.L)] / 0.6744897501960817;
    if (!(sigma == sigma)) bad = true;
    const double var = sigma * sigma;
    for (int l = 0; l < Lt.L; ++l)
      for (int b = 0; b < 3; ++b) {
        const int lev = l + 1;
        const double cnt = (double)Lt.H[lev] * Lt.W[lev];
        const double dvar = st[WlStats::sumsq(c, l, b, Lt.L)] / cnt;
        const double t = var / sqrt(fmax(dvar - var, 2.220446049250313e-16));
        st[WlStats::thr(c, l, b, Lt.L)] = t;
        if (Lt.L <= 3) st[WlStats::thrh(c, l, b)] = 0.5 * t;
      }
  }
  st[WlStats::FLAG] = bad ? 1.0 : 0.0;
}

// ---- host side ----------------------------------------------------------------------------------
// One launcher per kernel family (each argument list once; a path's launchers are in its unit),
// then the two drivers: wl_run_haar (the fused path, wavelet_haar.hip) and wl_run (one launch per
// level: bior1.5 streaming, db1 tiled).  The product's forms are the ones written out; every
// branch that only a tuning knob reaches is inside #ifdef IDN_TUNING_BUILD, so the product
// library instantiates only the kernels it can launch.

// ---- launchers: the shared kernels --------------------------------------------------------------
void wl_clear_stats(const WlCall& C, const WlLayout& Lt) {
  hipLaunchKernelGGL(wl_init_stats, dim3((Lt.n * WL_STATS + 255) / 256), dim3(256), 0, C.st,
                     C.stats, Lt.n, C.ycc_keys);
}
void wl_minmax_exact(const WlCall& C, const WlLayout& Lt) {
  const int64_t np = (int64_t)Lt.h * Lt.w;
  // a few long-lived workgroups per image: per-wave reduction + atomics are the fixed cost
  const int gx = (int)std::min<int64_t>((np / 4 + 255) / 256, 24);
  hipLaunchKernelGGL(wl_color_minmax, dim3(gx, Lt.n), dim3(256), 0, C.st, C.src, C.in64, Lt.h,
                     Lt.w, C.row_stride, C.stats);
}
void wl_sum_partials(const WlCall& C, const WlLayout& Ls) {
  hipLaunchKernelGGL(wl_sumsq, dim3(Ls.n * 3 * Ls.L * 3), dim3(256), 0, C.st, C.stats, C.part, Ls);
}
void wl_thresholds(const WlCall& C, const WlLayout& Lt) {
  hipLaunchKernelGGL(wl_thresh, dim3(Lt.n), dim3(64), 0, C.st, C.stats, Lt);
}

// the fused path applies: db1, 1 <= L <= 3, both sides divisible by 2^L, room for its partials
static bool wl_haar_ok(int wavelet, const WlLayout& Lt, const uint8_t* src, int64_t row_stride) {
  if (wavelet != IDN_WAVELET_DB1 || Lt.L < 1 || Lt.L > 3 || tuned("IDN_WAVELET_FUSED", 1) == 0)
    return false;
  const int B = 1 << Lt.L;
  if (Lt.h % B || Lt.w % B) return false;
  if (src && (((uintptr_t)src & 3) || (row_stride & 3))) return false;  // dword row loads
  const int64_t ns = Lt.L == 3 ? 4 : 1;
  const int64_t nwg = ((int64_t)(Lt.h / B) * (Lt.w / B) * ns + WLH_WG - 1) / WLH_WG;
  return (int64_t)Lt.L * nwg <= (int64_t)(Lt.part_per_img / 9);
}

// The per-level paths: bior1.5 (streaming forms) and db1 outside the fused path (tiled forms).
// The product's forms are the ones written out here; the tuning library's knobs swap in the A/B
// forms, inside the launchers and in the guarded lines below.
static void wl_run(const WlCall& C, const WlLayout& Lt, bool bior) {
  wl_clear_stats(C, Lt);
  // u8 input in whole 8x8 blocks with dword-aligned rows: the Haar path's proxy min / max
  // (wl_h3_stats<true>: fp32 proxies, fp64 rescans of the steps near an extreme); else the fp64
  // chain on every pixel
  if (!C.ycc_keys && C.src && Lt.h % 8 == 0 && Lt.w % 8 == 0 && C.row_stride % 4 == 0 &&
      ((uintptr_t)C.src & 3) == 0 && tuned("IDN_WAVELET_MMPROXY", 1))
    wl_minmax_proxy(C, Lt);
  else if (!C.ycc_keys) wl_minmax_exact(C, Lt);
  // sigma from level-1 dd codes (wl_haar_median<1, true, ..>) when the channel's input-plane slot
  // holds codes + keys + positions (2.25 band sizes); else the radix select over the fp64 band
  const size_t bsz1 = (size_t)Lt.H[1] * Lt.W[1];
  const bool codes =
      (bsz1 + 3) / 4 + 2 * bsz1 <= (size_t)Lt.h * Lt.w && tuned("IDN_WAVELET_CODEMED", 1);
  for (int l = 1; l <= Lt.L; ++l) {
    if (bior) wl_stream_analysis(C, Lt, l, codes);
    else wl_tiled_analysis(C, Lt, l, codes);
  }
  // the code median also reduces the sums of squares and sets the thresholds
  const bool fuse = codes && tuned("IDN_WAVELET_FUSETHR", 1);
  const double* part_f = fuse ? C.part : nullptr;
  if (!fuse) wl_sum_partials(C, Lt);
  if (!codes) wl_band_median(C, Lt);
  else wl_code_median(C, Lt, part_f, wl_dd32(bior, codes));
  if (!fuse) wl_thresholds(C, Lt);
  for (int l = Lt.L; l >= 1; --l) {
    if (!bior) wl_tiled_synthesis(C, Lt, l, wl_fm_synthesis(l, false), IDN_WAVELET_DB1);
#ifdef IDN_TUNING_BUILD
    else if (!wl_stream_synthesis_on(l))
      wl_tiled_synthesis(C, Lt, l, wl_stream_fm_synthesis(Lt, l, codes), IDN_WAVELET_BIOR15);
#endif
    else wl_stream_synthesis(C, Lt, l, codes);
  }
}

}  // namespace idn

extern "C" size_t idn_wavelet_workspace_size(int n, int h, int w, int wavelet, int levels) {
  using namespace idn;
  if (n <= 0 || h <= 0 || w <= 0 || (wavelet != IDN_WAVELET_DB1 && wavelet != IDN_WAVELET_BIOR15))
    return 0;
  return wl_layout(n, h, w, wavelet, levels).bytes;
}

extern "C" size_t idn_wavelet_stats_offset(int n, int h, int w, int wavelet, int levels) {
  using namespace idn;
  if (n <= 0 || h <= 0 || w <= 0 || (wavelet != IDN_WAVELET_DB1 && wavelet != IDN_WAVELET_BIOR15))
    return 0;
  return wl_layout(n, h, w, wavelet, levels).stats_off;
}

namespace idn {
static int wavelet_impl(const uint8_t* src, const double* in_f64,
                        const unsigned long long* ycc_keys, uint8_t* out_u8, float* out_f32, int n,
                        int h, int w, int64_t row_stride, int wavelet, int levels, void* workspace,
                        size_t ws_bytes, void* stream) {
  IDN_CHECK_ARG(src || in_f64, "idn_wavelet_denoise_u8: no input");
  IDN_CHECK_ARG(out_u8 || out_f32, "idn_wavelet_denoise_u8: no output");
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0, "idn_wavelet_denoise_u8: bad shape");
  IDN_CHECK_ARG((int64_t)h * w < ((int64_t)1 << 31), "idn_wavelet_denoise_u8: image too large");
  IDN_CHECK_ARG(row_stride >= (int64_t)w * 3, "idn_wavelet_denoise_u8: row_stride < w*3");
  IDN_CHECK_ARG(wavelet == IDN_WAVELET_DB1 || wavelet == IDN_WAVELET_BIOR15,
                "idn_wavelet_denoise_u8: unknown wavelet %d", wavelet);
  if (n == 0) return IDN_OK;
  const WlLayout Lt = wl_layout(n, h, w, wavelet, levels);
  IDN_CHECK_ARG(Lt.L >= 1 && Lt.L <= WL_MAXL, "idn_wavelet_denoise_u8: levels %d out of range", Lt.L);
  // pywt needs every level's input at least one sample long; skimage warns but proceeds
  for (int l = 1; l <= Lt.L; ++l)
    IDN_CHECK_ARG(Lt.H[l - 1] >= 1 && Lt.W[l - 1] >= 1, "idn_wavelet_denoise_u8: image too small");
  if (int e = check_workspace_got("idn_wavelet_denoise_u8", workspace, ws_bytes, Lt.bytes,
                                  IDN_EWORKSPACE))
    return e;
  const WlCall C{src, in_f64, ycc_keys, out_u8, out_f32, row_stride, (wreal*)workspace,
                 (double*)((char*)workspace + Lt.stats_off),
                 (double*)((char*)workspace + Lt.part_off), as_stream(stream)};
  if (!wl_haar_ok(wavelet, Lt, src, row_stride)) wl_run(C, Lt, wavelet == IDN_WAVELET_BIOR15);
  else wl_run_haar(C, Lt);
  IDN_CHECK_LAUNCH("idn_wavelet_denoise_u8");
  return IDN_OK;
}
}  // namespace idn

extern "C" int idn_wavelet_denoise_u8(const uint8_t* src, const double* in_f64, uint8_t* out_u8,
                                      float* out_f32, int n, int h, int w, int64_t row_stride,
                                      int wavelet, int levels, void* workspace, size_t ws_bytes,
                                      void* stream) {
  return idn::wavelet_impl(src, in_f64, nullptr, out_u8, out_f32, n, h, w, row_stride, wavelet,
                           levels, workspace, ws_bytes, stream);
}

extern "C" int idn_wavelet_denoise_ycc(const double* in_f64, const uint64_t* ycc_keys,
                                       uint8_t* out_u8, float* out_f32, int n, int h, int w,
                                       int wavelet, int levels, void* workspace, size_t ws_bytes,
                                       void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(in_f64 && ycc_keys, "idn_wavelet_denoise_ycc: null input or keys");
  return wavelet_impl(nullptr, in_f64, reinterpret_cast<const unsigned long long*>(ycc_keys),
                      out_u8, out_f32, n, h, w, (int64_t)w * 3, wavelet, levels, workspace,
                      ws_bytes, stream);
}
