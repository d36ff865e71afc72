// Wavelet denoiser, the general path: every option of skimage 0.14.2's denoise_wavelet that the
// tuned paths (wavelet.hip has their map) do not take -- the wavelets db2, sym4 and coif5 next to
// db1 and bior1.5, method BayesShrink | VisuShrink, mode soft | hard, sigma estimated or given per
// image and channel on the device, convert2ycbcr on or off, one or three channels.  Entered
// through idn_wavelet_denoise_general; no call of the other entry points reaches this unit, and it
// changes no kernel of theirs.  tests/wavelet_general_model.py is the definition.
//
// One launch per level, as the tiled path, but with the filter length at run time: the taps come
// from the __constant__ table of wavelet_taps.inc (tools/gen_wavelet_taps.py, from PyWavelets)
// through LDS, and the tiles are sized by F in dynamic LDS.  The order in which pywt adds an
// output's taps depends on the output's position (wg_tap), so the tap index is a run-time value
// in any form of the kernel; templates on the wavelet would only unroll the loops.
//
// Planes.  The unit of work is one channel plane, p = image * C + channel.  The workspace keeps
// the tiled path's layout -- "pseudo-images" of three planes: plane p is channel p % 3 of
// pseudo-image p / 3 -- so that the shared kernels (wl_init_stats, wl_color_minmax, wl_median) and
// the statistics block apply unchanged.  With C = 3 a pseudo-image is an image.  With C = 1 three
// images share a pseudo-image, so a one-channel batch costs one plane of work per image, not
// three; the last pseudo-image may have one or two planes without an image, which the analysis
// fills with zeros and every later kernel skips.
//
//   colour range  convert2ycbcr only: wl_color_minmax (fp64, exact)
//   analysis      wg_dwt, levels 1..L.  Level 1 loads x / 255 or the float64 value of the plane's
//                 channel (plain), or the normalised Y / Cb / Cr value (convert2ycbcr).  All four
//                 bands keep pywt's operation order -- axis 0 then axis 1, taps in pywt's order,
//                 multiply then add, no FMA -- so the exact zeros of dd_1, and with them the
//                 sigma median, are pywt's.  Every band is stored in fp64: hard thresholding
//                 decides on the fp64 coefficient.
//   sigma         given (sigma_dev, read by wg_thresh) or wl_median over the fp64 dd_1 band
//   thresholds    wg_sumsq (BayesShrink only) and wg_thresh
//   synthesis     wg_synth, levels L..1, details thresholded as they are staged; level 1 fuses
//                 the clip(s), the colour transform and the u8 / f32 stores
#include "wavelet_common.hpp"
#include "abi_args.hpp"

namespace idn {

#include "wavelet_taps.inc"

constexpr int WG_TY = RB_TY, WG_TX = RB_TX;  // analysis tile: output coefficients per band
constexpr int WG_MAXL = 10;                  // thr(2, L-1, 2, L) = 10 + 18 L stays below MN64
constexpr int WG_SO = 32;                    // synthesis tile: output samples per side
constexpr int WG_BAD = 252;                  // stats [252, 255): plane has no finite sigma / range

struct WgCall {
  int C, P;     // channels per image, planes = n * C
  int wavelet;  // idn_wavelet
  int ycc, hard, visu;
  double visu_k;            // sqrt(2 log(h w))
  const double* sigma_dev;  // P doubles or null
};

// LDS doubles of the two kernels (the host sizes the launch with the same expressions)
__host__ __device__ constexpr int wg_nx(int F) { return 2 * WG_TX + F - 2; }   // staged columns
__host__ __device__ constexpr int wg_ny(int F) { return 2 * WG_TY + F - 2; }   // staged rows
__host__ __device__ constexpr int wg_nxp(int F) { return wg_nx(F) | 1; }       // odd row stride
__host__ __device__ constexpr int wg_dwt_lds(int F) {  // taps, input tile, axis-0 low and high
  return 2 * WG_MAXF + wg_ny(F) * wg_nxp(F) + 2 * WG_TY * wg_nxp(F);
}
__host__ __device__ constexpr int wg_scr(int F) { return WG_SO / 2 + F / 2 - 1; }  // staged coefficients per side
__host__ __device__ constexpr int wg_synth_lds(int F) {  // taps, four bands, axis-1 'a' and 'd'
  return 2 * WG_MAXF + 4 * wg_scr(F) * (wg_scr(F) + 1) + 2 * wg_scr(F) * (WG_SO + 1);
}

// tap of step s of the output centred at i on an axis of length n (pywt's
// downsampling_convolution): ascending for i < n; for i >= n the overhanging taps first,
// descending from i - n to 0, then the rest ascending
__device__ __forceinline__ int wg_tap(int s, int over) {
  return over < 0 || s > over ? s : over - s;
}

// ---- analysis -----------------------------------------------------------------------------------
// grid (tiles, pseudo-images * 3), 256 threads: one WG_TY x WG_TX tile of the four bands of one
// plane.  The (2 WG_TY + F - 2) x (2 WG_TX + F - 2) input samples are staged in LDS, axis 0 runs
// into vl / vh, axis 1 from there into the stores (rows of WG_TX consecutive doubles).
__global__ __launch_bounds__(256) void wg_dwt(wreal* __restrict__ ws, size_t img_floats,
                                              const double* __restrict__ stats, WgCall G, int F,
                                              int level, size_t in_off, int Hin, int Win,
                                              size_t out_off, int Ho, int Wo, int tiles_x,
                                              const uint8_t* __restrict__ src,
                                              const double* __restrict__ in64, int64_t row_stride) {
  extern __shared__ double wg_lds[];
  const int NX = wg_nx(F), NY = wg_ny(F), NXP = wg_nxp(F);
  double* flo = wg_lds;
  double* fhi = wg_lds + WG_MAXF;
  double* in = wg_lds + 2 * WG_MAXF;  // [NY][NXP]
  double* vl = in + NY * NXP;         // [WG_TY][NXP]
  double* vh = vl + WG_TY * NXP;
  const int t = threadIdx.x;
  const int p = blockIdx.y, pimg = p / 3, pc = p - pimg * 3;
  const bool live = p < G.P;
  const int img = p / G.C, ch = p - img * G.C;
  wreal* base = ws + (size_t)pimg * img_floats;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int i0 = ti * WG_TY, j0 = tj * WG_TX;
  const int r0 = 2 * i0 + 2 - F, q0 = 2 * j0 + 2 - F;  // input coordinate of staged [0][0]
  if (t < F) {
    flo[t] = WG_TAPS[G.wavelet][0][t];
    fhi[t] = WG_TAPS[G.wavelet][1][t];
  }
  double mn = 0.0, inv = 1.0;
  if (level == 1 && G.ycc) {
    double mx;
    wl_minmax64(stats + (size_t)pimg * WL_STATS, pc, mn, mx);
    inv = mx - mn;
  }
  for (int k = t; k < NY * NX; k += 256) {
    const int rr = k / NX, q = k - rr * NX;
    const int y = sym_idx(r0 + rr, Hin), x = sym_idx(q0 + q, Win);
    double v = 0.0;
    if (!live) {
      // a plane without an image: zeros, so that the median reads defined memory
    } else if (level > 1) {
      v = base[in_off + (size_t)pc * 4 * Hin * Win + (size_t)y * Win + x];
    } else if (G.ycc) {
      double px[3];
      load_rgb64(src, in64, img, Hin, Win, row_stride, y, x, px);
      v = (ycbcr_c(px, ch) - mn) / inv;  // skimage: channel = out - min; channel /= max - min
    } else if (in64) {
      v = in64[(((int64_t)img * Hin + y) * Win + x) * G.C + ch];
    } else {  // img_as_float: x * (1 / 255)
      v = (double)src[((int64_t)img * Hin + y) * row_stride + (int64_t)x * G.C + ch] * (1.0 / 255.0);
    }
    in[rr * NXP + q] = v;
  }
  __syncthreads();
  // axis 0 first (pywt dwtn): output row i0 + ii is centred at input row 2 (i0 + ii) + 1, tap j
  // reads staged row 2 ii + F - 1 - j
  for (int k = t; k < WG_TY * NX; k += 256) {
    const int ii = k / NX, q = k - ii * NX;
    double lo = 0.0, hi = 0.0;
    if (i0 + ii < Ho) {
      const int over = 2 * (i0 + ii) + 1 - Hin;
      for (int s = 0; s < F; ++s) {
        const int j = wg_tap(s, over);
        const double v = in[(2 * ii + F - 1 - j) * NXP + q];
        lo = __dadd_rn(lo, __dmul_rn(flo[j], v));  // pywt: multiply, then add
        hi = __dadd_rn(hi, __dmul_rn(fhi[j], v));
      }
    }
    vl[ii * NXP + q] = lo;
    vh[ii * NXP + q] = hi;
  }
  __syncthreads();
  const size_t bsz = (size_t)Ho * Wo;
  wreal* ob = base + out_off + (size_t)pc * 4 * bsz;
  for (int k = t; k < WG_TY * WG_TX; k += 256) {
    const int ii = k / WG_TX, jj = k - ii * WG_TX;
    const int oi = i0 + ii, oj = j0 + jj;
    if (oi >= Ho || oj >= Wo) continue;
    const int over = 2 * oj + 1 - Win;
    double aa = 0.0, ad = 0.0, da = 0.0, dd = 0.0;
    for (int s = 0; s < F; ++s) {
      const int j = wg_tap(s, over);
      const double lv = vl[ii * NXP + 2 * jj + F - 1 - j], hv = vh[ii * NXP + 2 * jj + F - 1 - j];
      aa = __dadd_rn(aa, __dmul_rn(flo[j], lv));  // key 'aa': axis 0 low, axis 1 low
      ad = __dadd_rn(ad, __dmul_rn(fhi[j], lv));  // key 'ad': axis 0 low, axis 1 high
      da = __dadd_rn(da, __dmul_rn(flo[j], hv));  // key 'da': axis 0 high, axis 1 low
      dd = __dadd_rn(dd, __dmul_rn(fhi[j], hv));
    }
    const size_t e = (size_t)oi * Wo + oj;
    ob[e] = aa;
    ob[bsz + e] = ad;
    ob[2 * bsz + e] = da;
    ob[3 * bsz + e] = dd;
  }
}

// ---- sums of squares (BayesShrink) --------------------------------------------------------------
// block = (plane, level, band): the band's sum of squares in a fixed order
__global__ __launch_bounds__(256) void wg_sumsq(const wreal* __restrict__ ws, size_t img_floats,
                                                double* __restrict__ stats, WlLayout Lt, int P) {
  int u = blockIdx.x;
  const int b = u % 3;
  u /= 3;
  const int l = u % Lt.L;
  const int p = u / Lt.L;
  if (p >= P) return;
  const int pimg = p / 3, pc = p - pimg * 3, lev = l + 1;
  const size_t bsz = (size_t)Lt.H[lev] * Lt.W[lev];
  const wreal* d = ws + (size_t)pimg * img_floats + Lt.off_band[lev] + ((size_t)pc * 4 + 1 + b) * bsz;
  double s = 0.0;
  for (size_t k = threadIdx.x; k < bsz; k += 256) s += d[k] * d[k];
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    stats[(size_t)pimg * WL_STATS + WlStats::sumsq(pc, l, b, Lt.L)] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- thresholds ---------------------------------------------------------------------------------
// one thread per plane: sigma from sigma_dev or from the median, then BayesShrink's threshold per
// band or VisuShrink's one threshold
__global__ void wg_thresh(double* __restrict__ stats, WlLayout Lt, WgCall G) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= G.P) return;
  const int pimg = p / 3, pc = p - pimg * 3;
  double* st = stats + (size_t)pimg * WL_STATS;
  bool bad = false;
  if (G.ycc) {
    double mn, mx;
    wl_minmax64(st, pc, mn, mx);
    if (!(mx > mn)) bad = true;  // 0.14.2 divides by zero: NaN everywhere
  }
  const double sigma = G.sigma_dev ? G.sigma_dev[p] : st[WlStats::median(pc, Lt.L)] / 0.6744897501960817;
  if (!(sigma == sigma)) bad = true;  // no nonzero dd_1: np.median of nothing
  const double var = sigma * sigma;
  for (int l = 0; l < Lt.L; ++l)
    for (int b = 0; b < 3; ++b) {
      double th;
      if (G.visu) {
        th = sigma * G.visu_k;
      } else {
        const double cnt = (double)Lt.H[l + 1] * Lt.W[l + 1];
        const double dvar = st[WlStats::sumsq(pc, l, b, Lt.L)] / cnt;
        th = var / sqrt(fmax(dvar - var, 2.220446049250313e-16));
      }
      st[WlStats::thr(pc, l, b, Lt.L)] = th;
    }
  st[WG_BAD + pc] = bad ? 1.0 : 0.0;
}

// ---- synthesis ----------------------------------------------------------------------------------
// pywt.threshold: soft (wavelet_common.hpp) or hard, d where |d| >= t
__device__ __forceinline__ double wg_shrink(double d, double t, int hard) {
  if (hard) return fabs(d) >= t ? d : 0.0;
  return soft(d, t);
}

// One plane's WG_SO x WG_SO output tile of level `level` from the (WG_SO / 2 + F / 2 - 1)^2
// coefficients of its four bands: staged in LDS with the details thresholded, pywt idwtn's axis-1
// pass ('a' from aa / ad, 'd' from da / dd), then the axis-0 pass; each pass is
// upsampling_convolution_valid_sf's even / odd sums, lowpass sum plus highpass sum.  Thread t
// receives v[2 i + r] = output (2 ((t + 256 i) / WG_SO) + r, (t + 256 i) % WG_SO).
__device__ __forceinline__ void wg_synth_tile(double* lds, int F, int wavelet,
                                              const wreal* __restrict__ A, size_t bsz, int Nh,
                                              int Nw, int m0, int n0, const double (&thr)[3],
                                              int hard, double (&v)[4]) {
  const int HF = F / 2, CR = wg_scr(F), CRP = CR + 1, SP = WG_SO + 1;
  double* rlo = lds;
  double* rhi = lds + WG_MAXF;
  double* co = lds + 2 * WG_MAXF;  // [4][CR][CRP]
  double* sa = co + 4 * CR * CRP;  // [CR][SP]
  double* sd = sa + CR * SP;
  const int t = threadIdx.x;
  if (t < F) {
    rlo[t] = WG_TAPS[wavelet][2][t];
    rhi[t] = WG_TAPS[wavelet][3][t];
  }
  // coefficients past the band's end feed only outputs past the level's valid length, which are
  // never stored: clamped reads keep them finite
  for (int k = t; k < 4 * CR * CR; k += 256) {
    const int b = k / (CR * CR), rc = k - b * CR * CR, r = rc / CR, cc = rc - r * CR;
    const double x = A[(size_t)b * bsz + (size_t)min(m0 + r, Nh - 1) * Nw + min(n0 + cc, Nw - 1)];
    co[(b * CR + r) * CRP + cc] = b > 0 ? wg_shrink(x, thr[b - 1], hard) : x;
  }
  __syncthreads();
  for (int k = t; k < CR * (WG_SO / 2); k += 256) {  // axis 1: column pairs
    const int r = k / (WG_SO / 2), nn = k - r * (WG_SO / 2);
#pragma unroll
    for (int half = 0; half < 2; ++half) {  // 'a' from bands 0, 1; 'd' from bands 2, 3
      const double* cl = co + ((2 * half) * CR + r) * CRP + nn + HF - 1;
      const double* cd = co + ((2 * half + 1) * CR + r) * CRP + nn + HF - 1;
      double le = 0.0, lo = 0.0, he = 0.0, ho = 0.0;
      for (int j = 0; j < HF; ++j) {
        le = __dadd_rn(le, __dmul_rn(rlo[2 * j], cl[-j]));
        lo = __dadd_rn(lo, __dmul_rn(rlo[2 * j + 1], cl[-j]));
        he = __dadd_rn(he, __dmul_rn(rhi[2 * j], cd[-j]));
        ho = __dadd_rn(ho, __dmul_rn(rhi[2 * j + 1], cd[-j]));
      }
      double* o = (half ? sd : sa) + r * SP + 2 * nn;
      o[0] = le + he;
      o[1] = lo + ho;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {  // axis 0: row pairs
    const int k = t + 256 * i, m = k / WG_SO, q = k - m * WG_SO;
    double le = 0.0, lo = 0.0, he = 0.0, ho = 0.0;
    for (int j = 0; j < HF; ++j) {
      const double a = sa[(m + HF - 1 - j) * SP + q], d = sd[(m + HF - 1 - j) * SP + q];
      le = __dadd_rn(le, __dmul_rn(rlo[2 * j], a));
      lo = __dadd_rn(lo, __dmul_rn(rlo[2 * j + 1], a));
      he = __dadd_rn(he, __dmul_rn(rhi[2 * j], d));
      ho = __dadd_rn(ho, __dmul_rn(rhi[2 * j + 1], d));
    }
    v[2 * i] = le + he;
    v[2 * i + 1] = lo + ho;
  }
  __syncthreads();  // the LDS is restaged by the next call
}
static_assert(WG_SO * WG_SO == 4 * 256, "four outputs per thread");
__device__ __forceinline__ int wg_row(int e) { return 2 * ((threadIdx.x + 256 * (e >> 1)) / WG_SO) + (e & 1); }
__device__ __forceinline__ int wg_col(int e) { return (threadIdx.x + 256 * (e >> 1)) % WG_SO; }

// levels L..2: grid (tiles, pseudo-images * 3); the reconstruction goes to the level-(l-1) 'aa'
// slot, cropped to that level's size (the analysis has consumed it)
__global__ __launch_bounds__(256) void wg_synth(wreal* __restrict__ ws, size_t img_floats,
                                                const double* __restrict__ stats, WgCall G, int F,
                                                int level, int L, size_t in_off, int Nh, int Nw,
                                                size_t out_off, int Hout, int Wout, int tiles_x) {
  extern __shared__ double wg_lds[];
  const int p = blockIdx.y, pimg = p / 3, pc = p - pimg * 3;
  if (p >= G.P) return;
  wreal* base = ws + (size_t)pimg * img_floats;
  const size_t bsz = (size_t)Nh * Nw;
  const double* st = stats + (size_t)pimg * WL_STATS;
  const double thr[3] = {st[WlStats::thr(pc, level - 1, 0, L)], st[WlStats::thr(pc, level - 1, 1, L)],
                         st[WlStats::thr(pc, level - 1, 2, L)]};
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int p0 = ti * WG_SO, q0 = tj * WG_SO;
  double v[4];
  wg_synth_tile(wg_lds, F, G.wavelet, base + in_off + (size_t)pc * 4 * bsz, bsz, Nh, Nw, p0 / 2,
                q0 / 2, thr, G.hard, v);
  wreal* out = base + out_off + (size_t)pc * 4 * Hout * Wout;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = p0 + wg_row(e), x = q0 + wg_col(e);
    if (y < Hout && x < Wout) out[(size_t)y * Wout + x] = v[e];
  }
}

// level 1: grid (tiles, pseudo-images); the three planes of the pseudo-image in turn.
//   convert2ycbcr: the planes are Y, Cb, Cr of one image -- inner clip [0, 1], * (max - min) + min,
//                  ycbcr2rgb, outer clip, as wl_synth_final
//   plain:         each plane is a channel of its own image: one clip [0, 1]
// then the u8 cast (uint8)(255 v) and / or the f32 store.  A plane without a finite sigma (or, in
// YCbCr, an image with a constant channel) gives 0, as the tuned paths do.
__global__ __launch_bounds__(256) void wg_synth_final(const wreal* __restrict__ ws, size_t img_floats,
                                                      const double* __restrict__ stats, WgCall G,
                                                      int F, int L, size_t in_off, int Nh, int Nw,
                                                      int h, int w, int tiles_x,
                                                      uint8_t* __restrict__ out_u8, int64_t row_stride,
                                                      float* __restrict__ out_f32) {
  extern __shared__ double wg_lds[];
  const int pimg = blockIdx.y;
  const wreal* base = ws + (size_t)pimg * img_floats + in_off;
  const size_t bsz = (size_t)Nh * Nw;
  const double* st = stats + (size_t)pimg * WL_STATS;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int p0 = ti * WG_SO, q0 = tj * WG_SO;
  double res[3][4];
  for (int pc = 0; pc < 3; ++pc) {
    const int p = pimg * 3 + pc;
    if (p >= G.P) break;  // uniform over the workgroup
    const double thr[3] = {st[WlStats::thr(pc, 0, 0, L)], st[WlStats::thr(pc, 0, 1, L)],
                           st[WlStats::thr(pc, 0, 2, L)]};
    double v[4];
    wg_synth_tile(wg_lds, F, G.wavelet, base + (size_t)pc * 4 * bsz, bsz, Nh, Nw, p0 / 2, q0 / 2,
                  thr, G.hard, v);
    double mn = 0.0, sc = 1.0;
    if (G.ycc) {
      double mx;
      wl_minmax64(st, pc, mn, mx);
      sc = mx - mn;
    }
    const bool bad = st[WG_BAD + pc] != 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double x = fmin(fmax(v[e], 0.0), 1.0);
      if (G.ycc) x = x * sc + mn;
      else if (bad) x = 0.0;
      if (pc == 0) res[0][e] = x;  // (selects: no dynamic register indexing)
      else if (pc == 1) res[1][e] = x;
      else res[2][e] = x;
    }
  }
  const bool bad3 = st[WG_BAD] != 0.0 || st[WG_BAD + 1] != 0.0 || st[WG_BAD + 2] != 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = p0 + wg_row(e), x = q0 + wg_col(e);
    if (y >= h || x >= w) continue;
    if (G.ycc) {
      // ycbcr2rgb as wl_synth_final: numpy.linalg.inv's matrix, fma-chain dot, then clip [0, 1]
      const double Y = res[0][e] - 16.0, Cb = res[1][e] - 128.0, Cr = res[2][e] - 128.0;
      res[0][e] = dot3(Y, Cb, Cr, 0.004566210045662101, 1.1808799897950177e-09, 0.006258928969943937);
      res[1][e] = dot3(Y, Cb, Cr, 0.004566210045662101, -0.0015363236860449021, -0.003188110949655707);
      res[2][e] = dot3(Y, Cb, Cr, 0.004566210045662101, 0.007910716233554741, 1.1977497040511743e-08);
    }
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
      const int p = pimg * 3 + pc;
      if (p >= G.P) break;
      const int img = p / G.C, ch = p - img * G.C;
      double vv = res[pc][e];
      if (G.ycc) {
        vv = fmin(fmax(vv, 0.0), 1.0);
        if (bad3) vv = 0.0;
      }
      if (out_u8)
        out_u8[((int64_t)img * h + y) * row_stride + (int64_t)x * G.C + ch] = (uint8_t)(int)(255.0 * vv);
      if (out_f32) out_f32[(((int64_t)img * h + y) * w + x) * G.C + ch] = (float)vv;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
// the tiled path's layout over pseudo-images of three planes; the input-plane slots (the median's
// scratch) hold a level-1 band, which outgrows the image when the filter is longer than it
struct WgLayout {
  WlLayout Lt;  // n = pseudo-images
  size_t slot;  // elements per input-plane slot
};
static WgLayout wg_layout(int n, int h, int w, int c, int wv, int levels) {
  WgLayout G;
  WlLayout& Lt = G.Lt;
  Lt = WlLayout{};
  Lt.n = (int)(((int64_t)n * c + 2) / 3);
  Lt.h = h;
  Lt.w = w;
  Lt.F = WG_FLEN[wv];
  if (levels <= 0) {
    const int ml = std::min(wl_max_level(h, Lt.F), wl_max_level(w, Lt.F));
    levels = std::max(ml - 3, 1);
  }
  Lt.L = levels;
  Lt.H[0] = h;
  Lt.W[0] = w;
  const int H1 = (h + Lt.F - 1) / 2, W1 = (w + Lt.F - 1) / 2;
  G.slot = std::max((size_t)h * w, (size_t)H1 * W1);
  size_t off = 3 * G.slot;
  for (int l = 1; l <= Lt.L && l <= WG_MAXL; ++l) {
    Lt.H[l] = (Lt.H[l - 1] + Lt.F - 1) / 2;
    Lt.W[l] = (Lt.W[l - 1] + Lt.F - 1) / 2;
    Lt.off_band[l] = off;
    off += (size_t)12 * Lt.H[l] * Lt.W[l];
  }
  Lt.img_floats = align_up(off, 64);
  Lt.stats_off = (size_t)Lt.n * Lt.img_floats * sizeof(wreal);
  Lt.part_per_img = 0;
  Lt.part_off = Lt.stats_off + (size_t)Lt.n * WL_STATS * sizeof(double);
  Lt.bytes = Lt.part_off;
  return G;
}

static void wg_run(const WlCall& C, const WgLayout& WL, const WgCall& G) {
  const WlLayout& Lt = WL.Lt;
  const int F = Lt.F;
  wl_clear_stats(C, Lt);
  if (G.ycc) wl_minmax_exact(C, Lt);
  const size_t dwt_lds = sizeof(double) * wg_dwt_lds(F), syn_lds = sizeof(double) * wg_synth_lds(F);
  for (int l = 1; l <= Lt.L; ++l) {
    const int tx = (Lt.W[l] + WG_TX - 1) / WG_TX, ty = (Lt.H[l] + WG_TY - 1) / WG_TY;
    hipLaunchKernelGGL(wg_dwt, dim3(tx * ty, Lt.n * 3), dim3(256), dwt_lds, C.st, C.ws,
                       Lt.img_floats, C.stats, G, F, l, l == 1 ? (size_t)0 : Lt.off_band[l - 1],
                       Lt.H[l - 1], Lt.W[l - 1], Lt.off_band[l], Lt.H[l], Lt.W[l], tx, C.src,
                       C.in64, C.row_stride);
  }
  if (!G.visu)
    hipLaunchKernelGGL(wg_sumsq, dim3(Lt.n * 3 * Lt.L * 3), dim3(256), 0, C.st, C.ws,
                       Lt.img_floats, C.stats, Lt, G.P);
  if (!G.sigma_dev) {  // the radix select over the fp64 dd_1 band; its scratch is the plane's slot
    WlLayout Lm = Lt;
    Lm.h = (int)WL.slot;
    Lm.w = 1;
    wl_band_median(C, Lm);
  }
  hipLaunchKernelGGL(wg_thresh, dim3((G.P + 63) / 64), dim3(64), 0, C.st, C.stats, Lt, G);
  for (int l = Lt.L; l >= 1; --l) {
    const int Hout = Lt.H[l - 1], Wout = Lt.W[l - 1];
    const int tx = (Wout + WG_SO - 1) / WG_SO, ty = (Hout + WG_SO - 1) / WG_SO;
    if (l >= 2)
      hipLaunchKernelGGL(wg_synth, dim3(tx * ty, Lt.n * 3), dim3(256), syn_lds, C.st, C.ws,
                         Lt.img_floats, C.stats, G, F, l, Lt.L, Lt.off_band[l], Lt.H[l], Lt.W[l],
                         Lt.off_band[l - 1], Hout, Wout, tx);
    else
      hipLaunchKernelGGL(wg_synth_final, dim3(tx * ty, Lt.n), dim3(256), syn_lds, C.st, C.ws,
                         Lt.img_floats, C.stats, G, F, Lt.L, Lt.off_band[1], Lt.H[1], Lt.W[1], Lt.h,
                         Lt.w, tx, C.out_u8, C.row_stride, C.out_f32);
  }
}

static bool wg_shape_ok(int n, int h, int w, int c, int wavelet) {
  return n > 0 && h > 0 && w > 0 && (c == 1 || c == 3) && wavelet >= 0 && wavelet < WG_NWAV &&
         (int64_t)h * w < ((int64_t)1 << 31) && (int64_t)n * c <= 3 * 21845;
}

}  // namespace idn

extern "C" size_t idn_wavelet_general_workspace_size(int n, int h, int w, int c, int wavelet,
                                                     int levels) {
  using namespace idn;
  if (!wg_shape_ok(n, h, w, c, wavelet)) return 0;
  const WgLayout WL = wg_layout(n, h, w, c, wavelet, levels);
  if (WL.Lt.L < 1 || WL.Lt.L > WG_MAXL) return 0;
  return WL.Lt.bytes;
}

extern "C" int idn_wavelet_denoise_general(const uint8_t* src, const double* in_f64, uint8_t* out_u8,
                                           float* out_f32, int n, int h, int w, int c,
                                           int64_t row_stride, int wavelet, int levels, int method,
                                           int mode, int convert2ycbcr, const double* sigma_dev,
                                           void* workspace, size_t ws_bytes, void* stream) {
  using namespace idn;
  const char* fn = "idn_wavelet_denoise_general";
  IDN_CHECK_ARG((src != nullptr) != (in_f64 != nullptr), "%s: exactly one of src / in_f64", fn);
  IDN_CHECK_ARG(out_u8 || out_f32, "%s: no output", fn);
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0, "%s: bad shape", fn);
  IDN_CHECK_ARG(c == 1 || c == 3, "%s: c = %d (1 or 3)", fn, c);
  IDN_CHECK_ARG(wavelet >= 0 && wavelet < WG_NWAV, "%s: unknown wavelet %d", fn, wavelet);
  IDN_CHECK_ARG(method == IDN_WAVELET_BAYES || method == IDN_WAVELET_VISU, "%s: unknown method %d",
                fn, method);
  IDN_CHECK_ARG(mode == IDN_WAVELET_SOFT || mode == IDN_WAVELET_HARD, "%s: unknown mode %d", fn, mode);
  IDN_CHECK_ARG(!(convert2ycbcr && c != 3), "%s: convert2ycbcr needs c = 3", fn);
  IDN_CHECK_ARG((int64_t)h * w < ((int64_t)1 << 31), "%s: image too large", fn);
  IDN_CHECK_ARG((int64_t)n * c <= 3 * 21845, "%s: more than 65535 planes", fn);
  IDN_CHECK_ARG(row_stride >= (int64_t)w * c, "%s: row_stride < w*c", fn);
  if (n == 0) return IDN_OK;
  const WgLayout WL = wg_layout(n, h, w, c, wavelet, levels);
  const WlLayout& Lt = WL.Lt;
  IDN_CHECK_ARG(Lt.L >= 1 && Lt.L <= WG_MAXL, "%s: levels %d out of range (1..%d)", fn, Lt.L, WG_MAXL);
  if (int e = check_workspace_got(fn, workspace, ws_bytes, Lt.bytes, IDN_EWORKSPACE)) return e;
  const WlCall C{src, in_f64, nullptr, out_u8, out_f32, row_stride, (wreal*)workspace,
                 (double*)((char*)workspace + Lt.stats_off), nullptr, as_stream(stream)};
  WgCall G;
  G.C = c;
  G.P = n * c;
  G.wavelet = wavelet;
  G.ycc = convert2ycbcr ? 1 : 0;
  G.hard = mode == IDN_WAVELET_HARD;
  G.visu = method == IDN_WAVELET_VISU;
  G.visu_k = std::sqrt(2.0 * std::log((double)((int64_t)h * w)));
  G.sigma_dev = sigma_dev;
  wg_run(C, WL, G);
  IDN_CHECK_LAUNCH(fn);
  return IDN_OK;
}
