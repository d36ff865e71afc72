// What the units of the wavelet denoiser share (wavelet.hip has the map of the units): the filters
// and constants, the workspace layout and statistics block, the __device__ __forceinline__ helpers
// that more than one unit uses, one call's arguments (WlCall), and at the end the declarations of
// the host functions through which the units call one another.
#pragma once
#include "idn_common.hpp"

#include <cmath>
#include <mutex>
#include <type_traits>

#include <math.h>

#include <algorithm>

#include "ycc.hpp"

namespace idn {

using wreal = double;  // workspace / arithmetic type of the transform
constexpr wreal S2 = 0.7071067811865476;
constexpr wreal B1 = 0.016572815184059706;
constexpr wreal B2 = 0.12153397801643785;

// fused multiply-add in the arithmetic type T (the build has -ffp-contract=off: no implicit fma)
template <typename T>
__device__ __forceinline__ T fma_t(T a, T b, T c) {
  if constexpr (sizeof(T) == 4) return __fmaf_rn(a, b, c);
  else return __fma_rn(a, b, c);
}

template <int WV> struct Wav;
template <> struct Wav<IDN_WAVELET_DB1> {
  static constexpr int F = 2;
  static constexpr wreal dlo[2] = {S2, S2};
  static constexpr wreal dhi[2] = {-S2, S2};
  static constexpr wreal rlo[2] = {S2, S2};
  static constexpr wreal rhi[2] = {S2, -S2};
};
template <> struct Wav<IDN_WAVELET_BIOR15> {
  static constexpr int F = 10;
  static constexpr wreal dlo[10] = {B1, -B1, -B2, B2, S2, S2, B2, -B2, -B1, B1};
  static constexpr wreal dhi[10] = {0, 0, 0, 0, -S2, S2, 0, 0, 0, 0};
  static constexpr wreal rlo[10] = {0, 0, 0, 0, S2, S2, 0, 0, 0, 0};
  static constexpr wreal rhi[10] = {B1, B1, -B2, -B2, S2, -S2, B2, B2, -B1, -B1};
};

inline int wl_filter_len(int wv) { return wv == IDN_WAVELET_DB1 ? 2 : 10; }

// pywt dwt_max_level: floor(log2(n / (F - 1))) with integer division, 0 if n < F - 1
inline int wl_max_level(int n, int F) {
  if (F <= 1 || n < F - 1) return 0;
  int q = n / (F - 1), l = 0;
  while (q > 1) {
    q >>= 1;
    ++l;
  }
  return l;
}

constexpr int WL_MAXL = 12;
constexpr int RB_TY = 8, RB_TX = 32, RB_R = 4;  // analysis tile (wl_dwt_rb)
constexpr int WL_STATS = 256;  // doubles of per-image stats
constexpr int WL_N32U = 156;   // stats [156, 159): u32 counts of the N32 analysis' uncertain codes
constexpr int WLH_WG = 128;  // threads per workgroup (wl_layout sizes the partials for it)

struct WlLayout {
  int n, h, w, F, L;
  int H[WL_MAXL + 1], W[WL_MAXL + 1];  // H[0] = h; H[l] = band height of level l
  size_t off_band[WL_MAXL + 1];        // element offset of level l's 3x4 bands inside an image
  size_t img_floats;                   // wreal elements per image (planes + bands)
  size_t stats_off;                    // byte offset of the stats region (after all images)
  int tiles_x[WL_MAXL + 1], tiles[WL_MAXL + 1];  // DWT tiles per level (partial-sum slots)
  int bands[WL_MAXL + 1];              // bior1.5 streaming analysis: row bands per strip
  double sq_grid[WL_MAXL + 1];         // ... and the grid its sum-of-squares partials round to
  size_t part_tile0[WL_MAXL + 1];      // first tile index of level l in the partials array
  size_t part_per_img;                 // partial sums per image: 3 channels x 3 bands x tiles
  size_t part_off;                     // byte offset of the partial sums region
  size_t bytes;
};

// stats region per image (doubles): [0..6) min/max as u32 pairs, [8..) sumsq[3][L][3],
// [8+9L..) median[3], thr as double[3][L][3] after that, [255] degenerate flag
struct WlStats {
  __host__ __device__ static int sumsq(int c, int l, int b, int L) { return 8 + (c * L + l) * 3 + b; }
  __host__ __device__ static int median(int c, int L) { return 8 + 9 * L + c; }
  __host__ __device__ static int thr(int c, int l, int b, int L) { return 8 + 9 * L + 3 + (c * L + l) * 3 + b; }
  // half thresholds for the integer Haar synthesis (written for L <= 3 only: [170, 197))
  __host__ __device__ static int thrh(int c, int l, int b) { return 170 + (c * 3 + l) * 3 + b; }
  static constexpr int FLAG = 255;
  static constexpr int DIAG = 248;  // [248..251) nonzero count of the finest dd per channel
  static constexpr int MN64 = 200;  // [200..203) fp64 channel min (u64 bits), [203..206) max
  static constexpr int MX64 = 203;
};
constexpr int WL_EBINS = 64;  // exponent bins of |dd|: bin = clamp(exponent - (1023 - 61), 0, 63)
// fine bins of |dd| keys: exponent (clamped as above) and the top 4 mantissa bits, monotone in
// the key; the clamped exponent bins keep one sub-bin
constexpr int WL_FBINS = WL_EBINS * 16;
__device__ __forceinline__ unsigned long long absbits(double v) {
  return (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
}
__device__ __forceinline__ int wl_fbin(unsigned long long key) {
  const int e = (int)(key >> 52) - (1023 - 61);
  if (e < 0) return 0;
  if (e > WL_EBINS - 1) return WL_FBINS - 1;
  return e * 16 + (int)((key >> 48) & 15u);
}

// rows per sum-of-squares group of the streaming analysis: 5, the step loop's unroll, so a group
// ends at the same static position of every unrolled iteration (no per-row test or branch)
constexpr int WS_G = 5;
// Row bands per strip so that the grid fills whole rounds of resident workgroups: for each
// candidate band count b the time is ~ rounds(b) x (rows per band + warm-up rows), rounds(b) =
// ceil(units * b / resident).  (A grid of 2.5 rounds leaves the chip half idle for the last one.)
inline int best_bands(int64_t units, int M, int warm, int64_t resident, int min_rows) {
  const int bmax = std::max(1, std::min(64, M / std::max(min_rows, 1)));
  int best = 1;
  double bestc = 1e300;
  for (int b = 1; b <= bmax; ++b) {
    const double rounds = std::ceil((double)(units * b) / (double)std::max<int64_t>(resident, 1));
    const double c = rounds * ((M + b - 1) / b + warm);
    if (c < bestc * 0.999) {
      bestc = c;
      best = b;
    }
  }
  return best;
}
// resident workgroups per CU of a kernel at a block size (cached; 1 if the query fails)
inline int occ_wgs(const void* kernel, int block) {
  static std::mutex mu;
  static const void* keys[32];
  static int blocks[32], vals[32], nk = 0;
  std::lock_guard<std::mutex> g(mu);
  for (int i = 0; i < nk; ++i)
    if (keys[i] == kernel && blocks[i] == block) return vals[i];
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, 0) != hipSuccess || nb < 1)
    nb = 1;
  if (nk < 32) {
    keys[nk] = kernel;
    blocks[nk] = block;
    vals[nk++] = nb;
  }
  return nb;
}

__device__ __forceinline__ int sym_idx(int i, int n) {  // pywt 'symmetric' (half-sample)
  if ((unsigned)i < (unsigned)n) return i;  // interior: no division
  const int period = 2 * n;
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - 1 - i;
}

__device__ __forceinline__ void ycbcr64(double x0, double x1, double x2, double (&o)[3]) {
  o[0] = __dadd_rn(dot3(x0, x1, x2, 65.481, 128.553, 24.966), 16.0);
  o[1] = __dadd_rn(dot3(x0, x1, x2, -37.797, -74.203, 112.0), 128.0);
  o[2] = __dadd_rn(dot3(x0, x1, x2, 112.0, -93.786, -18.214), 128.0);
}

__device__ __forceinline__ void load_rgb64(const uint8_t* __restrict__ src,
                                           const double* __restrict__ in64, int img, int h, int w,
                                           int64_t row_stride, int y, int x, double (&v)[3]) {
  if (in64) {
    const double* s = in64 + (((int64_t)img * h + y) * w + x) * 3;
    v[0] = s[0];
    v[1] = s[1];
    v[2] = s[2];
  } else {
    const uint8_t* s = src + (int64_t)img * h * row_stride + (int64_t)y * row_stride + (int64_t)x * 3;
    v[0] = (double)s[0] * (1.0 / 255.0);
    v[1] = (double)s[1] * (1.0 / 255.0);
    v[2] = (double)s[2] * (1.0 / 255.0);
  }
}

__device__ __forceinline__ void wl_minmax64(const double* st, int c, double& mn, double& mx) {
  const unsigned long long* u64 = reinterpret_cast<const unsigned long long*>(st);
  mn = dkey_inv(u64[WlStats::MN64 + c]);
  mx = dkey_inv(u64[WlStats::MX64 + c]);
}

// channel c of skimage rgb2ycbcr for one pixel (same fma chain as ycbcr64)
__device__ __forceinline__ double ycbcr_c(const double (&v)[3], int c) {
  if (c == 0) return __dadd_rn(dot3(v[0], v[1], v[2], 65.481, 128.553, 24.966), 16.0);
  if (c == 1) return __dadd_rn(dot3(v[0], v[1], v[2], -37.797, -74.203, 112.0), 128.0);
  return __dadd_rn(dot3(v[0], v[1], v[2], 112.0, -93.786, -18.214), 128.0);
}

// fp32 band storage (IDN_WAVELET_FDET, default on): bands that only the synthesis (or the next
// analysis) reads round-trip through HBM as fp32 (relative 6e-8; the thresholds come from the fp64
// sums of squares taken before the store).  Band mask fmask: bit b (0 aa, 1 ad, 2 da, 3 dd) = band
// b of the level is fp32, bit 4 = the analysis's input 'aa' (level above) is fp32.
//   level 1: ad, da (dd stays fp64 for the sigma median's exact keys), aa when L > 1;
//   levels >= 2: ad, da, dd, aa when l < L (the coarsest 'aa' and the synthesis's reconstructions
//   in the 'aa' slots stay fp64)
constexpr int WL_FB_AIN = 16;
__host__ __device__ __forceinline__ bool wl_fband(int fmask, int b) { return (fmask >> b) & 1; }

__device__ __forceinline__ double uniform_f64(double v) {  // a wave-uniform double into SGPRs
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)b);
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}
__device__ __forceinline__ int ycc_w(int c, int k) {  // rgb2ycbcr coefficients x 1000
  constexpr int W[3][3] = {{65481, 128553, 24966}, {-37797, -74203, 112000}, {112000, -93786, -18214}};
  return W[c][k];
}

// pywt.threshold(d, t, 'soft') = d * max(1 - t/|d|, 0) = sign(d) * max(|d| - t, 0): the same value
// to a few ulps (t >= 0), without the fp64 division per coefficient
__device__ __forceinline__ wreal soft(wreal d, wreal t) {
  const wreal m = fabs(d) - t;
  return m > 0.0 ? __builtin_copysign(m, d) : 0.0;
}

// A knob whose value feeds an expression is read through tuned(): its default, a constant, in
// the product library (idn_common.hpp's knob).
constexpr auto tuned = knob;

// bior1.5 with the code median: the level-1 dd band in fp32 too (the median recomputes its exact
// values from the input, bior_dd2x2; the synthesis reads it as fp32 either way)
inline bool wl_dd32(bool bior, bool codes) {
  return bior && codes && tuned("IDN_WAVELET_FDET", 1) && tuned("IDN_WAVELET_DD32", 1);
}
// band masks (wl_fband) of level l: what the analysis stores, what the synthesis loads
inline int wl_fm_analysis(const WlLayout& Lt, int l, bool dd32) {
  if (!tuned("IDN_WAVELET_FDET", 1)) return 0;
  return (l == 1 ? (dd32 ? 0b1110 : 0b0110) : 0b1110 | WL_FB_AIN) | (l < Lt.L ? 0b0001 : 0);
}
inline int wl_fm_synthesis(int l, bool dd32) {
  return !tuned("IDN_WAVELET_FDET", 1) ? 0 : l == 1 && !dd32 ? 0b0110 : 0b1110;
}

struct WlCall {  // one call's arguments as the entry point received them, the workspace regions
  const uint8_t* src;                  // u8 input, or
  const double* in64;                  // f64 input
  const unsigned long long* ycc_keys;  // nullable: the colour range, already reduced
  uint8_t* out_u8;
  float* out_f32;
  int64_t row_stride;
  wreal* ws;
  double *stats, *part;  // ws + Lt.stats_off, ws + Lt.part_off
  hipStream_t st;
};

// ---- the seams: host functions defined in one unit and called from another ----------------------
// wavelet.hip: the launchers of the kernels every path shares
void wl_clear_stats(const WlCall& C, const WlLayout& Lt);
void wl_minmax_exact(const WlCall& C, const WlLayout& Lt);
void wl_sum_partials(const WlCall& C, const WlLayout& Ls);
void wl_thresholds(const WlCall& C, const WlLayout& Lt);
// wavelet_haar.hip: the fused path (Lt.L = 1, 2, 3), and what wl_run borrows from it -- the u8
// min / max from fp32 proxies, and sigma by the radix select over the level-1 fp64 dd band or by
// the code median over that band's codes (dd32: the band is fp32, the exact keys are recomputed
// from the input)
void wl_run_haar(const WlCall& C, const WlLayout& Lt);
void wl_minmax_proxy(const WlCall& C, const WlLayout& Lt);
void wl_band_median(const WlCall& C, const WlLayout& Lt);
void wl_code_median(const WlCall& C, const WlLayout& Lt, const double* part, bool dd32);
// wavelet_stream.hip: bior1.5, one level per call; the geometry that wl_layout sizes partials by
int ws_strips(int Wo);
int ws_bands(int n, int Ho, int Wo, int strips, int level);
int ws_resident(int level, int block);
void wl_stream_analysis(const WlCall& C, const WlLayout& Lt, int l, bool codes);
void wl_stream_synthesis(const WlCall& C, const WlLayout& Lt, int l, bool codes);
bool wl_stream_synthesis_on(int l);
int wl_stream_fm_synthesis(const WlLayout& Lt, int l, bool codes);
// wavelet_tiled.hip: db1 outside the fused path, one level per call (bior1.5 synthesis: tuning only)
void wl_tiled_analysis(const WlCall& C, const WlLayout& Lt, int l, bool codes);
void wl_tiled_synthesis(const WlCall& C, const WlLayout& Lt, int l, int fmask, int wavelet);

}  // namespace idn
