// Wavelet denoiser, the fused Haar path: db1, L <= 3, sides divisible by 2^L (wavelet.hip has the
// map of the units), with haar3.hpp's single-read form for L = 3 on u8.  Entered through
// wl_run_haar.  The sigma medians of every path are compiled here (wavelet_sigma.hpp), and three
// kernels also serve the per-level paths of wl_run: wl_median (through wl_band_median),
// wl_haar_median<1, true, ..> (through wl_code_median) and the u8 proxy min / max
// wl_h3_stats<true> (through wl_minmax_proxy).
#include "wavelet_common.hpp"
#include "wavelet_sigma.hpp"

namespace idn {

// ---- Haar fast path: every level is local to a 2^L x 2^L block ---------------------------------
// For db1 with h and w divisible by 2^L, pywt's 'symmetric' extension never triggers and level l's
// coefficients of a 2^L x 2^L block depend on that block alone.  So the whole denoiser runs as
//   wl_color_minmax -> wl_haar_analyze -> wl_sumsq -> wl_median -> wl_thresh -> wl_haar_synth
// where wl_haar_analyze reads the image once and writes only the finest dd band (for sigma) and
// per-workgroup sums of squares of every detail band, and wl_haar_synth reads the image again,
// recomputes the analysis of its block, thresholds, synthesises all levels, converts back to
// RGB and stores the U8 / f32 output: no fp64 band ever makes a round trip through HBM except dd1.
// The arithmetic is op for op the general path's (multiply then add, axis 0 then axis 1; the
// synthesis sums A, AD, DA, DD in that order), so the coefficients are bitwise the same.
constexpr int WLH_IT = 4;    // wl_haar_analyze: chunks of WLH_WG sub-blocks per thread

// pywt idwt2 of one coefficient quadruple to output (r, s) of its 2x2 group (details thresholded)
__device__ __forceinline__ wreal ihaar(wreal A, wreal AD, wreal DA, wreal DD, int r, int s) {
  const wreal fd = r ? -S2 : S2, gd = s ? -S2 : S2;
  wreal acc = 0;
  acc = acc + S2 * S2 * A;
  acc = acc + S2 * gd * AD;
  acc = acc + fd * S2 * DA;
  acc = acc + fd * gd * DD;
  return acc;
}

// one row of 4 pixels (x .. x+3) of image img, normalised YCbCr per channel: v[s][c]
__device__ __forceinline__ void haar_row4(const uint8_t* __restrict__ src,
                                          const double* __restrict__ in64, int img, int h, int w,
                                          int64_t row_stride, int y, int x, const wreal (&mn)[3],
                                          const wreal (&inv)[3], wreal (&v)[4][3]) {
  double px[4][3];
  if (in64) {
    const double* p = in64 + (((int64_t)img * h + y) * w + x) * 3;
#pragma unroll
    for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = p[k];
  } else {  // 12 bytes, 4-byte aligned (checked on the host): three dword loads
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (int64_t)img * h * row_stride +
                                                          (int64_t)y * row_stride + (int64_t)x * 3);
    const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
    for (int k = 0; k < 12; ++k)
      px[k / 3][k % 3] = (double)((d[k >> 2] >> (8 * (k & 3))) & 0xFFu) * (1.0 / 255.0);
  }
  // the synthesis is continuous in the coefficients: a reciprocal multiply (<= 1 ulp from the
  // quotient) is enough here; sigma's exact zeros come from wl_haar_analyze's exact quotients
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const wreal rcp = 1.0 / inv[c];
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s][c] = (ycbcr_c(px[s], c) - mn[c]) * rcp;
  }
}

// Work split: one thread per 4x4 sub-block (levels 1 and 2 in registers); for L = 3 the four
// threads of an 8x8 block are consecutive lanes and level 3 runs on their level-2 approximations
// gathered by shuffles (redundantly in all four; only sub-block 0 counts its squares).
template <int L>
struct HaarSplit {
  static constexpr int B = 1 << L;          // block side
  static constexpr int SB = B < 4 ? B : 4;  // sub-block side per thread
  static constexpr int NS = (B / SB) * (B / SB);
  static constexpr int QS = SB / 2;         // level-1 groups per sub-block side
};

// channel c of one row of 4 pixels (x .. x+3), normalised: v[s]
__device__ __forceinline__ void haar_row4_c(const uint8_t* __restrict__ src,
                                            const double* __restrict__ in64, int img, int h, int w,
                                            int64_t row_stride, int y, int x, int c, wreal mn,
                                            wreal inv, wreal (&v)[4]) {
  double px[4][3];
  if (in64) {
    const double* p = in64 + (((int64_t)img * h + y) * w + x) * 3;
#pragma unroll
    for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = p[k];
  } else {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (int64_t)img * h * row_stride +
                                                          (int64_t)y * row_stride + (int64_t)x * 3);
    const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
    for (int k = 0; k < 12; ++k)
      px[k / 3][k % 3] = (double)((d[k >> 2] >> (8 * (k & 3))) & 0xFFu) * (1.0 / 255.0);
  }
  // (Y - min) / (max - min) correctly rounded without a division per value: q0 = a * (1/b),
  // q1 = q0 + (a - q0 b)(1/b) with exact fma residuals (Markstein) -- bitwise the IEEE quotient
  // (also checked over every u8 triple for 24 channel ranges: tools/check_div.c)
  const wreal rcp = 1.0 / inv;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const wreal a = ycbcr_c(px[s], c) - mn;
    const wreal q0 = a * rcp;
    v[s] = __fma_rn(__fma_rn(-q0, inv, a), rcp, q0);
  }
}

// level 1 of channel c of one thread's 4x4 sub-block (L >= 2)
__device__ __forceinline__ void haar_sub4_c(const uint8_t* __restrict__ src,
                                            const double* __restrict__ in64, int img, int h, int w,
                                            int64_t row_stride, int y0, int x0, int c, wreal mn,
                                            wreal inv, wreal (&a1)[4], wreal (&d1)[3][4]) {
#pragma unroll
  for (int qy = 0; qy < 2; ++qy) {
    wreal r0[4], r1[4];
    haar_row4_c(src, in64, img, h, w, row_stride, y0 + 2 * qy, x0, c, mn, inv, r0);
    haar_row4_c(src, in64, img, h, w, row_stride, y0 + 2 * qy + 1, x0, c, mn, inv, r1);
#pragma unroll
    for (int qx = 0; qx < 2; ++qx) {
      const int k = qy * 2 + qx;
      haar2x2(r0[2 * qx], r0[2 * qx + 1], r1[2 * qx], r1[2 * qx + 1], a1[k], d1[0][k], d1[1][k],
              d1[2][k]);
    }
  }
}

// level 1 of one thread's sub-block, all channels: a1[c][k] approximations, d1[c][band][k] details
template <int L>
__device__ __forceinline__ void haar_sub_analysis(
    const uint8_t* __restrict__ src, const double* __restrict__ in64, int img, int h, int w,
    int64_t row_stride, int y0, int x0, const wreal (&mn)[3], const wreal (&inv)[3],
    wreal (&a1)[3][HaarSplit<L>::QS * HaarSplit<L>::QS],
    wreal (&d1)[3][3][HaarSplit<L>::QS * HaarSplit<L>::QS]) {
  using HS = HaarSplit<L>;
#pragma unroll
  for (int qy = 0; qy < HS::QS; ++qy) {
    wreal r0[4][3], r1[4][3];
    if constexpr (HS::SB == 4) {
      haar_row4(src, in64, img, h, w, row_stride, y0 + 2 * qy, x0, mn, inv, r0);
      haar_row4(src, in64, img, h, w, row_stride, y0 + 2 * qy + 1, x0, mn, inv, r1);
    } else {  // 2x2 sub-block (L = 1): two pixels per row
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        double p0[3], p1[3];
        load_rgb64(src, in64, img, h, w, row_stride, y0 + 2 * qy, x0 + s, p0);
        load_rgb64(src, in64, img, h, w, row_stride, y0 + 2 * qy + 1, x0 + s, p1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          r0[s][c] = (ycbcr_c(p0, c) - mn[c]) / inv[c];
          r1[s][c] = (ycbcr_c(p1, c) - mn[c]) / inv[c];
        }
      }
    }
#pragma unroll
    for (int qx = 0; qx < HS::QS; ++qx)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = qy * HS::QS + qx;
        haar2x2(r0[2 * qx][c], r0[2 * qx + 1][c], r1[2 * qx][c], r1[2 * qx + 1][c], a1[c][k],
                d1[c][0][k], d1[c][1][k], d1[c][2][k]);
      }
  }
}

template <int L>
__global__ __launch_bounds__(WLH_WG) void wl_haar_analyze(
    const uint8_t* __restrict__ src, const double* __restrict__ in64, int h, int w,
    int64_t row_stride, wreal* __restrict__ ws, size_t img_floats, size_t dd_off,
    const double* __restrict__ stats, double* __restrict__ part, size_t part_per_img) {
  using HS = HaarSplit<L>;
  constexpr int B = HS::B, QS = HS::QS;
  const int img = blockIdx.y;
  const int nbx = w / B, nblk = nbx * (h / B);
  const double* st = stats + (size_t)img * WL_STATS;
  __shared__ double red[3 * L * 3][WLH_WG / 64];
  const size_t W1 = (size_t)(w / 2), bsz = (size_t)(h / 2) * W1;
  // one channel at a time (keeps the live state to one channel's coefficients and sums)
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    wreal mn, mx;
    wl_minmax64(st, c, mn, mx);
    const wreal inv = mx - mn;
    double sq[L][3];
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
      for (int b = 0; b < 3; ++b) sq[l][b] = 0.0;
    // WLH_IT chunks of WLH_WG sub-blocks per thread, summed in registers before the one wave
    // reduction per channel (the reductions, not the arithmetic, dominated at one chunk)
#pragma unroll 1
    for (int it = 0; it < WLH_IT; ++it) {
      const int tid = (blockIdx.x * WLH_IT + it) * WLH_WG + threadIdx.x;
      const int blk = tid / HS::NS, sub = tid % HS::NS;
      const bool act = blk < nblk;  // uniform over each block's NS consecutive lanes
      int y0 = 0, x0 = 0;
      if (act) {
        const int by = blk / nbx, bx = blk - by * nbx;
        const int sy = sub / (B / HS::SB), sx = sub % (B / HS::SB);
        y0 = by * B + sy * HS::SB;
        x0 = bx * B + sx * HS::SB;
      }
      wreal a2 = 0;
      if (act) {
        wreal a1[QS * QS], d1[3][QS * QS];
        if constexpr (QS == 2) {
          haar_sub4_c(src, in64, img, h, w, row_stride, y0, x0, c, mn, inv, a1, d1);
        } else {  // L = 1: a 2x2 block per thread
          wreal r[2][2];
#pragma unroll
          for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
              double px[3];
              load_rgb64(src, in64, img, h, w, row_stride, y0 + rr, x0 + ss, px);
              r[rr][ss] = (ycbcr_c(px, c) - mn) / inv;
            }
          haar2x2(r[0][0], r[0][1], r[1][0], r[1][1], a1[0], d1[0][0], d1[1][0], d1[2][0]);
        }
        // the finest dd is kept only as its fine-bin code (0: exact zero, else wl_fbin + 1): the
        // sigma median recomputes the exact values of the one or two bins it needs
        uint16_t* cdp = reinterpret_cast<uint16_t*>(ws + img * img_floats + dd_off +
                                                    (size_t)c * 4 * bsz + 3 * bsz);
#pragma unroll
        for (int k = 0; k < QS * QS; ++k) {
#pragma unroll
          for (int b = 0; b < 3; ++b) sq[0][b] += d1[b][k] * d1[b][k];
          const unsigned long long key = absbits(d1[2][k]);
          cdp[(size_t)(y0 / 2 + k / QS) * W1 + x0 / 2 + k % QS] =
              (uint16_t)(key ? wl_fbin(key) + 1 : 0);
        }
        if constexpr (L >= 2) {  // level 2 on the thread's 2x2 level-1 approximations
          wreal ad, da, dd;
          haar2x2(a1[0], a1[1], a1[2], a1[3], a2, ad, da, dd);
          sq[1][0] += ad * ad;
          sq[1][1] += da * da;
          sq[1][2] += dd * dd;
        }
      }
      if constexpr (L == 3) {  // level 3 across the block's 4 lanes (all lanes take part)
        const int base = (threadIdx.x & 63) & ~3;
        const wreal x00 = __shfl(a2, base), x01 = __shfl(a2, base + 1);
        const wreal x10 = __shfl(a2, base + 2), x11 = __shfl(a2, base + 3);
        wreal aa, ad, da, dd;
        haar2x2(x00, x01, x10, x11, aa, ad, da, dd);
        if (act && sub == 0) {
          sq[2][0] += ad * ad;
          sq[2][1] += da * da;
          sq[2][2] += dd * dd;
        }
      }
    }
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double v = sq[l][b];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[(c * L + l) * 3 + b][threadIdx.x >> 6] = v;
      }
  }
  __syncthreads();
  // workgroup sums of squares in a fixed order (wave shuffles, then the two waves)
  if (threadIdx.x < 3 * L * 3) {
    const int k = threadIdx.x, b = k % 3, l = (k / 3) % L, c = k / (3 * L);
    double t = red[k][0];
#pragma unroll
    for (int wv = 1; wv < WLH_WG / 64; ++wv) t += red[k][wv];
    part[img * part_per_img + (size_t)(c * 3 + b) * (part_per_img / 9) + (size_t)l * gridDim.x +
         blockIdx.x] = t;
  }
}

template <int L>
__global__ __launch_bounds__(WLH_WG) __attribute__((amdgpu_waves_per_eu(3))) void wl_haar_synth(
    const uint8_t* __restrict__ src, const double* __restrict__ in64, int h, int w,
    int64_t row_stride, const double* __restrict__ stats, uint8_t* __restrict__ out_u8,
    float* __restrict__ out_f32) {
  using HS = HaarSplit<L>;
  constexpr int B = HS::B, QS = HS::QS;
  const int img = blockIdx.y;
  const int nbx = w / B, nblk = nbx * (h / B);
  const int tid = blockIdx.x * WLH_WG + threadIdx.x;
  const int blk = tid / HS::NS, sub = tid % HS::NS;
  const bool act = blk < nblk;
  const double* st = stats + (size_t)img * WL_STATS;
  const bool bad = st[WlStats::FLAG] != 0.0;
  wreal mn[3], inv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    wreal mx;
    wl_minmax64(st, c, mn[c], mx);
    inv[c] = mx - mn[c];
  }
  auto thr = [&](int c, int l, int b) { return st[WlStats::thr(c, l, b, L)]; };
  int y0 = 0, x0 = 0;
  if (act) {
    const int by = blk / nbx, bx = blk - by * nbx;
    const int sy = sub / (B / HS::SB), sx = sub % (B / HS::SB);
    y0 = by * B + sy * HS::SB;
    x0 = bx * B + sx * HS::SB;
  }
  wreal a1[3][QS * QS], d1[3][3][QS * QS];
  if (act) haar_sub_analysis<L>(src, in64, img, h, w, row_stride, y0, x0, mn, inv, a1, d1);
  if constexpr (L >= 2) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wreal a2 = 0, ad2 = 0, da2 = 0, dd2 = 0;
      if (act) haar2x2(a1[c][0], a1[c][1], a1[c][2], a1[c][3], a2, ad2, da2, dd2);
      if constexpr (L == 3) {  // level 3 across the block's 4 lanes, synthesised back to a2
        const int base = (threadIdx.x & 63) & ~3;
        const wreal x00 = __shfl(a2, base), x01 = __shfl(a2, base + 1);
        const wreal x10 = __shfl(a2, base + 2), x11 = __shfl(a2, base + 3);
        wreal aa, ad, da, dd;
        haar2x2(x00, x01, x10, x11, aa, ad, da, dd);
        a2 = ihaar(aa, soft(ad, thr(c, 2, 0)), soft(da, thr(c, 2, 1)), soft(dd, thr(c, 2, 2)),
                   sub >> 1, sub & 1);
      }
      const wreal AD = soft(ad2, thr(c, 1, 0)), DA = soft(da2, thr(c, 1, 1));
      const wreal DD = soft(dd2, thr(c, 1, 2));
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < 2; ++s) a1[c][r * 2 + s] = ihaar(a2, AD, DA, DD, r, s);
    }
  }
  if (!act) return;
  // level 1 per 2x2 group with the pixels' own details, colour, casts.  A 4x4 sub-block's rows
  // are 12 contiguous bytes: packed and stored as three dwords per row (single-byte stores made
  // 14x the L2 write requests of the output bytes)
  const bool dw =
      QS == 2 && out_u8 && ((reinterpret_cast<uintptr_t>(out_u8) | (uintptr_t)row_stride) & 3) == 0;
  uint32_t rowp[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
#pragma unroll
  for (int k = 0; k < QS * QS; ++k) {
    const int qy = k / QS, qx = k % QS;
    if (qx == 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) rowp[r][j] = 0u;
    }
    wreal A[3], AD[3], DA[3], DD[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      A[c] = a1[c][k];
      AD[c] = soft(d1[c][0][k], thr(c, 0, 0));
      DA[c] = soft(d1[c][1][k], thr(c, 0, 1));
      DD[c] = soft(d1[c][2][k], thr(c, 0, 2));
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        // one pixel at a time (three channels live): inner denoise_wavelet clip (0.14.2), then
        // * (max - min) + min, YCbCr -> RGB, clip, cast
        wreal o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double vv = fmin(fmax((double)ihaar(A[c], AD[c], DA[c], DD[c], r, s), 0.0), 1.0);
          o[c] = vv * inv[c] + mn[c];
        }
        const double Y = o[0] - 16.0, Cb = o[1] - 128.0, Cr = o[2] - 128.0;
        double o3[3];
        o3[0] = dot3(Y, Cb, Cr, 0.004566210045662101, 1.1808799897950177e-09, 0.006258928969943937);
        o3[1] = dot3(Y, Cb, Cr, 0.004566210045662101, -0.0015363236860449021, -0.003188110949655707);
        o3[2] = dot3(Y, Cb, Cr, 0.004566210045662101, 0.007910716233554741, 1.1977497040511743e-08);
        const int y = y0 + 2 * qy + r, x = x0 + 2 * qx + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double vv = fmin(fmax(o3[c], 0.0), 1.0);
          if (bad) vv = 0.0;
          const uint32_t u = (uint32_t)(int)(255.0 * vv);
          if (dw) {
            const int bi = (2 * qx + s) * 3 + c;
            rowp[r][bi >> 2] |= u << (8 * (bi & 3));
          } else if (out_u8) {
            out_u8[(int64_t)img * h * row_stride + (int64_t)y * row_stride + (int64_t)x * 3 + c] =
                (uint8_t)u;
          }
          if (out_f32) out_f32[(((int64_t)img * h + y) * w + x) * 3 + c] = (float)vv;
        }
      }
    if (dw && qx == QS - 1) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        uint32_t* p = reinterpret_cast<uint32_t*>(out_u8 + (int64_t)img * h * row_stride +
                                                  (int64_t)(y0 + 2 * qy + r) * row_stride +
                                                  (int64_t)x0 * 3);
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = rowp[r][j];
      }
    }
  }
}

// ---- Haar statistics for u8 input (L >= 2): integer moments instead of fp64 planes ---------------
// BayesShrink needs per (channel, level, band) the sum of squared detail coefficients, and the
// sigma median the fine-bin codes of the finest dd.  For u8 input every Haar detail is an integer
// combination of the pixels times a constant (the channel offsets and the minimum cancel in the
// +-1 combinations):
//     d(c, l) = 2^-l (w_c . D) / (255000 (max_c - min_c)),   w_c = rgb2ycbcr row c x 1000
// with D the integer RGB vector of the band's combination.  So the sums follow from exact integer
// second moments of D (six per band), summed in int32 per thread and in fp64 after that -- a
// rounding-level difference from pywt's own fp64 sums, like any other summation order -- and the
// dd codes from T = w_c . D_dd, ~25 integer / fp64 ops per pixel where wl_haar_analyze recomputes
// the normalised fp64 planes (~100).
// The codes must equal those of the reference's fp64 dd (the median recomputes exact values per
// code).  Its deviation from the exact value 0.5 T / (255000 inv) is below 1e-12 / inv (rounded
// 1/255, YCbCr dot, offset, difference and quotient, each <= 2.8e-14 absolute at magnitude <= 256,
// then the 2x2 combination), so |dd_ref - a| <= 2e-12 / inv for the fp64 approximation a, i.e.
// a relative 1.02e-6 / |T| <= 3.4e-7 for |T| >= 3.  When the mantissa bits below the code's four
// are >= 2^33 away from both ends, a is >= 2^-19 (relative) from every bin edge, so the code is
// certain.  Everything else -- T == 0 (an exact zero or a rounding residue), |T| < 3, values next
// to an edge -- is evaluated exactly (wl_dd1_key, the median's own evaluation).  Groups whose
// pixel pairs are equal RGB triples (rows or columns) have dd exactly 0 in the reference (x - x)
// and need no evaluation; the rest are queued in LDS and evaluated densely by the whole workgroup
// between iterations (heavily clipped noise makes ~6 % of the codes uncertain: evaluated inline,
// every wave would pay for them).
// Channels whose range is only rounding noise (Cb / Cr of a gray image, range ~1e-14) get sums
// that differ from the fp64 planes' (which are noise themselves); their thresholds cannot move the
// output, which is min + v * range for such a channel.
constexpr int WLS_IT = 16;  // sub-blocks per thread (int32 moments stay below 2^31: <= 1.07e9)
constexpr int WLS_XMAX = WLH_WG * 12;  // uncertain codes one iteration can queue (12 per thread)
constexpr int WLS_XCAP = 2 * WLS_XMAX;  // the queue is evaluated once more than half full
__device__ __forceinline__ void haar_int(int x00, int x01, int x10, int x11, int& aa, int& ad,
                                         int& da, int& dd) {
  const int lo0 = x00 + x10, lo1 = x01 + x11, hi0 = x00 - x10, hi1 = x01 - x11;
  aa = lo0 + lo1;
  ad = lo0 - lo1;
  da = hi0 + hi1;
  dd = hi0 - hi1;
}
__device__ __forceinline__ void mom_add(int (&m)[6], int r, int g, int b) {
  m[0] += __mul24(r, r);
  m[1] += __mul24(g, g);
  m[2] += __mul24(b, b);
  m[3] += __mul24(r, g);
  m[4] += __mul24(r, b);
  m[5] += __mul24(g, b);
}

template <int L>
__global__ __launch_bounds__(WLH_WG) void wl_haar_stats(
    const uint8_t* __restrict__ src, int h, int w, int64_t row_stride, wreal* __restrict__ ws,
    size_t img_floats, size_t dd_off, const double* __restrict__ stats, double* __restrict__ part,
    size_t part_per_img) {
  static_assert(L == 2 || L == 3, "4x4 sub-blocks per thread");
  using HS = HaarSplit<L>;
  constexpr int B = HS::B;
  const int img = blockIdx.y;
  const int nbx = w / B, nblk = nbx * (h / B);
  const double* st = stats + (size_t)img * WL_STATS;
  __shared__ double red[3 * L * 3][WLH_WG / 64];
  __shared__ uint32_t xq[WLS_XCAP];  // queued uncertain codes: position * 4 + channel
  __shared__ uint32_t xq_n;
  // levels 2..L moments in LDS, one private column per thread ([k][thread]: consecutive lanes on
  // consecutive banks, ds_add_u32 without conflicts): 36 fewer VGPRs than register accumulators,
  // which with the one-ahead prefetch brings the kernel from 2 to 3 waves per SIMD
  // (level 3: one column per 8x8 block, written by its sub-block-0 lane only)
  __shared__ int ml2[3 * 6][WLH_WG];
  __shared__ int ml3[L == 3 ? 3 * 6 : 1][WLH_WG / 4];
#pragma unroll
  for (int k = 0; k < 3 * 6; ++k) ml2[k][threadIdx.x] = 0;
  if (L == 3 && threadIdx.x < WLH_WG / 4)
#pragma unroll
    for (int k = 0; k < 3 * 6; ++k) ml3[k][threadIdx.x] = 0;
  if (threadIdx.x == 0) xq_n = 0u;
  __syncthreads();
  const size_t W1 = (size_t)(w / 2), bsz = (size_t)(h / 2) * W1;
  // per-channel scales, uniform: kept in SGPRs (min / range / reciprocal are re-read by the rare
  // exact path only) -- the moments already hold 54 VGPRs
  wreal sc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    wreal mn, mx;
    wl_minmax64(st, c, mn, mx);
    sc[c] = uniform_f64(0.5 / (255000.0 * (mx - mn)));
  }
  int mom[3][6];  // level 1 (levels >= 2: mlds)
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int k = 0; k < 6; ++k) mom[b][k] = 0;
  auto mom_lds = [&](int l, int b, int r, int g, int bl) {  // level l >= 1 (0-based)
    const int ld = l == 1 ? WLH_WG : WLH_WG / 4;  // row pitch of the level's array
    int* m = l == 1 ? &ml2[b * 6][threadIdx.x] : &ml3[(L == 3 ? b : 0) * 6][threadIdx.x >> 2];
    atomicAdd(m + 0 * ld, __mul24(r, r));
    atomicAdd(m + 1 * ld, __mul24(g, g));
    atomicAdd(m + 2 * ld, __mul24(bl, bl));
    atomicAdd(m + 3 * ld, __mul24(r, g));
    atomicAdd(m + 4 * ld, __mul24(r, bl));
    atomicAdd(m + 5 * ld, __mul24(g, bl));
  };
  const uint8_t* ib = src + (int64_t)img * h * row_stride;
  uint16_t* cdp0 = reinterpret_cast<uint16_t*>(ws + img * img_floats + dd_off + 3 * bsz);
  // sub-block geometry of iteration `it`; its 4 rows x 12 bytes (dword aligned: checked on the
  // host) are loaded one iteration ahead
  auto geom = [&](int it, int& sub, int& y0, int& x0) -> bool {
    const int tid = (blockIdx.x * WLS_IT + it) * WLH_WG + threadIdx.x;
    const int blk = tid / HS::NS;
    sub = tid % HS::NS;
    const int by = blk / nbx, bx = blk - by * nbx;
    y0 = by * B + (sub >> 1) * 4;
    x0 = bx * B + (sub & 1) * 4;
    return blk < nblk;  // uniform over each block's NS consecutive lanes
  };
  auto load_q = [&](int it, uint32_t (&qq)[4][3]) {
    int sub, y0, x0;
    if (!geom(it, sub, y0, x0)) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(ib + (int64_t)(y0 + r) * row_stride +
                                                            (int64_t)x0 * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) qq[r][k] = p[k];
    }
  };
  uint32_t qn[4][3] = {};
  load_q(0, qn);
#pragma unroll 1
  for (int it = 0; it < WLS_IT; ++it) {
    int sub, y0, x0;
    const bool act = geom(it, sub, y0, x0);
    uint32_t q[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) q[r][k] = qn[r][k];
    if (it + 1 < WLS_IT) load_q(it + 1, qn);
    int a2[3] = {0, 0, 0};
    if (act) {
      auto px = [&](int r, int k) { return (int)((q[r][k >> 2] >> (8 * (k & 3))) & 0xFFu); };
      int a1[4][3];
#pragma unroll
      for (int gy = 0; gy < 2; ++gy)
#pragma unroll
        for (int gx = 0; gx < 2; ++gx) {
          int D[3][3];  // band (ad, da, dd) x rgb
#pragma unroll
          for (int ch = 0; ch < 3; ++ch)
            haar_int(px(2 * gy, 6 * gx + ch), px(2 * gy, 6 * gx + 3 + ch),
                     px(2 * gy + 1, 6 * gx + ch), px(2 * gy + 1, 6 * gx + 3 + ch),
                     a1[gy * 2 + gx][ch], D[0][ch], D[1][ch], D[2][ch]);
#pragma unroll
          for (int b = 0; b < 3; ++b) mom_add(mom[b], D[b][0], D[b][1], D[b][2]);
          const size_t cpos = (size_t)(y0 / 2 + gy) * W1 + (size_t)(x0 / 2 + gx);
          uint32_t code[3], unsure = 0u;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int T = __mul24(ycc_w(c, 0), D[2][0]) + __mul24(ycc_w(c, 1), D[2][1]) +
                          __mul24(ycc_w(c, 2), D[2][2]);
            const uint32_t aT = (uint32_t)(T < 0 ? -T : T);
            const uint32_t hi = (uint32_t)__double2hiint((double)aT * sc[c]);
            code[c] = (uint32_t)min(max((int)(hi >> 16) - (1023 - 61) * 16, 0), WL_FBINS - 1) + 1u;
            if (!(aT >= 3u && (hi & 0xFFFFu) - 2u <= 0xFFFBu)) unsure |= 1u << c;
          }
          if (unsure) {
            // equal RGB triples along rows or columns: the reference's dd is x - x = 0 exactly
            auto trip = [&](int r, int k) { return px(r, k) | (px(r, k + 1) << 8) | (px(r, k + 2) << 16); };
            const int t00 = trip(2 * gy, 6 * gx), t01 = trip(2 * gy, 6 * gx + 3);
            const int t10 = trip(2 * gy + 1, 6 * gx), t11 = trip(2 * gy + 1, 6 * gx + 3);
            if ((t00 == t01 && t10 == t11) || (t00 == t10 && t01 == t11)) {
#pragma unroll
              for (int c = 0; c < 3; ++c)
                if ((unsure >> c) & 1u) code[c] = 0u;
              unsure = 0u;
            }
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if ((unsure >> c) & 1u)  // queued: evaluated exactly below (at most 12 per thread)
              xq[atomicAdd(&xq_n, 1u)] = (uint32_t)cpos * 4u + (uint32_t)c;
            else
              cdp0[(size_t)c * 4 * bsz * (sizeof(wreal) / sizeof(uint16_t)) + cpos] = (uint16_t)code[c];
          }
        }
      int D2[3][3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        haar_int(a1[0][ch], a1[1][ch], a1[2][ch], a1[3][ch], a2[ch], D2[0][ch], D2[1][ch],
                 D2[2][ch]);
#pragma unroll
      for (int b = 0; b < 3; ++b) mom_lds(1, b, D2[b][0], D2[b][1], D2[b][2]);
    }
    if constexpr (L == 3) {  // level 3 across the block's 4 lanes (all lanes take part)
      const int base = (threadIdx.x & 63) & ~3;
      int D3[3][3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        int aa;
        haar_int(__shfl(a2[ch], base), __shfl(a2[ch], base + 1), __shfl(a2[ch], base + 2),
                 __shfl(a2[ch], base + 3), aa, D3[0][ch], D3[1][ch], D3[2][ch]);
      }
      if (act && sub == 0)
#pragma unroll
        for (int b = 0; b < 3; ++b) mom_lds(2, b, D3[b][0], D3[b][1], D3[b][2]);
    }
    // the queued uncertain codes, densely over the workgroup, once the queue could overflow in
    // the next iteration (and after the last one)
    __syncthreads();
    const uint32_t nq = xq_n;  // workgroup-uniform
    if (nq > (uint32_t)(WLS_XCAP - WLS_XMAX) || (it == WLS_IT - 1 && nq)) {
      for (uint32_t i = threadIdx.x; i < nq; i += WLH_WG) {
        const uint32_t e = xq[i], pos = e >> 2;
        const int c = (int)(e & 3u);
        wreal mnc, mxc;
        wl_minmax64(st, c, mnc, mxc);
        const wreal invc = mxc - mnc;
        const unsigned long long key = wl_dd1_key<true>(src, nullptr, img, h, w, row_stride, pos,
                                                        (int)W1, c, mnc, invc, 1.0 / invc);
        cdp0[(size_t)c * 4 * bsz * (sizeof(wreal) / sizeof(uint16_t)) + pos] =
            (uint16_t)(key ? (uint32_t)wl_fbin(key) + 1u : 0u);
      }
      __syncthreads();
      if (threadIdx.x == 0) xq_n = 0u;
      __syncthreads();
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double w0 = ycc_w(c, 0), w1 = ycc_w(c, 1), w2 = ycc_w(c, 2);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const double s = ldexp(sc[c], -l);  // 2^-(l+1) / (255000 inv)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        int m[6];
#pragma unroll
        for (int k = 0; k < 6; ++k)
          m[k] = l == 0 ? mom[b][k]
                 : l == 1 ? ml2[b * 6 + k][threadIdx.x]
                          : ((threadIdx.x & 3) == 0 ? ml3[(L == 3 ? b : 0) * 6 + k][threadIdx.x >> 2] : 0);
        double v = w0 * w0 * (double)m[0] + w1 * w1 * (double)m[1] + w2 * w2 * (double)m[2] +
                   2.0 * (w0 * w1 * (double)m[3] + w0 * w2 * (double)m[4] + w1 * w2 * (double)m[5]);
        v *= s * s;
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[(c * L + l) * 3 + b][wave] = v;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * L * 3) {
    const int k = threadIdx.x, b = k % 3, l = (k / 3) % L, c = k / (3 * L);
    double t = red[k][0];
#pragma unroll
    for (int wv = 1; wv < WLH_WG / 64; ++wv) t += red[k][wv];
    part[img * part_per_img + (size_t)(c * 3 + b) * (part_per_img / 9) + (size_t)l * gridDim.x +
         blockIdx.x] = t;
  }
}

// ---- Haar synthesis for u8 input (L >= 2) from the integer combinations -------------------------
// The same algebra as wl_haar_stats: with s1 = 0.5 / (255000 inv) and k = 2 (off - min) / inv,
//     level-l detail  d_l = 2^-(l-1) s1 (w_c . D_l),     level-L approximation
//     a_L = 2^-(L-1) s1 (w_c . S_L) + 2^(L-1) k          (S_L: the integer RGB sum of the block)
// so no normalised plane is evaluated: per coefficient three 24-bit integer multiply-adds, one
// conversion and one multiply.  pywt's idwt2 of one 2x2 group is 0.5 (A +- AD +- DA +- DD) in
// its four outputs; the 0.5 is folded into the coefficients and the soft thresholds (a power of
// two commutes with soft()) and the four outputs come from a butterfly: 8 adds per group and
// channel where ihaar takes 4 multiplies + 4 adds per output.  De-normalisation, YCbCr -> RGB and
// the x255 cast fold into three fma chains per pixel.  Every coefficient agrees with the fp64
// planes' to a few ulps (the error analysis of wl_haar_stats), so outputs agree to ~1e-15 and
// the U8 cast can differ only where 255 x sits on an integer (the documented tolerance).
__device__ __forceinline__ double tdot_sum(int c, const int (&v)[3]) {
  // w_c . S for the non-negative block sums: Y's weights are all positive and its dot reaches
  // 3.6e9 at level 3, past int32: two exact signed parts (<= 2.1e9 each) added in fp64 (an
  // unsigned sum was converted as signed by the compiler).  Cb / Cr stay within +-1.9e9
  if (c == 0)
    return (double)(__mul24(65481, v[0]) + __mul24(24966, v[2])) + (double)__mul24(128553, v[1]);
  return (double)(__mul24(ycc_w(c, 0), v[0]) + __mul24(ycc_w(c, 1), v[1]) +
                  __mul24(ycc_w(c, 2), v[2]));
}
__device__ __forceinline__ double tdot(int c, int d0, int d1, int d2) {  // details: |T| <= 1.83e9
  return (double)(__mul24(ycc_w(c, 0), d0) + __mul24(ycc_w(c, 1), d1) + __mul24(ycc_w(c, 2), d2));
}
// soft(x, t) as x - clamp(x, -t, t): the same value as soft() (x -+ t rounds alike; 0 inside),
// three fp64 ops instead of a compare and two selects
__device__ __forceinline__ double soft_c(double x, double t) { return x - fmin(fmax(x, -t), t); }
// outputs (r, s) = (0,0), (0,1), (1,0), (1,1) of A + g_s AD + f_r DA + f_r g_s DD
__device__ __forceinline__ void haar_bfly(double A, double AD, double DA, double DD, double (&x)[4]) {
  const double p = A + AD, m = A - AD, q0 = DA + DD, q1 = DA - DD;
  x[0] = p + q0;
  x[1] = m + q1;
  x[2] = p - q0;
  x[3] = m - q1;
}

// S32: the level-1 stage (details, soft thresholds, butterflies, clip, de-normalisation,
// YCbCr -> RGB) in fp32 with v_med3 clamps, as bior1.5's synthesis: it is continuous in its
// inputs and no exact zero depends on it (the levels above stay fp64; ~1e-7 on the [0, 1]
// output against the 1e-5 tolerance).  false: all fp64 (A/B: IDN_WAVELET_HS32=0)
template <int L, bool S32 = true>
__global__ __launch_bounds__(WLH_WG) void wl_haar_synth_int(const uint8_t* __restrict__ src, int h,
                                                            int w, int64_t row_stride,
                                                            const double* __restrict__ stats,
                                                            uint8_t* __restrict__ out_u8,
                                                            float* __restrict__ out_f32) {
  static_assert(L == 2 || L == 3, "4x4 sub-blocks per thread");
  using HS = HaarSplit<L>;
  constexpr int B = HS::B;
  const int img = blockIdx.y;
  const int nbx = w / B, nblk = nbx * (h / B);
  const int tid = blockIdx.x * WLH_WG + threadIdx.x;
  const int blk = tid / HS::NS, sub = tid % HS::NS;
  const bool act = blk < nblk;
  const double* st = stats + (size_t)img * WL_STATS;
  const bool bad = st[WlStats::FLAG] != 0.0;  // image-uniform: zeros (0.14.2's NaN -> U8 0)
  int y0 = 0, x0 = 0;
  uint32_t q[4][3] = {};
  if (act) {
    const int by = blk / nbx, bx = blk - by * nbx;
    y0 = by * B + (sub >> 1) * 4;
    x0 = bx * B + (sub & 1) * 4;
    const uint8_t* ib = src + (int64_t)img * h * row_stride;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(ib + (int64_t)(y0 + r) * row_stride +
                                                            (int64_t)x0 * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) q[r][k] = p[k];
    }
  }
  auto px = [&](int r, int k) { return (int)((q[r][k >> 2] >> (8 * (k & 3))) & 0xFFu); };
  // integer sums of the four level-1 groups and the level-2 combinations
  int S4[4][3];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int gy = g >> 1, gx = g & 1;
      S4[g][ch] = px(2 * gy, 6 * gx + ch) + px(2 * gy, 6 * gx + 3 + ch) +
                  px(2 * gy + 1, 6 * gx + ch) + px(2 * gy + 1, 6 * gx + 3 + ch);
    }
  int S16[3], D2[3][3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    haar_int(S4[0][ch], S4[1][ch], S4[2][ch], S4[3][ch], S16[ch], D2[0][ch], D2[1][ch], D2[2][ch]);
  int S64[3] = {0, 0, 0}, D3[3][3] = {};
  if constexpr (L == 3) {  // level 3 across the block's 4 lanes
    const int base = (threadIdx.x & 63) & ~3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      haar_int(__shfl(S16[ch], base), __shfl(S16[ch], base + 1), __shfl(S16[ch], base + 2),
               __shfl(S16[ch], base + 3), S64[ch], D3[0][ch], D3[1][ch], D3[2][ch]);
  }
  if (!act) return;
  if (bad) {
#pragma unroll 1
    for (int r = 0; r < 4; ++r)
#pragma unroll 1
      for (int k = 0; k < 12; ++k) {
        const int y = y0 + r, xx = x0 + k / 3, c = k % 3;
        if (out_u8) out_u8[(int64_t)img * h * row_stride + (int64_t)y * row_stride + (int64_t)xx * 3 + c] = 0;
        if (out_f32) out_f32[(((int64_t)img * h + y) * w + xx) * 3 + c] = 0.0f;
      }
    return;
  }
  // per-channel constants (uniform: SGPRs)
  double mnc[3], invc[3], s1c[3], kc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double mn, mx;
    wl_minmax64(st, c, mn, mx);
    mnc[c] = mn;
    invc[c] = mx - mn;
    s1c[c] = uniform_f64(0.5 / (255000.0 * invc[c]));
    kc[c] = uniform_f64(2.0 * ((c == 0 ? 16.0 : 128.0) - mn) / invc[c]);
  }
  // level L .. 2 per channel -> half the level-1 approximations of the four groups
  double Ah1[4][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s1 = s1c[c], k = kc[c];
    auto th = [&](int l, int b) { return st[WlStats::thrh(c, l, b)]; };
    double a2;  // level-2 approximation at this sub-block (after level-3 synthesis)
    if constexpr (L == 3) {
      const double Ah = tdot_sum(c, S64) * ldexp(s1, -3) + 2.0 * k;
      const double x3 = ldexp(s1, -3);
      double x[4];
      haar_bfly(Ah, soft_c(tdot(c, D3[0][0], D3[0][1], D3[0][2]) * x3, th(2, 0)),
                soft_c(tdot(c, D3[1][0], D3[1][1], D3[1][2]) * x3, th(2, 1)),
                soft_c(tdot(c, D3[2][0], D3[2][1], D3[2][2]) * x3, th(2, 2)), x);
      a2 = sub == 0 ? x[0] : sub == 1 ? x[1] : sub == 2 ? x[2] : x[3];
    } else {
      a2 = tdot_sum(c, S16) * ldexp(s1, -1) + 2.0 * k;
    }
    const double x2 = ldexp(s1, -2);
    double x[4];
    haar_bfly(0.5 * a2, soft_c(tdot(c, D2[0][0], D2[0][1], D2[0][2]) * x2, th(1, 0)),
              soft_c(tdot(c, D2[1][0], D2[1][1], D2[1][2]) * x2, th(1, 1)),
              soft_c(tdot(c, D2[2][0], D2[2][1], D2[2][2]) * x2, th(1, 2)), x);
#pragma unroll
    for (int g = 0; g < 4; ++g) Ah1[g][c] = 0.5 * x[g];
  }
  // YCbCr -> RGB x 255 (skimage's ycbcr2rgb rows) on (v' * inv + min - off)
  constexpr double R[3][3] = {{0.004566210045662101 * 255, 1.1808799897950177e-09 * 255, 0.006258928969943937 * 255},
                              {0.004566210045662101 * 255, -0.0015363236860449021 * 255, -0.003188110949655707 * 255},
                              {0.004566210045662101 * 255, 0.007910716233554741 * 255, 1.1977497040511743e-08 * 255}};
  const bool dw = out_u8 && ((reinterpret_cast<uintptr_t>(out_u8) | (uintptr_t)row_stride) & 3) == 0;
  uint32_t rowp[2][3];
  float x1f[3], thf[3][3], invf[3], mof[3];  // S32: the level-1 constants in fp32
  if constexpr (S32) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x1f[c] = (float)(0.5 * s1c[c]);
#pragma unroll
      for (int b = 0; b < 3; ++b) thf[c][b] = (float)st[WlStats::thrh(c, 0, b)];
      invf[c] = (float)invc[c];
      mof[c] = (float)(mnc[c] - (c == 0 ? 16.0 : 128.0));
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int gy = g >> 1, gx = g & 1;
    if (gx == 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) rowp[r][j] = 0u;
    }
    double v[4][3];  // the group's four pixels, three channels: v' (normalised)
    int D[3][3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int aa;
      haar_int(px(2 * gy, 6 * gx + ch), px(2 * gy, 6 * gx + 3 + ch), px(2 * gy + 1, 6 * gx + ch),
               px(2 * gy + 1, 6 * gx + 3 + ch), aa, D[0][ch], D[1][ch], D[2][ch]);
    }
    if constexpr (S32) {
      constexpr float Rf[3][3] = {
          {(float)(0.004566210045662101 * 255), (float)(1.1808799897950177e-09 * 255), (float)(0.006258928969943937 * 255)},
          {(float)(0.004566210045662101 * 255), (float)(-0.0015363236860449021 * 255), (float)(-0.003188110949655707 * 255)},
          {(float)(0.004566210045662101 * 255), (float)(0.007910716233554741 * 255), (float)(1.1977497040511743e-08 * 255)}};
      float vf[4][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float d[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {  // soft(x, t) = x - clamp(x, -t, t), one v_med3
          const float xb = (float)(__mul24(ycc_w(c, 0), D[b][0]) + __mul24(ycc_w(c, 1), D[b][1]) +
                                   __mul24(ycc_w(c, 2), D[b][2])) * x1f[c];
          d[b] = xb - __builtin_amdgcn_fmed3f(xb, -thf[c][b], thf[c][b]);
        }
        const float A = (float)Ah1[g][c];
        const float p = A + d[0], m = A - d[0], q0 = d[1] + d[2], q1 = d[1] - d[2];
        vf[0][c] = p + q0;
        vf[1][c] = m + q1;
        vf[2][c] = p - q0;
        vf[3][c] = m - q1;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i >> 1, s = i & 1;
        float e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
          e[c] = __fmaf_rn(__builtin_amdgcn_fmed3f(vf[i][c], 0.f, 1.f), invf[c], mof[c]);
        const int y = y0 + 2 * gy + r, xx = x0 + 2 * gx + s;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float o = __fmaf_rn(e[2], Rf[c][2], __fmaf_rn(e[1], Rf[c][1], e[0] * Rf[c][0]));
          const uint32_t u = (uint32_t)min(max((int)o, 0), 255);  // as the fp64 form
          if (dw) {
            const int bi = (2 * gx + s) * 3 + c;
            rowp[r][bi >> 2] |= u << (8 * (bi & 3));
          } else if (out_u8) {
            out_u8[(int64_t)img * h * row_stride + (int64_t)y * row_stride + (int64_t)xx * 3 + c] =
                (uint8_t)u;
          }
          if (out_f32)
            out_f32[(((int64_t)img * h + y) * w + xx) * 3 + c] =
                __builtin_amdgcn_fmed3f(o, 0.f, 255.f) * (1.f / 255.f);
        }
      }
    } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x1 = 0.5 * s1c[c];
      auto th = [&](int b) { return st[WlStats::thrh(c, 0, b)]; };
      double x[4];
      haar_bfly(Ah1[g][c], soft_c(tdot(c, D[0][0], D[0][1], D[0][2]) * x1, th(0)),
                soft_c(tdot(c, D[1][0], D[1][1], D[1][2]) * x1, th(1)),
                soft_c(tdot(c, D[2][0], D[2][1], D[2][2]) * x1, th(2)), x);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i][c] = x[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = i >> 1, s = i & 1;
      double e[3];  // clip [0, 1] (0.14.2), de-normalise, minus the YCbCr offset
#pragma unroll
      for (int c = 0; c < 3; ++c)
        e[c] = __fma_rn(fmin(fmax(v[i][c], 0.0), 1.0), invc[c], mnc[c] - (c == 0 ? 16.0 : 128.0));
      const int y = y0 + 2 * gy + r, xx = x0 + 2 * gx + s;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double o = __fma_rn(e[2], R[c][2], __fma_rn(e[1], R[c][1], e[0] * R[c][0]));
        // clip [0, 255] after the truncation (v_med3): the same byte for every o
        const uint32_t u = (uint32_t)min(max((int)o, 0), 255);
        if (dw) {
          const int bi = (2 * gx + s) * 3 + c;
          rowp[r][bi >> 2] |= u << (8 * (bi & 3));
        } else if (out_u8) {
          out_u8[(int64_t)img * h * row_stride + (int64_t)y * row_stride + (int64_t)xx * 3 + c] =
              (uint8_t)u;
        }
        if (out_f32)
          out_f32[(((int64_t)img * h + y) * w + xx) * 3 + c] = (float)(fmin(fmax(o, 0.0), 255.0) * (1.0 / 255.0));
      }
    }
    }  // S32
    if (dw && gx == 1) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        uint32_t* p = reinterpret_cast<uint32_t*>(out_u8 + (int64_t)img * h * row_stride +
                                                  (int64_t)(y0 + 2 * gy + r) * row_stride +
                                                  (int64_t)x0 * 3);
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = rowp[r][j];
      }
    }
  }
}

#include "haar3.hpp"

// ---- launchers: fused Haar forms and the code medians ------------------------------------------
template <int L, bool BAND, bool BIOR>
static void median_go(const WlCall& C, const WlLayout& Lt, const double* part, const WlLayout& Ls) {
  hipLaunchKernelGGL((wl_haar_median<L, BAND, BIOR>), dim3(Lt.n * 3), dim3(WLM_WG), 0, C.st, C.src,
                     C.in64, C.row_stride, C.ws, Lt.img_floats, C.stats, Lt, part, Ls);
}
template <bool GEN>
static void h3_synth_go(const WlCall& C, const WlLayout& Lt) {
  hipLaunchKernelGGL(wl_h3_synth<GEN>, dim3(h3_strips(Lt.w) * h3s_chunks(Lt.h), Lt.n),
                     dim3(WLH_WG), 0, C.st, C.src, Lt.h, Lt.w, C.row_stride,
                     (const double*)C.stats, C.out_u8, C.out_f32);
}
// the dword-store form takes a dword-aligned u8 output alone
static void h3_synthesis(const WlCall& C, const WlLayout& Lt) {
  if (C.out_f32 || !C.out_u8 || ((uintptr_t)C.out_u8 & 3) != 0) h3_synth_go<true>(C, Lt);
  else h3_synth_go<false>(C, Lt);
}
template <int L, bool S32>
static void synth_int_go(const WlCall& C, const WlLayout& Lt, int nwg) {
  hipLaunchKernelGGL((wl_haar_synth_int<L, S32>), dim3(nwg, Lt.n), dim3(WLH_WG), 0, C.st, C.src,
                     Lt.h, Lt.w, C.row_stride, C.stats, C.out_u8, C.out_f32);
}

template <int L>
static void run_haar(const WlCall& C, const WlLayout& Lt) {
  const int n = Lt.n;
  const int nthr = (Lt.h >> L) * (Lt.w >> L) * HaarSplit<L>::NS;
  const int nwg = (nthr + WLH_WG - 1) / WLH_WG;
  if constexpr (L == 3) {
    // u8 input (haar3.hpp): window sample, one statistics read, sigma, one synthesis read; the
    // window kernel also clears its image's statistics block (wl_init_stats' values)
    const int nwg1 = h3_strips(Lt.w) * h3_chunks(Lt.h);
    // (IDN_WAVELET_H3=0: the passes below; H3FB=1: the window's fallback, forced)
    if (C.src && !C.ycc_keys && (size_t)(3 * nwg1) <= Lt.part_per_img / 9 &&
        tuned("IDN_WAVELET_H3", 1)) {
      hipLaunchKernelGGL(wl_h3_window, dim3(n), dim3(H3_WIN_WG), 0, C.st, C.src, Lt.h, Lt.w,
                         C.row_stride, C.stats, tuned("IDN_WAVELET_H3FB", 0));
      hipLaunchKernelGGL(wl_h3_stats<false>, dim3(nwg1, n), dim3(WLH_WG), 0, C.st, C.src, Lt.h,
                         Lt.w, C.row_stride, C.ws, Lt.img_floats, C.stats, C.part, Lt.part_per_img);
      hipLaunchKernelGGL(wl_h3_sigma, dim3(n * 3), dim3(WLM_WG), 0, C.st, C.src, C.row_stride, C.ws,
                         Lt.img_floats, C.stats, Lt, (const double*)C.part, nwg1);
      h3_synthesis(C, Lt);
      return;
    }
  }
  wl_clear_stats(C, Lt);
  if (!C.ycc_keys) wl_minmax_exact(C, Lt);
  // statistics: u8 input at L >= 2 from integer moments, else from the normalised fp64 planes
  const bool ints = L >= 2 && C.src && tuned("IDN_WAVELET_INTSTATS", 1);
  int nwg_a = (nthr + WLH_WG * WLH_IT - 1) / (WLH_WG * WLH_IT);
  if constexpr (L >= 2) {
    if (ints) {
      nwg_a = (nthr + WLH_WG * WLS_IT - 1) / (WLH_WG * WLS_IT);
      hipLaunchKernelGGL((wl_haar_stats<L>), dim3(nwg_a, n), dim3(WLH_WG), 0, C.st, C.src, Lt.h,
                         Lt.w, C.row_stride, C.ws, Lt.img_floats, Lt.off_band[1], C.stats, C.part,
                         Lt.part_per_img);
    }
  }
  if (!ints)
    hipLaunchKernelGGL((wl_haar_analyze<L>), dim3(nwg_a, n), dim3(WLH_WG), 0, C.st, C.src, C.in64,
                       Lt.h, Lt.w, C.row_stride, C.ws, Lt.img_floats, Lt.off_band[1], C.stats,
                       C.part, Lt.part_per_img);
  WlLayout Ls = Lt;  // wl_sumsq view of the fused partials: nwg per level, levels back to back
  for (int l = 1; l <= L; ++l) {
    Ls.tiles[l] = nwg_a;
    Ls.part_tile0[l] = (size_t)(l - 1) * nwg_a;
  }
  // the median workgroups also reduce the sums of squares and set the thresholds
  const bool fuse = tuned("IDN_WAVELET_FUSETHR", 1) != 0;
#ifdef IDN_TUNING_BUILD  // IDN_WAVELET_FUSETHR=0: wl_sumsq and wl_thresh as separate launches
  if (!fuse) wl_sum_partials(C, Ls);
#endif
  median_go<L, false, false>(C, Lt, fuse ? (const double*)C.part : nullptr, Ls);
#ifdef IDN_TUNING_BUILD
  if (!fuse) wl_thresholds(C, Lt);
#endif
  // synthesis: u8 input at L >= 2 from the integer combinations (L = 3: haar3.hpp's fp32 form
  // with the level-1 groups paired), else on the normalised fp64 planes
  const bool ints_syn = L >= 2 && C.src && tuned("IDN_WAVELET_INTSYNTH", 1);
#ifdef IDN_TUNING_BUILD  // H3S=0 at L = 3: the round-4 kernel; HS32=0: its all-fp64 form
  if constexpr (L >= 2)
    if (ints_syn && !(L == 3 && knob("IDN_WAVELET_H3S", 1)))
      return knob("IDN_WAVELET_HS32", 1) ? synth_int_go<L, true>(C, Lt, nwg)
                                         : synth_int_go<L, false>(C, Lt, nwg);
#endif
  if constexpr (L == 3) {
    if (ints_syn) {
      hipLaunchKernelGGL(wl_h3_consts, dim3((3 * n + 63) / 64), dim3(64), 0, C.st, C.stats, n);
      return h3_synthesis(C, Lt);
    }
  }
  if constexpr (L == 2)
    if (ints_syn) return synth_int_go<2, true>(C, Lt, nwg);
  hipLaunchKernelGGL((wl_haar_synth<L>), dim3(nwg, n), dim3(WLH_WG), 0, C.st, C.src, C.in64, Lt.h,
                     Lt.w, C.row_stride, C.stats, C.out_u8, C.out_f32);
}

void wl_run_haar(const WlCall& C, const WlLayout& Lt) {
  if (Lt.L == 1) run_haar<1>(C, Lt);
  else if (Lt.L == 2) run_haar<2>(C, Lt);
  else run_haar<3>(C, Lt);
}

// ---- for wl_run: the proxy min / max and the medians of the per-level paths ----------------------
// u8 input in whole 8x8 blocks with dword-aligned rows (wl_run checks)
void wl_minmax_proxy(const WlCall& C, const WlLayout& Lt) {
  hipLaunchKernelGGL(wl_h3_stats<true>, dim3(h3_strips(Lt.w) * h3_chunks_mm(Lt.h), Lt.n),
                     dim3(WLH_WG), 0, C.st, C.src, Lt.h, Lt.w, C.row_stride, C.ws, Lt.img_floats,
                     C.stats, (double*)nullptr, (size_t)0);
}
void wl_band_median(const WlCall& C, const WlLayout& Lt) {
  hipLaunchKernelGGL(wl_median, dim3(Lt.n * 3), dim3(1024), 0, C.st, C.ws, Lt.img_floats,
                     C.stats, Lt);
}
void wl_code_median(const WlCall& C, const WlLayout& Lt, const double* part, bool dd32) {
  if (dd32) median_go<1, true, true>(C, Lt, part, Lt);
  else median_go<1, true, false>(C, Lt, part, Lt);
}

}  // namespace idn
