// Wavelet denoiser, the streaming path: bior1.5, one launch per level (wavelet.hip has the map of
// the units).  wl_dwt_stream walks a strip of columns down the rows for the analysis,
// wl_synth_final3 (and the tuning library's wl_synth_stream) for the synthesis.  Entered through
// wl_stream_analysis and wl_stream_synthesis, both called by wl_run; wl_layout sizes the
// partials by ws_strips and ws_bands.
#include "wavelet_common.hpp"

namespace idn {

// ---- 2b: bior1.5 analysis, streaming form ------------------------------------------------------
// pywt's bior1.5 decomposition pair in terms of input pairs: with s_k = x[2k] + x[2k+1] and
// e_k = x[2k+1] - x[2k] over the symmetrically extended input (output i uses x[2i-8 .. 2i+1]),
//   lo[i] = S2 s_{i-2} + B1 (e_i - e_{i-4}) + B2 (e_{i-3} - e_{i-1})     (10 taps -> 5 operations;
//           rounding within a few ulps of pywt's sum: aa / ad / da only feed the thresholds and
//           the synthesis, both checked within 1e-5)
//   hi[i] = (-S2 x[2i-3]) + S2 x[2i-4]                                  (pywt's order, exact:
//           the finest dd's exact zeros select the sigma median's population)
// One workgroup per (image, strip of SW output columns, band of output rows) walks down the rows,
// one input row pair per step.
//   column phase: thread u = staged input column 2 j0 - 8 + u (all three channels) normalises its
//     two new samples -- every sample once per strip (halo: 8 of 2 SW + 8 columns; the tiled
//     wl_dwt_rb normalised each sample ~1.7 times) -- and adds the pair to five running lowpass
//     accumulators (pair k contributes B1 e_k, -B2 e_k, S2 s_k, B2 e_k, -B1 e_k to outputs
//     k .. k+4); output row i's column lowpass / highpass go to LDS (double-buffered: one barrier
//     per step).  The raw samples of the next PF steps are in flight in a register ring.
//   row phase: thread (c, jj) runs the pair form along the row for the two adjacent outputs jj,
//     jj + 1: aa / da (lowpass of the column low / high), ad = S2 (v[2j-4] - v[2j-3]), dd in
//     pywt's exact order; band stores (fp32 bands per fmask), level-1 dd codes, sums of squares
// Row bands start four pairs early to fill the accumulators (4 / band height extra work).
#ifndef IDN_WS_MAXT  // A/B builds set it
#define IDN_WS_MAXT 512
#endif
constexpr int WS_MAXT = IDN_WS_MAXT;         // threads = staged columns per workgroup (max)
// output columns per strip (max): (threads - 8) / 2; tuning: IDN_WAVELET_WST threads (64..256)
inline int ws_maxsw() {
  const int t = std::min(std::max(knob("IDN_WAVELET_WST", WS_MAXT), 64), WS_MAXT) / 64 * 64;
  return (t - 8) / 2;
}
int ws_strips(int Wo) { return (Wo + ws_maxsw() - 1) / ws_maxsw(); }
inline int ws_sw(int Wo) {
  const int st = ws_strips(Wo);
  return ((Wo + st - 1) / st + 1) & ~1;
}
// bands of whole WS_G-row groups, >= 16 output rows each: as best_bands, costed by the rows of
// the longest band
int ws_bands(int n, int Ho, int Wo, int strips, int level) {
  const int groups = (Ho + WS_G - 1) / WS_G;
  // resident workgroups as a 512-thread launch would have them.  (The deeper 600x1000 levels
  // launch 320 threads; counting those -- twice the workgroups per CU -- picked more, shorter bands
  // and measured 20 % slower at levels 2-3: the analysis is throughput-bound there, and extra bands
  // only add warm-up rows, profiles/r04/wavelet/.)
  (void)Wo;
  const int block = WS_MAXT;
  const int64_t units = (int64_t)n * strips, resident = std::max<int64_t>(ws_resident(level, block), 1);
  const int bmax = std::max(1, std::min({64, Ho / 16, groups}));
  int best = 1;
  double bestc = 1e300;
  for (int b = 1; b <= bmax; ++b) {
    const double rounds = std::ceil((double)(units * b) / (double)resident);
    const double c = rounds * ((groups + b - 1) / b * WS_G + 4);
    if (c < bestc * 0.999) {
      bestc = c;
      best = b;
    }
  }
  return best;
}

template <int SRC>
struct WsRaw;  // the raw input of one step (two rows) for one staged column
template <> struct WsRaw<0> {  // u8 pixels: the raw dword holding each row's 3 bytes (see load)
  uint32_t p[2];
};
template <> struct WsRaw<1> {  // f64 pixels
  double p[2][3];
};
template <> struct WsRaw<2> {  // the level above's 'aa', three channels, fp64
  double p[2][3];
};
template <> struct WsRaw<3> {  // the level above's 'aa', three channels, fp32 (WL_FB_AIN)
  float p[2][3];
};
// prefetch depth (steps; divides 5): the u8 and fp32 rings are small, the fp64 ones are not.
// (Round 3 measured the fp32 'aa' ring at depth 5 1 % slower than depth 1 -- when no ring load was
// in flight past its own step, see the ring comments in wl_dwt_stream; with working prefetch
// depth 5 is the faster.)
#ifndef IDN_WS_PF0  // A/B builds set these
#define IDN_WS_PF0 5
#endif
#ifndef IDN_WS_WPE
#define IDN_WS_WPE 1
#endif
#ifndef IDN_S3_WPE
#define IDN_S3_WPE 1
#endif
#ifndef IDN_S3_PAD
#define IDN_S3_PAD 0
#endif
#ifndef IDN_WS_PF3  // the fp32 'aa' input of levels >= 2: a 5-step ring measured 2.773 -> 2.752 ms on
#define IDN_WS_PF3 5  // the op against 1 (levels 2 / 3: 283 -> 264 / 92 -> 88 us, profiles/r04/wavelet/)
#endif
#ifndef IDN_WS_PF1  // the live path's fp64 pixels (A/B builds set it)
#define IDN_WS_PF1 1
#endif
template <int SRC> constexpr int ws_pf() {
  return SRC == 0 ? IDN_WS_PF0 : SRC == 3 ? IDN_WS_PF3 : SRC == 1 ? IDN_WS_PF1 : 1;
}


// TL / TH: arithmetic of the lowpass / highpass paths.  fp64 throughout is pywt's precision; the
// product runs the lowpass outputs (aa, ad, da: continuous inputs of the thresholds' fp64 sums of
// squares and of the synthesis) in fp32, and at level 1 keeps the normalisation, the column
// highpass and dd in fp64 with pywt's op order (the finest dd's exact zeros select the sigma
// median's population); deeper levels (no median) run both paths in fp32.
// FM >= 0: the band storage mask (wl_fband) and CODES the level-1 code emission as compile-time
// constants (the product's masks: no per-band branches); FM = -1 takes both from the arguments.
// NT: threads per workgroup the LDS arrays are sized for (the product launches 512; instances
// sized for 64- and 256-thread strips measured slower at every band count: level 1 1.39 / 1.04
// ms vs 0.93, profiles/r04/wavelet/strips_sweep.txt)
template <int SRC, typename TL = wreal, typename TH = wreal, int FM = -1, int CODES = -1,
          int NT = WS_MAXT>
__global__ __launch_bounds__(NT, IDN_WS_WPE) void wl_dwt_stream(
    wreal* __restrict__ ws, size_t img_floats, const double* __restrict__ stats, size_t in_off,
    int Hin, int Win, size_t out_off, int Ho, int Wo, int SW, int strips, int bands, int groups,
    const uint8_t* __restrict__ src, const double* __restrict__ in64, int64_t row_stride,
    double* __restrict__ part, size_t part_per_img, size_t part_tile0, int emit_codes_arg,
    int fmask_arg, double sq_grid) {
  const int fmask = FM >= 0 ? FM : fmask_arg;
  const int emit_codes = CODES >= 0 ? CODES : emit_codes_arg;
  constexpr int PF = ws_pf<SRC>();
  // VL / VF: the column lowpass / highpass in the lowpass type (TL) at staged column u; VH: the
  // column highpass in TH for dd, even and odd columns in separate halves (column u at
  // (u & 1) * WS_MAXT / 2 + u / 2) so that the row threads' 16-byte reads (lane stride 4 columns)
  // fill whole bank rows -- interleaved fp64 columns put two lanes on every 16-byte slot
  constexpr bool SEPF = !std::is_same<TL, TH>::value;  // a separate TL copy of the highpass
  // N32 (round 6; u8 level 1 with an fp32 highpass): the normalisation is one fp32 affine map of
  // the bytes per channel, and the finest dd's codes come from the exact integer T = K00 - K10 -
  // K01 + K11 of the pixels' YCbCr keys K = w . rgb (the dd is 0.5 T / (255000 range) within
  // 2e-12 / range, as for the fused Haar: wl_haar_stats' certainty rule, the exact fp64 key where
  // it is not certain) -- sigma stays bit-identical while every coefficient runs in fp32
  constexpr bool N32 = SRC == 0 && std::is_same<TH, float>::value && CODES != 0;
  __shared__ TL VL[2][3][NT];
  __shared__ TL VF[SEPF ? 2 : 1][SEPF ? 3 : 1][SEPF ? NT : 1];
  __shared__ TH VH[2][3][NT];
  __shared__ int VK[N32 ? 2 : 1][N32 ? 3 : 1][N32 ? NT : 1];  // key column highpass, VH's layout
  __shared__ double RED[3][NT];
  const int img = blockIdx.z;
  const int strip = (int)blockIdx.x % strips, band = (int)blockIdx.x / strips;
  const int j0 = strip * SW;
  // the band: whole WS_G-row groups [ga, gb) (the last group of the image may be short)
  const int ga = (int)((int64_t)band * groups / bands), gb = (int)((int64_t)(band + 1) * groups / bands);
  const int ia = ga * WS_G, ib = min(gb * WS_G, Ho);
  const int t = threadIdx.x;
  wreal* base = ws + img * img_floats;
  // ---- column role
  const int NXs = 2 * SW + 8;
  const bool colt = t < NXs;
  const int qc = sym_idx(2 * j0 - 8 + t, Win);  // this thread's input column
  // u8 source: one unaligned dword per row, bytes 3 qc - 1 .. 3 qc + 2 (bytes 0..3 for column 0),
  // so it never reaches past the image's last byte; the pixel is at bit qsh of it.  The bytes are
  // extracted where the step is consumed (norm), PF steps later: packing three byte loads at load
  // time made every load wait for its data at once, and the ring prefetched nothing.
  const uint32_t qvo = qc > 0 ? 3u * (uint32_t)qc - 1u : 0u, qsh = qc > 0 ? 8u : 0u;
  wreal mn[3] = {0, 0, 0}, inv[3] = {1, 1, 1}, rcp[3] = {1, 1, 1};
  if (SRC < 2) {
    const double* st = stats + (size_t)img * WL_STATS;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wreal mx;
      wl_minmax64(st, c, mn[c], mx);
      inv[c] = mx - mn[c];
      rcp[c] = 1.0 / inv[c];
    }
  }
  // N32: x_c = sum_k A[c][k] b_k + Bc[c] (b the bytes) = ((w_c . b) / 255000 + off_c - min_c) / range_c
  float A32c[3][3] = {}, B32c[3] = {};
  double sc1[3] = {0.0, 0.0, 0.0};  // the finest dd per unit of T: 0.5 / (255000 range)
  if constexpr (N32) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sc1[c] = uniform_f64(0.5 / (255000.0 * inv[c]));
#pragma unroll
      for (int k = 0; k < 3; ++k) A32c[c][k] = (float)((double)ycc_w(c, k) / (255000.0 * inv[c]));
      B32c[c] = (float)(((c == 0 ? 16.0 : 128.0) - mn[c]) / inv[c]);
    }
  }
  rsrc_t rs;
  if (SRC == 0)
    rs = make_rsrc(src + (int64_t)img * Hin * row_stride, (uint32_t)((int64_t)Hin * row_stride));
  else if (SRC == 1)
    rs = make_rsrc(in64 + (int64_t)img * Hin * Win * 3, (uint32_t)((int64_t)Hin * Win * 24));
  auto load = [&](int k, WsRaw<SRC>& R) {
    const int rows[2] = {sym_idx(2 * k, Hin), sym_idx(2 * k + 1, Hin)};
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      if constexpr (SRC == 0) {
        const uint32_t so = (uint32_t)((int64_t)rows[h2] * row_stride);
        R.p[h2] = __builtin_amdgcn_raw_buffer_load_b32(rs, qvo, so, 0);
      } else if constexpr (SRC == 1) {
        const uint32_t so = (uint32_t)rows[h2] * (uint32_t)Win * 24u;
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3)
          R.p[h2][k3] = __longlong_as_double((long long)__builtin_amdgcn_raw_buffer_load_b64(
              rs, (uint32_t)qc * 24u + 8u * k3, so, 0));
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const wreal* X = base + in_off + (size_t)c * 4 * Hin * Win;
          const size_t e = (size_t)rows[h2] * Win + qc;
          if constexpr (SRC == 3) R.p[h2][c] = reinterpret_cast<const float*>(X)[e];
          else R.p[h2][c] = X[e];
        }
      }
    }
  };
  // channel c of row h2 of the raw step: normalised (SRC 0 / 1) or the aa sample (SRC 2)
  auto norm = [&](const WsRaw<SRC>& R, int h2, int c) -> wreal {
    if constexpr (SRC >= 2) {
      return (wreal)R.p[h2][c];
    } else {
      double px[3];
#pragma unroll
      for (int k3 = 0; k3 < 3; ++k3) {
        if constexpr (SRC == 0) px[k3] = (double)((R.p[h2] >> (qsh + 8 * k3)) & 0xFFu) * (1.0 / 255.0);
        else px[k3] = R.p[h2][k3];
      }
      const wreal a = ycbcr_c(px, c) - mn[c];
      if constexpr (SRC == 1) {
        return a / inv[c];
      } else {
        // skimage's (Y - min) / (max - min) as the IEEE quotient: reciprocal multiply + one
        // Markstein correction, exact over every u8 triple (tools/check_div.c)
        const wreal qq = a * rcp[c];
        return __fma_rn(__fma_rn(-qq, inv[c], a), rcp[c], qq);
      }
    }
  };
  TL acc[3][5];              // running column lowpass of outputs k .. k+4 (slot = output % 5)
  TH hd0[3], hd1[3];         // column highpass of pairs k-1, k-2 (hi[i] is pair i-2's)
  int kd0[3], kd1[3];        // N32: the key highpass K(row 2k) - K(row 2k+1) of the same pairs
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    kd0[c] = kd1[c] = 0;
    hd0[c] = hd1[c] = (TH)0;
#pragma unroll
    for (int r = 0; r < 5; ++r) acc[c][r] = (TL)0;
  }
  // ---- row role
  const int half = SW / 2;
  // task u = (channel rc, column pair jj): at level 1 spread over every wave of the workgroup in
  // contiguous runs, so that no wave sits at the step's barrier without row work (934 vs 962 us);
  // deeper levels keep u = t (spread measured 273 vs 262 us at level 2: profiles/r04/wavelet/)
  const int nwv = (int)(blockDim.x >> 6);  // waves of the launch (NT is only the maximum)
  const int rw = SRC < 2 ? (3 * half + nwv - 1) / nwv : 64;  // tasks per wave
  const int u = SRC < 2 ? (t >> 6) * rw + (t & 63) : t;
  const bool rowt = (t & 63) < rw && u < 3 * half;
  const int rc = rowt ? u / half : 0, jj = rowt ? 2 * (u - rc * half) : 0;
  const int oj = j0 + jj;
  const bool ok0 = rowt && oj < Wo, ok1 = rowt && oj + 1 < Wo;
  const size_t bsz = (size_t)Ho * Wo;
  // Sums of squares, independent of the band split (batch size, device): each row thread sums
  // its two outputs of a WS_G-row group's rows in row order (sq), and at the group's last row rounds
  // that partial to a multiple of sq_grid (a power of two) into sqa.  Sums of multiples of
  // sq_grid below 2^53 sq_grid are exact in fp64, and the layout sizes sq_grid so that the whole
  // band's sum stays below that (wl_layout): every later addition -- this thread's groups, the
  // workgroup's threads, wl_sumsq's tiles -- is exact, hence order-free.  (Rounding error per
  // partial <= sq_grid / 2, ~1e-10 of a typical band total.)
  double sq[3] = {0.0, 0.0, 0.0}, sqa[3] = {0.0, 0.0, 0.0};
  const double sq_inv = 1.0 / sq_grid;  // exact: a power of two

  const int k0 = ia - 4, M = ib - ia + 4;  // steps m = 0 .. M-1 cover pairs k = k0 + m
  WsRaw<SRC> rq[PF];                        // raw samples of steps m .. m + PF - 1 (slot m % PF)
  // the ring's loads are unconditional (rows past the band mirror into the image, sym_idx, and are
  // never used): a load under a branch leaves a phi whose copy waits for the data at once
#pragma unroll
  for (int f = 0; f < PF; ++f) load(k0 + f, rq[f]);
  for (int m0 = 0; m0 < M; m0 += 5) {
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int m = m0 + r;
      const int k = k0 + m;
      const int buf = m & 1;
      if (colt) {
        const int slot = r % PF;  // PF divides 5 (compile-time after unrolling)
        const WsRaw<SRC>& cur = rq[slot];
        float bf[2][3];   // N32: the pixel bytes as floats
        int bi[2][3];     //      and as integers
        if constexpr (N32) {
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int k3 = 0; k3 < 3; ++k3) {
              bi[h2][k3] = (int)((cur.p[h2] >> (qsh + 8 * k3)) & 0xFFu);
              bf[h2][k3] = (float)bi[h2][k3];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          TH h0, h1;
          TL l0, l1;
          if constexpr (N32) {
            const float y0 = __fmaf_rn(A32c[c][2], bf[0][2], __fmaf_rn(A32c[c][1], bf[0][1], __fmaf_rn(A32c[c][0], bf[0][0], B32c[c])));
            const float y1 = __fmaf_rn(A32c[c][2], bf[1][2], __fmaf_rn(A32c[c][1], bf[1][1], __fmaf_rn(A32c[c][0], bf[1][0], B32c[c])));
            l0 = (TL)y0;
            l1 = (TL)y1;
            h0 = (TH)y0;
            h1 = (TH)y1;
          } else {
            const auto x0 = norm(cur, 0, c), x1 = norm(cur, 1, c);
            l0 = (TL)x0;
            l1 = (TL)x1;
            h0 = (TH)x0;
            h1 = (TH)x1;
          }
          const TL sk = l0 + l1, ek = l1 - l0;
          const TH hk = (TH)(-S2) * h1 + (TH)S2 * h0;  // pywt: mul, add (no contraction)
          // pair k's contributions; slot (k + j) % 5 == (r + j) % 5 for the unrolled r
          acc[c][(r + 4) % 5] = (TL)(-B1) * ek;
          acc[c][(r + 3) % 5] = fma_t<TL>((TL)B2, ek, acc[c][(r + 3) % 5]);
          acc[c][(r + 2) % 5] = fma_t<TL>((TL)S2, sk, acc[c][(r + 2) % 5]);
          acc[c][(r + 1) % 5] = fma_t<TL>((TL)(-B2), ek, acc[c][(r + 1) % 5]);
          const TL lo = fma_t<TL>((TL)B1, ek, acc[c][r]);  // output k complete
          if (m >= 4) {
            VL[buf][c][t] = lo;
            VH[buf][c][(t & 1) * (NT / 2) + (t >> 1)] = hd1[c];
            if constexpr (SEPF) VF[buf][c][t] = (TL)hd1[c];
            if constexpr (N32) VK[buf][c][(t & 1) * (NT / 2) + (t >> 1)] = kd1[c];
          }
          hd1[c] = hd0[c];
          hd0[c] = hk;
          if constexpr (N32) {
            kd1[c] = kd0[c];
            kd0[c] = (__mul24(ycc_w(c, 0), bi[0][0]) + __mul24(ycc_w(c, 1), bi[0][1]) + __mul24(ycc_w(c, 2), bi[0][2])) -
                     (__mul24(ycc_w(c, 0), bi[1][0]) + __mul24(ycc_w(c, 1), bi[1][1]) + __mul24(ycc_w(c, 2), bi[1][2]));
          }
        }
      }
      // refill the slot PF steps ahead, after its last use and outside the column threads' branch
      // (every thread loads; a load under the branch, or into a slot still being read, is copied
      // into the ring at the join and that copy waits for the data at once)
      load(k + PF, rq[r % PF]);
      // accumulator fill, and the steps that pad the band to whole 5-step iterations: their column
      // work is wasted, but every iteration then runs all five steps (wave-uniform).  (A break out of
      // the unrolled steps merges, at the loop header, a path on which the latest ring load is that
      // step's, and the compiler's wait at every slot's first use drops to that path's: the ring
      // would prefetch nothing.)
      if (m < 4 || m >= M) continue;
      __syncthreads();
      const int i = k;  // output row
      if (rowt) {
        const TL* vl = &VL[buf][rc][2 * jj];
        const TH* vhe = &VH[buf][rc][jj];                 // element 2 jj + m, m even: vhe[m / 2]
        const TH* vho = &VH[buf][rc][NT / 2 + jj];   //                   m odd:  vho[m / 2]
        const TL* vf = SEPF ? &VF[buf][rc][2 * jj] : nullptr;
        TL o[2][3];  // [output][aa, ad, da]
        TH odd[2];   // [output] dd
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {  // column low -> aa / ad, column high -> da / dd
          TL S[6], E[6];
#pragma unroll
          for (int nn = 0; nn < 6; ++nn) {
            TL a0, a1;
            if (pass == 0) {
              a0 = vl[2 * nn];
              a1 = vl[2 * nn + 1];
            } else if constexpr (SEPF) {
              a0 = vf[2 * nn];
              a1 = vf[2 * nn + 1];
            } else {
              a0 = (TL)vhe[nn];
              a1 = (TL)vho[nn];
            }
            S[nn] = a0 + a1;
            E[nn] = a1 - a0;
          }
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            o[d][2 * pass] = fma_t<TL>((TL)S2, S[2 + d],
                                       fma_t<TL>((TL)B1, E[4 + d] - E[d], (TL)B2 * (E[1 + d] - E[3 + d])));
            if (pass == 0) o[d][1] = (TL)(-S2) * E[2 + d];
            else odd[d] = (TH)(-S2) * vho[d + 2] + (TH)S2 * vhe[d + 2];  // elements 2d+5, 2d+4
          }
        }
        const size_t e0 = (size_t)i * Wo + oj;
        uint32_t code[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          if (!(d ? ok1 : ok0)) continue;
          const double v1 = (double)o[d][1], v2 = (double)o[d][2], v3 = (double)odd[d];
          sq[0] = __fma_rn(v1, v1, sq[0]);  // (exact squares for the fp32 bands: = mul + add)
          sq[1] = __fma_rn(v2, v2, sq[1]);
          sq[2] = __fma_rn(v3, v3, sq[2]);
          if constexpr (N32) {
            const int* vke = &VK[buf][rc][jj];
            const int* vko = &VK[buf][rc][NT / 2 + jj];
            const int T = vke[d + 2] - vko[d + 2];  // elements 2d + 4 (even), 2d + 5 (odd)
            const uint32_t aT = (uint32_t)(T < 0 ? -T : T);
            const uint32_t hi = (uint32_t)__double2hiint((double)aT * sc1[rc]);
            code[d] = (uint32_t)min(max((int)(hi >> 16) - (1023 - 61) * 16, 0), WL_FBINS - 1) + 1u;
            if (!(aT >= 3u && (hi & 0xFFFFu) - 2u <= 0xFFFBu)) {
              // rare: the median workgroup sets this code from the exact fp64 key (the list sits
              // after the channel's codes, where the median's key scratch starts later)
              code[d] = 0u;
              uint32_t* lst = reinterpret_cast<uint32_t*>(base + (size_t)rc * Hin * Win + (bsz + 3) / 4);
              lst[atomicAdd(reinterpret_cast<uint32_t*>(const_cast<double*>(stats) + (size_t)img * WL_STATS + WL_N32U + rc), 1u)] =
                  (uint32_t)(i * Wo + oj + d);
            }
          } else {
            const unsigned long long key = absbits((double)odd[d]);
            code[d] = key ? wl_fbin(key) + 1 : 0;
          }
        }
        if (emit_codes) {  // the pair's two codes as one dword where it is aligned
          uint16_t* cp = reinterpret_cast<uint16_t*>(base + (size_t)rc * Hin * Win) + e0;
          if (ok1 && (e0 & 1) == 0) {
            *reinterpret_cast<uint32_t*>(cp) = code[0] | code[1] << 16;
          } else {
            if (ok0) cp[0] = (uint16_t)code[0];
            if (ok1) cp[1] = (uint16_t)code[1];
          }
        }
        wreal* ob = base + out_off + (size_t)rc * 4 * bsz;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double w0 = b < 3 ? (double)o[0][b] : (double)odd[0];
          const double w1 = b < 3 ? (double)o[1][b] : (double)odd[1];
          if (wl_fband(fmask, b)) {
            float* f = reinterpret_cast<float*>(ob + (size_t)b * bsz) + e0;
            if (ok1 && ((uintptr_t)f & 7) == 0) {  // both outputs, one aligned 8-byte store
              *reinterpret_cast<float2*>(f) = make_float2((float)w0, (float)w1);
            } else {
              if (ok0) f[0] = (float)w0;
              if (ok1) f[1] = (float)w1;
            }
          } else {
            wreal* f = ob + (size_t)b * bsz + e0;
            if (ok1 && ((uintptr_t)f & 15) == 0) {
              *reinterpret_cast<double2*>(f) = make_double2(w0, w1);
            } else {
              if (ok0) f[0] = w0;
              if (ok1) f[1] = w1;
            }
          }
        }
      }
      // the group ends at this row: i + 1 = ia - 3 + m is a multiple of WS_G = 5 exactly when
      // r = m - m0 = 3 (ia and m0 are multiples of 5)
      if (r == 3) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          sqa[b] = __fma_rn(__builtin_rint(sq[b] * sq_inv), sq_grid, sqa[b]);
          sq[b] = 0.0;
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)  // the image's last group when Ho is not a multiple of 5 (else 0)
    sqa[b] = __fma_rn(__builtin_rint(sq[b] * sq_inv), sq_grid, sqa[b]);
  // per-workgroup sums (exact, see above), channel by channel
  __syncthreads();
  double* red = &RED[0][0];
  if (rowt) {
#pragma unroll
    for (int b = 0; b < 3; ++b) red[b * NT + u] = sqa[b];
  }
  __syncthreads();
  if (t < 9) {
    const int c = t / 3, b = t - 3 * c;
    double s2 = 0.0;
    for (int g = 0; g < half; ++g) s2 += red[b * NT + c * half + g];
    part[img * part_per_img + (size_t)(c * 3 + b) * (part_per_img / 9) + part_tile0 + blockIdx.x] = s2;
  }
}

// resident workgroups of the product's streaming analysis of a level (level 1: u8 / fp32-lowpass;
// deeper: fp32 'aa' input), used by wl_layout's band count for every form of that level
int ws_resident(int level, int block) {
  const void* k = level == 1
      ? reinterpret_cast<const void*>(&wl_dwt_stream<0, float, wreal, 0b1111, 1>)
      : reinterpret_cast<const void*>(&wl_dwt_stream<3, float, float, 0b1111, 0>);
  return cu_count() * occ_wgs(k, block);
}

// ---- 6/7 (bior1.5): synthesis, streaming form -------------------------------------------------
// One workgroup per (image, strip of SWo output columns, band of output row pairs) walks down the
// band's coefficient rows; every coefficient is loaded and soft-thresholded once per strip (the
// tiled form staged 1.56x with its halos).  Output pair (2m, 2m+1) x (2n, 2n+1) uses coefficient
// rows m .. m+4 and columns n .. n+4 (pywt upsampling_convolution_valid_sf, c[j] = x[i - j]).
// Per step, coefficient row r:
//   stage    the row's 4 bands x 3 channels over columns [n0, n0 + SWo/2 + 4) into LDS (details
//            soft-thresholded), from a register ring SS_PF rows ahead; every load is issued
//            unconditionally (an fp32 band is read as the 8-byte pair holding its element, the
//            half picked by a select) so no load sits behind a branch and its wait
//   axis 1   thread (c, np): the pair form (synth_full) on row r for output columns 2np, 2np+1:
//            sa = idwt(aa, ad), sd = idwt(da, dd) -> a five-row register ring (shifted by moves)
//   axis 0   once five rows are in: output rows 2m, 2m+1 (m = r - 4) of both columns from the
//            ring; levels >= 2 store the reconstruction (fp64) into the level above's 'aa' slot,
//            level 1 (FINAL) clips, de-normalises and hands Y / Cb / Cr to LDS; there every pixel
//            pair is converted to BGR (inverse YCbCr, clip, U8 / f32) into an LDS row image that
//            the next step stores as whole dwords.
constexpr int SS_MAXT = 256;
constexpr int SS_MAXSW = 168;  // 3 x 84 column pairs <= 256 threads
inline int ss_strips(int Wout) { return (Wout + SS_MAXSW - 1) / SS_MAXSW; }
inline int ss_sw(int Wout) {
  const int st = ss_strips(Wout);
  return ((Wout + st - 1) / st + 3) & ~3;  // strips start on 4 pixels: 12-byte (dword) multiples
}
inline int ss_bands(int n, int Mo, int strips) {  // Mo output row pairs; bands >= 32 pairs
  const int want = (4096 + n * strips - 1) / (n * strips);
  return std::max(1, std::min(want, Mo / 32));
}
// the same on the measured residency of the launched kernel (>= 16 row pairs per band)
inline int ss_bands_occ(int n, int Mo, int strips, const void* kernel, int block) {
  return best_bands((int64_t)n * strips, Mo, 4, (int64_t)cu_count() * occ_wgs(kernel, block), 16);
}
constexpr int SS_PF = 4;                   // coefficient rows in flight ahead of the one staged
constexpr int SS_NCOL = SS_MAXSW / 2 + 4;  // staged coefficient columns (max)
constexpr int SS_ITEMS = 5;                // staging items per thread: 12 x SS_NCOL <= 5 x 256
constexpr int SS_OBW = SS_MAXSW * 3 / 4;   // dwords of one U8 BGR strip row

// T: the synthesis arithmetic.  double: pywt's fp64 (bit-identical to the tiled form's pair
// arithmetic); float: fp32 coefficients, taps, de-normalisation and YCbCr -> RGB (the synthesis
// is continuous in its inputs and no exact zero depends on it: ~3e-7 from the fp64 form on the
// [0, 1] output scale, against the 1e-5 tolerance), with levels >= 2 storing their
// reconstruction as fp32 (the level above reads its 'aa' through WL_FB bit 0).
template <typename T>
__device__ __forceinline__ void synth_bior(const T (&cl)[5], const T (&cd)[5], T& ev, T& od) {
  const T common = fma_t<T>((T)B1, cd[0] - cd[4], (T)B2 * (cd[3] - cd[1]));
  ev = fma_t<T>((T)S2, cl[2] + cd[2], common);
  od = fma_t<T>((T)S2, cl[2] - cd[2], common);
}
// type-exact helpers (the plain builtins are the double versions: a float argument would be
// promoted and the arithmetic done in fp64)
template <typename T>
__device__ __forceinline__ T abs_t(T x) {
  if constexpr (sizeof(T) == 4) return __builtin_fabsf(x);
  else return __builtin_fabs(x);
}
#ifndef IDN_SOFT_MED3  // fp32 soft thresholds as d - med3(d, -t, t) (A/B: 0 = compare / copysign)
#define IDN_SOFT_MED3 1
#endif
template <typename T>
__device__ __forceinline__ T clip01_t(T x) {
  if constexpr (sizeof(T) == 4) return __builtin_fminf(__builtin_fmaxf(x, 0.f), 1.f);
  else return __builtin_fmin(__builtin_fmax(x, 0.0), 1.0);
}
template <typename T>
__device__ __forceinline__ T soft_t(T d, T t) {
  // fp32: d - clamp(d, -t, t), one v_med3 and a subtraction -- the same value (d -+ t rounds as
  // |d| - t does, +0 inside the threshold) for the compare / copysign / select of the fp64 form
  if constexpr (sizeof(T) == 4) {
    if (IDN_SOFT_MED3) return d - __builtin_amdgcn_fmed3f(d, -t, t);
    const T m = abs_t<T>(d) - t;
    return m > 0.f ? __builtin_copysignf(m, d) : 0.f;
  } else {
    const T m = abs_t<T>(d) - t;
    return m > 0.0 ? __builtin_copysign(m, d) : 0.0;
  }
}
template <typename T>
__device__ __forceinline__ T dot3_t(T x0, T x1, T x2, T m0, T m1, T m2) {
  return fma_t<T>(x2, m2, fma_t<T>(x1, m1, x0 * m0));
}

template <bool FINAL, typename T = wreal>
__global__ __launch_bounds__(SS_MAXT) void wl_synth_stream(
    wreal* __restrict__ ws, size_t img_floats, const double* __restrict__ stats, int level, int L,
    size_t in_off, int Nh, int Nw, size_t out_off, int Hout, int Wout, size_t out_chan_stride,
    int fmask, int SWo, int strips, int bands, uint8_t* __restrict__ out_u8, int64_t row_stride,
    float* __restrict__ out_f32) {
  __shared__ T SB[2][12][SS_NCOL];  // staged row: [c * 4 + band][column]
  __shared__ T YB[FINAL ? 3 : 1][2][FINAL ? SS_MAXSW : 1];
  __shared__ uint32_t OB[FINAL ? 2 : 1][FINAL ? SS_OBW : 1];
  __shared__ T TH[12];  // soft thresholds by [c * 4 + band] (0 for aa)
  const int img = blockIdx.z;
  const int strip = (int)blockIdx.x % strips, band = (int)blockIdx.x / strips;
  const int x0 = strip * SWo, n0 = x0 / 2;
  const int Mo = (Hout + 1) / 2;  // output row pairs
  const int ma = (int)((int64_t)band * Mo / bands), mb = (int)((int64_t)(band + 1) * Mo / bands);
  const int t = threadIdx.x;
  wreal* base = ws + img * img_floats;
  const double* st = stats + (size_t)img * WL_STATS;
  const size_t bsz = (size_t)Nh * Nw;
  const int ncol = SWo / 2 + 4;
  const int nitems = 12 * ncol;
  // staging items k = t + 256 u -> (band cb, column); items past the end load a valid address
  const wreal* ip[SS_ITEMS];
  int icb[SS_ITEMS], icl[SS_ITEMS];
  uint32_t fb = 0;  // bit u: item u's band is stored fp32
#pragma unroll
  for (int u = 0; u < SS_ITEMS; ++u) {
    const int k = t + SS_MAXT * u;
    const bool ok = k < nitems;
    const int cb = ok ? k / ncol : 0;
    icb[u] = ok ? cb : -1;
    icl[u] = ok ? k - cb * ncol : 0;
    ip[u] = base + in_off + (size_t)cb * bsz;
    fb |= (uint32_t)wl_fband(fmask, cb & 3) << u;
  }
  if (t < 12) TH[t] = (T)((t & 3) ? st[WlStats::thr(t >> 2, level - 1, (t & 3) - 1, L)] : 0.0);
  __syncthreads();
  // coefficients past the band's end feed only outputs past the level's valid length (never
  // stored): clamped reads keep them finite
  auto load = [&](int r, double (&v)[SS_ITEMS], uint32_t& odd) {
    const size_t rb = (size_t)min(r, Nh - 1) * Nw;
    odd = 0;
#pragma unroll
    for (int u = 0; u < SS_ITEMS; ++u) {
      const size_t e = rb + min(n0 + icl[u], Nw - 1);
      const uint32_t f = (fb >> u) & 1u;
      v[u] = ip[u][e >> f];
      odd |= ((uint32_t)e & f) << u;
    }
  };
  // ---- axis roles: thread (c, np)
  const int half = SWo / 2;
  const bool ct = t < 3 * half;
  const int c = ct ? t / half : 0, np = ct ? t - c * half : 0;
  T ring[5][4];  // coefficient rows r-4 .. r of (sa(2np), sa(2np+1), sd(2np), sd(2np+1))
#pragma unroll
  for (int s5 = 0; s5 < 5; ++s5)
#pragma unroll
    for (int q = 0; q < 4; ++q) ring[s5][q] = (T)0;
  T mn = 0, sc = 0;
  bool bad = false;
  if (FINAL) {
    wreal mn64, mx64;
    wl_minmax64(st, c, mn64, mx64);
    sc = (T)(mx64 - mn64);
    mn = (T)mn64;
    bad = st[WlStats::FLAG] != 0.0;
  }
  // FINAL: the strip's U8 row bytes, stored whole dwords when the rows are dword aligned
  const int nb = 3 * min(SWo, Wout - x0);
  const bool al = ((uintptr_t)out_u8 & 3) == 0 && (row_stride & 3) == 0;
  auto flush = [&](int m) {
    if (!out_u8) return;
    const int nw = SWo * 3 / 4;
    for (int k = t; k < 2 * nw; k += SS_MAXT) {
      const int rr2 = k >= nw, d = k - rr2 * nw;
      const int y = 2 * m + rr2;
      if (y >= Hout || 4 * d >= nb) continue;
      uint8_t* orow = out_u8 + ((int64_t)img * Hout + y) * row_stride + (int64_t)x0 * 3;
      const uint32_t wv = OB[rr2][d];
      if (al && 4 * d + 4 <= nb) {
        reinterpret_cast<uint32_t*>(orow)[d] = wv;
      } else {
        for (int bi = 4 * d; bi < min(4 * d + 4, nb); ++bi) orow[bi] = (uint8_t)(wv >> (8 * (bi & 3)));
      }
    }
  };
  const int r0 = ma, R = (mb - ma) + 4;  // coefficient rows r0 .. r0 + R - 1
  double pf[SS_PF][SS_ITEMS];
  uint32_t podd[SS_PF];
#pragma unroll
  for (int f = 0; f < SS_PF; ++f)
    if (f < R) load(r0 + f, pf[f], podd[f]);
  for (int s0 = 0; s0 < R; s0 += SS_PF) {
#pragma unroll
    for (int rs = 0; rs < SS_PF; ++rs) {
      const int sidx = s0 + rs;
      if (sidx >= R) break;
      const int r = r0 + sidx, buf = sidx & 1;
      // stage row r (details soft-thresholded; thr = 0 keeps aa), refill its prefetch slot
#pragma unroll
      for (int u = 0; u < SS_ITEMS; ++u) {
        const wreal x = pf[rs][u];
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
        const float h = __uint_as_float((uint32_t)(((podd[rs] >> u) & 1u) ? bits >> 32 : bits));
        const T xt = ((fb >> u) & 1u) ? (T)h : (T)x;
        if (icb[u] >= 0) SB[buf][icb[u]][icl[u]] = soft_t<T>(xt, TH[icb[u]]);
      }
      if (sidx + SS_PF < R) load(r + SS_PF, pf[rs], podd[rs]);
      __syncthreads();
      if (FINAL && sidx >= 5) flush(r - 5);  // the previous step's U8 rows
      if (ct) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {  // sa: aa (lowpass) / ad (highpass); sd: da / dd
          const T* lo = SB[buf][c * 4 + 2 * pb];
          const T* hi = SB[buf][c * 4 + 2 * pb + 1];
          T cl[5], cd[5];
#pragma unroll
          for (int j = 0; j < 5; ++j) {  // c[j] = column np + 4 - j
            cl[j] = lo[np + 4 - j];
            cd[j] = hi[np + 4 - j];
          }
          synth_bior<T>(cl, cd, ring[4][2 * pb], ring[4][2 * pb + 1]);
        }
      }
      if (sidx >= 4) {
        const int m = r - 4;  // output row pair 2m, 2m+1
        T v[2][2];            // [row][column]
#pragma unroll
        for (int col = 0; col < 2; ++col) {
          T cl[5], cd[5];
#pragma unroll
          for (int j = 0; j < 5; ++j) {  // c[j] = coefficient row m + 4 - j
            cl[j] = ring[4 - j][col];
            cd[j] = ring[4 - j][2 + col];
          }
          synth_bior<T>(cl, cd, v[0][col], v[1][col]);
        }
        if (!FINAL) {
          T* out = reinterpret_cast<T*>(base + out_off + (size_t)c * out_chan_stride);
          const int x = x0 + 2 * np;
#pragma unroll
          for (int rr2 = 0; rr2 < 2; ++rr2) {
            const int y = 2 * m + rr2;
            if (!ct || y >= Hout || x >= Wout) continue;
            T* o = out + (size_t)y * Wout + x;
            if (x + 1 < Wout && ((uintptr_t)o & (2 * sizeof(T) - 1)) == 0) {
              if constexpr (sizeof(T) == 4) *reinterpret_cast<float2*>(o) = make_float2(v[rr2][0], v[rr2][1]);
              else *reinterpret_cast<double2*>(o) = make_double2(v[rr2][0], v[rr2][1]);
            } else {
              o[0] = v[rr2][0];
              if (x + 1 < Wout) o[1] = v[rr2][1];
            }
          }
        } else {
          // inner clip (0.14.2) and de-normalisation
          if (ct) {
#pragma unroll
            for (int rr2 = 0; rr2 < 2; ++rr2)
#pragma unroll
              for (int col = 0; col < 2; ++col)
                YB[c][rr2][2 * np + col] = clip01_t<T>(v[rr2][col]) * sc + mn;
          }
          __syncthreads();
          // pixel pairs: thread q -> row q / half, pixels 2 (q % half), +1
          if (t < 2 * half) {
            const int rr2 = t >= half, pp = t - rr2 * half;
            const int y = 2 * m + rr2;
            uint16_t* ob = reinterpret_cast<uint16_t*>(&OB[rr2][0]) + 3 * pp;
            uint32_t b6[2] = {0u, 0u};  // the pair's 6 bytes
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              const int xx = 2 * pp + p;
              // ycbcr2rgb: (arr - [16,128,128]) @ inv(ycbcr_from_rgb).T (fma-chain dot), clip
              const T Y = YB[0][rr2][xx] - (T)16, Cb = YB[1][rr2][xx] - (T)128,
                      Cr = YB[2][rr2][xx] - (T)128;
              T o3[3];
              o3[0] = dot3_t<T>(Y, Cb, Cr, (T)0.004566210045662101, (T)1.1808799897950177e-09,
                                (T)0.006258928969943937);
              o3[1] = dot3_t<T>(Y, Cb, Cr, (T)0.004566210045662101, (T)-0.0015363236860449021,
                                (T)-0.003188110949655707);
              o3[2] = dot3_t<T>(Y, Cb, Cr, (T)0.004566210045662101, (T)0.007910716233554741,
                                (T)1.1977497040511743e-08);
#pragma unroll
              for (int k3 = 0; k3 < 3; ++k3) {
                T vv = clip01_t<T>(o3[k3]);
                if (bad) vv = (T)0;
                const int bi = 3 * p + k3;
                b6[bi >> 2] |= (uint32_t)(uint8_t)(int)((T)255 * vv) << (8 * (bi & 3));
                if (out_f32 && y < Hout && x0 + xx < Wout)
                  out_f32[(((int64_t)img * Hout + y) * Wout + x0 + xx) * 3 + k3] = (float)vv;
              }
            }
            ob[0] = (uint16_t)b6[0];
            ob[1] = (uint16_t)(b6[0] >> 16);
            ob[2] = (uint16_t)b6[1];
          }
        }
      }
#pragma unroll
      for (int s5 = 0; s5 < 4; ++s5)
#pragma unroll
        for (int q = 0; q < 4; ++q) ring[s5][q] = ring[s5 + 1][q];
    }
  }
  if (FINAL && R >= 5) {
    __syncthreads();
    flush(r0 + R - 5);
  }
}

// ---- 7b (bior1.5): level-1 synthesis, fp32, three channels per thread ----------------------------
// wl_synth_stream<true, float> splits a column pair's three channels over three threads, so the
// YCbCr -> RGB step needs a second barrier per coefficient row (and 48 register moves shift its
// ring).  Here thread np owns output columns 2np, 2np+1 of ALL three channels: one barrier per
// coefficient row, and the five-row ring rotates by index (the loop is unrolled by 10 = lcm(5,
// S3_PF)).  Thread t < SWo/2 + 4 stages coefficient column n0 + t of the 12 (channel, band) rows;
// FM (compile time) says which bands are fp32 in HBM (aa / ad / da; the finest dd is fp64), so each
// thread keeps S3_PF rows of raw loads in flight with no per-item selects.  The U8 rows go through
// an LDS row image flushed as dwords after the next step's barrier.  Arithmetic as
// wl_synth_stream<.., float>.
constexpr int S3_T = 256;
constexpr int S3_MAXSW = 2 * (S3_T - 4);  // 504 output columns per strip
constexpr int S3_PF = 1;                  // coefficient rows in flight ahead of the one staged
inline int s3_strips(int Wout) { return (Wout + S3_MAXSW - 1) / S3_MAXSW; }
inline int s3_sw(int Wout) {
  const int st = s3_strips(Wout);
  return ((Wout + st - 1) / st + 3) & ~3;  // multiple of 4 pixels (12-byte strip starts)
}
template <int FM>
struct S3Raw {  // one coefficient row of one staged column: the 12 (channel, band) values
  float f[3][4];   // fp32 bands, by s3_slot (unused slots are never written)
  double d[3][2];  // fp64 bands
};
template <int FM>
__device__ __forceinline__ constexpr int s3_slot(int b) {  // slot of band b in f (fp32) or d (fp64)
  int k = 0;
  for (int q = 0; q < b; ++q) k += (((FM >> q) & 1) == ((FM >> b) & 1)) ? 1 : 0;
  return k;
}
// FINAL = false (levels >= 2): the same structure without the colour step; the three channels'
// reconstructions go to the level below's 'aa' slots as fp32 (out_off + c * out_chan_stride).
template <int FM, bool FINAL = true>
__global__ __launch_bounds__(S3_T, IDN_S3_WPE) void wl_synth_final3(
    wreal* __restrict__ ws, size_t img_floats, const double* __restrict__ stats, int L,
    size_t in_off, int Nh, int Nw, int Hout, int Wout, int SWo, int strips, int bands,
    uint8_t* __restrict__ out_u8, int64_t row_stride, float* __restrict__ out_f32, int level = 1,
    size_t out_off = 0, size_t out_chan_stride = 0) {
  static_assert(!FINAL || (FM & 0b0110) == 0b0110, "level 1: ad / da fp32");
  __shared__ float SB[2][12][S3_T];                  // staged row: [c * 4 + band][column]
  __shared__ uint32_t OB[FINAL ? 2 : 1][2][FINAL ? S3_MAXSW * 3 / 4 : 1];  // U8 rows (FINAL)
  __shared__ float TH[12];
  const int img = blockIdx.z;
  const int strip = (int)blockIdx.x % strips, band = (int)blockIdx.x / strips;
  const int x0 = strip * SWo, n0 = x0 / 2;
  const int Mo = (Hout + 1) / 2;
  const int ma = (int)((int64_t)band * Mo / bands), mb = (int)((int64_t)(band + 1) * Mo / bands);
  const int t = threadIdx.x;
  const wreal* base = ws + img * img_floats + in_off;
  const double* st = stats + (size_t)img * WL_STATS;
  const size_t bsz = (size_t)Nh * Nw;
  const int half = SWo / 2, ncol = half + 4;
  if (t < 12) TH[t] = (float)((t & 3) ? st[WlStats::thr(t >> 2, level - 1, (t & 3) - 1, L)] : 0.0);
  float mn[3], sc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    wreal a, b;
    wl_minmax64(st, c, a, b);
    mn[c] = (float)a;
    sc[c] = (float)(b - a);
  }
  const bool bad = st[WlStats::FLAG] != 0.0;
  // staging role: coefficient column n0 + t (clamped: columns past the band's end feed only
  // outputs past the valid width, never stored)
  const bool stg = t < ncol;
  const int scol = min(n0 + t, Nw - 1);
  auto load = [&](int r, S3Raw<FM>& R) {
    const size_t e = (size_t)min(r, Nh - 1) * Nw + scol;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const wreal* X = base + (size_t)(c * 4 + b) * bsz;
        if ((FM >> b) & 1) R.f[c][s3_slot<FM>(b)] = reinterpret_cast<const float*>(X)[e];
        else R.d[c][s3_slot<FM>(b)] = X[e];
      }
  };
  // compute role: column pair np (outputs x0 + 2np, +1), all three channels
  const bool cmp = t < half;
  const int np = t;
  float ring[3][5][4];  // [c][slot = coefficient row % 5][sa(2np), sa(2np+1), sd(2np), sd(2np+1)]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5)
#pragma unroll
      for (int q = 0; q < 4; ++q) ring[c][s5][q] = 0.f;
  const int nb = 3 * min(SWo, Wout - x0);  // U8 bytes of the strip's rows
  const bool al = ((uintptr_t)out_u8 & 3) == 0 && (row_stride & 3) == 0;
  auto flush = [&](int m, int ob) {  // output rows 2m, 2m+1 from OB[ob]
    if (!FINAL || !out_u8) return;
    const int nw = (nb + 3) / 4;
    for (int k = t; k < 2 * nw; k += S3_T) {
      const int rr2 = k >= nw, d = k - rr2 * nw;
      const int y = 2 * m + rr2;
      if (y >= Hout) continue;
      uint8_t* orow = out_u8 + ((int64_t)img * Hout + y) * row_stride + (int64_t)x0 * 3;
      const uint32_t wv = OB[ob][rr2][d];
      if (al && 4 * d + 4 <= nb) {
        reinterpret_cast<uint32_t*>(orow)[d] = wv;
      } else {
        for (int bi = 4 * d; bi < min(4 * d + 4, nb); ++bi) orow[bi] = (uint8_t)(wv >> (8 * (bi & 3)));
      }
    }
  };
  __syncthreads();  // TH
  const int r0 = ma, R = (mb - ma) + 4;  // coefficient rows r0 .. r0 + R - 1
  // IDN_S3_PAD (A/B builds): wl_dwt_stream's ring form -- unconditional refills, the last iteration
  // padded instead of left by a break
  S3Raw<FM> pf[S3_PF];
  if (stg || IDN_S3_PAD) {
#pragma unroll
    for (int f = 0; f < S3_PF; ++f)
      if (IDN_S3_PAD || f < R) load(r0 + f, pf[f]);
  }
  for (int s0 = 0; s0 < R; s0 += 10) {
#pragma unroll
    for (int rs = 0; rs < 10; ++rs) {
      const int sidx = s0 + rs;
      if (!IDN_S3_PAD && sidx >= R) break;
      const int r = r0 + sidx, buf = sidx & 1, slot = rs % 5;
      if (stg) {  // stage row r (details soft-thresholded), refill its prefetch slot
        const S3Raw<FM>& q = pf[rs % S3_PF];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const float x = ((FM >> b) & 1) ? q.f[c][s3_slot<FM>(b)] : (float)q.d[c][s3_slot<FM>(b)];
            SB[buf][c * 4 + b][t] = b ? soft_t<float>(x, TH[c * 4 + b]) : x;
          }
        if (!IDN_S3_PAD && sidx + S3_PF < R) load(r + S3_PF, pf[rs % S3_PF]);
      }
      if (IDN_S3_PAD) {
        load(r + S3_PF, pf[rs % S3_PF]);
        if (sidx >= R) continue;
      }
      __syncthreads();
      if (sidx >= 5) flush(r - 5, buf ^ 1);  // the previous step's U8 rows
      if (cmp) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) {  // sa: aa / ad; sd: da / dd
            const float* lo = SB[buf][c * 4 + 2 * pb];
            const float* hi = SB[buf][c * 4 + 2 * pb + 1];
            float cl[5], cd[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {  // c[j] = column np + 4 - j
              cl[j] = lo[np + 4 - j];
              cd[j] = hi[np + 4 - j];
            }
            synth_bior<float>(cl, cd, ring[c][slot][2 * pb], ring[c][slot][2 * pb + 1]);
          }
      }
      if (!FINAL && sidx >= 4 && cmp) {  // reconstruction of the level below, fp32
        const int m = r - 4;
        const int x = x0 + 2 * np;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float v[2][2];  // [row][column]
#pragma unroll
          for (int col = 0; col < 2; ++col) {
            float cl[5], cd[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
              cl[j] = ring[c][(rs + 5 - j) % 5][col];
              cd[j] = ring[c][(rs + 5 - j) % 5][2 + col];
            }
            synth_bior<float>(cl, cd, v[0][col], v[1][col]);
          }
          float* out = reinterpret_cast<float*>(ws + img * img_floats + out_off +
                                                (size_t)c * out_chan_stride);
#pragma unroll
          for (int rr2 = 0; rr2 < 2; ++rr2) {
            const int y = 2 * m + rr2;
            if (y >= Hout || x >= Wout) continue;
            float* o = out + (size_t)y * Wout + x;
            if (x + 1 < Wout && ((uintptr_t)o & 7) == 0) {
              *reinterpret_cast<float2*>(o) = make_float2(v[rr2][0], v[rr2][1]);
            } else {
              o[0] = v[rr2][0];
              if (x + 1 < Wout) o[1] = v[rr2][1];
            }
          }
        }
      }
      if (FINAL && sidx >= 4 && cmp) {
        const int m = r - 4;  // output row pair 2m, 2m+1
        float Yv[3][2][2];    // [c][row][column], de-normalised
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int col = 0; col < 2; ++col) {
            float cl[5], cd[5], v0, v1;
#pragma unroll
            for (int j = 0; j < 5; ++j) {  // c[j] = coefficient row m + 4 - j
              cl[j] = ring[c][(rs + 5 - j) % 5][col];
              cd[j] = ring[c][(rs + 5 - j) % 5][2 + col];
            }
            synth_bior<float>(cl, cd, v0, v1);
            Yv[c][0][col] = clip01_t<float>(v0) * sc[c] + mn[c];
            Yv[c][1][col] = clip01_t<float>(v1) * sc[c] + mn[c];
          }
#pragma unroll
        for (int rr2 = 0; rr2 < 2; ++rr2) {
          const int y = 2 * m + rr2;
          uint32_t b6[2] = {0u, 0u};  // the pair's 6 bytes
          float o6[6];
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const float Y = Yv[0][rr2][p] - 16.f, Cb = Yv[1][rr2][p] - 128.f, Cr = Yv[2][rr2][p] - 128.f;
            float o3[3];
            // (float) of the fp64 constants, as wl_synth_stream (a float literal of the decimal
            // can round differently: double rounding)
            o3[0] = dot3_t<float>(Y, Cb, Cr, (float)0.004566210045662101, (float)1.1808799897950177e-09,
                                  (float)0.006258928969943937);
            o3[1] = dot3_t<float>(Y, Cb, Cr, (float)0.004566210045662101, (float)-0.0015363236860449021,
                                  (float)-0.003188110949655707);
            o3[2] = dot3_t<float>(Y, Cb, Cr, (float)0.004566210045662101, (float)0.007910716233554741,
                                  (float)1.1977497040511743e-08);
#pragma unroll
            for (int k3 = 0; k3 < 3; ++k3) {
              float vv = clip01_t<float>(o3[k3]);
              if (bad) vv = 0.f;
              const int bi = 3 * p + k3;
              o6[bi] = vv;
              b6[bi >> 2] |= (uint32_t)(uint8_t)(int)(255.f * vv) << (8 * (bi & 3));
            }
          }
          uint16_t* ob = reinterpret_cast<uint16_t*>(&OB[buf][rr2][0]) + 3 * np;
          ob[0] = (uint16_t)b6[0];
          ob[1] = (uint16_t)(b6[0] >> 16);
          ob[2] = (uint16_t)b6[1];
          const int x = x0 + 2 * np;
          if (out_f32 && y < Hout && x < Wout) {
            float* o = out_f32 + (((int64_t)img * Hout + y) * Wout + x) * 3;
            if (x + 1 < Wout && ((uintptr_t)o & 7) == 0) {
              reinterpret_cast<float2*>(o)[0] = make_float2(o6[0], o6[1]);
              reinterpret_cast<float2*>(o)[1] = make_float2(o6[2], o6[3]);
              reinterpret_cast<float2*>(o)[2] = make_float2(o6[4], o6[5]);
            } else {
#pragma unroll
              for (int k = 0; k < 6; ++k)
                if (k < 3 || x + 1 < Wout) o[k] = o6[k];
            }
          }
        }
      }
    }
  }
  if (FINAL && R >= 5) {
    __syncthreads();
    flush(r0 + R - 5, (R - 1) & 1);
  }
}

// ---- launchers: streaming forms (bior1.5) -------------------------------------------------------
template <int SRC, typename TL, typename TH, int FM, int CODES>
static void dwt_stream_go(const WlCall& C, const WlLayout& Lt, int l, int emit, int fm) {
  const int sw = ws_sw(Lt.W[l]);
  const int strips = Lt.tiles_x[l], bands = Lt.bands[l], groups = (Lt.H[l] + WS_G - 1) / WS_G;
  const dim3 grid((unsigned)(strips * bands), 1, (unsigned)Lt.n);
  const dim3 blk((unsigned)((2 * sw + 8 + 63) / 64 * 64));
  hipLaunchKernelGGL((wl_dwt_stream<SRC, TL, TH, FM, CODES>), grid, blk, 0, C.st, C.ws,
                     Lt.img_floats, C.stats, l == 1 ? (size_t)0 : Lt.off_band[l - 1], Lt.H[l - 1],
                     Lt.W[l - 1], Lt.off_band[l], Lt.H[l], Lt.W[l], sw, strips, bands, groups,
                     C.src, C.in64, C.row_stride, C.part, Lt.part_per_img, Lt.part_tile0[l], emit,
                     fm, Lt.sq_grid[l]);
}
// The band masks a source can meet, as compile-time constants (fm's bit 4 = WL_FB_AIN chose SRC 3
// and is not the kernel's); anything else through the runtime-mask instance.
template <int SRC, typename TL, typename TH>
static void dwt_stream_pick(const WlCall& C, const WlLayout& Lt, int l, int emit, int fm) {
  const int fmb = fm & 0b1111;
  if constexpr (SRC == 3) {  // fp32 'aa' in: fp32 bands out (all but the coarsest 'aa'), no codes
    if (fmb == 0b1111) dwt_stream_go<3, TL, TH, 0b1111, 0>(C, Lt, l, emit, fm);
    else dwt_stream_go<3, TL, TH, 0b1110, 0>(C, Lt, l, emit, fm);
  } else {
    if constexpr (SRC == 0 || SRC == 1)
      if (fmb == 0b1111 && emit) return dwt_stream_go<SRC, TL, TH, 0b1111, 1>(C, Lt, l, emit, fm);
    if constexpr (SRC == 0) {
      if (fmb == 0b1110 && emit) return dwt_stream_go<0, TL, TH, 0b1110, 1>(C, Lt, l, emit, fm);
#ifdef IDN_TUNING_BUILD  // codes with the level-1 dd in fp64: IDN_WAVELET_DD32=0
      if (fmb == 0b0111 && emit) return dwt_stream_go<0, TL, TH, 0b0111, 1>(C, Lt, l, emit, fm);
      if (fmb == 0b0110 && emit) return dwt_stream_go<0, TL, TH, 0b0110, 1>(C, Lt, l, emit, fm);
#endif
    }
    dwt_stream_go<SRC, TL, TH, -1, -1>(C, Lt, l, emit, fm);
  }
}
// Level 1 reads the image (u8 or f64), normalises in fp64 and keeps the highpass path in fp64
// (the finest dd's exact zeros); its lowpass path, and both paths of the deeper levels (fp32 'aa'
// in), run in fp32.  Level 1 leaves the dd codes for the code median when it will run (codes).
void wl_stream_analysis(const WlCall& C, const WlLayout& Lt, int l, bool codes) {
  const bool dd32 = wl_dd32(true, codes);
  const int fm = wl_fm_analysis(Lt, l, dd32), emit = (l == 1 && codes) ? 1 : 0;
#ifdef IDN_TUNING_BUILD
  // IDN_WAVELET_A32 bit 0: level 1's lowpass path in fp32; bit 1: deeper levels in fp32;
  // bit 2 (with bit 0, u8 input and the code median): level 1's normalisation and highpass
  // in fp32 too, the codes from exact integer keys (wl_dwt_stream's N32; sigma bit-identical
  // by test, but 1041 vs 849 us per 256 images: gfx950 issues fp64 FMA at the fp32 rate, and
  // the key staging adds instructions and registers -- profiles/r06/wavelet/n32_ab.txt)
  const int a32 = knob("IDN_WAVELET_A32", 3);
  const bool f1 = (a32 & 1) != 0, fd = (a32 & 2) != 0;
  if (l > 1 && !(fm & WL_FB_AIN))  // IDN_WAVELET_FDET=0: the level above's 'aa' is fp64
    return fd ? dwt_stream_pick<2, float, float>(C, Lt, l, 0, fm)
              : dwt_stream_pick<2, wreal, wreal>(C, Lt, l, 0, fm);
  if (l > 1 && !fd) return dwt_stream_pick<3, wreal, wreal>(C, Lt, l, 0, fm);
  if (l == 1 && !f1)
    return C.in64 ? dwt_stream_pick<1, wreal, wreal>(C, Lt, 1, emit, fm)
                  : dwt_stream_pick<0, wreal, wreal>(C, Lt, 1, emit, fm);
  if (l == 1 && !C.in64 && (a32 & 4) && emit && dd32)  // N32: codes, dd in fp32 (1110 / 1111)
    return (fm & 1) ? dwt_stream_go<0, float, float, 0b1111, 1>(C, Lt, 1, emit, fm)
                    : dwt_stream_go<0, float, float, 0b1110, 1>(C, Lt, 1, emit, fm);
#endif
  if (l > 1) dwt_stream_pick<3, float, float>(C, Lt, l, 0, fm);
  else if (C.in64) dwt_stream_pick<1, float, wreal>(C, Lt, 1, emit, fm);
  else dwt_stream_pick<0, float, wreal>(C, Lt, 1, emit, fm);
}
// IDN_WAVELET_SSTREAM bit 0: level 1 streams, bit 1: the deeper levels (else the tiled form)
bool wl_stream_synthesis_on(int l) {
  return (tuned("IDN_WAVELET_SSTREAM", 3) & (l == 1 ? 1 : 2)) != 0;
}
// wl_fm_synthesis, and bit 0 where level l + 1's synthesis left its reconstruction in this level's
// 'aa' slot as fp32
int wl_stream_fm_synthesis(const WlLayout& Lt, int l, bool codes) {
  const bool aa32 = l < Lt.L && wl_stream_synthesis_on(l + 1) && tuned("IDN_WAVELET_S32", 1);
  return wl_fm_synthesis(l, wl_dd32(true, codes)) | (aa32 ? 0b0001 : 0);
}
// FINAL: level 1 to the output image; else the reconstruction (fp32) into level l - 1's 'aa' slots
template <int FM, bool FINAL>
static void synth3_go(const WlCall& C, const WlLayout& Lt, int l) {
  const int Hout = Lt.H[l - 1], Wout = Lt.W[l - 1];
  const int strips = s3_strips(Wout), sw = s3_sw(Wout);
  // the band count from the measured residency of one instance per kind
  const void* occ = FINAL ? reinterpret_cast<const void*>(&wl_synth_final3<0b0111, true>)
                          : reinterpret_cast<const void*>(&wl_synth_final3<0b1111, false>);
  const int bands = ss_bands_occ(Lt.n, (Hout + 1) / 2, strips, occ, S3_T);
  hipLaunchKernelGGL((wl_synth_final3<FM, FINAL>), dim3((unsigned)(strips * bands), 1, (unsigned)Lt.n),
                     dim3(S3_T), 0, C.st, C.ws, Lt.img_floats, C.stats, Lt.L, Lt.off_band[l],
                     Lt.H[l], Lt.W[l], Hout, Wout, sw, strips, bands,
                     FINAL ? C.out_u8 : (uint8_t*)nullptr, C.row_stride,
                     FINAL ? C.out_f32 : (float*)nullptr, l, FINAL ? (size_t)0 : Lt.off_band[l - 1],
                     FINAL ? (size_t)0 : (size_t)4 * Hout * Wout);
}
#ifdef IDN_TUNING_BUILD
template <bool FINAL, typename T>
static void synth_stream_go(const WlCall& C, const WlLayout& Lt, int l, int fm) {
  const int Hout = Lt.H[l - 1], Wout = Lt.W[l - 1];
  const int strips = ss_strips(Wout), sw = ss_sw(Wout);
  const int bands = ss_bands_occ(Lt.n, (Hout + 1) / 2, strips,
                                 reinterpret_cast<const void*>(&wl_synth_stream<false, float>), SS_MAXT);
  hipLaunchKernelGGL((wl_synth_stream<FINAL, T>), dim3((unsigned)(strips * bands), 1, (unsigned)Lt.n),
                     dim3(SS_MAXT), 0, C.st, C.ws, Lt.img_floats, C.stats, l, Lt.L, Lt.off_band[l],
                     Lt.H[l], Lt.W[l], FINAL ? (size_t)0 : Lt.off_band[l - 1], Hout, Wout,
                     FINAL ? (size_t)0 : (size_t)4 * Hout * Wout, fm, sw, strips, bands,
                     FINAL ? C.out_u8 : (uint8_t*)nullptr, C.row_stride,
                     FINAL ? C.out_f32 : (float*)nullptr);
}
#endif
// fp32, three channels per thread, the level's band masks as compile-time constants
void wl_stream_synthesis(const WlCall& C, const WlLayout& Lt, int l, bool codes) {
  const int fm = wl_stream_fm_synthesis(Lt, l, codes);
#ifdef IDN_TUNING_BUILD
  // IDN_WAVELET_S32=0: fp64 arithmetic; IDN_WAVELET_S3=0: a channel per thread (wl_synth_stream);
  // IDN_WAVELET_S3D=w: that form too at the deeper levels whose output is narrower than w
  // (measured 2.93 -> 2.85 ms per 256 images for wl_synth_final3 at levels >= 2, and no better
  // with a width floor of 200 or 384: profiles/r03/wavelet/s3d_ab.txt)
  const bool s32 = knob("IDN_WAVELET_S32", 1) != 0;
  const bool s3 = s32 && knob("IDN_WAVELET_S3", 1) != 0 &&
                  (l >= 2 ? Lt.W[l - 1] >= knob("IDN_WAVELET_S3D", 0) && (fm == 0b1111 || fm == 0b1110)
                          : (fm & 0b0110) == 0b0110);
  if (!s3 && l >= 2)
    return s32 ? synth_stream_go<false, float>(C, Lt, l, fm)
               : synth_stream_go<false, wreal>(C, Lt, l, fm);
  if (!s3)
    return s32 ? synth_stream_go<true, float>(C, Lt, 1, fm)
               : synth_stream_go<true, wreal>(C, Lt, 1, fm);
#endif
  if (l >= 2 && fm == 0b1111) synth3_go<0b1111, false>(C, Lt, l);
  else if (l >= 2) synth3_go<0b1110, false>(C, Lt, l);
  else if (fm == 0b1111) synth3_go<0b1111, true>(C, Lt, 1);
  else if (fm == 0b1110) synth3_go<0b1110, true>(C, Lt, 1);
  else if (fm == 0b0111) synth3_go<0b0111, true>(C, Lt, 1);
  else synth3_go<0b0110, true>(C, Lt, 1);
}

}  // namespace idn
