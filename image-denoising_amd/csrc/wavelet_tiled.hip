// Wavelet denoiser, the tiled path: db1 outside the fused Haar path (odd sides, L > 3), one launch
// per level (wavelet.hip has the map of the units).  wl_dwt_rb is the register-blocked analysis
// tile, wl_synth / wl_synth_final the LDS-tiled separable synthesis.  Entered through
// wl_tiled_analysis and wl_tiled_synthesis, both called by wl_run.
#include "wavelet_common.hpp"

namespace idn {

// ---- 2: one analysis level ----------------------------------------------------------------------

// Register-blocked analysis tile: RB_TY x RB_TX output coefficients per band, all three channels
// in one 256-thread workgroup.
//   axis 0: thread (c, q) owns staged input column q of channel c (3 x NX threads); it loads the
//           NY input samples of its column (u8 / f64 pixels normalised on the fly, or the level
//           above's 'aa' plane), all loads in flight at once, and runs the F-tap lowpass and
//           highpass down the column in registers into S.vl / S.vh.
//   axis 1: thread (c, ii, group) computes R consecutive output columns of all four bands from
//           2R + F - 2 staged values of S.vl and S.vh (wave w = channel w).
//   the four bands go out through LDS (reusing vl / vh) as whole rows, so each wave's stores are
//   contiguous (register-blocked lanes stored 8-byte pieces at a 32-byte stride: 4x the L2 write
//   requests).
// LDS traffic is ~10 accesses per input pixel (round 1's per-output gathers: ~42).
template <int WV>
struct DwtRB {
  static constexpr int F = Wav<WV>::F;
  static constexpr int NX = 2 * RB_TX + F - 2;  // staged input columns
  static constexpr int NY = 2 * RB_TY + F - 2;  // input rows per column
  // row stride: odd (the 8 rows of a 32-lane read fall on distinct banks) and large enough for
  // vl + vh to hold the band staging buffer
  static constexpr int NXP = (NX + 1 > 2 * (RB_TX + 1) ? NX + 1 : 2 * (RB_TX + 1)) | 1;
  wreal vl[3][RB_TY][NXP], vh[3][RB_TY][NXP];
};
static_assert(3 * RB_TY * (RB_TX / RB_R) == 192, "axis-1 items: one per thread of waves 0-2");
constexpr int RB_OBS = RB_TX + 1;  // band staging row stride (doubles): conflict-free b64 stores


// SRC: 0 = u8 image, 1 = f64 image (level 1, normalised per channel), 2 = the 'aa' planes of the
// level above (levels >= 2; wl_dwt_stream: 2 fp64, 3 fp32).  Grid (tiles, 1, n).
template <int WV, int SRC>
__global__ __launch_bounds__(256) void wl_dwt_rb(wreal* __restrict__ ws, size_t img_floats,
                                                 const double* __restrict__ stats, size_t in_off,
                                                 int Hin, int Win, size_t out_off, int Ho, int Wo,
                                                 int tiles_x, const uint8_t* __restrict__ src,
                                                 const double* __restrict__ in64,
                                                 int64_t row_stride, double* __restrict__ part,
                                                 size_t part_per_img, size_t part_tile0,
                                                 int emit_codes, int fmask, int coop) {
  using Wv = Wav<WV>;
  constexpr int F = Wv::F, NX = DwtRB<WV>::NX, NY = DwtRB<WV>::NY;
  __shared__ DwtRB<WV> S;
  const int img = blockIdx.z;
  wreal* base = ws + img * img_floats;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int i0 = ti * RB_TY, j0 = tj * RB_TX;
  const int r0 = 2 * i0 + 2 - F, q0 = 2 * j0 + 2 - F;  // input coordinate of staged [0][0]
  const int t = threadIdx.x;
  wreal x[NY];
  // u8 input, cooperative form (IDN_WAVELET_COOP, default on): every staged pixel is loaded and
  // normalised once for its three channels by one of the 256 threads, through LDS in two halves
  // of rows (aliasing vl / vh), instead of once per channel by the three (channel, column)
  // threads -- the same fp64 operations per sample, a third of the u8 -> fp64 conversions
  const bool coop_u8 = SRC == 0 && coop;
  if (coop_u8) {
    constexpr int HR = NY / 2;  // NY = 2 RB_TY + F - 2 is even
    constexpr int IT = (HR * NX + 255) / 256;
    static_assert(sizeof(S) >= sizeof(wreal) * 3 * HR * NX, "normalised half fits in vl + vh");
    wreal(*nz)[HR][NX] = reinterpret_cast<wreal(*)[HR][NX]>(&S.vl[0][0][0]);
    const double* st = stats + (size_t)img * WL_STATS;
    wreal mn[3], inv[3], rcp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wreal mx;
      wl_minmax64(st, c, mn[c], mx);
      inv[c] = mx - mn[c];
      rcp[c] = 1.0 / inv[c];
    }
    const uint8_t* im = src + (int64_t)img * Hin * row_stride;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      uint32_t raw[IT];
#pragma unroll
      for (int it = 0; it < IT; ++it) {  // all loads in flight before any use
        const int k = t + 256 * it, rr = k / NX, q = k - rr * NX;
        raw[it] = 0;
        if (k < HR * NX) {
          const uint8_t* p = im + (int64_t)sym_idx(r0 + hf * HR + rr, Hin) * row_stride +
                             (int64_t)sym_idx(q0 + q, Win) * 3;
          raw[it] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
      }
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int k = t + 256 * it, rr = k / NX, q = k - rr * NX;
        if (k < HR * NX) {
          double px[3];
#pragma unroll
          for (int kk = 0; kk < 3; ++kk)
            px[kk] = (double)((raw[it] >> (8 * kk)) & 0xFFu) * (1.0 / 255.0);
#pragma unroll
          for (int c = 0; c < 3; ++c) {  // as the per-channel form below, op for op
            const wreal a = ycbcr_c(px, c) - mn[c];
            const wreal qq = a * rcp[c];
            nz[c][rr][q] = __fma_rn(__fma_rn(-qq, inv[c], a), rcp[c], qq);
          }
        }
      }
      __syncthreads();
      if (t < 3 * NX) {
        const int c = t / NX, q = t - c * NX;
#pragma unroll
        for (int rr = 0; rr < HR; ++rr) x[hf * HR + rr] = nz[c][rr][q];
      }
      __syncthreads();  // nz is rewritten by the next half / becomes vl / vh
    }
  }
  if (t < 3 * NX) {
    const int c = t / NX, q = t - c * NX;
    const int xx = sym_idx(q0 + q, Win);
    if (coop_u8) {
      // x holds the column already
    } else if (SRC == 2) {
      if (fmask & WL_FB_AIN) {  // the level above stored its 'aa' as fp32
        const float* X = reinterpret_cast<const float*>(base + in_off + (size_t)c * 4 * Hin * Win) + xx;
#pragma unroll
        for (int r = 0; r < NY; ++r) x[r] = (wreal)X[(size_t)sym_idx(r0 + r, Hin) * Win];
      } else {
        const wreal* X = base + in_off + (size_t)c * 4 * Hin * Win + xx;
#pragma unroll
        for (int r = 0; r < NY; ++r) x[r] = X[(size_t)sym_idx(r0 + r, Hin) * Win];
      }
    } else {
      const double* st = stats + (size_t)img * WL_STATS;
      wreal mn, mx;
      wl_minmax64(st, c, mn, mx);
      const wreal inv = mx - mn, rcp = 1.0 / inv;
      if (SRC == 0) {
        const uint8_t* col = src + (int64_t)img * Hin * row_stride + (int64_t)xx * 3;
        uint32_t raw[NY];
#pragma unroll
        for (int r = 0; r < NY; ++r) {  // all loads in flight before any use
          const uint8_t* p = col + (int64_t)sym_idx(r0 + r, Hin) * row_stride;
          raw[r] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
#pragma unroll
        for (int r = 0; r < NY; ++r) {
          double px[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) px[k] = (double)((raw[r] >> (8 * k)) & 0xFFu) * (1.0 / 255.0);
          // skimage: channel = out - min; channel /= max - min, as the IEEE quotient (reciprocal
          // multiply + one Markstein correction, exact over every u8 triple: tools/check_div.c)
          const wreal a = ycbcr_c(px, c) - mn;
          const wreal qq = a * rcp;
          x[r] = __fma_rn(__fma_rn(-qq, inv, a), rcp, qq);
        }
      } else {
        double px[NY][3];
#pragma unroll
        for (int r = 0; r < NY; ++r)
          load_rgb64(src, in64, img, Hin, Win, row_stride, sym_idx(r0 + r, Hin), xx, px[r]);
#pragma unroll
        for (int r = 0; r < NY; ++r) x[r] = (ycbcr_c(px[r], c) - mn) / inv;
      }
    }
    // axis 0 first (pywt dwtn order): output row ii uses staged rows 2ii + F-1-p
#pragma unroll
    for (int ii = 0; ii < RB_TY; ++ii) {
      wreal lo = 0, hi = 0;
#pragma unroll
      for (int p = 0; p < F; ++p) {
        const wreal v = x[2 * ii + F - 1 - p];
        // the highpass keeps pywt's mul-then-add (dd's exact zeros feed the sigma median); the
        // lowpass only reaches aa / ad / da, whose rounding the thresholds and the synthesis
        // absorb (1e-16 relative), so it takes fmas
        if (Wv::dlo[p] != 0) lo = __fma_rn(Wv::dlo[p], v, lo);
        if (Wv::dhi[p] != 0) hi = __dadd_rn(hi, __dmul_rn(Wv::dhi[p], v));  // pywt: mul, then add
      }
      S.vl[c][ii][q] = lo;
      S.vh[c][ii][q] = hi;
    }
  }
  __syncthreads();
  // wave = channel (waves 0-2); lane bits [5] g / 4, [4:2] ii, [1:0] g % 4: a 32-lane half reads
  // 8 rows x 4 column groups, whose ds_read_b64 addresses (row stride NX + 1, 8 doubles per
  // group) fall on distinct bank pairs (lanes g / g + 4 of one row were 2-way conflicts)
  const int c = t >> 6, ii = (t >> 2) & 7, g = ((t >> 5) & 1) * 4 + (t & 3);
  const int i = i0 + ii, jl = g * RB_R;
  constexpr int NC = 2 * RB_R + F - 2;  // staged columns one thread reads
  wreal l[NC], h[NC];
  if (t < 192) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      l[k] = S.vl[c][ii][2 * jl + k];
      h[k] = S.vh[c][ii][2 * jl + k];
    }
  }
  __syncthreads();  // vl / vh become the output staging buffer
  // rows padded to RB_OBS = RB_TX + 1 doubles: the 16 lanes of a ds_write_b64 group (4 rows x 4
  // column groups) hit distinct bank pairs (an unpadded stride made them 4-way conflicts)
  static_assert(sizeof(S) >= sizeof(wreal) * 3 * 4 * RB_TY * RB_OBS, "band staging fits");
  wreal(*ob)[4][RB_TY][RB_OBS] = reinterpret_cast<wreal(*)[4][RB_TY][RB_OBS]>(&S.vl[0][0][0]);
  double sq[3] = {0.0, 0.0, 0.0};
  if (t < 192) {
#pragma unroll
  for (int r = 0; r < RB_R; ++r) {
    wreal aa = 0, ad = 0, da = 0, dd = 0;
#pragma unroll
    for (int qq = 0; qq < F; ++qq) {  // then axis 1: output column j uses staged cols 2j + F-1-q
      const wreal lv = l[2 * r + F - 1 - qq], hv = h[2 * r + F - 1 - qq];
      if (Wv::dlo[qq] != 0) {
        aa = __fma_rn(Wv::dlo[qq], lv, aa);  // key 'aa': axis 0 low, axis 1 low
        da = __fma_rn(Wv::dlo[qq], hv, da);  // key 'da': axis 0 high, axis 1 low
      }
      if (Wv::dhi[qq] != 0) {
        ad = __fma_rn(Wv::dhi[qq], lv, ad);                 // key 'ad': axis 0 low, axis 1 high
        dd = __dadd_rn(dd, __dmul_rn(Wv::dhi[qq], hv));  // pywt's order: exact zeros
      }
    }
    // level 1: the fine-bin code of |dd| (0: exact zero) for the sigma median
    // (wl_haar_median<BAND>), in this channel's unused input-plane slot
    if (emit_codes && i < Ho && j0 + jl + r < Wo) {
      const unsigned long long key = absbits(dd);
      reinterpret_cast<uint16_t*>(base + (size_t)c * Hin * Win)[(size_t)i * Wo + j0 + jl + r] =
          (uint16_t)(key ? wl_fbin(key) + 1 : 0);
    }
    ob[c][0][ii][jl + r] = aa;
    ob[c][1][ii][jl + r] = ad;
    ob[c][2][ii][jl + r] = da;
    ob[c][3][ii][jl + r] = dd;
    if (i < Ho && j0 + jl + r < Wo) {
      sq[0] += ad * ad;
      sq[1] += da * da;
      sq[2] += dd * dd;
    }
  }
  // per-tile sums of squares of the three detail bands of this wave's channel, fixed order
  // (wl_sumsq adds the tiles)
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    double v = sq[b];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((t & 63) == 0)
      part[img * part_per_img + (size_t)(c * 3 + b) * (part_per_img / 9) + part_tile0 +
           blockIdx.x] = v;
  }
  }
  __syncthreads();
  // coalesced band stores: rows of RB_TX coefficients, 16 lanes x 16 bytes per row; fp32 bands
  // (fmask) in the first half of their slot
  const size_t bsz = (size_t)Ho * Wo;
  constexpr int PR = RB_TX / 2;  // coefficient pairs per row
  for (int k = t; k < 3 * 4 * RB_TY * PR; k += 256) {
    const int row = k / PR, pr = k - row * PR;  // row = (c * 4 + band) * RB_TY + ii
    const int cb = row / RB_TY, iy = row - cb * RB_TY;  // wave-uniform (4 rows of one band)
    const int oi = i0 + iy, oj = j0 + 2 * pr;
    if (oi >= Ho || oj >= Wo) continue;
    const wreal* sv = &ob[0][0][0][0] + (size_t)row * RB_OBS + 2 * pr;
    if (wl_fband(fmask, cb & 3)) {
      float* dst = reinterpret_cast<float*>(base + out_off + (size_t)cb * bsz) + (size_t)oi * Wo + oj;
      dst[0] = (float)sv[0];
      if (oj + 1 < Wo) dst[1] = (float)sv[1];
    } else {
      wreal* dst = base + out_off + (size_t)cb * bsz + (size_t)oi * Wo + oj;
      dst[0] = sv[0];
      if (oj + 1 < Wo) dst[1] = sv[1];
    }
  }
}

// ---- 6/7: synthesis, LDS-tiled and separable ---------------------------------------------------
// One workgroup per ST_O x ST_O output tile of the level being synthesised: it stages the
// (ST_O/2 + HF-1)^2 coefficients of the four bands the tile needs (details soft-thresholded on
// load), runs pywt idwtn's axis-1 pass into LDS ('a' from
// aa/ad, 'd' from da/dd) and then the axis-0 pass, each as upsampling_convolution_valid_sf's
// sum_even / sum_odd (lowpass sum + highpass sum, multiply then add, zero taps skipped); each
// thread computes an output pair from one set of HF coefficients.
// Levels L..2 write the approximation of the level below (cropped to its size); level 1
// (FINAL) runs the three channels of the tile in turn and fuses the inner clip [0, 1],
// de-normalisation, YCbCr -> RGB, the outer clip and the U8 / f32 stores.
// Round 1's per-pixel form gathered 36 coefficients per channel and pixel from L2 (7.0 ms per
// 256 bior1.5 images for the last level alone).
constexpr int ST_O = 32;

template <int WV>
struct SynthTile {
  static constexpr int F = Wav<WV>::F, HF = F / 2;
  static constexpr int CR = ST_O / 2 + HF - 1;  // staged coefficient rows / cols
  wreal co[4][CR][CR + 1];
  wreal sa[CR][ST_O + 1], sd[CR][ST_O + 1];
};

// one upsampling_convolution_valid_sf output pair (even, odd) from the HF coefficients
// c[j] = x[i - j]: lowpass part of the even / odd filter taps, multiply then add, zero taps
// skipped (they add +-0)
template <int WV, bool HI>
__device__ __forceinline__ void synth_pair(const wreal (&c)[Wav<WV>::F / 2], wreal& ev, wreal& od) {
  using Wv = Wav<WV>;
  constexpr int HF = Wv::F / 2;
  ev = 0;
  od = 0;
#pragma unroll
  for (int j = 0; j < HF; ++j) {
    const wreal fe = HI ? Wv::rhi[2 * j] : Wv::rlo[2 * j];
    const wreal fo = HI ? Wv::rhi[2 * j + 1] : Wv::rlo[2 * j + 1];
    if (fe != 0) ev = __dadd_rn(ev, __dmul_rn(fe, c[j]));
    if (fo != 0) od = __dadd_rn(od, __dmul_rn(fo, c[j]));
  }
}

// synthesise one channel's tile (bands at A, band size Nh x Nw, coefficient origin (m0, n0));
// thread t receives the tile outputs (row 2 * (t / ST_O) + r, column t % ST_O) for the row pairs
// of i (v[2 i + r]).  Split in two so a caller can keep the next channel's loads in flight while
// this one is synthesised: synth_load issues the thread's staging loads, synth_run stages them
// (details soft-thresholded) and runs the two passes.
template <int WV>
struct SynthLoad {
  static constexpr int CR = SynthTile<WV>::CR;
  static constexpr int RPT = 256 / CR;            // staging: band rows per pass (CR columns each)
  static constexpr int NRW = 4 * CR;              // band rows to stage
  static constexpr int NLD = (NRW + RPT - 1) / RPT;
  static_assert(NLD <= 32, "odd-index bits");
  wreal x[NLD];
  uint32_t odd;  // bit u set when x[u] holds an fp32 band pair whose odd element is wanted
};
template <int WV>
__device__ __forceinline__ void synth_load(SynthLoad<WV>& L, const wreal* __restrict__ A,
                                           size_t bsz, int Nh, int Nw, int m0, int n0, int fmask) {
  using SL = SynthLoad<WV>;
  const int cc = threadIdx.x % SL::CR, rr0 = threadIdx.x / SL::CR;
  // coefficients past the band's end feed only outputs past the level's valid length (pywt's
  // stage-2 valid convolution), which are never stored: clamped reads keep them finite
  const int col = min(n0 + cc, Nw - 1);
  L.odd = 0;
#pragma unroll
  for (int u = 0; u < SL::NLD; ++u) {  // all loads in flight before any use
    const int br = min(rr0 + SL::RPT * u, SL::NRW - 1);  // band * CR + row
    const int b = br / SL::CR, r = br - b * SL::CR;
    const size_t e = (size_t)min(m0 + r, Nh - 1) * Nw + col;
    // an fp32 band is read as the 8-byte pair holding element e (the same dwordx2 load for every
    // lane; the band's unique bytes halve), the half is picked in synth_run
    const bool f = wl_fband(fmask, b);
    L.x[u] = A[(size_t)b * bsz + (f ? e >> 1 : e)];
    if (f) L.odd |= (uint32_t)(e & 1) << u;
  }
}
// one output pair of the full synthesis step, lowpass band coefficients cl[j] and highpass
// cd[j] (c[j] = x[i - j]), written to (ev, od).  Haar / generic: pywt's sums (synth_pair).
// bior1.5: rlo has the two taps S2 (even, odd) at j = 2, and rhi's even / odd taps are
// B1, -B2, +-S2, B2, -B1, so with common = B1 (d0 - d4) + B2 (d3 - d1)
//   ev = common + S2 (a + d2),  od = common + S2 (a - d2)      (a = cl[2], d = cd)
// 8 operations for the pair instead of pywt's 26; the rounding differs from pywt's by a few ulps
// (the synthesis is checked within 1e-5, and no exact zero depends on it).
template <int WV>
__device__ __forceinline__ void synth_full(const wreal (&cl)[Wav<WV>::F / 2],
                                           const wreal (&cd)[Wav<WV>::F / 2], wreal& ev,
                                           wreal& od) {
  if constexpr (WV == IDN_WAVELET_BIOR15) {
    const wreal common = __fma_rn(B1, cd[0] - cd[4], B2 * (cd[3] - cd[1]));
    ev = __fma_rn(S2, cl[2] + cd[2], common);
    od = __fma_rn(S2, cl[2] - cd[2], common);
  } else {
    wreal le, lo, he, ho;
    synth_pair<WV, false>(cl, le, lo);
    synth_pair<WV, true>(cd, he, ho);
    ev = __dadd_rn(le, he);
    od = __dadd_rn(lo, ho);
  }
}

template <int WV, typename Between>
__device__ __forceinline__ void synth_run(SynthTile<WV>& S, const SynthLoad<WV>& L,
                                          const wreal (&thr)[3], wreal (&v)[ST_O * ST_O / 256],
                                          int fmask, Between between) {
  using SL = SynthLoad<WV>;
  constexpr int HF = SynthTile<WV>::HF, CR = SL::CR;
  const int cc = threadIdx.x % CR, rr0 = threadIdx.x / CR;
#pragma unroll
  for (int u = 0; u < SL::NLD; ++u) {
    const int br = rr0 + SL::RPT * u;
    if (rr0 < SL::RPT && br < SL::NRW) {
      const int b = br / CR, r = br - b * CR;
      wreal x = L.x[u];
      if (wl_fband(fmask, b)) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
        x = (wreal)__uint_as_float((uint32_t)(((L.odd >> u) & 1u) ? bits >> 32 : bits));
      }
      S.co[b][r][cc] = b > 0 ? soft(x, thr[b - 1]) : x;
    }
  }
  __syncthreads();
  between();  // the staged registers are free: e.g. the next channel's loads
  for (int k = threadIdx.x; k < CR * (ST_O / 2); k += 256) {  // axis 1: column pairs
    const int r = k / (ST_O / 2), nn = k - r * (ST_O / 2);
    wreal c0[HF], c1[HF], c2[HF], c3[HF];
#pragma unroll
    for (int j = 0; j < HF; ++j) {
      const int col = nn + HF - 1 - j;
      c0[j] = S.co[0][r][col];
      c1[j] = S.co[1][r][col];
      c2[j] = S.co[2][r][col];
      c3[j] = S.co[3][r][col];
    }
    synth_full<WV>(c0, c1, S.sa[r][2 * nn], S.sa[r][2 * nn + 1]);
    synth_full<WV>(c2, c3, S.sd[r][2 * nn], S.sd[r][2 * nn + 1]);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < ST_O * ST_O / 512; ++i) {  // axis 0: row pairs
    const int k = threadIdx.x + 256 * i;
    const int m = k / ST_O, q = k - m * ST_O;
    wreal ca[HF], cd[HF];
#pragma unroll
    for (int j = 0; j < HF; ++j) {
      ca[j] = S.sa[m + HF - 1 - j][q];
      cd[j] = S.sd[m + HF - 1 - j][q];
    }
    synth_full<WV>(ca, cd, v[2 * i], v[2 * i + 1]);
  }
  __syncthreads();  // S is restaged by the next call
}
template <int WV>
__device__ __forceinline__ void synth_tile(SynthTile<WV>& S, const wreal* __restrict__ A,
                                           size_t bsz, int Nh, int Nw, int m0, int n0,
                                           const wreal (&thr)[3], wreal (&v)[ST_O * ST_O / 256],
                                           int fmask) {
  SynthLoad<WV> L;
  synth_load<WV>(L, A, bsz, Nh, Nw, m0, n0, fmask);
  synth_run<WV>(S, L, thr, v, fmask, [] {});
}
// output position of v[e] of thread t: (row, column) inside the tile
__device__ __forceinline__ int synth_row(int e) {
  return 2 * ((threadIdx.x + 256 * (e >> 1)) / ST_O) + (e & 1);
}
__device__ __forceinline__ int synth_col(int e) { return (threadIdx.x + 256 * (e >> 1)) % ST_O; }

// levels L..2: grid (tiles, n * 3); the level-(l-1) 'aa' slot receives the reconstruction
template <int WV>
__global__ __launch_bounds__(256) void wl_synth(wreal* __restrict__ ws, size_t img_floats,
                                                const double* __restrict__ stats, int level, int L,
                                                size_t in_off, int Nh, int Nw, size_t out_off,
                                                int Hout, int Wout, size_t out_chan_stride,
                                                int tiles_x, int fmask) {
  __shared__ SynthTile<WV> S;
  const int img = blockIdx.y / 3, c = blockIdx.y % 3;
  wreal* base = ws + img * img_floats;
  const size_t bsz = (size_t)Nh * Nw;
  const double* st = stats + (size_t)img * WL_STATS;
  const wreal thr[3] = {st[WlStats::thr(c, level - 1, 0, L)], st[WlStats::thr(c, level - 1, 1, L)],
                        st[WlStats::thr(c, level - 1, 2, L)]};
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int p0 = ti * ST_O, q0 = tj * ST_O;
  wreal v[ST_O * ST_O / 256];
  synth_tile<WV>(S, base + in_off + (size_t)c * 4 * bsz, bsz, Nh, Nw, p0 / 2, q0 / 2, thr, v, fmask);
  wreal* out = base + out_off + (size_t)c * out_chan_stride;
#pragma unroll
  for (int i = 0; i < ST_O * ST_O / 256; ++i) {
    const int p = p0 + synth_row(i), q = q0 + synth_col(i);
    if (p < Hout && q < Wout) out[(size_t)p * Wout + q] = v[i];
  }
}

// level 1 of all three channels + colour + casts: grid (tiles, n)
template <int WV>
__global__ __launch_bounds__(256) void wl_synth_final(const wreal* __restrict__ ws,
                                                      size_t img_floats,
                                                      const double* __restrict__ stats, int L,
                                                      size_t in_off, int Nh, int Nw, int h, int w,
                                                      int tiles_x, uint8_t* __restrict__ out_u8,
                                                      int64_t row_stride,
                                                      float* __restrict__ out_f32, int fmask) {
  __shared__ SynthTile<WV> S;
  __shared__ uint32_t obuf[ST_O][ST_O * 3 / 4];  // the tile's U8 BGR rows
  constexpr int NV = ST_O * ST_O / 256;
  const int img = blockIdx.y;
  const wreal* base = ws + img * img_floats + in_off;
  const size_t bsz = (size_t)Nh * Nw;
  const double* st = stats + (size_t)img * WL_STATS;
  const bool bad = st[WlStats::FLAG] != 0.0;
  const int ti = blockIdx.x / tiles_x, tj = blockIdx.x - ti * tiles_x;
  const int p0 = ti * ST_O, q0 = tj * ST_O;
  double ych[3][NV];
  // channel c + 1's coefficient loads are issued as soon as channel c is staged in LDS, so they
  // are in flight while channel c is synthesised (the level-1 synthesis is bound by these fp64
  // reads: 37.5 B per output pixel)
  SynthLoad<WV> ld;
  synth_load<WV>(ld, base, bsz, Nh, Nw, p0 / 2, q0 / 2, fmask);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    wreal mn, mx;
    wl_minmax64(st, c, mn, mx);
    const wreal sc = mx - mn;
    const wreal thr[3] = {st[WlStats::thr(c, 0, 0, L)], st[WlStats::thr(c, 0, 1, L)],
                          st[WlStats::thr(c, 0, 2, L)]};
    wreal v[NV];
    synth_run<WV>(S, ld, thr, v, fmask, [&] {
      if (c < 2)
        synth_load<WV>(ld, base + (size_t)(c + 1) * 4 * bsz, bsz, Nh, Nw, p0 / 2, q0 / 2, fmask);
    });
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      // inner denoise_wavelet clip (0.14.2), then * (max - min) + min
      const double x = fmin(fmax((double)v[i], 0.0), 1.0);
      const double yv = x * sc + mn;
      if (c == 0) ych[0][i] = yv;  // (selects: no dynamic register indexing)
      else if (c == 1) ych[1][i] = yv;
      else ych[2][i] = yv;
    }
  }
  uint8_t* ob = reinterpret_cast<uint8_t*>(&obuf[0][0]);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int y = p0 + synth_row(i), x = q0 + synth_col(i);
    // ycbcr2rgb: (arr - [16,128,128]) @ inv(ycbcr_from_rgb).T (numpy.linalg.inv, full precision,
    // fma-chain dot as numpy's matmul), then clip [0, 1]
    const double Y = ych[0][i] - 16.0, Cb = ych[1][i] - 128.0, Cr = ych[2][i] - 128.0;
    double o3[3];
    o3[0] = dot3(Y, Cb, Cr, 0.004566210045662101, 1.1808799897950177e-09, 0.006258928969943937);
    o3[1] = dot3(Y, Cb, Cr, 0.004566210045662101, -0.0015363236860449021, -0.003188110949655707);
    o3[2] = dot3(Y, Cb, Cr, 0.004566210045662101, 0.007910716233554741, 1.1977497040511743e-08);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double vv = fmin(fmax(o3[c], 0.0), 1.0);
      if (bad) vv = 0.0;
      ob[synth_row(i) * (ST_O * 3) + synth_col(i) * 3 + c] = (uint8_t)(int)(255.0 * vv);
      if (out_f32 && y < h && x < w) out_f32[(((int64_t)img * h + y) * w + x) * 3 + c] = (float)vv;
    }
  }
  if (!out_u8) return;
  __syncthreads();
  uint8_t* orow = out_u8 + (int64_t)img * h * row_stride + (int64_t)q0 * 3;
  if (q0 + ST_O <= w && ((uintptr_t)orow & 3) == 0 && (row_stride & 3) == 0) {
    for (int k = threadIdx.x; k < ST_O * ST_O * 3 / 4; k += 256) {  // whole dwords of full rows
      const int r = k / (ST_O * 3 / 4), d = k - r * (ST_O * 3 / 4);
      if (p0 + r < h)
        reinterpret_cast<uint32_t*>(orow + (int64_t)(p0 + r) * row_stride)[d] = obuf[r][d];
    }
  } else {
    for (int k = threadIdx.x; k < ST_O * ST_O * 3; k += 256) {
      const int r = k / (ST_O * 3), b = k - r * (ST_O * 3);
      if (p0 + r < h && q0 + b / 3 < w) orow[(int64_t)(p0 + r) * row_stride + b] = ob[r * (ST_O * 3) + b];
    }
  }
}

// ---- launchers: tiled forms ---------------------------------------------------------------------
template <int SRC>
static void dwt_rb_go(const WlCall& C, const WlLayout& Lt, int l, int emit_codes, int fmask,
                      int coop) {
  hipLaunchKernelGGL((wl_dwt_rb<IDN_WAVELET_DB1, SRC>), dim3(Lt.tiles[l], 1, Lt.n), dim3(256), 0,
                     C.st, C.ws, Lt.img_floats, C.stats, l == 1 ? (size_t)0 : Lt.off_band[l - 1],
                     Lt.H[l - 1], Lt.W[l - 1], Lt.off_band[l], Lt.H[l], Lt.W[l], Lt.tiles_x[l],
                     C.src, C.in64, C.row_stride, C.part, Lt.part_per_img, Lt.part_tile0[l],
                     emit_codes, fmask, coop);
}
// level 1 leaves the dd codes for the code median when it will run (codes)
void wl_tiled_analysis(const WlCall& C, const WlLayout& Lt, int l, bool codes) {
  const int fmask = wl_fm_analysis(Lt, l, false);
  const int coop = tuned("IDN_WAVELET_COOP", 1) ? 1 : 0;  // u8 level 1: cooperative staging
  if (l > 1) dwt_rb_go<2>(C, Lt, l, 0, fmask, coop);
  else if (C.in64) dwt_rb_go<1>(C, Lt, 1, codes ? 1 : 0, fmask, coop);
  else dwt_rb_go<0>(C, Lt, 1, codes ? 1 : 0, fmask, coop);
}
// level l >= 2: the level-(l-1) 'aa' slot (consumed by the analysis already) receives the
// reconstruction; level 1: the output image
template <int WV>
static void synth_tile_go(const WlCall& C, const WlLayout& Lt, int l, int fmask) {
  const int Hout = Lt.H[l - 1], Wout = Lt.W[l - 1];
  const int tx = (Wout + ST_O - 1) / ST_O, ty = (Hout + ST_O - 1) / ST_O;
  if (l >= 2)
    hipLaunchKernelGGL((wl_synth<WV>), dim3(tx * ty, Lt.n * 3), dim3(256), 0, C.st, C.ws,
                       Lt.img_floats, C.stats, l, Lt.L, Lt.off_band[l], Lt.H[l], Lt.W[l],
                       Lt.off_band[l - 1], Hout, Wout, (size_t)4 * Hout * Wout, tx, fmask);
  else
    hipLaunchKernelGGL((wl_synth_final<WV>), dim3(tx * ty, Lt.n), dim3(256), 0, C.st, C.ws,
                       Lt.img_floats, C.stats, Lt.L, Lt.off_band[1], Lt.H[1], Lt.W[1], Lt.h, Lt.w,
                       tx, C.out_u8, C.row_stride, C.out_f32, fmask);
}
void wl_tiled_synthesis(const WlCall& C, const WlLayout& Lt, int l, int fmask, int wavelet) {
#ifdef IDN_TUNING_BUILD  // bior1.5 comes here only by IDN_WAVELET_SSTREAM
  if (wavelet == IDN_WAVELET_BIOR15) return synth_tile_go<IDN_WAVELET_BIOR15>(C, Lt, l, fmask);
#endif
  synth_tile_go<IDN_WAVELET_DB1>(C, Lt, l, fmask);
}

}  // namespace idn
