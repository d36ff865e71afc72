// Wavelet denoiser, sigma = median(|finest dd| != 0) / ppf(0.75) in its two general forms:
// wl_median (radix select over the fp64 band) and wl_haar_median (over the analysis' dd codes),
// with the device helpers they share with wl_haar_stats (wavelet_haar.hip) and wl_h3_sigma
// (haar3.hpp): the rank selection on an LDS histogram, and the exact |dd| key of one level-1
// position recomputed from the input (db1: wl_dd1_*, on haar2x2; bior1.5: wl_bior_dd1_*, on
// bior_dd2x2).  Included by wavelet_haar.hip alone, which launches both kernels: with the
// callers of select_bin / radix_pass spread over units the compiler specialises them differently.
#pragma once
#include "wavelet_common.hpp"

namespace idn {

// ---- 4: sigma = median(|finest dd| != 0) / ppf(0.75) ------------------------------------------
// The median is over the NONZERO coefficients, so which coefficients are exactly zero must match
// the reference: the analysis runs in fp64 with pywt's op order (normalise (Y - min)/(max - min),
// axis 0 then axis 1, multiply then add), under which equal samples give an exact 0.
// Exact rank selection over the nonzero |d| of one band, on the IEEE bits (non-negative doubles
// order like their bit patterns).  Radix passes of <= 11 bits: the first two run over the band
// (the first also counts the nonzero keys), then the keys sharing the selected 22-bit prefix are
// compacted into a scratch slot and the last four passes run over that (typically a few hundred
// keys).  The upper middle rank (even counts) costs one more band pass: it equals the lower value
// while enough keys are <= it, otherwise it is the smallest key above it.  Compaction slots are
// allocated once per wave (ballot + popcount).
struct RadixState {
  unsigned long long prefix, pmask;
  uint32_t rank;
};


// block-wide selection over an LDS histogram: the bin holding rank `rank` and the rank within
// it.  Thread i owns bins [i*per, (i+1)*per); the thread whose count range holds the rank finds
// the bin (a serial scan of 2048 LDS bins by one thread costs ~100k cycles).  lower_mid: select
// the lower middle rank (total-1)/2 instead, and return the total through *total.
struct BinSel {
  uint32_t bin, rank;
};
__device__ BinSel select_bin(const uint32_t* hist, int nb, uint32_t rank, uint32_t* total,
                             bool lower_mid) {
  __shared__ uint32_t sel_bin, sel_rank, wsum[32], tot_s;
  const int T = blockDim.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int per = (nb + T - 1) / T, b0 = threadIdx.x * per, b1 = min(b0 + per, nb);
  uint32_t own = 0;
  for (int b = b0; b < b1; ++b) own += hist[b];
  uint32_t inc = own;  // inclusive scan within the wave
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int k = 0; k < (T + 63) / 64; ++k) {
      const uint32_t t = wsum[k];
      wsum[k] = acc;
      acc += t;
    }
    tot_s = acc;
    sel_bin = (uint32_t)(nb - 1);  // fallback: rank beyond the total
    sel_rank = 0;
  }
  __syncthreads();
  if (lower_mid) {
    if (total) *total = tot_s;
    rank = tot_s ? (tot_s - 1) / 2 : 0;
  }
  const uint32_t excl = wsum[wv] + inc - own;
  if (own && rank >= excl && rank < excl + own) {
    uint32_t acc = excl;
    int b = b0;
    for (; b < b1 - 1; ++b) {
      if (acc + hist[b] > rank) break;
      acc += hist[b];
    }
    sel_bin = (uint32_t)b;
    sel_rank = rank - acc;
  }
  __syncthreads();
  const BinSel r{sel_bin, sel_rank};
  __syncthreads();
  return r;
}

// one histogram pass over keys[0..n) (only keys matching the prefix); narrows the state.
// total (optional) receives the number of nonzero keys seen (first pass only).
__device__ void radix_pass(const double* __restrict__ d, size_t n, int sh, int wd, RadixState& rsx,
                           uint32_t* hist, uint32_t* total) {
  const int nb = 1 << wd;
  for (int k = threadIdx.x; k < nb; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  const unsigned long long prefix = rsx.prefix, pmask = rsx.pmask;
  // 8 loads in flight per thread (a one-load-per-iteration loop is latency-bound)
  for (size_t k0 = threadIdx.x; k0 < n; k0 += 8 * (size_t)blockDim.x) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const size_t k = k0 + (size_t)u * blockDim.x;
      v[u] = k < n ? d[k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned long long key = absbits(v[u]);
      if (key != 0 && (key & pmask) == prefix) atomicAdd(&hist[(key >> sh) & (nb - 1)], 1u);
    }
  }
  __syncthreads();
  const BinSel bs = select_bin(hist, nb, rsx.rank, total, total != nullptr);
  rsx.prefix |= (unsigned long long)bs.bin << sh;
  rsx.pmask |= (unsigned long long)(nb - 1) << sh;
  rsx.rank = bs.rank;
  __syncthreads();
}

__global__ __launch_bounds__(1024) void wl_median(wreal* __restrict__ ws, size_t img_floats,
                                                  double* __restrict__ stats, WlLayout Lt) {
  const int img = blockIdx.x / 3, c = blockIdx.x % 3;
  const size_t bsz = (size_t)Lt.H[1] * Lt.W[1];
  const wreal* d = ws + img * img_floats + Lt.off_band[1] + (size_t)c * 4 * bsz + 3 * bsz;  // dd
  // scratch: this channel's input-plane slot (h*w >= band size), unused by the transform
  double* scratch = ws + img * img_floats + (size_t)c * Lt.h * Lt.w;
  __shared__ uint32_t hist[2048];
  __shared__ uint32_t total_s, m_s, le_s;
  __shared__ unsigned long long gt_s;
  if (threadIdx.x == 0) {
    m_s = 0;
    le_s = 0;
    gt_s = ~0ull;
  }
  RadixState rsx{0ull, 0ull, 0u};
  radix_pass(d, bsz, 52, 11, rsx, hist, &total_s);  // also counts the nonzero keys
  const uint32_t total = total_s;
  double med;
  if (total == 0) {
    med = NAN;  // np.median of an empty selection
  } else {
    const uint32_t klo = (total - 1) / 2, khi = total / 2;
    radix_pass(d, bsz, 41, 11, rsx, hist, nullptr);
    // compact the keys with the selected 22-bit prefix (wave-aggregated slot allocation)
    const int lane = threadIdx.x & 63;
    const size_t nr = (bsz + 1023) / 1024 * 1024;
    for (size_t k = threadIdx.x; k < nr; k += 1024) {
      const double v = k < bsz ? d[k] : 0.0;
      const unsigned long long key = absbits(v);
      const bool hit = key != 0 && (key & rsx.pmask) == rsx.prefix;
      const unsigned long long m = __ballot(hit);
      if (m) {
        uint32_t base = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) base = atomicAdd(&m_s, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader);
        if (hit) scratch[base + __popcll(m & ((1ull << lane) - 1))] = v;
      }
    }
    __syncthreads();
    const size_t mcnt = m_s;
    radix_pass(scratch, mcnt, 30, 11, rsx, hist, nullptr);
    radix_pass(scratch, mcnt, 19, 11, rsx, hist, nullptr);
    radix_pass(scratch, mcnt, 8, 11, rsx, hist, nullptr);
    radix_pass(scratch, mcnt, 0, 8, rsx, hist, nullptr);
    const unsigned long long lo_key = rsx.prefix;
    const double vlo = __longlong_as_double((long long)lo_key);
    double vhi = vlo;
    if (khi != klo) {
      uint32_t le = 0;
      unsigned long long gt = ~0ull;
      for (size_t k = threadIdx.x; k < bsz; k += 1024) {
        const unsigned long long key = absbits(d[k]);
        if (key == 0) continue;
        if (key <= lo_key) ++le;
        else gt = key < gt ? key : gt;
      }
      for (int o = 32; o > 0; o >>= 1) {
        le += __shfl_xor(le, o);
        const unsigned long long og = (unsigned long long)__shfl_xor((long long)gt, o);
        gt = og < gt ? og : gt;
      }
      if (lane == 0) {
        atomicAdd(&le_s, le);
        atomicMin(&gt_s, gt);
      }
      __syncthreads();
      if (le_s <= khi) vhi = __longlong_as_double((long long)gt_s);
    }
    med = (vlo + vhi) / 2.0;  // np.median: mean of the two middle values
  }
  if (threadIdx.x == 0) {
    stats[(size_t)img * WL_STATS + WlStats::median(c, Lt.L)] = med;
    stats[(size_t)img * WL_STATS + WlStats::DIAG + c] = (double)total;  // diagnostics
  }
}

// pywt dwt2 of one 2x2 group, rows 2i / 2i+1 (x0j / x1j), columns 2j / 2j+1
__device__ __forceinline__ void haar2x2(wreal x00, wreal x01, wreal x10, wreal x11, wreal& aa,
                                        wreal& ad, wreal& da, wreal& dd) {
  const wreal lo0 = S2 * x10 + S2 * x00, lo1 = S2 * x11 + S2 * x01;    // axis 0 low
  const wreal hi0 = -S2 * x10 + S2 * x00, hi1 = -S2 * x11 + S2 * x01;  // axis 0 high
  aa = S2 * lo1 + S2 * lo0;
  ad = -S2 * lo1 + S2 * lo0;
  da = S2 * hi1 + S2 * hi0;
  dd = -S2 * hi1 + S2 * hi0;
}

// sigma for the fused path.  wl_haar_analyze left one fine-bin code per finest dd (u16: 0 for an
// exact zero, else wl_fbin(|dd|) + 1).  Pass 1: histogram of the codes, block-wide selection of
// the fine bin holding the lower middle rank.  Pass 2: the positions of that bin's codes (and of
// the next nonempty bin's, where the upper middle rank may live) are compacted; the exact |dd| of
// just those positions are recomputed from the input (wl_dd1_key: the analysis' loads and op
// order), and the remaining digits are selected on them.  The fp64 band never goes through HBM.
template <bool MARK>
__device__ unsigned long long wl_dd1_key(const uint8_t* __restrict__ src,
                                         const double* __restrict__ in64, int img, int h, int w,
                                         int64_t row_stride, uint32_t pos, int W1, int c, wreal mn,
                                         wreal inv, wreal rcp) {
  const int i = (int)(pos / (uint32_t)W1), j = (int)(pos - (uint32_t)i * (uint32_t)W1);
  wreal r[2][2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      double px[3];
      load_rgb64(src, in64, img, h, w, row_stride, 2 * i + rr, 2 * j + ss, px);
      const wreal a = ycbcr_c(px, c) - mn;
      if (MARK) {  // haar_row4_c
        const wreal q0 = a * rcp;
        r[rr][ss] = __fma_rn(__fma_rn(-q0, inv, a), rcp, q0);
      } else {  // L = 1: the plain quotient
        r[rr][ss] = a / inv;
      }
    }
  wreal aa, ad, da, dd;
  haar2x2(r[0][0], r[0][1], r[1][0], r[1][1], aa, ad, da, dd);
  return absbits(dd);
}

// the same for u8 input, split into the loads (two rows of 6 bytes as 3 half-words each: row
// starts are 4-byte aligned on this path, 6 j is even) and the arithmetic, so that a thread can
// keep several positions' loads in flight
struct Dd1Raw {
  uint32_t r[2][3];
};
__device__ __forceinline__ Dd1Raw wl_dd1_load(const uint8_t* __restrict__ src, int img, int h,
                                              int64_t row_stride, uint32_t pos, int W1) {
  const int i = (int)(pos / (uint32_t)W1), j = (int)(pos - (uint32_t)i * (uint32_t)W1);
  Dd1Raw q;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(
        src + ((int64_t)img * h + 2 * i + rr) * row_stride + (int64_t)6 * j);
#pragma unroll
    for (int k = 0; k < 3; ++k) q.r[rr][k] = p[k];
  }
  return q;
}
template <bool MARK>
__device__ __forceinline__ unsigned long long wl_dd1_eval(const Dd1Raw& q, int c, wreal mn,
                                                          wreal inv, wreal rcp) {
  wreal r[2][2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      double px[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int b = ss * 3 + ch;
        px[ch] = (double)((q.r[rr][b >> 1] >> (8 * (b & 1))) & 0xFFu) * (1.0 / 255.0);
      }
      const wreal a = ycbcr_c(px, c) - mn;
      if (MARK) {
        const wreal q0 = a * rcp;
        r[rr][ss] = __fma_rn(__fma_rn(-q0, inv, a), rcp, q0);
      } else {
        r[rr][ss] = a / inv;
      }
    }
  wreal aa, ad, da, dd;
  haar2x2(r[0][0], r[0][1], r[1][0], r[1][1], aa, ad, da, dd);
  return absbits(dd);
}

// bior1.5: the level-1 highpass has two taps, so a finest dd is the 2x2 combination of the
// normalised samples at rows 2i-4, 2i-3 and columns 2j-4, 2j-3 (pywt 'symmetric' indices), in
// wl_dwt_stream's op order: the column highpass (two products, then their sum) of both columns,
// then the row highpass.  The sigma median recomputes the few exact values it needs from the input
// (wl_haar_median<1, true, true>), so the analysis keeps the level-1 dd band in fp32 only -- all
// that the synthesis reads of it.
__device__ __forceinline__ double bior_dd2x2(double x00, double x01, double x10, double x11) {
  const double h0 = (-S2) * x10 + S2 * x00, h1 = (-S2) * x11 + S2 * x01;  // x[row][column]
  return (-S2) * h1 + S2 * h0;
}
struct BiorDdRaw {  // u8: the dword holding each sample's 3 bytes, and the bit offset of the pixel
  uint32_t v[2][2];
  uint32_t sh[2];
};
__device__ __forceinline__ BiorDdRaw wl_bior_dd1_load(rsrc_t rs, int h, int w, int64_t row_stride,
                                                      uint32_t pos, int W1) {
  const int i = (int)(pos / (uint32_t)W1), j = (int)(pos - (uint32_t)i * (uint32_t)W1);
  const int y[2] = {sym_idx(2 * i - 4, h), sym_idx(2 * i - 3, h)};
  const int x[2] = {sym_idx(2 * j - 4, w), sym_idx(2 * j - 3, w)};
  BiorDdRaw q;
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) q.sh[cc] = x[cc] > 0 ? 8u : 0u;
  // bytes 3x - 1 .. 3x + 2 (0 .. 3 at x = 0): never past the end.  The whole offset goes in the
  // per-lane operand (a per-lane row offset in the scalar one becomes a loop over the lanes)
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
      q.v[rr][cc] = __builtin_amdgcn_raw_buffer_load_b32(
          rs, (uint32_t)((int64_t)y[rr] * row_stride) + (x[cc] > 0 ? 3u * (uint32_t)x[cc] - 1u : 0u),
          0u, 0);
  return q;
}
__device__ __forceinline__ unsigned long long wl_bior_dd1_eval(const BiorDdRaw& q, int c, wreal mn,
                                                               wreal inv, wreal rcp) {
  double r[2][2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      double px[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        px[ch] = (double)((q.v[rr][cc] >> (q.sh[cc] + 8 * ch)) & 0xFFu) * (1.0 / 255.0);
      const wreal a = ycbcr_c(px, c) - mn;  // wl_dwt_stream's norm (u8: reciprocal + Markstein)
      const wreal q0 = a * rcp;
      r[rr][cc] = __fma_rn(__fma_rn(-q0, inv, a), rcp, q0);
    }
  return absbits(bior_dd2x2(r[0][0], r[0][1], r[1][0], r[1][1]));
}
__device__ unsigned long long wl_bior_dd1_key64(const double* __restrict__ in64, int img, int h,
                                                int w, uint32_t pos, int W1, int c, wreal mn,
                                                wreal inv) {
  const int i = (int)(pos / (uint32_t)W1), j = (int)(pos - (uint32_t)i * (uint32_t)W1);
  const int y[2] = {sym_idx(2 * i - 4, h), sym_idx(2 * i - 3, h)};
  const int x[2] = {sym_idx(2 * j - 4, w), sym_idx(2 * j - 3, w)};
  double r[2][2];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      double px[3];
      load_rgb64(nullptr, in64, img, h, w, 0, y[rr], x[cc], px);
      r[rr][cc] = (ycbcr_c(px, c) - mn) / inv;  // wl_dwt_stream's norm for f64 input
    }
  return absbits(bior_dd2x2(r[0][0], r[0][1], r[1][0], r[1][1]));
}

// threads per (image, channel): several workgroups per CU overlap phases (512 measured 0.7 %
// faster on the whole bior1.5 op than 256 and 1024)
constexpr int WLM_WG = 512;
#ifndef IDN_WLM_IT  // A/B builds set it
#define IDN_WLM_IT 8
#endif
constexpr int WLM_IT = IDN_WLM_IT;
#ifndef IDN_WLM_HQ  // A/B builds set it
#define IDN_WLM_HQ 6
#endif
constexpr int HQ = IDN_WLM_HQ;  // Haar median: candidate positions per thread and round  // code groups (4 codes, 8 bytes) in flight per lane, passes 1-2
constexpr int WLM_NH = 8;    // histogram copies (32 KB of LDS; 16 measured slower: fewer workgroups per CU)
// BAND: the general path (any wavelet; level-1 dd stored in fp64 by wl_dwt_rb, which also left
// the codes at the start of the channel's input-plane slot): the exact keys of a position are
// read from the band instead of recomputed from the pixels.  L is unused then.  BIOR (with BAND):
// the codes as BAND, the keys recomputed from the input (bior_dd2x2; the band is fp32).
// The channel's sums of squares of every detail band over the analysis' per-tile partials (one
// wave per band, lanes over the tiles in a fixed order: deterministic, and exact for bior1.5 whose
// partials sit on a power-of-two grid) and its BayesShrink thresholds -- wl_sumsq's and
// wl_thresh's work for one channel, at the end of its median workgroup.  The degenerate-image
// flag is only ever raised here (wl_init_stats cleared it), so the three channels' workgroups
// cannot undo one another.
__device__ void wl_sums_thresh(double* __restrict__ st, const double* __restrict__ part_img, int c,
                               const WlLayout& Ls, const WlLayout& Lt, double med, wreal mn,
                               wreal mx) {
  __shared__ double sums[3 * WL_MAXL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < 3 * Lt.L; k += WLM_WG / 64) {
    const int l = k / 3, b = k - 3 * l, lev = l + 1;
    const double* p = part_img + (size_t)(c * 3 + b) * (Ls.part_per_img / 9) + Ls.part_tile0[lev];
    double s = 0.0;
    for (int t = lane; t < Ls.tiles[lev]; t += 64) s += p[t];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sums[k] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sigma = med / 0.6744897501960817;
  const bool bad = !(mx > mn) || !(sigma == sigma);  // 0.14.2: NaN everywhere -> U8 0
  const double var = sigma * sigma;
  for (int l = 0; l < Lt.L; ++l)
    for (int b = 0; b < 3; ++b) {
      const double sq = sums[3 * l + b];
      st[WlStats::sumsq(c, l, b, Lt.L)] = sq;
      const double cnt = (double)Lt.H[l + 1] * Lt.W[l + 1];
      const double t = var / sqrt(fmax(sq / cnt - var, 2.220446049250313e-16));
      st[WlStats::thr(c, l, b, Lt.L)] = t;
      if (Lt.L <= 3) st[WlStats::thrh(c, l, b)] = 0.5 * t;
    }
  if (bad) st[WlStats::FLAG] = 1.0;
}

// part (non-null): the channel's sums of squares over the analysis partials (wl_sumsq's work, in
// the partials layout Ls) and its BayesShrink thresholds (wl_thresh's) follow the median in the
// same workgroup -- two launches less per op
template <int L, bool BAND = false, bool BIOR = false>
__global__ __launch_bounds__(WLM_WG) void wl_haar_median(const uint8_t* __restrict__ src,
                                                       const double* __restrict__ in64,
                                                       int64_t row_stride,
                                                       wreal* __restrict__ ws, size_t img_floats,
                                                       double* __restrict__ stats, WlLayout Lt,
                                                       const double* __restrict__ part = nullptr,
                                                       WlLayout Ls = WlLayout{}) {
  constexpr bool MARK = L >= 2;
  const int img = blockIdx.x / 3, c = blockIdx.x % 3;
  const int W1 = Lt.W[1];
  const uint32_t bsz = (uint32_t)Lt.H[1] * (uint32_t)W1;
  const wreal* band_dd = ws + img * img_floats + Lt.off_band[1] + (size_t)c * 4 * bsz + 3 * bsz;
  double* slot = ws + img * img_floats + (size_t)c * Lt.h * Lt.w;
  const uint16_t* codes = BAND ? reinterpret_cast<const uint16_t*>(slot)
                               : reinterpret_cast<const uint16_t*>(band_dd);
  // scratch (the unused input-plane slot of this channel, h*w doubles; after the codes in BAND
  // mode): [0, bsz) keys of the selected bin, then positions of the selected bin and of the next
  double* keys = slot + (BAND ? (bsz + 3) / 4 : 0);
  uint32_t* pos_sel = reinterpret_cast<uint32_t*>(keys + bsz);
  uint32_t* pos_next = pos_sel + bsz;
  double* st = stats + (size_t)img * WL_STATS;
  wreal mn, mx;
  wl_minmax64(st, c, mn, mx);
  const wreal inv = mx - mn, rcp = 1.0 / inv;
  // WLM_NH copies of the histogram (by lane: the codes crowd into few bins, one copy would
  // serialise the LDS atomics); copy k lives at hist[k * WL_FBINS ..]
  __shared__ uint32_t hist[WLM_NH * WL_FBINS];
  __shared__ uint32_t m_s, mn_s, le_s, next_s;
  __shared__ unsigned long long nmin_s, gt_s;
  if (BAND && BIOR && !in64) {
    // the codes the N32 analysis could not certify (wl_dwt_stream): the exact fp64 key's code
    const uint32_t nu = *reinterpret_cast<const uint32_t*>(stats + (size_t)img * WL_STATS + WL_N32U + c);
    if (nu) {
      const uint32_t* lst = reinterpret_cast<const uint32_t*>(slot + (bsz + 3) / 4);
      uint16_t* cw = reinterpret_cast<uint16_t*>(slot);
      const rsrc_t rs = make_rsrc(src + (int64_t)img * Lt.h * row_stride, (uint32_t)((int64_t)Lt.h * row_stride));
      for (uint32_t t = threadIdx.x; t < nu; t += WLM_WG) {
        const uint32_t pos = lst[t];
        const unsigned long long key =
            wl_bior_dd1_eval(wl_bior_dd1_load(rs, Lt.h, Lt.w, row_stride, pos, W1), c, mn, inv, rcp);
        cw[pos] = (uint16_t)(key ? (uint32_t)wl_fbin(key) + 1u : 0u);
      }
      __syncthreads();
    }
  }
  for (int k = threadIdx.x; k < WLM_NH * WL_FBINS; k += WLM_WG) hist[k] = 0u;
  if (threadIdx.x == 0) {
    m_s = 0;
    mn_s = 0;
    le_s = 0;
    next_s = WL_FBINS;
    nmin_s = ~0ull;
    gt_s = ~0ull;
  }
  __syncthreads();
  // codes in 8-byte groups of 4 (the code array is 8-byte aligned), 8 groups in flight per lane:
  // every workgroup of the grid is resident at once, so each phase costs its latency chain
  const uint32_t ngrp = bsz / 4;
  const uint2* cg = reinterpret_cast<const uint2*>(codes);
  auto code_at = [](const uint2& g, int q) -> uint32_t {
    return ((q < 2 ? g.x : g.y) >> (16 * (q & 1))) & 0xFFFFu;
  };
  for (uint32_t g0 = threadIdx.x; g0 < ngrp; g0 += WLM_IT * WLM_WG) {
    uint2 gv[WLM_IT];
#pragma unroll
    for (int u = 0; u < WLM_IT; ++u) {
      const uint32_t g = g0 + (uint32_t)u * WLM_WG;
      gv[u] = g < ngrp ? cg[g] : uint2{0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < WLM_IT; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t cd = code_at(gv[u], q);
        if (cd) atomicAdd(&hist[(threadIdx.x & (WLM_NH - 1)) * WL_FBINS + cd - 1], 1u);
      }
  }
  for (uint32_t k = ngrp * 4 + threadIdx.x; k < bsz; k += WLM_WG) {  // tail codes
    const uint32_t cd = codes[k];
    if (cd) atomicAdd(&hist[(threadIdx.x & (WLM_NH - 1)) * WL_FBINS + cd - 1], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < WL_FBINS; b += WLM_WG) {  // fold the copies into copy 0
    uint32_t v = 0;
#pragma unroll
    for (int cp = 0; cp < WLM_NH; ++cp) v += hist[cp * WL_FBINS + b];
    hist[b] = v;
  }
  __syncthreads();
  uint32_t total = 0;
  const BinSel bs = select_bin(hist, WL_FBINS, 0u, &total, true);
  const int bsel = (int)bs.bin;
  for (int b = threadIdx.x; b < WL_FBINS; b += WLM_WG)
    if (b > bsel && hist[b]) atomicMin(&next_s, (uint32_t)b);
  __syncthreads();
  double med;
  if (total == 0) {
    med = NAN;  // np.median of an empty selection
  } else {
    const uint32_t klo = (total - 1) / 2, khi = total / 2;
    const uint32_t csel = (uint32_t)bsel + 1, cnext = next_s + 1;
    const int lane = threadIdx.x & 63;
    // pass 2: positions of the selected and the next bin.  Each lane counts its hits (selected
    // bin in the low half-word, next bin in the high one), one wave scan places them and one
    // LDS atomic per wave and iteration allocates the slots (per-hit ballots with an atomic each
    // serialise: a 3 % bin hits nearly every wave-wide ballot).
    auto place = [&](uint32_t cnt2, uint32_t& off_sel, uint32_t& off_next) {
      uint32_t inc = cnt2;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= o) inc += t;
      }
      const uint32_t tot = (uint32_t)__shfl((int)inc, 63);
      uint32_t base_sel = 0, base_next = 0;
      if (lane == 63) {
        if (tot & 0xFFFFu) base_sel = atomicAdd(&m_s, tot & 0xFFFFu);
        if (tot >> 16) base_next = atomicAdd(&mn_s, tot >> 16);
      }
      base_sel = (uint32_t)__shfl((int)base_sel, 63);
      base_next = (uint32_t)__shfl((int)base_next, 63);
      const uint32_t excl = inc - cnt2;
      off_sel = base_sel + (excl & 0xFFFFu);
      off_next = base_next + (excl >> 16);
    };
    for (uint32_t gb = 0; gb < ngrp; gb += WLM_IT * WLM_WG) {  // uniform trip count: the scan needs
      const uint32_t g0 = gb + threadIdx.x;                // every lane of the wave
      uint2 gv[WLM_IT];
#pragma unroll
      for (int u = 0; u < WLM_IT; ++u) {
        const uint32_t g = g0 + (uint32_t)u * WLM_WG;
        gv[u] = g < ngrp ? cg[g] : uint2{0u, 0u};
      }
      uint32_t cnt2 = 0;
#pragma unroll
      for (int u = 0; u < WLM_IT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t cd = code_at(gv[u], q);
          cnt2 += (cd == csel ? 1u : 0u) + (cd == cnext ? 0x10000u : 0u);
        }
      if (__ballot(cnt2 != 0) == 0) continue;  // wave-uniform
      uint32_t os, on;
      place(cnt2, os, on);
      if (cnt2) {
#pragma unroll
        for (int u = 0; u < WLM_IT; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t cd = code_at(gv[u], q);
            const uint32_t p = 4 * (g0 + (uint32_t)u * WLM_WG) + (uint32_t)q;
            if (cd == csel) pos_sel[os++] = p;
            if (cd == cnext) pos_next[on++] = p;
          }
      }
    }
    for (uint32_t k0 = ngrp * 4; k0 < bsz; k0 += WLM_WG) {  // tail codes (every lane takes part)
      const uint32_t k = k0 + threadIdx.x;
      const uint32_t cd = k < bsz ? codes[k] : 0u;
      const uint32_t cnt2 = (cd == csel ? 1u : 0u) + (cd == cnext ? 0x10000u : 0u);
      uint32_t os, on;
      place(cnt2, os, on);
      if (cd == csel) pos_sel[os] = k;
      if (cd == cnext) pos_next[on] = k;
    }
    __syncthreads();
    const uint32_t mcnt = m_s, ncnt = mn_s;
    // the selected bin's keys live in LDS when they fit: the level-1 histogram is dead now and
    // the radix passes use only its first 2048 words
    constexpr uint32_t LDS_KEYS = (WLM_NH * WL_FBINS - 2048) / 2;
    double* kb = mcnt <= LDS_KEYS ? reinterpret_cast<double*>(hist + 2048) : keys;
    // the exact keys of the selected bin, recomputed from the input (u8: 8 positions' loads in
    // flight per thread; the recompute is latency-bound otherwise)
    if (BAND && BIOR) {
      if (in64) {
        for (uint32_t t = threadIdx.x; t < mcnt; t += WLM_WG)
          kb[t] = __longlong_as_double((long long)wl_bior_dd1_key64(in64, img, Lt.h, Lt.w,
                                                                     pos_sel[t], W1, c, mn, inv));
      } else {
        const rsrc_t rs = make_rsrc(src + (int64_t)img * Lt.h * row_stride,
                                    (uint32_t)((int64_t)Lt.h * row_stride));
        // BQ positions per thread and round: all positions first (clamped, unconditional: a load
        // under a branch is waited for at once), then all their pixels.  BQ = 6 keeps the kernel
        // at <= 80 VGPRs: three 512-thread workgroups per CU, the whole grid resident at once
        constexpr int BQ = 6;
        for (uint32_t t0 = threadIdx.x; t0 < mcnt; t0 += BQ * WLM_WG) {
          uint32_t pp[BQ];
#pragma unroll
          for (int u = 0; u < BQ; ++u) pp[u] = pos_sel[min(t0 + (uint32_t)u * WLM_WG, mcnt - 1)];
          BiorDdRaw q[BQ];
#pragma unroll
          for (int u = 0; u < BQ; ++u) q[u] = wl_bior_dd1_load(rs, Lt.h, Lt.w, row_stride, pp[u], W1);
#pragma unroll
          for (int u = 0; u < BQ; ++u) {
            const uint32_t t = t0 + (uint32_t)u * WLM_WG;
            if (t < mcnt)
              kb[t] = __longlong_as_double((long long)wl_bior_dd1_eval(q[u], c, mn, inv, rcp));
          }
        }
      }
    } else if (BAND) {
      for (uint32_t t = threadIdx.x; t < mcnt; t += WLM_WG)
        kb[t] = __longlong_as_double((long long)absbits(band_dd[pos_sel[t]]));
    } else if (in64) {
      for (uint32_t t = threadIdx.x; t < mcnt; t += WLM_WG)
        kb[t] = __longlong_as_double((long long)wl_dd1_key<MARK>(
            src, in64, img, Lt.h, Lt.w, row_stride, pos_sel[t], W1, c, mn, inv, rcp));
    } else {
      for (uint32_t t0 = threadIdx.x; t0 < mcnt; t0 += HQ * WLM_WG) {
        // as the bior form: all positions first (clamped, unconditional), then their pixels
        uint32_t pp[HQ];
#pragma unroll
        for (int u = 0; u < HQ; ++u) pp[u] = pos_sel[min(t0 + (uint32_t)u * WLM_WG, mcnt - 1)];
        Dd1Raw q[HQ];
#pragma unroll
        for (int u = 0; u < HQ; ++u) q[u] = wl_dd1_load(src, img, Lt.h, row_stride, pp[u], W1);
#pragma unroll
        for (int u = 0; u < HQ; ++u) {
          const uint32_t t = t0 + (uint32_t)u * WLM_WG;
          if (t < mcnt)
            kb[t] = __longlong_as_double((long long)wl_dd1_eval<MARK>(q[u], c, mn, inv, rcp));
        }
      }
    }
    __syncthreads();
    const uint32_t rank_in = bs.rank;
    RadixState rsx{0ull, 0ull, rank_in};
    if (bsel > 0 && bsel < WL_FBINS - 1) {  // an unclamped bin: exponent and 4 mantissa bits known
      rsx.prefix = ((unsigned long long)(bsel / 16 + (1023 - 61)) << 52) |
                   ((unsigned long long)(bsel % 16) << 48);
      rsx.pmask = 0x7FFFull << 48;
      radix_pass(kb, mcnt, 37, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 26, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 15, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 4, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 0, 4, rsx, hist, nullptr);
    } else {
      radix_pass(kb, mcnt, 52, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 41, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 30, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 19, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 8, 11, rsx, hist, nullptr);
      radix_pass(kb, mcnt, 0, 8, rsx, hist, nullptr);
    }
    const unsigned long long lo_key = rsx.prefix;
    const double vlo = __longlong_as_double((long long)lo_key);
    double vhi = vlo;
    if (khi != klo) {
      if (rank_in + 1 < mcnt) {  // the upper middle rank is in the same bin
        uint32_t le = 0;
        unsigned long long gt = ~0ull;
        for (uint32_t k = threadIdx.x; k < mcnt; k += WLM_WG) {
          const unsigned long long key = absbits(kb[k]);
          if (key <= lo_key) ++le;
          else gt = key < gt ? key : gt;
        }
        for (int o = 32; o > 0; o >>= 1) {
          le += __shfl_xor(le, o);
          const unsigned long long og = (unsigned long long)__shfl_xor((long long)gt, o);
          gt = og < gt ? og : gt;
        }
        if (lane == 0) {
          atomicAdd(&le_s, le);
          atomicMin(&gt_s, gt);
        }
        __syncthreads();
        if (le_s <= rank_in + 1) vhi = __longlong_as_double((long long)gt_s);
      } else {  // it is the smallest key of the next nonempty bin
        unsigned long long nmin = ~0ull;
        for (uint32_t t = threadIdx.x; t < ncnt; t += WLM_WG) {
          unsigned long long key;
          if (BAND && BIOR) {
            if (in64) {
              key = wl_bior_dd1_key64(in64, img, Lt.h, Lt.w, pos_next[t], W1, c, mn, inv);
            } else {
              const rsrc_t rs = make_rsrc(src + (int64_t)img * Lt.h * row_stride,
                                          (uint32_t)((int64_t)Lt.h * row_stride));
              key = wl_bior_dd1_eval(wl_bior_dd1_load(rs, Lt.h, Lt.w, row_stride, pos_next[t], W1),
                                     c, mn, inv, rcp);
            }
          } else if (BAND) {
            key = absbits(band_dd[pos_next[t]]);
          } else {
            key = wl_dd1_key<MARK>(src, in64, img, Lt.h, Lt.w, row_stride, pos_next[t], W1, c, mn,
                                   inv, rcp);
          }
          nmin = key < nmin ? key : nmin;
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long on = (unsigned long long)__shfl_xor((long long)nmin, o);
          nmin = on < nmin ? on : nmin;
        }
        if (lane == 0) atomicMin(&nmin_s, nmin);
        __syncthreads();
        vhi = __longlong_as_double((long long)nmin_s);
      }
    }
    med = (vlo + vhi) / 2.0;  // np.median: mean of the two middle values
  }
  if (threadIdx.x == 0) {
    st[WlStats::median(c, Lt.L)] = med;
    st[WlStats::DIAG + c] = (double)total;  // diagnostics
  }
  if (part) wl_sums_thresh(st, part + img * Ls.part_per_img, c, Ls, Lt, med, mn, mx);
}

}  // namespace idn
