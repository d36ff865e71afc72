// cv2.medianBlur(u8, ksize) for odd ksize 7..31 on interleaved HxWxC images, BORDER_REPLICATE,
// bit-exact: the value of rank K*K/2 of the KxK window, per channel.
//
// Constant-time histogram median, one wave per workgroup.  The wave owns 64 adjacent output bytes
// of a row (channels interleaved: the window neighbours of byte b are b +- j*C) and marches down
// a band of rows.  Every lane keeps the 256-bin histogram of its own window in LDS and per row
// step adds the K bytes of the entering row and subtracts the K bytes of the leaving one:
//   fine    [bin / 4][lane] dwords, a byte per bin   (K <= 15: a count is at most 225)
//           [bin / 2][lane] dwords, a u16 per bin    (K >= 17: at most 961)
//   coarse  [bin / 32][lane] dwords, a u16 per 16 bins
// Lane l only ever touches dwords of bank l (index = i * 64 + l), so every update is one
// conflict-free ds_add_u32 / ds_sub_u32 of 1 << shift on the lane's own dword; a count never
// leaves its field, so no carry or borrow crosses into the neighbouring bin.
// The rows come through a ring of K + 1 staged rows in LDS: each input row is read from memory
// once per wave (byte loads: any pointer alignment, any row_stride, any C), with the replicated
// columns resolved while staging (the staged column offsets do not depend on the row), and is
// read back twice, when it enters and when it leaves.  Rows above / below the image are staged
// again from the clamped row.
// The median is found in two tiers, with a cost that does not depend on the content: the 16
// coarse counts give the 16-bin group that holds the rank, the 16 fine bins of that group the bin.
#include "idn_common.hpp"

#include <algorithm>

namespace idn {

constexpr int MEDL_SEG = 64;         // output bytes per wave (one per lane)
constexpr int MEDL_BAND_ROWS = 128;  // rows a wave marches down (IDN_MEDIAN_LARGE_ROWS)
// a launch that does not fill 3/4 of the wave slots its LDS leaves on the device (8 per CU with
// byte bins, 4 with u16 bins) halves its bands, down to MEDL_BAND_MIN rows: a band refills K - 1
// rows at its top, so past one resident round shorter bands only add work
// (profiles/median_large/ab_band_rows.jsonl)
constexpr int MEDL_BAND_MIN = 32;

template <int K>
struct MedL {
  static constexpr int R = K / 2;
  static constexpr bool WIDE = K * K > 255;
  static constexpr int NS = (MEDL_SEG + 2 * R * 4 + 63) / 64;  // staged bytes per lane (C <= 4)
  static constexpr int SW = NS * 64;                           // ring row pitch, bytes
  static constexpr int FINE_DW = WIDE ? 128 : 64;              // fine dwords per lane
};

// Sixteen counts in 8 dwords of u16 pairs whose total exceeds r: the number of leading counts
// whose inclusive prefix sum is <= r (0..15), and in `below` that prefix sum.  Two tiers: the
// dword first (v_sad_u16 against 0 adds both halves to the running sum), then its low half.
__device__ __forceinline__ uint32_t rank_u16x16(const uint32_t (&d)[8], uint32_t r,
                                                uint32_t& below) {
  uint32_t tot = 0, di = 0, bel = 0, pick = d[0];
  bool le_prev = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    tot = __builtin_amdgcn_sad_u16(d[i], 0u, tot);
    if (i) pick = le_prev ? d[i] : pick;  // ends as d[di]: le is true for exactly the first di dwords
    const bool le = tot <= r;
    di += le;
    bel = le ? tot : bel;
    le_prev = le;
  }
  const uint32_t t = bel + (pick & 0xFFFFu);
  const bool le = t <= r;
  below = le ? t : bel;
  return 2 * di + le;
}

// the same for sixteen byte counts in 4 dwords (v_sad_u8), without the prefix sum
__device__ __forceinline__ uint32_t rank_u8x16(const uint32_t (&d)[4], uint32_t r) {
  uint32_t tot = 0, qi = 0, bel = 0, pick = d[0];
  bool le_prev = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    tot = __builtin_amdgcn_sad_u8(d[i], 0u, tot);
    if (i) pick = le_prev ? d[i] : pick;
    const bool le = tot <= r;
    qi += le;
    bel = le ? tot : bel;
    le_prev = le;
  }
  const uint32_t t0 = bel + (pick & 0xFFu);
  const uint32_t t1 = t0 + ((pick >> 8) & 0xFFu);
  const uint32_t t2 = t1 + ((pick >> 16) & 0xFFu);
  return 4 * qi + (t0 <= r) + (t1 <= r) + (t2 <= r);  // the dword's own count exceeds r - bel
}

template <int K>
__global__ __launch_bounds__(64) void median_large_u8_kernel(const uint8_t* __restrict__ src,
                                                             uint8_t* __restrict__ dst, int h,
                                                             int w, int c, int rb,
                                                             int64_t row_stride, int nseg,
                                                             int bands, int band_rows) {
  typedef MedL<K> P;
  constexpr int R = P::R;
  constexpr bool WIDE = P::WIDE;
  constexpr uint32_t RANK = (uint32_t)(K * K / 2);
  __shared__ uint32_t fine[P::FINE_DW * 64];
  __shared__ uint32_t coarse[8 * 64];
  __shared__ uint8_t ring[(K + 1) * P::SW];

  const int lane = threadIdx.x;
  const int item = blockIdx.x;
  const int seg = item % nseg, tq = item / nseg;
  const int band = tq % bands, img = tq / bands;
  const int y0 = band * band_rows;
  const int y1 = min(y0 + band_rows, h);
  if (y0 >= y1) return;
  const int b0 = seg * MEDL_SEG;

  const uint8_t* s = src + (int64_t)img * h * row_stride;
  uint8_t* d = dst + (int64_t)img * h * row_stride;

  // staged byte i of a row is row byte b0 - R*c + i with its pixel clamped into the image
  int coff[P::NS];
#pragma unroll
  for (int i = 0; i < P::NS; ++i) {
    const int p = b0 - R * c + lane + 64 * i;
    const int ch = (p + 64 * c) % c;
    const int px = clampi((p - ch) / c, 0, w - 1);
    coff[i] = px * c + ch;
  }

#pragma unroll
  for (int i = 0; i < P::FINE_DW; ++i) fine[i * 64 + lane] = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) coarse[i * 64 + lane] = 0u;

  auto load_row = [&](int t, uint32_t (&v)[P::NS]) {
    const uint8_t* row = s + (int64_t)clampi(y0 - R + t, 0, h - 1) * row_stride;
#pragma unroll
    for (int i = 0; i < P::NS; ++i) v[i] = row[coff[i]];
  };
  // the lane's K window bytes of a staged row, into (add) or out of (!add) its histogram
  auto update = [&](int slot, bool add) {
    const uint8_t* rp = ring + slot * P::SW + lane;
    uint32_t v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = rp[j * c];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint32_t* fp;
      uint32_t finc;
      if constexpr (WIDE) {
        fp = &fine[(v[j] >> 1) * 64 + lane];
        finc = 1u << ((v[j] & 1u) * 16u);
      } else {
        fp = &fine[(v[j] >> 2) * 64 + lane];
        finc = 1u << ((v[j] & 3u) * 8u);
      }
      uint32_t* cp = &coarse[(v[j] >> 5) * 64 + lane];
      const uint32_t cinc = 1u << (((v[j] >> 4) & 1u) * 16u);
      if (add) {
        __hip_atomic_fetch_add(fp, finc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(cp, cinc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        __hip_atomic_fetch_sub(fp, finc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_sub(cp, cinc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  };
  // the bin of rank RANK: smallest v with count(<= v) > RANK
  auto select = [&]() -> uint32_t {
    uint32_t cw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) cw[i] = coarse[i * 64 + lane];
    uint32_t below;
    const uint32_t ci = rank_u16x16(cw, RANK, below);
    const uint32_t rem = RANK - below;  // the group's own count exceeds rem
    uint32_t fi;
    if constexpr (WIDE) {
      uint32_t fw[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) fw[q] = fine[(ci * 8 + q) * 64 + lane];
      uint32_t unused;
      fi = rank_u16x16(fw, rem, unused);
    } else {
      uint32_t fw[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) fw[q] = fine[(ci * 4 + q) * 64 + lane];
      fi = rank_u8x16(fw, rem);
    }
    return ci * 16 + fi;
  };

  // step t stages input row y0 - R + t (clamped) into ring slot t % (K + 1); from t = K - 1 on the
  // histogram holds the window of output row y0 + t - (K - 1), and from t = K on the row staged at
  // t - K, whose slot is the one that step t + 1 overwrites, leaves first
  const int nsteps = (K - 1) + (y1 - y0);
  uint32_t cur[P::NS];
  load_row(0, cur);
  int slot = 0;
  for (int t = 0; t < nsteps; ++t) {
    uint32_t nxt[P::NS];
    load_row(t + 1, nxt);
#pragma unroll
    for (int i = 0; i < P::NS; ++i) ring[slot * P::SW + lane + 64 * i] = (uint8_t)cur[i];
    __syncthreads();
    const int old = slot == K ? 0 : slot + 1;
    if (t >= K) update(old, false);
    update(slot, true);
    if (t >= K - 1) {
      const uint32_t m = select();
      const int y = y0 + t - (K - 1);
      if (b0 + lane < rb) d[(int64_t)y * row_stride + b0 + lane] = (uint8_t)m;
    }
    __syncthreads();
    slot = old;
#pragma unroll
    for (int i = 0; i < P::NS; ++i) cur[i] = nxt[i];
  }
}

template <int K>
static int launch_one(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                      int64_t row_stride, hipStream_t st) {
  const int64_t rb = (int64_t)w * c;
  IDN_CHECK_ARG(rb < (int64_t)0x7FFFFF00, "idn_median_blur_u8: row too long");
  const int nseg = (int)((rb + MEDL_SEG - 1) / MEDL_SEG);
  const int forced = knob("IDN_MEDIAN_LARGE_ROWS", 0);  // tuning build: this band height, as given
  int band_rows = std::min(h, forced > 0 ? forced : MEDL_BAND_ROWS);
  int bands = (h + band_rows - 1) / band_rows;
  const int64_t fill = (int64_t)cu_count() * (MedL<K>::WIDE ? 4 : 8) * 3 / 4;
  while (forced <= 0 && band_rows > MEDL_BAND_MIN && (int64_t)n * nseg * bands < fill) {
    band_rows = std::max(MEDL_BAND_MIN, band_rows / 2);
    bands = (h + band_rows - 1) / band_rows;
  }
  band_rows = (h + bands - 1) / bands;  // equal bands
  bands = (h + band_rows - 1) / band_rows;
  const int64_t total = (int64_t)n * bands * nseg;
  IDN_CHECK_ARG(total < (int64_t)0x7FFFFFFF, "idn_median_blur_u8: batch too large");
  hipLaunchKernelGGL((median_large_u8_kernel<K>), dim3((unsigned)total), dim3(64), 0, st, src, dst,
                     h, w, c, (int)rb, row_stride, nseg, bands, band_rows);
  IDN_CHECK_LAUNCH("idn_median_blur_u8");
  return IDN_OK;
}

// odd ksize in 7..31 (checked by the caller, idn_median_blur_u8)
int launch_median_large(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                        int64_t row_stride, int ksize, hipStream_t st) {
  switch (ksize) {
#define IDN_MEDL_CASE(K) \
  case K: return launch_one<K>(src, dst, n, h, w, c, row_stride, st);
    IDN_MEDL_CASE(7) IDN_MEDL_CASE(9) IDN_MEDL_CASE(11) IDN_MEDL_CASE(13) IDN_MEDL_CASE(15)
    IDN_MEDL_CASE(17) IDN_MEDL_CASE(19) IDN_MEDL_CASE(21) IDN_MEDL_CASE(23) IDN_MEDL_CASE(25)
    IDN_MEDL_CASE(27) IDN_MEDL_CASE(29) IDN_MEDL_CASE(31)
#undef IDN_MEDL_CASE
  }
  return set_error(IDN_EUNSUPPORTED, "idn_median_blur_u8: ksize %d not supported (odd, 3..31)",
                   ksize);
}

}  // namespace idn
