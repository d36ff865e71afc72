// The linear smoothers beyond the reference's literal call sites: idn_box_blur_u8 at odd windows
// 5..31, idn_gaussian_blur_u8 at 7..31 and idn_gaussian_blur_sigma_u8 (any odd window 3..31 with a
// given sigma), bit-equal to tests/blur_model.py.  BORDER_REFLECT_101, repeated until the index is
// inside the image, so images smaller than the radius are legal.  Integers only.
//
// box_large_kernel is the first moment of csrc/wiener.hip's walk: one 256-thread workgroup owns
// BL_SR output rows x 256 interleaved byte columns of one image, a lane keeps the running sum of
// the last k samples of its column (the leaving sample comes from an LDS ring of bytes, so every
// sample is loaded from memory once), publishes it as one 2-byte LDS entry per row, four rows
// behind one barrier, and an output adds the k entries c apart of its window; from k = 21 on the
// lanes first add groups of 4 or 5 neighbouring entries.  The work per output does not grow with
// the window's area.  The result (2 S + k^2) / (2 k^2) equals (S + (k^2 - 1) / 2) / k^2 (k^2 is
// odd) and is one 32-bit multiply-high by floor(2^32 / k^2) + 1: tools/check_blur_div.c goes
// through every window and every sum 0 .. 255 k^2.
//
// gauss_large_kernel is a separable Q8 filter: taps t[0 .. k-1] (host: idn_gaussian_taps, zero
// outer taps trimmed away, so k here is the number of taps that run), row pass
// u[y][x] = sum_j t[j] s[y][x + j - r] <= 255 * 256 (16 bits), column pass
// (sum_i t[i] u[y + i - r][x] + 32768) >> 16, every product below 2^24 (v_mad_u32_u24).  A
// workgroup owns BL_SR output rows x gb_tw(c) byte columns and walks down its strip BL_RS = 4
// input rows at a time: the rows' bytes are staged in LDS (loads one step ahead, unconditional:
// the reflected address is always inside the image), the row pass leaves its 16-bit results in an
// LDS ring of BL_D rows, and the column pass produces 4 output rows from the k + 3 ring rows under
// them, so that one 16-bit LDS read feeds up to 4 multiply-adds.  The row pass has two forms.
// Below BL_ROW4_FROM taps a lane takes its byte column in each of the 4 staged rows (k byte reads
// per output); from there on it takes 4 neighbouring pixels of one channel (k + 3 byte reads for 4
// outputs, the loop padded to a multiple of 4 taps).  profiles/blur_large has the A/B
// (IDN_GB_ROW forces a form in the tuning build).  The taps sit in the low lanes of one VGPR and
// reach the multiply-adds through v_readlane (the loop counter is uniform): no tap is read from
// memory inside the loops.  Every tap is a byte: a centre tap of 256 is the identity and runs
// bl_copy_kernel.
#include "blur_large.hpp"
#include "abi_args.hpp"

#include <limits.h>
#include <math.h>

namespace idn {

constexpr int BL_KMAX = 31;                    // largest window side
constexpr int BL_SR = 128;                     // output rows per workgroup
constexpr int BL_TW = 256;                     // lanes; output byte columns per box workgroup
constexpr int BL_HALO = (BL_KMAX - 1) * 4;     // halo byte columns at 4 channels
constexpr int BL_NS = BL_TW + BL_HALO;         // staged byte columns of a tile
constexpr int BL_TWO_LEVEL = 21;               // narrowest box window summed in two levels
constexpr int BL_STEP = 4;                     // box: rows whose loads are in flight together
constexpr int BL_RS = 4;                       // gauss: input rows per step, outputs per lane
constexpr int BL_D = 36;                       // gauss: ring rows (a multiple of BL_RS)
constexpr int BL_ROW4_FROM = 25;               // gauss: fewest taps of the 4-pixel row pass
static_assert(BL_HALO <= BL_TW, "a lane carries at most one halo column");
static_assert(BL_D % BL_RS == 0 && BL_D >= BL_KMAX + BL_RS - 1, "the ring holds one column pass");
static_assert(BL_NS % 4 == 0, "staged rows keep their alignment");

// byte columns of a Gaussian tile: whole groups of 4 pixels (256, 256, 252, 256)
__host__ __device__ constexpr int gb_tw(int c) { return BL_TW / (4 * c) * (4 * c); }

// byte offset within a row of byte column j of the image extended by reflection (j >= -15 c)
__device__ __forceinline__ uint32_t bl_col(int j, int w, int c) {
  const int e = j + BL_KMAX * c;  // >= 0
  const int px = min(e / c - BL_KMAX, w - 1 + BL_KMAX);
  return (uint32_t)(reflect101(px, w) * c + e % c);
}

template <int C>
__global__ __launch_bounds__(256) void box_large_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int64_t row_stride,
    int k, int sr, int tiles, int strips, uint32_t half, uint32_t magic) {
  // column sums <= 31 * 255 and sums of 5 of them fit 16 bits
  __shared__ uint16_t cs[2][BL_STEP][BL_NS];
  __shared__ uint16_t gs[BL_STEP][BL_NS];  // behind a barrier of its own: one buffer
  __shared__ uint8_t ring[BL_KMAX + 1][BL_NS];  // a lane reads and writes its own columns only

  constexpr int c = C;
  const int t = threadIdx.x;
  const int wgs = tiles * strips;
  const int img = blockIdx.x / wgs;
  const int rem = blockIdx.x - img * wgs;
  const int strip = rem / tiles;
  const int tile = rem - strip * tiles;

  const int r = k >> 1;
  const int wb = w * c;
  const int halo = (k - 1) * c;
  const int jb = tile * BL_TW;
  const int jo = jb + t;  // this lane's output byte column
  const bool out_ok = jo < wb;
  const int y0 = strip * sr, y1 = min(y0 + sr, h);  // output rows [y0, y1)

  const uint32_t c0 = bl_col(jb - r * c + t, w, c);
  const bool has1 = t < halo;
  const uint32_t c1 = has1 ? bl_col(jb - r * c + BL_TW + t, w, c) : 0u;
  // whether any lane of this wave carries a halo column (wave-uniform)
  const bool wave_has1 = (int)__builtin_amdgcn_readfirstlane((uint32_t)t) < halo;

  const uint8_t* base = src + (int64_t)img * h * row_stride;
  const int r_first = y0 - r, r_last = y1 - 1 + r;
  auto row_of = [&](int y) -> int { return reflect101(min(y, r_last), h); };

  // the two-level horizontal sum of wide windows: ngrp groups of grp column sums each
  const bool two = k >= BL_TWO_LEVEL;
  const int grp = k >= 25 ? 5 : 4, ngrp = k / grp;
  const int gspan = (ngrp - 1) * grp * c;  // halo columns whose group sum an output reads
  const int depth = k + 1;                   // ring: row y is in slot (y - r_first) % depth
  uint32_t a0 = 0, a1 = 0;                   // running column sums
  uint8_t n0[BL_STEP], n1[BL_STEP];
#pragma unroll
  for (int i = 0; i < BL_STEP; ++i) {
    const int64_t ro = (int64_t)row_of(r_first + i) * row_stride;
    n0[i] = base[ro + c0];
    n1[i] = 0;
    if (wave_has1) n1[i] = base[ro + c1];
  }
  int slot = 0, sbuf = 0;
  for (int rs = r_first; rs <= r_last; rs += BL_STEP, sbuf ^= 1) {
    uint8_t v0[BL_STEP], v1[BL_STEP];
#pragma unroll
    for (int i = 0; i < BL_STEP; ++i) {
      v0[i] = n0[i];
      v1[i] = n1[i];
    }
    if (rs + BL_STEP <= r_last) {  // the next step's samples, in flight across this step's barriers
#pragma unroll
      for (int i = 0; i < BL_STEP; ++i) {
        const int64_t ro = (int64_t)row_of(rs + BL_STEP + i) * row_stride;
        n0[i] = base[ro + c0];
        if (wave_has1) n1[i] = base[ro + c1];
      }
    }
    // the column sums after each of the step's rows (rows past r_last repeat it and are not used)
#pragma unroll
    for (int i = 0; i < BL_STEP; ++i) {
      const int y = rs + i;
      const int lslot = slot + 1 == depth ? 0 : slot + 1;  // row y - k (depth = k + 1)
      const bool leaves = y - k >= r_first;
      {
        const uint32_t e = v0[i];
        const uint32_t l = leaves ? (uint32_t)ring[lslot][t] : 0u;
        ring[slot][t] = (uint8_t)e;
        a0 += e - l;
        cs[sbuf][i][t] = (uint16_t)a0;
      }
      if (has1) {
        const uint32_t e = v1[i];
        const uint32_t l = leaves ? (uint32_t)ring[lslot][BL_TW + t] : 0u;
        ring[slot][BL_TW + t] = (uint8_t)e;
        a1 += e - l;
        cs[sbuf][i][BL_TW + t] = (uint16_t)a1;
      }
      slot = lslot;
    }
    __syncthreads();  // one per step: the next step writes the other half of cs
    if (rs + BL_STEP - 1 - r < y0) continue;  // no row of this step is an output row yet
    if (two) {
#pragma unroll
      for (int i = 0; i < BL_STEP; ++i) {
        {
          const uint16_t* tap = &cs[sbuf][i][t];
          uint32_t g = 0;
#pragma unroll 5
          for (int j = 0; j < grp; ++j) g += tap[j * c];
          gs[i][t] = (uint16_t)g;
        }
        if (t < gspan) {
          const uint16_t* tap = &cs[sbuf][i][BL_TW + t];
          uint32_t g = 0;
#pragma unroll 5
          for (int j = 0; j < grp; ++j) g += tap[j * c];
          gs[i][BL_TW + t] = (uint16_t)g;
        }
      }
      __syncthreads();
    }
    if (!out_ok) continue;
#pragma unroll
    for (int i = 0; i < BL_STEP; ++i) {
      const int yo = rs + i - r;
      if (yo < y0 || yo >= y1) continue;
      uint32_t s = 0;
      if (two) {
        const uint16_t* gtap = &gs[i][t];
#pragma unroll 4
        for (int j = 0; j < ngrp; ++j) s += gtap[j * grp * c];
        const uint16_t* tap = &cs[sbuf][i][t + ngrp * grp * c];
        for (int j = 0; j < k - ngrp * grp; ++j) s += tap[j * c];
      } else {
        // the middle column sum, then pairs from both ends: several reads in flight at once
        const uint16_t* tap = &cs[sbuf][i][t];
        s = tap[r * c];
#pragma unroll 4
        for (int j = 0; j < r; ++j) s += (uint32_t)tap[j * c] + tap[(k - 1 - j) * c];
      }
      // (2 s + k^2) / (2 k^2), exact: tools/check_blur_div.c
      dst[((int64_t)img * h + yo) * row_stride + jo] = (uint8_t)__umulhi(s + half, magic);
    }
  }
}

// tap i (uniform) out of the low lanes of tv.  A tap is a byte here (the launcher routes the one
// kernel with a tap of 256, the identity, to bl_copy_kernel), and the mask says so to the compiler,
// which then carries part of the row pass as v_dot4_u32_u8 over packed bytes
__device__ __forceinline__ uint32_t gb_tap(int tv, int i) {
  return (uint32_t)__builtin_amdgcn_readlane(tv, i) & 0xffu;
}

// the identity (a centre tap of 256, e.g. ksize 3 with sigma 0.1): rows of wb bytes, the padding
// untouched
__global__ __launch_bounds__(256) void bl_copy_kernel(const uint8_t* __restrict__ src,
                                                      uint8_t* __restrict__ dst, int64_t rows,
                                                      int wb, int64_t row_stride) {
  const int64_t total = rows * wb;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / wb, at = row * row_stride + (i - row * wb);
    dst[at] = src[at];
  }
}

struct GbTaps {
  uint32_t t[32];  // t[0 .. k-1], zeros behind them
};

template <int C, bool ROW4>
__global__ __launch_bounds__(256) void gauss_large_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int64_t row_stride,
    int k, int sr, int tiles, int strips, GbTaps taps) {
  __shared__ __attribute__((aligned(16))) uint8_t stg[BL_RS][BL_NS + 16];  // + 16: read past
  __shared__ __attribute__((aligned(16))) uint16_t ring[BL_D][BL_TW];

  constexpr int c = C;
  constexpr int tw = gb_tw(C);
  const int t = threadIdx.x;
  const int lane = t & 63, wv = t >> 6;
  const int wgs = tiles * strips;
  const int img = blockIdx.x / wgs;
  const int rem = blockIdx.x - img * wgs;
  const int strip = rem / tiles;
  const int tile = rem - strip * tiles;

  const int r = k >> 1;
  const int wb = w * c;
  const int ns = tw + (k - 1) * c;  // staged byte columns, <= BL_NS
  const int jb = tile * tw;
  const int jo = jb + t;
  const bool out_ok = t < tw && jo < wb;
  const int y0 = strip * sr, y1 = min(y0 + sr, h);

  const uint32_t c0 = bl_col(jb - r * c + t, w, c);
  const bool has1 = BL_TW + t < ns;
  const uint32_t c1 = has1 ? bl_col(jb - r * c + BL_TW + t, w, c) : 0u;
  const bool wave_has1 = BL_TW + (int)__builtin_amdgcn_readfirstlane((uint32_t)t) < ns;

  // lane i < k of every wave holds t[i]; the lanes behind hold 0 (the loops read up to lane 35)
  const int tv = lane < 32 ? (int)taps.t[lane] : 0;

  const uint8_t* base = src + (int64_t)img * h * row_stride;
  const int r_first = y0 - r, r_last = y1 - 1 + r;
  auto row_of = [&](int y) -> int { return reflect101(min(y, r_last), h); };

  uint8_t n0[BL_RS], n1[BL_RS];
#pragma unroll
  for (int i = 0; i < BL_RS; ++i) {
    const int64_t ro = (int64_t)row_of(r_first + i) * row_stride;
    n0[i] = base[ro + c0];
    n1[i] = 0;
    if (wave_has1) n1[i] = base[ro + c1];
  }
  const int nq = y1 - y0 + k - 1;  // input rows of the strip; ring row q is image row r_first + q
  for (int q0 = 0; q0 < nq; q0 += BL_RS) {
#pragma unroll
    for (int i = 0; i < BL_RS; ++i) {
      stg[i][t] = n0[i];
      if (has1) stg[i][BL_TW + t] = n1[i];
    }
    if (q0 + BL_RS < nq) {  // the next step's samples, in flight across this step's barriers
#pragma unroll
      for (int i = 0; i < BL_RS; ++i) {
        const int64_t ro = (int64_t)row_of(r_first + q0 + BL_RS + i) * row_stride;
        n0[i] = base[ro + c0];
        if (wave_has1) n1[i] = base[ro + c1];
      }
    }
    __syncthreads();
    if (ROW4) {
      // row pass: wave wv takes staged row wv, a lane 4 neighbouring pixels of one channel
      constexpr int units = tw / 4;
      if (lane < units) {
        const int b = (lane / c) * (4 * c) + lane % c;
        const uint8_t* p = &stg[wv][b];
        uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0, t1 = 0, t2 = 0, t3 = 0;
        for (int i = 0; i < k + 3; i += 4) {  // the reads past k + 2 meet taps that are 0
          uint32_t v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = p[(i + j) * c];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t t0 = gb_tap(tv, i + j);
            u0 = __umul24(v[j], t0) + u0;
            u1 = __umul24(v[j], t1) + u1;
            u2 = __umul24(v[j], t2) + u2;
            u3 = __umul24(v[j], t3) + u3;
            t3 = t2;
            t2 = t1;
            t1 = t0;
          }
        }
        uint16_t* o = &ring[(q0 + wv) % BL_D][b];
        o[0] = (uint16_t)u0;
        o[c] = (uint16_t)u1;
        o[2 * c] = (uint16_t)u2;
        o[3 * c] = (uint16_t)u3;
      }
    } else if (t < tw) {
      // first form: a lane takes its byte column in each of the 4 staged rows
      uint32_t u[BL_RS] = {0, 0, 0, 0};
      for (int i = 0; i < k; ++i) {
        const uint32_t t0 = gb_tap(tv, i);
#pragma unroll
        for (int j = 0; j < BL_RS; ++j) u[j] = __umul24((uint32_t)stg[j][t + i * c], t0) + u[j];
      }
#pragma unroll
      for (int j = 0; j < BL_RS; ++j) ring[(q0 + j) % BL_D][t] = (uint16_t)u[j];
    }
    __syncthreads();
    // column pass: output rows y0 + o0 .. y0 + o0 + 3 from ring rows o0 .. o0 + k + 2 = q0 + 3.
    // A row before the strip (o0 + j < 0) is not written, and a ring row before the first meets
    // only taps that are 0 in the rows that are
    const int o0 = q0 + 1 - k;
    if (o0 + BL_RS - 1 >= 0 && out_ok) {
      int sl = (o0 + BL_D) % BL_D;  // o0 >= 1 - k > -BL_D
      uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0, t1 = 0, t2 = 0, t3 = 0;
      for (int i = 0; i < k + 3; i += 4) {  // the reads past k + 2 meet taps that are 0
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = ring[sl][t];
          sl = sl + 1 == BL_D ? 0 : sl + 1;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t t0 = gb_tap(tv, i + j);
          u0 = __umul24(v[j], t0) + u0;
          u1 = __umul24(v[j], t1) + u1;
          u2 = __umul24(v[j], t2) + u2;
          u3 = __umul24(v[j], t3) + u3;
          t3 = t2;
          t2 = t1;
          t1 = t0;
        }
      }
      const uint32_t u[BL_RS] = {u0, u1, u2, u3};
#pragma unroll
      for (int j = 0; j < BL_RS; ++j) {
        const int yo = y0 + o0 + j;
        if (o0 + j >= 0 && yo < y1)
          dst[((int64_t)img * h + yo) * row_stride + jo] = (uint8_t)((u[j] + 32768u) >> 16);
      }
    }
  }
}

static int bl_grid(int n, int h, int64_t wb, int tw, int sr, int* tiles, int* strips,
                   unsigned* grid, const char* name) {
  const int64_t nt = (wb + tw - 1) / tw, nst = ((int64_t)h + sr - 1) / sr;
  if (wb > INT_MAX - BL_KMAX * 4 - BL_TW || (int64_t)n * nt * nst > INT_MAX)
    return batch_too_large(name);
  *tiles = (int)nt;
  *strips = (int)nst;
  *grid = (unsigned)((int64_t)n * nt * nst);
  return IDN_OK;
}

int launch_box_large(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                     int64_t row_stride, int k, hipStream_t s, const char* name) {
  int tiles, strips;
  unsigned grid;
  if (int e = bl_grid(n, h, (int64_t)w * c, BL_TW, BL_SR, &tiles, &strips, &grid, name)) return e;
  const uint32_t k2 = (uint32_t)(k * k);
  const uint32_t half = (k2 - 1) / 2, magic = (uint32_t)((1ull << 32) / k2 + 1);
#define IDN_BOX_LAUNCH(C)                                                                      \
  hipLaunchKernelGGL((box_large_kernel<C>), dim3(grid), dim3(256), 0, s, src, dst, h, w,       \
                     row_stride, k, BL_SR, tiles, strips, half, magic)
  switch (c) {
    case 1: IDN_BOX_LAUNCH(1); break;
    case 2: IDN_BOX_LAUNCH(2); break;
    case 3: IDN_BOX_LAUNCH(3); break;
    default: IDN_BOX_LAUNCH(4); break;
  }
#undef IDN_BOX_LAUNCH
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

int launch_gauss_large(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                       int64_t row_stride, int ksize, const uint16_t* taps, hipStream_t s,
                       const char* name) {
  // zero outer taps narrow the window (four of them at 29 and 31 with sigma 0)
  int lo = 0;
  while (lo < ksize / 2 && taps[lo] == 0) ++lo;
  const int k = ksize - 2 * lo;
  if (k == 1) {  // the centre tap is 256
    const int64_t blocks = ((int64_t)n * h * w * c + 255) / 256;
    hipLaunchKernelGGL(bl_copy_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256),
                       0, s, src, dst, (int64_t)n * h, w * c, row_stride);
    IDN_CHECK_LAUNCH(name);
    return IDN_OK;
  }
  GbTaps tp = {};
  for (int i = 0; i < k; ++i) tp.t[i] = taps[lo + i];  // <= 255 each: two or more are not 0
  int tiles, strips;
  unsigned grid;
  if (int e = bl_grid(n, h, (int64_t)w * c, gb_tw(c), BL_SR, &tiles, &strips, &grid, name))
    return e;
  // the row pass: four pixels of a channel per lane from BL_ROW4_FROM on, one output per lane and
  // row below (IDN_GB_ROW, tuning build only: 0 / 1 force a form)
  const int row_knob = knob("IDN_GB_ROW", -1);
  const bool row4 = row_knob < 0 ? k >= BL_ROW4_FROM : row_knob != 0;
#define IDN_GAUSS_LAUNCH(C)                                                                    \
  if (row4)                                                                                    \
    hipLaunchKernelGGL((gauss_large_kernel<C, true>), dim3(grid), dim3(256), 0, s, src, dst, h, \
                       w, row_stride, k, BL_SR, tiles, strips, tp);                            \
  else                                                                                         \
    hipLaunchKernelGGL((gauss_large_kernel<C, false>), dim3(grid), dim3(256), 0, s, src, dst,  \
                       h, w, row_stride, k, BL_SR, tiles, strips, tp)
  switch (c) {
    case 1: IDN_GAUSS_LAUNCH(1); break;
    case 2: IDN_GAUSS_LAUNCH(2); break;
    case 3: IDN_GAUSS_LAUNCH(3); break;
    default: IDN_GAUSS_LAUNCH(4); break;
  }
#undef IDN_GAUSS_LAUNCH
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

// the Q8 taps of tests/blur_model.py (host only)
int gaussian_taps(int ksize, double sigma, uint16_t* taps, const char* name) {
  IDN_CHECK_ARG(taps, "%s: null pointer (taps)", name);
  if (ksize < 3 || ksize > BL_KMAX || !(ksize & 1))
    return set_error(IDN_EUNSUPPORTED, "%s: ksize %d not supported (odd, 3..%d)", name, ksize,
                     BL_KMAX);
  IDN_CHECK_ARG(sigma >= 0.0 && isfinite(sigma), "%s: sigma must be finite and >= 0 (got %g)",
                name, sigma);
  if (sigma == 0.0 && ksize <= 7) {
    static const uint16_t small[3][7] = {
        {64, 128, 64}, {16, 64, 96, 64, 16}, {8, 28, 56, 72, 56, 28, 8}};
    for (int i = 0; i < ksize; ++i) taps[i] = small[ksize / 2 - 1][i];
    return IDN_OK;
  }
  const double s = sigma > 0.0 ? sigma : 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8;
  const int r = ksize / 2;
  double g[BL_KMAX], sum = 0.0;
  for (int i = 0; i < ksize; ++i) {
    const double d = (double)(i - r);
    g[i] = i == r ? 1.0 : exp(-(d * d) / (2.0 * s * s));
  }
  for (int i = 0; i < ksize; ++i) sum += g[i];
  int total = 0;
  for (int i = 0; i < ksize; ++i) {
    taps[i] = (uint16_t)rint(256.0 * (g[i] / sum));
    total += taps[i];
  }
  taps[r] = (uint16_t)(taps[r] + 256 - total);
  return IDN_OK;
}

}  // namespace idn

extern "C" int idn_gaussian_taps(int ksize, double sigma, uint16_t* taps) {
  return idn::gaussian_taps(ksize, sigma, taps, "idn_gaussian_taps");
}
