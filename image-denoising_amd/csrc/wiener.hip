// idn_wiener_u8: the pixelwise adaptive Wiener (Lee) filter, scipy.signal.wiener on every channel
// plane of a u8 batch, bit-equal to tests/wiener_model.py.
//
// With the integer sums S1 = sum t and S2 = sum t^2 over the kh x kw window of a sample x
// (n = kh kw; taps outside the image are 0, or the mirrored samples under reflect101):
//   m = double(S1) / n     v = double(S2) / n - m * m            (the product rounds, then the
//   r = v == 0 ? m : (v < noise ? m : (x - m) * (1 - noise / v) + m)   difference: no FMA)
// Given no noise, a first pass forms Q = sum over the plane of (n S2 - S1^2), an exact integer below
// 2^64 for planes of at most 2^28 samples, and noise = double(Q) / double(n^2 H W).
//
// wiener_kernel: one 256-thread workgroup owns WN_SR output rows x 256 interleaved byte columns
// of one image (a lane's channel is its byte column mod c).  The window's columns reach (kw - 1) c
// byte columns further, <= 90: the first lanes of the workgroup carry such a halo column besides
// their own.  Every sample of the tile is loaded from memory once: a lane keeps the last kh + 1
// samples of its column in an LDS ring of bytes, so that the sample leaving the window (kh rows
// up) and the output's own sample (kh / 2 rows up, another lane's column) come from LDS, not from
// a second and third load.  The loads of WN_STEP rows are asked for one step ahead, without a
// condition (a row or column outside the image is read somewhere inside it and masked when used),
// so that they are in flight together across the barriers.  Per input row a lane adds the
// entering sample and its square to its running column sums, subtracts the leaving one, publishes
// the pair as one 8-byte LDS entry (two buffers, one barrier per row), and every lane adds the kw
// entries c apart that make up its output's window; from kw = 21 on the lanes first add groups of
// 4 or 5 neighbouring entries into a second LDS row (one more barrier), and an output adds kw / 4
// or kw / 5 group sums and the few entries left over, since kw 8-byte reads per output are what
// the LDS then limits.  The work per output is at most about 20 LDS reads and a constant: it does
// not grow with the window's area.  The Q pass (QPASS) runs the same walk, adds
// n S2 - S1^2 per lane in 64 bits, per channel in LDS, and issues one 64-bit integer atomic add
// per workgroup; the filter pass then recomputes the sums and turns Q into the noise on the
// device.  Integer sums and integer atomics: no result depends on the order of execution or on
// the batch an image came in.
#include "idn_common.hpp"
#include "abi_args.hpp"

#include <limits.h>

namespace idn {

constexpr int WN_SR = 128;                    // output rows per workgroup
constexpr int WN_TW = 256;                    // output byte columns per workgroup
constexpr int WN_KMAX = 31;                   // largest window side
constexpr int WN_HALO = (WN_KMAX - 1) * 3;    // halo byte columns at 3 channels
constexpr int WN_NS = WN_TW + WN_HALO;        // staged byte columns of a tile
constexpr int WN_TWO_LEVEL = 21;              // narrowest window summed in two levels
constexpr int WN_STEP = 4;                    // rows whose loads are in flight together
constexpr int64_t WN_EST_MAX = 1ll << 28;     // samples per plane the 64-bit Q holds
static_assert(WN_HALO <= WN_TW, "a lane carries at most one halo column");
static_assert(961ull * 65025ull <= 0xFFFFFFFFull, "32-bit window sums");

struct WnCol {
  uint32_t off;   // byte offset of the (border-mapped) source column within a row
  uint32_t mask;  // 0: the column contributes zeros (off is 0 then)
};

// staged column s of the tile: byte column jb - rw c + s of the image, extended by the border
__device__ __forceinline__ WnCol wn_col(int j, int w, int c, int rw, int border) {
  const WnCol none = {0u, 0u};
  const int wb = w * c;
  if (j < -rw * c || j >= wb + rw * c) return none;  // beyond every window of the image
  const int e = j + WN_KMAX * c;                      // >= 0
  int px = e / c - WN_KMAX;
  const int ch = e % c;
  if (px < 0 || px >= w) {
    if (border == IDN_WIENER_ZERO) return none;
    px = reflect101(px, w);
  }
  return WnCol{(uint32_t)(px * c + ch), ~0u};
}

// s / n for an integer window sum s: the product with r = 1 / n and Markstein's correction.  It
// equals the IEEE quotient for every window size and every sum the filter can form, 0 .. 255^2 n:
// tools/check_wiener_div.c goes through all 2.2e9 of them
__device__ __forceinline__ double wn_div(double s, double n, double r) {
  const double q0 = s * r;
  return __builtin_fma(__builtin_fma(-q0, n, s), r, q0);
}

template <bool QPASS, int C>
__global__ __launch_bounds__(256) void wiener_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst_u8, double* __restrict__ dst_f64,
    int h, int w, int64_t row_stride, int kh, int kw, int border, int sr, int two_from,
    int tiles, int strips, const double* __restrict__ noise, int64_t noise_image_stride,
    double* __restrict__ noise_out, unsigned long long* __restrict__ q) {
  __shared__ __attribute__((aligned(16))) v2u cs[2][WN_NS];
  __shared__ __attribute__((aligned(16))) v2u gs[WN_NS];  // behind a barrier of its own: one buffer
  __shared__ uint8_t ring[WN_KMAX + 1][WN_NS];
  __shared__ unsigned long long qs[3];

  constexpr int c = C;
  const int t = threadIdx.x;
  const int wgs = tiles * strips;
  const int img = blockIdx.x / wgs;
  const int rem = blockIdx.x - img * wgs;
  const int strip = rem / tiles;
  const int tile = rem - strip * tiles;

  const int rh = kh >> 1, rw = kw >> 1;
  const int wb = w * c;
  const int halo = (kw - 1) * c;
  const uint32_t np = (uint32_t)(kh * kw);
  const int jb = tile * WN_TW;
  const int jo = jb + t;  // this lane's output byte column
  const bool out_ok = jo < wb;
  const int ch = jo % c;
  const int y0 = strip * sr, y1 = min(y0 + sr, h);  // output rows [y0, y1)

  const WnCol c0 = wn_col(jb - rw * c + t, w, c, rw, border);
  const bool has1 = t < halo;
  const WnCol c1 = has1 ? wn_col(jb - rw * c + WN_TW + t, w, c, rw, border) : WnCol{0u, 0u};
  // whether any lane of this wave carries a halo column (wave-uniform)
  const bool wave_has1 = (int)__builtin_amdgcn_readfirstlane((uint32_t)t) < halo;

  const uint8_t* base = src + (int64_t)img * h * row_stride;
  const int r_first = y0 - rh, r_last = y1 - 1 + rh;
  // an extended row of the walk: the image row it reads (always inside the image) and whether it
  // counts (a row outside the image is zeros under the zero border)
  auto row_of = [&](int r) -> int {
    r = min(r, r_last);
    if (r < 0 || r >= h) r = border == IDN_WIENER_ZERO ? clampi(r, 0, h - 1) : reflect101(r, h);
    return r;
  };
  auto row_mask = [&](int r) -> uint32_t {
    return (border == IDN_WIENER_ZERO && (r < 0 || r >= h)) ? 0u : ~0u;
  };

  double nz = 0.0, dn = 0.0, rn = 0.0;
  if (!QPASS) {
    dn = (double)np;
    rn = 1.0 / dn;
    if (noise) {
      nz = noise[(int64_t)img * noise_image_stride + ch];
    } else {
      nz = (double)q[img * c + ch] / (double)((uint64_t)np * np * (uint64_t)h * (uint64_t)w);
    }
    if (noise_out && rem == 0 && t < c) noise_out[img * c + t] = nz;  // t < c: ch == t
  } else {
    if (t < 3) qs[t] = 0;
  }

  // the two-level horizontal sum of wide windows: ngrp groups of grp column sums each
  const bool two = kw >= two_from;
  const int grp = kw >= 25 ? 5 : 4, ngrp = kw / grp;
  const int gspan = (ngrp - 1) * grp * c;  // halo columns whose group sum an output reads
  const int depth = kh + 1;                  // ring slots: row r lives in slot (r - r_first) % depth
  uint32_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;  // running column sums of t and t^2
  unsigned long long qacc = 0;
  uint8_t n0[WN_STEP], n1[WN_STEP];
#pragma unroll
  for (int k = 0; k < WN_STEP; ++k) {
    const int64_t ro = (int64_t)row_of(r_first + k) * row_stride;
    n0[k] = base[ro + c0.off];
    n1[k] = 0;
    if (wave_has1) n1[k] = base[ro + c1.off];
  }
  int slot = 0;
  for (int rs = r_first; rs <= r_last; rs += WN_STEP) {
    uint8_t v0[WN_STEP], v1[WN_STEP];
#pragma unroll
    for (int k = 0; k < WN_STEP; ++k) {
      v0[k] = n0[k];
      v1[k] = n1[k];
    }
    if (rs + WN_STEP <= r_last) {  // the next step's samples, in flight across this step's barriers
#pragma unroll
      for (int k = 0; k < WN_STEP; ++k) {
        const int64_t ro = (int64_t)row_of(rs + WN_STEP + k) * row_stride;
        n0[k] = base[ro + c0.off];
        if (wave_has1) n1[k] = base[ro + c1.off];
      }
    }
#pragma unroll
    for (int k = 0; k < WN_STEP; ++k) {
      const int r = rs + k;
      if (r > r_last) break;
      const uint32_t rm = row_mask(r);
      const int lslot = slot + 1 == depth ? 0 : slot + 1;  // row r - kh (depth = kh + 1)
      const bool leaves = r - kh >= r_first;
      const int buf = (r - r_first) & 1;
      {
        const uint32_t e = (uint32_t)v0[k] & rm & c0.mask;
        const uint32_t l = leaves ? (uint32_t)ring[lslot][t] : 0u;
        ring[slot][t] = (uint8_t)e;
        a0 += e - l;
        b0 += e * e - l * l;
        cs[buf][t] = v2u{a0, b0};
      }
      if (has1) {
        const uint32_t e = (uint32_t)v1[k] & rm & c1.mask;
        const uint32_t l = leaves ? (uint32_t)ring[lslot][WN_TW + t] : 0u;
        ring[slot][WN_TW + t] = (uint8_t)e;
        a1 += e - l;
        b1 += e * e - l * l;
        cs[buf][WN_TW + t] = v2u{a1, b1};
      }
      __syncthreads();
      const int yo = r - rh;
      if (two && yo >= y0) {
        // wide windows: sums of grp neighbouring column sums first, so that an output adds
        // kw / grp of them (and kw % grp single ones) instead of kw
        {
          const v2u* tap = &cs[buf][t];
          uint32_t g1 = 0, g2 = 0;
#pragma unroll 5
          for (int i = 0; i < grp; ++i) {
            const v2u v = tap[i * c];
            g1 += v.x;
            g2 += v.y;
          }
          gs[t] = v2u{g1, g2};
        }
        if (t < gspan) {
          const v2u* tap = &cs[buf][WN_TW + t];
          uint32_t g1 = 0, g2 = 0;
#pragma unroll 5
          for (int i = 0; i < grp; ++i) {
            const v2u v = tap[i * c];
            g1 += v.x;
            g2 += v.y;
          }
          gs[WN_TW + t] = v2u{g1, g2};
        }
        __syncthreads();
      }
      if (yo >= y0 && out_ok) {
        uint32_t s1 = 0, s2 = 0;
        if (two) {
          const v2u* gtap = &gs[t];
#pragma unroll 4
          for (int j = 0; j < ngrp; ++j) {
            const v2u v = gtap[j * grp * c];
            s1 += v.x;
            s2 += v.y;
          }
          const v2u* tap = &cs[buf][t + ngrp * grp * c];
          for (int i = 0; i < kw - ngrp * grp; ++i) {
            const v2u v = tap[i * c];
            s1 += v.x;
            s2 += v.y;
          }
        } else {
          // the window's kw column sums: the middle one, then pairs from both ends, several
          // reads in flight at once (one read per trip would wait out the LDS latency kw times)
          const v2u* tap = &cs[buf][t];
          const v2u mid = tap[rw * c];
          s1 = mid.x;
          s2 = mid.y;
#pragma unroll 4
          for (int i = 0; i < rw; ++i) {
            const v2u lo = tap[i * c], hi = tap[(kw - 1 - i) * c];
            s1 += lo.x + hi.x;
            s2 += lo.y + hi.y;
          }
        }
        if (QPASS) {
          qacc += (unsigned long long)np * s2 - (unsigned long long)s1 * s1;
        } else {
          // the output's own sample: row r - rh of the ring, staged column t + rw c.  Inside the
          // image no mask touched it
          const int cslot = slot - rh < 0 ? slot - rh + depth : slot - rh;
          const double xc = (double)ring[cslot][t + rw * c];
          const double m = wn_div((double)s1, dn, rn);
          const double var = wn_div((double)s2, dn, rn) - m * m;
          double res = m;
          if (var != 0.0 && !(var < nz)) res = (xc - m) * (1.0 - nz / var) + m;
          const int64_t row = (int64_t)img * h + yo;
          if (dst_f64) dst_f64[row * wb + jo] = res;
          if (dst_u8) {
            const double b = fmin(fmax(rint(res), 0.0), 255.0);  // a NaN gives 0
            dst_u8[row * row_stride + jo] = (uint8_t)(int)b;
          }
        }
      }
      slot = lslot;
    }
  }
  if (QPASS) {
    if (qacc) atomicAdd(&qs[ch], qacc);  // integer, LDS
    __syncthreads();
    if (t < c && qs[t]) atomicAdd(&q[img * c + t], qs[t]);  // one vector atomic per workgroup
  }
}

template <bool QPASS>
static void wn_launch(int c, unsigned grid, hipStream_t s, const uint8_t* src, uint8_t* dst_u8,
                      double* dst_f64, int h, int w, int64_t row_stride, int kh, int kw,
                      int border, int sr, int two_from, int tiles, int strips,
                      const double* noise,
                      int64_t noise_image_stride, double* noise_out, unsigned long long* q) {
  if (c == 1)
    hipLaunchKernelGGL((wiener_kernel<QPASS, 1>), dim3(grid), dim3(256), 0, s, src, dst_u8,
                       dst_f64, h, w, row_stride, kh, kw, border, sr, two_from, tiles, strips,
                       noise, noise_image_stride, noise_out, q);
  else
    hipLaunchKernelGGL((wiener_kernel<QPASS, 3>), dim3(grid), dim3(256), 0, s, src, dst_u8,
                       dst_f64, h, w, row_stride, kh, kw, border, sr, two_from, tiles, strips,
                       noise, noise_image_stride, noise_out, q);
}

}  // namespace idn

extern "C" size_t idn_wiener_workspace_size(int n, int c) {
  if (n <= 0 || (c != 1 && c != 3)) return 0;
  return (size_t)n * c * sizeof(uint64_t);
}

extern "C" int idn_wiener_u8(const uint8_t* src, uint8_t* dst_u8, double* dst_f64, int n, int h,
                             int w, int c, int64_t row_stride, int kh, int kw, int border,
                             const double* noise, int64_t noise_image_stride, double* noise_out,
                             void* workspace, size_t ws_bytes, void* stream) {
  using namespace idn;
  const char* name = "idn_wiener_u8";
  IDN_CHECK_ARG(src, "%s: null pointer (src)", name);
  IDN_CHECK_ARG(dst_u8 || dst_f64, "%s: both destinations are null", name);
  if (int e = check_not_in_place(name, src, dst_u8, "dst_u8 == src")) return e;
  if (int e = check_image_1_or_3(name, n, h, w, c, row_stride)) return e;
  IDN_CHECK_ARG(kh >= 1 && kh <= WN_KMAX && (kh & 1) && kw >= 1 && kw <= WN_KMAX && (kw & 1),
                "%s: window sides must be odd and in 1..%d (got %d x %d)", name, WN_KMAX, kh, kw);
  IDN_CHECK_ARG(border == IDN_WIENER_ZERO || border == IDN_WIENER_REFLECT101,
                "%s: unknown border %d", name, border);
  IDN_CHECK_ARG(border != IDN_WIENER_REFLECT101 || (kh / 2 < h && kw / 2 < w),
                "%s: reflect101 needs kh/2 < h and kw/2 < w (window %d x %d, image %d x %d)", name,
                kh, kw, h, w);
  IDN_CHECK_ARG(((uintptr_t)dst_f64 & 7) == 0, "%s: dst_f64 must be 8-byte aligned", name);
  IDN_CHECK_ARG(((uintptr_t)noise & 7) == 0 && ((uintptr_t)noise_out & 7) == 0,
                "%s: noise and noise_out must be 8-byte aligned", name);
  IDN_CHECK_ARG(!noise || noise_image_stride == 0 || noise_image_stride == c,
                "%s: noise_image_stride must be 0 or c (got %lld)", name,
                (long long)noise_image_stride);
  if (n == 0) return IDN_OK;
  // IDN_WN_SR (tuning build only): output rows per workgroup
  const int sr_knob = knob("IDN_WN_SR", WN_SR);
  const int sr = sr_knob < 1 ? 1 : sr_knob;
  // IDN_WN_TWO (tuning build only): the narrowest window summed in two levels (at least 8)
  const int two_knob = knob("IDN_WN_TWO", WN_TWO_LEVEL);
  const int two_from = two_knob < 8 ? 8 : two_knob;
  const int64_t wb = (int64_t)w * c;
  const int64_t tiles = (wb + WN_TW - 1) / WN_TW, strips = ((int64_t)h + sr - 1) / sr;
  if (wb > INT_MAX - WN_KMAX * 3 - WN_TW || (int64_t)n * tiles * strips > INT_MAX)
    return batch_too_large(name);
  unsigned long long* q = nullptr;
  if (!noise) {
    if ((int64_t)h * w > WN_EST_MAX)
      return set_error(IDN_EUNSUPPORTED, "%s: the noise estimate takes planes of at most 2^28 "
                       "samples (got %d x %d)", name, h, w);
    if (int e = check_workspace(name, workspace, ws_bytes, idn_wiener_workspace_size(n, c)))
      return e;
    q = static_cast<unsigned long long*>(workspace);
  }

  const hipStream_t s = as_stream(stream);
  const unsigned grid = (unsigned)((int64_t)n * tiles * strips);
  if (q) {
    if (hipMemsetAsync(q, 0, (size_t)n * c * sizeof(uint64_t), s) != hipSuccess)
      return set_error(IDN_EHIP, "%s: clearing the workspace failed", name);
    wn_launch<true>(c, grid, s, src, nullptr, nullptr, h, w, row_stride, kh, kw, border, sr,
                    two_from, (int)tiles, (int)strips, nullptr, 0, nullptr, q);
    IDN_CHECK_LAUNCH(name);
  }
  wn_launch<false>(c, grid, s, src, dst_u8, dst_f64, h, w, row_stride, kh, kw, border, sr,
                   two_from, (int)tiles, (int)strips, noise, noise_image_stride, noise_out, q);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}
