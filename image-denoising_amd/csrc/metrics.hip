// Quality metrics of skimage 0.14.2 on u8 image pairs that already live on the device:
// compare_mse and compare_ssim(multichannel=True, uniform window, sample covariance).  Not on the
// reference's preprocessing path: they score a denoiser of the bank against the clean batch.
//
// SSIM.  With the integer window sums sx, sy, sxx, syy, sxy of one win x win window (NP = win^2)
//   cx = NP sxx - sx^2   cy = NP syy - sy^2   cxy = NP sxy - sx sy            (exact integers)
//   A1 = 2 sx sy + C1 NP^2           B1 = sx^2 + sy^2 + C1 NP^2
//   A2 = 2 cxy   + C2 NP (NP - 1)    B2 = cx + cy     + C2 NP (NP - 1)
//   S  = (A1 A2) / (B1 B2)                                                    (float64)
// is skimage's S (vx = NP / (NP - 1) (uxx - ux^2), ...) multiplied through by NP^2 and NP (NP - 1).
// For win <= 11 every integer fits 32 bits, so the moments are carried exactly and only the two
// products, the division and the sums round.  skimage filters with reflection and crops
// (win - 1) / 2 from each side: only the windows that lie wholly inside the image enter the mean.
//
// ssim_strip_kernel: one 256-thread workgroup owns MT_SR output rows x TL interleaved byte columns
// of one image pair; a lane owns one byte column (its channel is lane % C: TL is a multiple of C).
// Per input row a lane adds the entering byte pair to its five vertical moments and subtracts the
// pair that leaves the window (the row win rows up, re-read through L1), publishes the moments as
// one 16-byte LDS entry (sx | sy << 16, sxx, syy, sxy; two buffers, one barrier per row), and the
// TL - (win - 1) C lanes with a whole window to their right add the win entries C lanes apart and
// evaluate S.  A lane's S values add up in row order, the workgroup's per channel in a fixed LDS
// tree, and the workgroup stores its channel sums (and its share of the squared error: every byte
// is counted by exactly one workgroup) as one 32-byte partial.  ssim_final_kernel adds the partials
// of an image in a fixed order: no floating-point atomics, the result does not depend on timing
// or on the batch the pair came in.
//
// mse_partial_kernel: flat two-input reduction, 16-byte buffer loads at any alignment, 8 per lane
// in flight per input (copy.hip's burst), exact integer sums; the partials are added by
// mse_final_kernel and divided once in float64: bit-equal to numpy's mean of the squared
// float64 differences, whose partial sums all stay below 2^53.
#include "idn_common.hpp"
#include "abi_args.hpp"

#include <limits.h>

namespace idn {

constexpr int MT_SR = 32;                  // output rows per ssim workgroup
constexpr int MSE_NL = 8;                  // 16-byte units per lane of one mse workgroup
constexpr uint32_t MSE_UNITS = MSE_NL * 256u;
constexpr uint32_t MT_OOB = 0x40000000u;   // buffer offset past every image (images < 1 GiB)
constexpr int64_t MT_IMG_MAX = 0x40000000; // largest image the buffer offsets address

constexpr int ssim_tile(int c) { return c == 3 ? 255 : 256; }

// ---- SSIM -----------------------------------------------------------------------------------------

template <int WIN, int C>
__global__ __launch_bounds__(256) void ssim_strip_kernel(const uint8_t* __restrict__ a,
                                                         const uint8_t* __restrict__ b, int h,
                                                         int wb, int64_t stride_a,
                                                         int64_t stride_b, int tiles, int strips,
                                                         double c1s, double c2s,
                                                         double* __restrict__ part) {
  constexpr int HALO = (WIN - 1) * C;
  constexpr int TL = ssim_tile(C);
  constexpr int TOUT = TL - HALO;
  constexpr int NPX = TL / C;
  constexpr uint32_t NP = WIN * WIN;
  static_assert(TL % C == 0 && TOUT % C == 0 && HALO <= TOUT, "tile shape");
  static_assert(2ull * (NP * 255ull) * (NP * 255ull) <= 0xFFFFFFFFull, "32-bit moments");

  __shared__ __attribute__((aligned(16))) v4u vs[2][256];
  __shared__ double red[256];
  __shared__ uint32_t sse_wg;

  const int t = threadIdx.x;
  const int wgs = tiles * strips;
  const int img = blockIdx.x / wgs;
  const int rem = blockIdx.x - img * wgs;
  const int strip = rem / tiles;
  const int tile = rem - strip * tiles;

  const int y0 = strip * MT_SR;
  const int y_in_end = min(y0 + MT_SR, h - WIN + 1) + WIN - 1;  // input rows [y0, y_in_end)
  // squared error: the rows and columns this workgroup alone counts
  const int own_rows_end = strip == strips - 1 ? h : y0 + MT_SR;
  const int j = tile * TOUT + t;
  const bool col_ok = t < TL && j < wb;
  const bool out_ok = t < TOUT && j < wb - HALO;
  const bool own_col = col_ok && (t < TOUT || tile == tiles - 1);

  const uint8_t* pa = a + (int64_t)img * h * stride_a + j;  // dereferenced under col_ok only
  const uint8_t* pb = b + (int64_t)img * h * stride_b + j;

  if (t == 0) sse_wg = 0;
  uint32_t vp = 0, vxx = 0, vyy = 0, vxy = 0, sse = 0;
  double acc = 0.0;
  uint32_t xa = 0, xb = 0, la = 0, lb = 0;  // entering and leaving byte pair of row y
  if (col_ok) {
    xa = pa[(int64_t)y0 * stride_a];
    xb = pb[(int64_t)y0 * stride_b];
  }
  for (int y = y0; y < y_in_end; ++y) {
    // next row's pairs, in flight across this row's barrier
    uint32_t na = 0, nb = 0, nla = 0, nlb = 0;
    if (col_ok && y + 1 < y_in_end) {
      na = pa[(int64_t)(y + 1) * stride_a];
      nb = pb[(int64_t)(y + 1) * stride_b];
      if (y + 1 - WIN >= y0) {
        nla = pa[(int64_t)(y + 1 - WIN) * stride_a];
        nlb = pb[(int64_t)(y + 1 - WIN) * stride_b];
      }
    }
    vp += (xa | (xb << 16)) - (la | (lb << 16));
    vxx += xa * xa - la * la;
    vyy += xb * xb - lb * lb;
    vxy += xa * xb - la * lb;
    if (own_col && y < own_rows_end) {
      const int d = (int)xa - (int)xb;
      sse += (uint32_t)(d * d);
    }
    const int buf = (y - y0) & 1;
    vs[buf][t] = v4u{vp, vxx, vyy, vxy};
    __syncthreads();
    if (y - y0 >= WIN - 1 && out_ok) {
      uint32_t hp = 0, hxx = 0, hyy = 0, hxy = 0;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const v4u v = vs[buf][t + k * C];
        hp += v.x;
        hxx += v.y;
        hyy += v.z;
        hxy += v.w;
      }
      const uint32_t sx = hp & 0xFFFFu, sy = hp >> 16;
      const uint32_t sxsy = sx * sy, sx2 = sx * sx, sy2 = sy * sy;
      const uint32_t cx = NP * hxx - sx2, cy = NP * hyy - sy2;
      const int32_t cxy = (int32_t)(NP * hxy) - (int32_t)sxsy;
      const double A1 = (double)(2u * sxsy) + c1s;
      const double B1 = (double)(sx2 + sy2) + c1s;
      const double A2 = (double)(2 * cxy) + c2s;
      const double B2 = (double)(cx + cy) + c2s;
      acc += (A1 * A2) / (B1 * B2);
    }
    xa = na;
    xb = nb;
    la = nla;
    lb = nlb;
  }

  // per channel: lanes t, t + C, ... in a fixed tree over the pixel index t / C
  red[t] = acc;
  if (sse) atomicAdd(&sse_wg, sse);  // integer, LDS: <= 256 lanes * 42 rows * 255^2 < 2^32
  __syncthreads();
  const int p = t / C;
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < TL && p < s && p + s < NPX) red[t] += red[t + s * C];
    __syncthreads();
  }
  double* q = part + (int64_t)blockIdx.x * 4;
  if (t < C) q[t] = red[t];
  if (t == 0) reinterpret_cast<uint64_t*>(q)[3] = sse_wg;
}

// the fixed-order sum of a 256-entry LDS array into entry 0
template <typename T>
__device__ __forceinline__ void tree256(T* r, int t) {
  for (int s = 128; s >= 1; s >>= 1) {
    __syncthreads();
    if (t < s) r[t] += r[t + s];
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void ssim_final_kernel(const double* __restrict__ part, int wgs,
                                                         int c, double count, double nelem,
                                                         double* __restrict__ ssim_out,
                                                         double* __restrict__ ch_out,
                                                         double* __restrict__ mse_out) {
  __shared__ double rs[3][256];
  __shared__ uint64_t re[256];
  const int t = threadIdx.x;
  const int img = blockIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  uint64_t e = 0;
  for (int i = t; i < wgs; i += 256) {
    const double* q = part + ((int64_t)img * wgs + i) * 4;
    for (int ch = 0; ch < c; ++ch) s[ch] += q[ch];
    e += reinterpret_cast<const uint64_t*>(q)[3];
  }
  for (int ch = 0; ch < 3; ++ch) rs[ch][t] = s[ch];
  re[t] = e;
  for (int ch = 0; ch < c; ++ch) tree256(rs[ch], t);
  tree256(re, t);
  if (t == 0) {
    double m[3];
    for (int ch = 0; ch < c; ++ch) {
      m[ch] = rs[ch][0] / count;
      if (ch_out) ch_out[(int64_t)img * c + ch] = m[ch];
    }
    ssim_out[img] = c == 3 ? ((m[0] + m[1]) + m[2]) / 3.0 : m[0];
    if (mse_out) mse_out[img] = (double)re[0] / nelem;
  }
}

// ---- MSE ------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t sq_diff4(uint32_t x, uint32_t y) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = (int)((x >> (8 * k)) & 255u) - (int)((y >> (8 * k)) & 255u);
    s += (uint32_t)(d * d);
  }
  return s;
}

// An image is `rows` rows of `rowlen` bytes (a compact image: one row of h*w*c bytes), cut into
// 16-byte units; a unit that crosses the row's end is read byte by byte.
__global__ __launch_bounds__(256) void mse_partial_kernel(const uint8_t* __restrict__ a,
                                                          const uint8_t* __restrict__ b,
                                                          uint32_t rows, uint32_t rowlen,
                                                          uint32_t stride_a, uint32_t stride_b,
                                                          int64_t pitch_a, int64_t pitch_b,
                                                          uint32_t upr, uint32_t total_units,
                                                          uint32_t wgs,
                                                          uint64_t* __restrict__ part) {
  __shared__ uint32_t sse_wg;
  const uint32_t t = threadIdx.x;
  const uint32_t img = blockIdx.x / wgs;
  const uint32_t wg = blockIdx.x - img * wgs;
  const uint8_t* ia = a + (int64_t)img * pitch_a;
  const uint8_t* ib = b + (int64_t)img * pitch_b;
  const rsrc_t ra = make_rsrc(ia, (rows - 1) * stride_a + rowlen);
  const rsrc_t rb = make_rsrc(ib, (rows - 1) * stride_b + rowlen);
  if (t == 0) sse_wg = 0;
  __syncthreads();

  v4u va[MSE_NL], vb[MSE_NL];
#pragma unroll
  for (int i = 0; i < MSE_NL; ++i) {
    const uint32_t u = wg * MSE_UNITS + 256u * i + t;
    const uint32_t row = u / upr, off = (u - row * upr) * 16u;
    const bool full = u < total_units && off + 16u <= rowlen;
    va[i] = __builtin_amdgcn_raw_buffer_load_b128(ra, full ? row * stride_a + off : MT_OOB, 0, 0);
    vb[i] = __builtin_amdgcn_raw_buffer_load_b128(rb, full ? row * stride_b + off : MT_OOB, 0, 0);
  }
  uint32_t sse = 0;  // <= 8 units * 16 bytes * 255^2 per lane, * 256 lanes < 2^32
#pragma unroll
  for (int i = 0; i < MSE_NL; ++i)
    sse += sq_diff4(va[i].x, vb[i].x) + sq_diff4(va[i].y, vb[i].y) + sq_diff4(va[i].z, vb[i].z) +
           sq_diff4(va[i].w, vb[i].w);
#pragma unroll
  for (int i = 0; i < MSE_NL; ++i) {
    const uint32_t u = wg * MSE_UNITS + 256u * i + t;
    const uint32_t row = u / upr, off = (u - row * upr) * 16u;
    if (u < total_units && off + 16u > rowlen) {
      for (uint32_t e = off; e < rowlen; ++e) {
        const int d = (int)ia[(int64_t)row * stride_a + e] - (int)ib[(int64_t)row * stride_b + e];
        sse += (uint32_t)(d * d);
      }
    }
  }
  if (sse) atomicAdd(&sse_wg, sse);
  __syncthreads();
  if (t == 0) part[blockIdx.x] = sse_wg;
}

__global__ __launch_bounds__(256) void mse_final_kernel(const uint64_t* __restrict__ part, int wgs,
                                                        double nelem,
                                                        double* __restrict__ mse_out) {
  __shared__ uint64_t re[256];
  const int t = threadIdx.x;
  uint64_t e = 0;
  for (int i = t; i < wgs; i += 256) e += part[(int64_t)blockIdx.x * wgs + i];
  re[t] = e;
  tree256(re, t);
  if (t == 0) mse_out[blockIdx.x] = (double)re[0] / nelem;
}

// ---- host side --------------------------------------------------------------------------------------

struct SsimGeom {
  int tiles, strips;
};

static SsimGeom ssim_geom(int h, int w, int c, int win) {
  const int tout = ssim_tile(c) - (win - 1) * c;
  SsimGeom g;
  g.tiles = ((w - win + 1) * c + tout - 1) / tout;
  g.strips = ((h - win + 1) + MT_SR - 1) / MT_SR;
  return g;
}

// mse workgroups per image; a compact image (both strides == w*c) is one row of h*w*c bytes
static int64_t mse_wgs(int h, int w, int c, bool compact) {
  const int64_t units = compact ? ((int64_t)h * w * c + 15) / 16 : (int64_t)h * (((int64_t)w * c + 15) / 16);
  return (units + MSE_UNITS - 1) / MSE_UNITS;
}

static bool win_ok(int win) { return win >= 3 && win <= 11 && (win & 1); }
// the two images of a metric; their pointers and strides are worded together
static int check_pair(const char* name, const uint8_t* a, const uint8_t* b, int n, int h, int w,
                      int c, int64_t row_stride_a, int64_t row_stride_b) {
  IDN_CHECK_ARG(a && b, "%s: null pointer", name);
  if (int e = check_shape(name, n, h, w)) return e;
  if (int e = check_channels_1_or_3(name, c)) return e;
  IDN_CHECK_ARG(row_stride_a >= (int64_t)w * c && row_stride_b >= (int64_t)w * c,
                "%s: row_stride %lld / %lld < w*c", name, (long long)row_stride_a,
                (long long)row_stride_b);
  return IDN_OK;
}

template <int WIN>
static void launch_ssim(int c, unsigned grid, hipStream_t st, const uint8_t* a, const uint8_t* b,
                        int h, int wb, int64_t sa, int64_t sb, SsimGeom g, double c1s, double c2s,
                        double* part) {
  if (c == 3)
    hipLaunchKernelGGL((ssim_strip_kernel<WIN, 3>), dim3(grid), dim3(256), 0, st, a, b, h, wb, sa,
                       sb, g.tiles, g.strips, c1s, c2s, part);
  else
    hipLaunchKernelGGL((ssim_strip_kernel<WIN, 1>), dim3(grid), dim3(256), 0, st, a, b, h, wb, sa,
                       sb, g.tiles, g.strips, c1s, c2s, part);
}

}  // namespace idn

extern "C" size_t idn_metrics_workspace_size(int n, int h, int w, int c, int win_size) {
  using namespace idn;
  if (n <= 0 || h <= 0 || w <= 0 || (c != 1 && c != 3)) return 0;
  size_t need = (size_t)n * (size_t)mse_wgs(h, w, c, false) * sizeof(uint64_t);
  if (win_ok(win_size) && h >= win_size && w >= win_size) {
    const SsimGeom g = ssim_geom(h, w, c, win_size);
    const size_t s = (size_t)n * g.tiles * g.strips * 4 * sizeof(double);
    if (s > need) need = s;
  }
  return need;
}

extern "C" int idn_mse_u8(const uint8_t* a, const uint8_t* b, double* mse_out, int n, int h, int w,
                          int c, int64_t row_stride_a, int64_t row_stride_b, void* workspace,
                          size_t workspace_bytes, void* stream) {
  using namespace idn;
  if (int e = check_pair("idn_mse_u8", a, b, n, h, w, c, row_stride_a, row_stride_b)) return e;
  IDN_CHECK_ARG(mse_out, "idn_mse_u8: null pointer (mse_out)");
  if (n == 0) return IDN_OK;
  const int64_t wc = (int64_t)w * c;
  if ((int64_t)h * row_stride_a > MT_IMG_MAX || (int64_t)h * row_stride_b > MT_IMG_MAX)
    return set_error(IDN_EUNSUPPORTED, "idn_mse_u8: images above 1 GiB are not supported");
  const bool compact = row_stride_a == wc && row_stride_b == wc;
  const int64_t wgs = mse_wgs(h, w, c, compact);
  const size_t need = (size_t)n * (size_t)wgs * sizeof(uint64_t);
  if (int e = check_workspace("idn_mse_u8", workspace, workspace_bytes, need)) return e;
  if ((int64_t)n * wgs > (int64_t)INT_MAX) return batch_too_large("idn_mse_u8");
  const uint32_t rows = compact ? 1u : (uint32_t)h;
  const uint32_t rowlen = compact ? (uint32_t)(h * wc) : (uint32_t)wc;
  const uint32_t upr = (rowlen + 15u) / 16u;
  uint64_t* part = static_cast<uint64_t*>(workspace);
  hipLaunchKernelGGL(mse_partial_kernel, dim3((unsigned)(n * wgs)), dim3(256), 0, as_stream(stream),
                     a, b, rows, rowlen, (uint32_t)row_stride_a, (uint32_t)row_stride_b,
                     (int64_t)h * row_stride_a, (int64_t)h * row_stride_b, upr, rows * upr,
                     (uint32_t)wgs, part);
  IDN_CHECK_LAUNCH("idn_mse_u8");
  hipLaunchKernelGGL(mse_final_kernel, dim3((unsigned)n), dim3(256), 0, as_stream(stream), part,
                     (int)wgs, (double)((int64_t)h * wc), mse_out);
  IDN_CHECK_LAUNCH("idn_mse_u8");
  return IDN_OK;
}

extern "C" int idn_ssim_u8(const uint8_t* a, const uint8_t* b, double* ssim_out,
                           double* ssim_ch_out, double* mse_out, int n, int h, int w, int c,
                           int64_t row_stride_a, int64_t row_stride_b, int win_size,
                           void* workspace, size_t workspace_bytes, void* stream) {
  using namespace idn;
  if (int e = check_pair("idn_ssim_u8", a, b, n, h, w, c, row_stride_a, row_stride_b)) return e;
  IDN_CHECK_ARG(ssim_out, "idn_ssim_u8: null pointer (ssim_out)");
  IDN_CHECK_ARG(win_ok(win_size), "idn_ssim_u8: win_size must be odd and in 3..11 (got %d)",
                win_size);
  IDN_CHECK_ARG(h >= win_size && w >= win_size,
                "idn_ssim_u8: win_size %d exceeds the image (%d x %d)", win_size, h, w);
  if (n == 0) return IDN_OK;
  const SsimGeom g = ssim_geom(h, w, c, win_size);
  const int64_t wgs = (int64_t)g.tiles * g.strips;
  const size_t need = (size_t)n * (size_t)wgs * 4 * sizeof(double);
  if (int e = check_workspace("idn_ssim_u8", workspace, workspace_bytes, need)) return e;
  if ((int64_t)n * wgs > (int64_t)INT_MAX) return batch_too_large("idn_ssim_u8");
  const double np = (double)(win_size * win_size);
  const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double c1s = c1 * (np * np), c2s = c2 * (np * (np - 1.0));
  double* part = static_cast<double*>(workspace);
  const unsigned grid = (unsigned)(n * wgs);
  const hipStream_t st = as_stream(stream);
  const int wb = w * c;
  switch (win_size) {
    case 3: launch_ssim<3>(c, grid, st, a, b, h, wb, row_stride_a, row_stride_b, g, c1s, c2s, part); break;
    case 5: launch_ssim<5>(c, grid, st, a, b, h, wb, row_stride_a, row_stride_b, g, c1s, c2s, part); break;
    case 7: launch_ssim<7>(c, grid, st, a, b, h, wb, row_stride_a, row_stride_b, g, c1s, c2s, part); break;
    case 9: launch_ssim<9>(c, grid, st, a, b, h, wb, row_stride_a, row_stride_b, g, c1s, c2s, part); break;
    default: launch_ssim<11>(c, grid, st, a, b, h, wb, row_stride_a, row_stride_b, g, c1s, c2s, part); break;
  }
  IDN_CHECK_LAUNCH("idn_ssim_u8");
  const double count = (double)((int64_t)(h - win_size + 1) * (w - win_size + 1));
  hipLaunchKernelGGL(ssim_final_kernel, dim3((unsigned)n), dim3(256), 0, st, part, (int)wgs, c,
                     count, (double)((int64_t)h * w * c), ssim_out, ssim_ch_out, mse_out);
  IDN_CHECK_LAUNCH("idn_ssim_u8");
  return IDN_OK;
}
