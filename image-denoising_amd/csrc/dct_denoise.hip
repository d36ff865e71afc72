// idn_dct_denoise_u8: the sliding 8x8 DCT hard-threshold denoiser (Yu & Sapiro, IPOL 2011) on a u8
// batch, in fp32; tests/dct_model.py is the definition.
//
// Every 8x8 patch of every plane is transformed (D = Cm P Cm^T), its coefficients below the
// plane's threshold are zeroed (the DC term stays), it is transformed back, and every sample is
// the mean of the up to 64 patches that cover it.  With three channels and color = 1 the planes
// are the orthonormal 3-point DCT of the channels, and the result is transformed back.
//
// dct_denoise_kernel: one wave per plane, C waves per workgroup, which owns DD_TW = 57 output
// columns x sr output rows of one image.  Lane l of a wave owns the patch column j = x0 - 7 + l
// (64 patch columns cover 57 output columns completely) and walks down the image:
//   - the row transform of the 8 samples (r, j..j+7) of a new image row r is computed once and
//     kept in a ring of 8 rows x 8 coefficients (registers; the row loop is unrolled by 8 so that
//     every ring index is a constant), where the 8 patches that contain the row find it;
//   - the patch with the top row p = r - 7 then takes 8 column transforms, the threshold and 8
//     inverse column transforms, and adds the result into a second ring, acc, that is still in
//     the row-DCT domain: the inverse row transform is linear, so it runs once per (row, patch
//     column), on the sum of the 8 patches above one another, when row p leaves the ring;
//   - the 8 spatial values a lane then holds for the columns j..j+7 go to LDS, and the lane of
//     output column x adds the 8 values of the patch columns x-7..x in that order, divides by the
//     number of patches that exist there and, under the colour transform, meets the other two
//     planes in LDS.
// 18 one-dimensional transforms per patch instead of 32.  Every sum has a fixed order and nothing
// is an atomic: the same bits on every call and in every batch.  The rows' bytes are asked for
// one row ahead.  A patch column or row outside the image is computed on clamped addresses and
// contributes zeros.
#include "idn_common.hpp"
#include "abi_args.hpp"
#include "dct8.hpp"

#include <limits.h>
#include <math.h>

namespace idn {

constexpr int DD_SR = 128;  // output rows per workgroup
constexpr int DD_TW = 57;   // output columns per workgroup: 64 patch columns less the 7 of the halo
constexpr int DD_P = 8;     // the patch side
static_assert(DD_TW + DD_P - 1 == 64, "one patch column per lane of a wave");

// the orthonormal 3-point DCT of the channels: rows [1,1,1]/sqrt3, [1,0,-1]/sqrt2, [1,-2,1]/sqrt6
__device__ __forceinline__ double dd_m(int r, int c) {
  const double r3 = 0.57735026918962584, r2 = 0.70710678118654757, r6 = 0.40824829046386307;
  if (r == 0) return r3;
  if (r == 1) return c == 0 ? r2 : (c == 1 ? 0.0 : -r2);
  return c == 1 ? -2.0 * r6 : r6;
}

template <int C, bool COLOR>
__global__ __launch_bounds__(64 * C) void dct_denoise_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst_u8, float* __restrict__ dst_f32,
    int h, int w, int64_t row_stride, int sr, int tiles, int strips,
    const double* __restrict__ sigma, int64_t sigma_image_stride, double factor) {
  static_assert(!COLOR || C == 3, "the colour transform needs three channels");
  constexpr int NB = COLOR ? 3 : 1;  // bytes a lane reads per sample
  __shared__ float stage[C][64 + DD_P];
  __shared__ float hz[C][DD_P][64];
  __shared__ float planes[C][64];

  const int k = threadIdx.x >> 6;  // this wave's plane; also the channel it writes
  const int l = threadIdx.x & 63;
  const int wgs = tiles * strips;
  const int img = blockIdx.x / wgs;
  const int rem = blockIdx.x - img * wgs;
  const int strip = rem / tiles;
  const int tile = rem - strip * tiles;
  const int x0 = tile * DD_TW;
  const int y0 = strip * sr, y1 = min(y0 + sr, h);  // output rows [y0, y1)
  const int j = x0 - (DD_P - 1) + l;                // this lane's patch column
  const bool patch_ok = j >= 0 && j <= w - DD_P;
  const int p0 = max(y0 - (DD_P - 1), 0);           // first and last patch row of the walk
  const int p1 = min(y1 - 1, h - DD_P);

  // the plane's threshold, and the row and the column of the colour matrix this wave applies
  float thr, fm0 = 1.f, fm1 = 0.f, fm2 = 0.f, bm0 = 1.f, bm1 = 0.f, bm2 = 0.f;
  {
    const double* sg = sigma + (int64_t)img * sigma_image_stride;
    double sp = sg[k];
    if (COLOR) {
      const double m0 = dd_m(k, 0), m1 = dd_m(k, 1), m2 = dd_m(k, 2);
      fm0 = (float)m0, fm1 = (float)m1, fm2 = (float)m2;
      const double s0 = sg[0], s1 = sg[1], s2 = sg[2];
      sp = sqrt((m0 * m0) * (s0 * s0) + (m1 * m1) * (s1 * s1) + (m2 * m2) * (s2 * s2));
      // column k of the matrix: the inverse transform gives channel k
      bm0 = (float)dd_m(0, k), bm1 = (float)dd_m(1, k), bm2 = (float)dd_m(2, k);
    }
    thr = (float)(factor * sp);
  }
  const float thr1 = thr * DCT_INV_C4;  // one index of the coefficient in {0, 4}
  const float thr2 = thr * 8.0f;        // both

  // the two samples a lane stages per row: columns j and (the first 7 lanes) j + 64, clamped
  const uint8_t* base = src + (int64_t)img * h * row_stride;
  const int ca = clampi(j, 0, w - 1), cb = clampi(j + 64, 0, w - 1);
  const int oa = COLOR ? ca * 3 : ca * C + k, ob = COLOR ? cb * 3 : cb * C + k;
  const bool second = l < DD_P - 1;

  uint8_t na[NB], nb[NB];
  auto fetch = [&](int r) {
    const uint8_t* row = base + (int64_t)min(r, h - 1) * row_stride;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      na[i] = row[oa + i];
      nb[i] = row[ob + i];
    }
  };
  auto plane_value = [&](const uint8_t (&v)[NB]) -> float {
    if (COLOR) return fm0 * (float)v[0] + fm1 * (float)v[1] + fm2 * (float)v[2];
    return (float)v[0];
  };
  // the row transform of the fetched row; asks for the bytes of row `next`
  auto row_dct = [&](int next, float (&out)[8]) {
    stage[k][l] = plane_value(na);
    if (second) stage[k][64 + l] = plane_value(nb);
    fetch(next);
    __syncthreads();
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = stage[k][l + i];
    dct8_fwd(x, out);
    __syncthreads();
  };

  float rc[8][8], acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[i][v] = 0.f;

  fetch(p0);
#pragma unroll
  for (int i = 0; i < DD_P - 1; ++i) row_dct(p0 + i + 1, rc[i]);

  const int cx = min(x0 + l, w - DD_P) - max(x0 + l - (DD_P - 1), 0) + 1;
  const bool out_ok = l < DD_TW && x0 + l < w;

  for (int pb = p0; pb < y1; pb += 8) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int p = pb + s;
      if (p >= y1) break;
      if (p <= p1) {
        row_dct(p + DD_P, rc[(s + 7) & 7]);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          float col[8], d[8], z[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) col[i] = rc[(s + i) & 7][v];
          dct8_fwd(col, d);
          const bool v04 = v == 0 || v == 4;
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (u == 0 && v == 0) continue;  // the DC term stays
            const bool u04 = u == 0 || u == 4;
            const float t = (u04 && v04) ? thr2 : ((u04 || v04) ? thr1 : thr);
            d[u] = fabsf(d[u]) >= t ? d[u] : 0.f;
          }
          dct8_inv(d, z);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[(s + i) & 7][v] += z[i];
        }
      }
      if (p >= y0) {  // row p has met every patch that contains it
        float val[8];
        dct8_inv(acc[s], val);
#pragma unroll
        for (int i = 0; i < 8; ++i) hz[k][i][l] = patch_ok ? val[i] : 0.f;
        __syncthreads();
        float r = 0.f;
        if (out_ok) {
          float sum = hz[k][0][l + 7];
#pragma unroll
          for (int i = 1; i < 8; ++i) sum += hz[k][i][l + 7 - i];
          const int cy = min(p, h - DD_P) - max(p - (DD_P - 1), 0) + 1;
          r = sum / (float)(cy * cx);
        }
        if (COLOR) {
          planes[k][l] = r;
          __syncthreads();
          r = bm0 * planes[0][l] + bm1 * planes[C > 1 ? 1 : 0][l] + bm2 * planes[C > 2 ? 2 : 0][l];
        }
        if (out_ok) {
          const int64_t row = (int64_t)img * h + p;
          const int xo = (x0 + l) * C + k;
          if (dst_f32) dst_f32[row * ((int64_t)w * C) + xo] = r;
          if (dst_u8) dst_u8[row * row_stride + xo] = (uint8_t)(int)fminf(fmaxf(rintf(r), 0.f), 255.f);
        }
      }
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[s][v] = 0.f;  // the slot is row p + 8 from here on
    }
  }
}

template <int C, bool COLOR>
static void dd_launch(unsigned grid, hipStream_t s, const uint8_t* src, uint8_t* dst_u8,
                      float* dst_f32, int h, int w, int64_t row_stride, int sr, int tiles,
                      int strips, const double* sigma, int64_t sigma_image_stride, double factor) {
  hipLaunchKernelGGL((dct_denoise_kernel<C, COLOR>), dim3(grid), dim3(64 * C), 0, s, src, dst_u8,
                     dst_f32, h, w, row_stride, sr, tiles, strips, sigma, sigma_image_stride,
                     factor);
}

}  // namespace idn

extern "C" size_t idn_dct_denoise_workspace_size(int n, int h, int w, int c) {
  (void)n, (void)h, (void)w, (void)c;
  return 0;  // the thresholds are formed in the kernel's prologue
}

extern "C" int idn_dct_denoise_u8(const uint8_t* src, uint8_t* dst_u8, float* dst_f32, int n,
                                  int h, int w, int c, int64_t row_stride, int patch, int color,
                                  const double* sigma, int64_t sigma_image_stride, double factor,
                                  void* workspace, size_t ws_bytes, void* stream) {
  using namespace idn;
  const char* name = "idn_dct_denoise_u8";
  IDN_CHECK_ARG(src && sigma, "%s: null pointer (src or sigma)", name);
  IDN_CHECK_ARG(dst_u8 || dst_f32, "%s: both destinations are null", name);
  if (int e = check_not_in_place(name, src, dst_u8, "dst_u8 == src")) return e;
  if (int e = check_image_1_or_3(name, n, h, w, c, row_stride)) return e;
  IDN_CHECK_ARG(color == 0 || (color == 1 && c == 3),
                "%s: color must be 0, or 1 with 3 channels (got %d with %d)", name, color, c);
  IDN_CHECK_ARG(((uintptr_t)dst_f32 & 3) == 0, "%s: dst_f32 must be 4-byte aligned", name);
  IDN_CHECK_ARG(((uintptr_t)sigma & 7) == 0, "%s: sigma must be 8-byte aligned", name);
  IDN_CHECK_ARG(sigma_image_stride == 0 || sigma_image_stride == c,
                "%s: sigma_image_stride must be 0 or c (got %lld)", name,
                (long long)sigma_image_stride);
  IDN_CHECK_ARG(__builtin_isfinite(factor) && factor >= 0.0, "%s: factor must be finite and not negative",
                name);
  if (patch != DD_P)
    return set_error(IDN_EUNSUPPORTED, "%s: only patch 8 is built (got %d; 16 is not)", name,
                     patch);
  if (h < DD_P || w < DD_P)
    return set_error(IDN_EUNSUPPORTED, "%s: the image must be at least 8 x 8 (got %d x %d)", name,
                     h, w);
  (void)workspace, (void)ws_bytes;  // idn_dct_denoise_workspace_size is 0: nothing to hold
  if (n == 0) return IDN_OK;
  const int sr = DD_SR;
  const int64_t tiles = ((int64_t)w + DD_TW - 1) / DD_TW, strips = ((int64_t)h + sr - 1) / sr;
  if ((int64_t)w * c > INT_MAX - 256 || (int64_t)n * tiles * strips > INT_MAX)
    return batch_too_large(name);

  const hipStream_t s = as_stream(stream);
  const unsigned grid = (unsigned)((int64_t)n * tiles * strips);
  if (c == 1)
    dd_launch<1, false>(grid, s, src, dst_u8, dst_f32, h, w, row_stride, sr, (int)tiles,
                        (int)strips, sigma, sigma_image_stride, factor);
  else if (color)
    dd_launch<3, true>(grid, s, src, dst_u8, dst_f32, h, w, row_stride, sr, (int)tiles,
                       (int)strips, sigma, sigma_image_stride, factor);
  else
    dd_launch<3, false>(grid, s, src, dst_u8, dst_f32, h, w, row_stride, sr, (int)tiles,
                        (int)strips, sigma, sigma_image_stride, factor);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}
