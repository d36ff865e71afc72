// Separable 8-bit stencils on interleaved HxWxC images for gfx950:
//   cv2.GaussianBlur(u8, (3,3)|(5,5), 0)   and   cv2.blur(u8, (3,3)),  BORDER_REFLECT_101.
//
// Reference call sites: lib/model/test.py:224,241,1767; lib/roi_data_layer/minibatch.py:119,136,
// 1636-1643.  OpenCV 3.4.2 semantics restated in oracle/filters.c.
//
// Lane layout (shared with the median, stripe.hpp): a row of RB = W*C bytes is cut into
// segments of <= 1008 output bytes; a wave owns one segment, lane l the 16-byte chunk
// [seg_start - 8 + 16 l, +16).  The horizontal halo comes from the neighbouring lanes by DPP
// wave shifts, so each byte is fetched once per row; row/segment edges rebuild the reflected
// bytes in registers.
//
// Arithmetic (vertical first, stencil_common.hpp): each input row is split once into u16 lanes,
// the K vertical taps run on the lane's own 16 bytes from a K-deep register ring (v_mad_u32_u24
// for the 6x tap), then the horizontal taps run once per OUTPUT row on the vertical sums, whose
// halos arrive by DPP (v_pk_mad_u16 for the 6x tap).  The Gaussian weights and the +128 rounding
// bias are arranged so the cv2 result lands in the high byte of each u16 lane (one v_perm packs 4
// bytes); the box mean uses (S*7280 + 33200) >> 16.
//
// Four memory forms, picked by pick_form() below.  "Lane rows" are what stripe_ok() takes: C = 3,
// rows and strides of 8 k bytes, >= 32 bytes, >= 5 rows, 8-byte aligned pointers, images < 1 GiB.
//   pitched tile  stencil_u8_pt   stencil_pitched.hpp   compact lane rows of 16 k + 8 bytes,
//                 <= 3024 B (the 600x1000x3 batch): one 3-wave workgroup per band, the band's rows
//                 fetched by LDS-DMA into tile rows of 3072 B, u16 lanes of adjacent bytes
//   flat tile     stencil_u8_lds  stencil_tile.hip      the other compact lane rows <= 3024 B: the
//                 band's rows fetched flat into LDS
//   stripe        stencil_u8_vf   stencil_stripe.hip    strided or wider lane rows, each row
//                 segment loaded from HBM: burst bands for rows of <= 4 segments, long bands of
//                 independent waves beyond
//   generic       stencil_u8_generic  (here)            anything else: one thread per pixel
// idn_gaussian_blob_f32 (the Gaussian with the float32 blob epilogue) exists on the two tiles
// only: it needs h > ksize and a 16-byte aligned blob as well, and refuses every other layout.
//
// This unit holds the dispatcher, the entry points, the generic kernel and the float64 filters.
#include "stencil_common.hpp"
#include "abi_args.hpp"
#include "blur_large.hpp"

namespace idn {

// ---- generic path ------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(256) void stencil_u8_generic(const uint8_t* __restrict__ src,
                                                          uint8_t* __restrict__ dst, int n, int h,
                                                          int w, int c, int64_t row_stride) {
  constexpr int K = Stencil<OP>::K;
  constexpr int R = K / 2;
  const int64_t npix = (int64_t)n * h * w;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(p % w);
    const int64_t t = p / w;
    const int y = (int)(t % h);
    const int img = (int)(t / h);
    const uint8_t* s = src + (int64_t)img * h * row_stride;
    uint8_t* d = dst + (int64_t)img * h * row_stride + (int64_t)y * row_stride + (int64_t)x * c;
    for (int ch = 0; ch < c; ++ch) {
      uint32_t S = 0;
#pragma unroll
      for (int i = -R; i <= R; ++i) {
        const uint8_t* sr = s + (int64_t)reflect101(y + i, h) * row_stride;
#pragma unroll
        for (int j = -R; j <= R; ++j) {
          uint32_t v = sr[(int64_t)reflect101(x + j, w) * c + ch];
          uint32_t wgt;
          if constexpr (OP == OP_GAUSS5) {
            constexpr uint32_t a[5] = {1, 4, 6, 4, 1};
            wgt = a[i + R] * a[j + R];
          } else if constexpr (OP == OP_GAUSS3) {
            constexpr uint32_t a[3] = {1, 2, 1};
            wgt = a[i + R] * a[j + R];
          } else {
            wgt = 1;
          }
          S += wgt * v;
        }
      }
      uint32_t out;
      if constexpr (OP == OP_GAUSS5) out = (S + 128) >> 8;
      else if constexpr (OP == OP_GAUSS3) out = (S + 8) >> 4;
      else out = (2 * S + 9) / 18;
      d[ch] = (uint8_t)out;
    }
  }
}

// ---- float64 path (the reference's quirk branches filter the float64 output of random_noise) ----
// cv2.GaussianBlur / cv2.blur on CV_64F: separable double filter, BORDER_REFLECT_101, no rounding.
template <int OP>
__device__ __forceinline__ double f64_tap(int i) {
  if constexpr (OP == OP_GAUSS5) {
    constexpr double a[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    return a[i];
  } else if constexpr (OP == OP_GAUSS3) {
    constexpr double a[3] = {0.25, 0.5, 0.25};
    return a[i];
  } else {
    return 1.0;
  }
}

// Summation order follows OpenCV's 64F engines so results agree to the last ulp for the Gaussian:
// RowFilter<double> sums taps left to right; SymmColumnFilter<double> forms
// ky0*c + ky1*(r+1 + r-1) + ky2*(r+2 + r-2).  cv2.blur's 64F path uses running row/column sums
// (RowSum/ColumnSum), which this direct 3x3 sum matches only to a few ulp.
template <int OP>
__global__ __launch_bounds__(256) void stencil_f64(const double* __restrict__ src,
                                                   double* __restrict__ dst, int n, int h, int w,
                                                   int c) {
  constexpr int K = Stencil<OP>::K;
  constexpr int R = K / 2;
  const int64_t total = (int64_t)n * h * w * c;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int ch = (int)(e % c);
    int64_t t = e / c;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h);
    const int img = (int)(t / h);
    const double* s = src + (int64_t)img * h * w * c;
    double rs[K];
#pragma unroll
    for (int i = -R; i <= R; ++i) {
      const double* row = s + (int64_t)reflect101(y + i, h) * w * c;
      double racc = f64_tap<OP>(0) * row[(int64_t)reflect101(x - R, w) * c + ch];
#pragma unroll
      for (int j = -R + 1; j <= R; ++j)
        racc = __dadd_rn(racc, __dmul_rn(f64_tap<OP>(j + R), row[(int64_t)reflect101(x + j, w) * c + ch]));
      rs[i + R] = racc;
    }
    double acc;
    if constexpr (OP == OP_BOX3) {
      acc = __dadd_rn(__dadd_rn(rs[0], rs[1]), rs[2]) * (1.0 / 9.0);
    } else {
      acc = __dmul_rn(f64_tap<OP>(R), rs[R]);
#pragma unroll
      for (int k = 1; k <= R; ++k)
        acc = __dadd_rn(acc, __dmul_rn(f64_tap<OP>(R + k), __dadd_rn(rs[R + k], rs[R - k])));
    }
    dst[e] = acc;
  }
}

template <int OP>
static int launch_f64(const double* src, double* dst, int n, int h, int w, int c, hipStream_t st,
                      const char* name) {
  const int64_t total = (int64_t)n * h * w * c;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL((stencil_f64<OP>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, n, h, w, c);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

// ---- dispatch --------------------------------------------------------------------------------
enum StencilForm { FORM_PITCHED, FORM_TILE, FORM_STRIPE, FORM_GENERIC };

// tile_min_h: the tiles take images of more rows than this
static StencilForm pick_form(int c, int64_t rb, int64_t row_stride, int h, const void* src,
                             const void* dst, int tile_min_h) {
  if (!stripe_ok(c, rb, row_stride, h, src, dst)) return FORM_GENERIC;
  if (row_stride != rb || rb > TILE_RBMAX || h <= tile_min_h) return FORM_STRIPE;
#ifdef IDN_TUNING_BUILD
  if (knob("IDN_STENCIL_FORM", 1) != 1) return FORM_TILE;  // A/B: the flat tile for every row
#endif
  return rb % 16 == 8 ? FORM_PITCHED : FORM_TILE;
}

template <int OP>
static void launch_generic(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                           int64_t row_stride, hipStream_t st) {
  const int64_t npix = (int64_t)n * h * w;
  int64_t blocks = (npix + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL((stencil_u8_generic<OP>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst,
                     n, h, w, c, row_stride);
}

static int launch_stencil(StencilOp op, const uint8_t* src, uint8_t* dst, int n, int h, int w,
                          int c, int64_t row_stride, hipStream_t st, const char* name) {
  const int K = op == OP_GAUSS5 ? 5 : 3;
  const int64_t rb = (int64_t)w * c;
  const TileCall tc = {src, dst, nullptr, nullptr, n, h, (int)rb, st, name};
  int rc = IDN_OK;
  switch (pick_form(c, rb, row_stride, h, src, dst, K - 1)) {
    case FORM_PITCHED: rc = stencil_pitched(op, tc); break;
    case FORM_TILE: rc = stencil_tile(op, tc); break;
    case FORM_STRIPE: rc = stencil_stripe(op, src, dst, n, h, rb, row_stride, st, name); break;
    case FORM_GENERIC:
      if (op == OP_GAUSS3) launch_generic<OP_GAUSS3>(src, dst, n, h, w, c, row_stride, st);
      else if (op == OP_GAUSS5) launch_generic<OP_GAUSS5>(src, dst, n, h, w, c, row_stride, st);
      else launch_generic<OP_BOX3>(src, dst, n, h, w, c, row_stride, st);
      break;
  }
  if (rc) return rc;
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

}  // namespace idn

// 3 and 5 with the window's own sigma, and the 3 box, run the kernels above; every other odd
// window up to 31 and every given sigma the kernels of blur_large_u8.hip
static int gaussian_blur_any(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                             int64_t row_stride, int ksize, double sigma, void* stream,
                             const char* name) {
  using namespace idn;
  if (int e = check_filter_args(src, dst, n, h, w, c, row_stride, name)) return e;
  uint16_t taps[32];
  if (int e = gaussian_taps(ksize, sigma, taps, name)) return e;
  if (n == 0) return IDN_OK;
  if (ksize == 3 && sigma == 0.0)
    return launch_stencil(OP_GAUSS3, src, dst, n, h, w, c, row_stride, as_stream(stream), name);
  if (ksize == 5 && sigma == 0.0)
    return launch_stencil(OP_GAUSS5, src, dst, n, h, w, c, row_stride, as_stream(stream), name);
  return launch_gauss_large(src, dst, n, h, w, c, row_stride, ksize, taps, as_stream(stream),
                            name);
}

extern "C" int idn_gaussian_blur_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                                    int64_t row_stride, int ksize, void* stream) {
  return gaussian_blur_any(src, dst, n, h, w, c, row_stride, ksize, 0.0, stream,
                           "idn_gaussian_blur_u8");
}

extern "C" int idn_gaussian_blur_sigma_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                                          int c, int64_t row_stride, int ksize, double sigma,
                                          void* stream) {
  return gaussian_blur_any(src, dst, n, h, w, c, row_stride, ksize, sigma, stream,
                           "idn_gaussian_blur_sigma_u8");
}

extern "C" int idn_box_blur_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                               int64_t row_stride, int ksize, void* stream) {
  using namespace idn;
  if (int e = check_filter_args(src, dst, n, h, w, c, row_stride, "idn_box_blur_u8")) return e;
  if (ksize < 3 || ksize > 31 || !(ksize & 1))
    return set_error(IDN_EUNSUPPORTED, "idn_box_blur_u8: ksize %d not supported (odd, 3..31)",
                     ksize);
  if (n == 0) return IDN_OK;
  if (ksize == 3)
    return launch_stencil(OP_BOX3, src, dst, n, h, w, c, row_stride, as_stream(stream),
                          "idn_box_blur_u8");
  return launch_box_large(src, dst, n, h, w, c, row_stride, ksize, as_stream(stream),
                          "idn_box_blur_u8");
}

extern "C" int idn_gaussian_blur_f64(const double* src, double* dst, int n, int h, int w, int c,
                                     int ksize, void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(src && dst && src != dst, "idn_gaussian_blur_f64: bad pointers");
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0 && c >= 1 && c <= 4, "idn_gaussian_blur_f64: bad shape");
  if (n == 0) return IDN_OK;
  if (ksize == 3) return launch_f64<OP_GAUSS3>(src, dst, n, h, w, c, as_stream(stream), "idn_gaussian_blur_f64");
  if (ksize == 5) return launch_f64<OP_GAUSS5>(src, dst, n, h, w, c, as_stream(stream), "idn_gaussian_blur_f64");
  return set_error(IDN_EUNSUPPORTED, "idn_gaussian_blur_f64: ksize %d not supported", ksize);
}

extern "C" int idn_box_blur_f64(const double* src, double* dst, int n, int h, int w, int c,
                                int ksize, void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(src && dst && src != dst, "idn_box_blur_f64: bad pointers");
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0 && c >= 1 && c <= 4, "idn_box_blur_f64: bad shape");
  if (n == 0) return IDN_OK;
  if (ksize == 3) return launch_f64<OP_BOX3>(src, dst, n, h, w, c, as_stream(stream), "idn_box_blur_f64");
  return set_error(IDN_EUNSUPPORTED, "idn_box_blur_f64: ksize %d not supported", ksize);
}

// ---- fused blob epilogue -----------------------------------------------------------------------
// cv2.GaussianBlur(u8, (k, k), 0) -> prep_im_for_blob at scale 1.0 (lib/utils/blob.py:33-47,
// lib/model/test.py:49-83): blob = float32(float64(filtered) - mean[ch]), dense (n, h, w, 3)
// float32, written by the filter kernel itself (the u8 filtered image never reaches HBM).
extern "C" int idn_gaussian_blob_f32(const uint8_t* src, float* blob, int n, int h, int w, int c,
                                     int64_t row_stride, int ksize, const double* mean,
                                     void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(blob && mean, "idn_gaussian_blob_f32: null pointer");
  if (int e = check_filter_args(src, (uint8_t*)blob, n, h, w, c, row_stride,
                                "idn_gaussian_blob_f32")) return e;
  if (n == 0) return IDN_OK;
  const int64_t rb = (int64_t)w * c;
  if (ksize >= 7 && ksize <= 31 && (ksize & 1))  // the caller composes the blur and idn_blob_f32
    return set_error(IDN_EUNSUPPORTED, "idn_gaussian_blob_f32: ksize %d is not fused", ksize);
  IDN_CHECK_ARG(ksize == 3 || ksize == 5, "idn_gaussian_blob_f32: ksize must be odd, 3..31");
  const StencilForm form = pick_form(c, rb, row_stride, h, src, blob, ksize);
  if ((form != FORM_PITCHED && form != FORM_TILE) || ((uintptr_t)blob & 15) != 0)
    return set_error(IDN_EUNSUPPORTED, "idn_gaussian_blob_f32: layout not fused");
  const StencilOp op = ksize == 5 ? OP_GAUSS5 : OP_GAUSS3;
  const TileCall tc = {src,  nullptr, blob, mean, n, h, (int)rb, as_stream(stream),
                       "idn_gaussian_blob_f32"};
  if (int rc = form == FORM_PITCHED ? stencil_pitched(op, tc) : stencil_tile(op, tc)) return rc;
  IDN_CHECK_LAUNCH("idn_gaussian_blob_f32");
  return IDN_OK;
}
