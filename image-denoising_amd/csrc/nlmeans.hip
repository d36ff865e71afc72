// Non-local means on u8 images: OpenCV 3.4's 8-bit integer scheme (cv2.fastNlMeansDenoising;
// fast_nlmeans_denoising_invoker.hpp with DistSquared, IT = int, WT = int), restated.  Not on the
// reference's preprocessing path: it is the denoiser a cv2-flavoured bank is expected to have.
// cv2 is not importable where this project is built, so parity with cv2 itself is unpinned (as
// for the Lab tables of idn_quant_u8); the numpy host model tests/nlm_model.py is the contract and
// the kernel matches it bit for bit.
//
//   fpm = INT_MAX / (s*s*255)     shift = ceil(log2(t*t))     mult = 2^shift / (t*t)
//   wt[a] = rint(fpm * exp(-(a*mult) / (h*h*C))), 0 where below 0.001 * fpm   (host, float64)
//   per pixel p, for each of the s*s offsets o, on the image extended by reflection (101):
//     ssd = sum over the t x t template and the channels of (E[p+q] - E[p+o+q])^2
//     w = wt[ssd >> shift];   wsum += w;   est[c] += w * E[p+o][c]
//   out[c] = min(255, (est[c] + wsum / 2) / wsum)
// est <= s*s*fpm*255 <= INT_MAX and wsum >= fpm (the zero offset weighs fpm), so u32 carries all.
//
// nlmeans_kernel<T, C>: a 256-thread workgroup owns NLM_OW(T) x 64 output pixels of one image.
// The tile and a halo of T/2 + s/2 pixels is staged once in LDS, reflected while staging, one u32
// per pixel (channel bytes packed, a fixed pitch of 84 so that row offsets are immediates), with
// the nonzero prefix of the weight table and one zero entry behind it.  After the one barrier the
// four waves never meet again: wave v owns output rows 16 v .. 16 v + 15.  A lane owns one
// column.  Per offset it takes its 16 + T - 1 rows of squared differences
//   D = |a|^2 + |b|^2 - 2 a.b   (v_dot4_u32_u8 on the packed pixels; |a|^2 does not depend on the
//                                offset and stays in registers),
// adds the T columns to its right through ds_bpermute (T = 7: D + D[+1], that + itself[+2], then
// [+4] of the pair sum and D[+6]: four permutes), runs the box sum down the row sums, and for each
// of its 16 rows looks the weight up in LDS (index clamped to n_weights, where the zero entry
// stands for the table's zero tail) and runs C + 1 24-bit multiply-adds into the row's u32
// accumulators.  Everything is unrolled over the rows, so the row sums and the 16 (C + 1)
// accumulators are registers, and each stage runs over all rows before the next starts: its LDS
// reads and permutes are in flight together (measured 100.5 -> 95.9 ms with the fixed pitch and
// the zero entry, -> 91.3 ms with the stages, 256 x 600 x 1000 x 3).  The
// 64 - (T - 1) lanes with a whole template to their right produce output.
//
// cv2.fastNlMeansDenoisingColored (idn_nlmeans_colored_u8) is two launches of the same kernel on a
// BGR source, with the 8-bit linear Lab conversions (COLOR_LBGR2Lab / COLOR_Lab2LBGR; lab_cvt.hpp)
// folded into its staging and output stages, so no Lab image ever lies in memory:
//   NLM_LAB_L  (C = 1): staging converts each staged BGR pixel and keeps L; the output stage writes
//              L' to a compact 1 byte/pixel plane (the caller's workspace).
//   NLM_LAB_AB (C = 2, a | b << 16, the other two bytes zero, so the dot products stay exact):
//              staging keeps (a, b); the output stage reads its pixel's L' from the plane,
//              converts (L', a', b') back and writes BGR.  b must sit in byte 2, not byte 1:
//              packed as a | b << 8 the two clamped shifts become one v_ashr_pk_u8_i32, whose
//              16-bit result hipcc (ROCm 7) stores as a dword without clearing the destination's
//              upper half, and byte 2 of the staged pixel is garbage.
// The cbrt table (and LabToYF_b for the way back) is staged in LDS behind the weights, before the
// tile: these two modes have one barrier more.  NLM_PLAIN is the kernel described above.
#include "idn_common.hpp"
#include "abi_args.hpp"
#include "lab_cvt.hpp"

#include <limits.h>
#include <math.h>

namespace idn {

constexpr int NLM_TH = 16;             // output rows per wave
constexpr int NLM_ROWS = 4 * NLM_TH;   // output rows per workgroup
constexpr int NLM_PITCH = 64 + 20;     // LDS tile pitch in pixels: 64 columns + the widest search
constexpr int nlm_ow(int t) { return 64 - (t - 1); }  // output columns per workgroup
constexpr int nlm_shift(int t) { return t == 3 ? 4 : (t == 5 ? 5 : 6); }

__device__ __forceinline__ uint32_t nlm_dot(uint32_t a, uint32_t b, uint32_t acc) {
  return __builtin_amdgcn_udot4(a, b, acc, false);
}

__device__ __forceinline__ uint32_t nlm_from_lane(uint32_t byte_addr, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)byte_addr, (int)v);
}

enum { NLM_PLAIN = 0, NLM_LAB_L = 1, NLM_LAB_AB = 2 };
constexpr int NLM_CBRT_BYTES = 3072 * 2, NLM_YF_BYTES = 512 * 2;  // LAB_CBRT_B, LAB_YF_B in LDS

// lplane: NLM_LAB_AB only, the L' plane the NLM_LAB_L launch wrote (n * h * w bytes)
template <int T, int C, int MODE = NLM_PLAIN>
__global__ __launch_bounds__(256) void nlmeans_kernel(const uint8_t* __restrict__ src,
                                                      uint8_t* __restrict__ dst, int h, int w,
                                                      int64_t row_stride, int sr, int tiles_x,
                                                      int tiles_y,
                                                      const int32_t* __restrict__ weights,
                                                      int n_weights,
                                                      const uint8_t* __restrict__ lplane) {
  static_assert(MODE == NLM_PLAIN ? (C == 1 || C == 3) : C == MODE, "mode and channel count");
  constexpr int TR = T / 2;
  constexpr int OW = nlm_ow(T);
  constexpr int SHIFT = nlm_shift(T);
  constexpr int STEPS = NLM_TH + T - 1;
  extern __shared__ uint32_t nlm_lds[];

  const int b = TR + sr;
  constexpr int twe = NLM_PITCH;
  const int cols = 64 + 2 * sr;         // staged columns: OW + 2 b
  const int the = NLM_ROWS + 2 * b;
  uint32_t* tile = nlm_lds;
  uint32_t* wt = nlm_lds + twe * the;

  const int tid = threadIdx.x;
  const int per_img = tiles_x * tiles_y;
  const int img = blockIdx.x / per_img;
  const int rem = blockIdx.x - img * per_img;
  const int ty = rem / tiles_x;
  const int tx = rem - ty * tiles_x;
  const int gx0 = tx * OW, gy0 = ty * NLM_ROWS;
  const uint8_t* simg = src + (int64_t)img * h * row_stride;

  // Lab modes: the cbrt table, then LabToYF_b, behind the n_weights + 1 weights
  uint16_t* ct = reinterpret_cast<uint16_t*>(wt + n_weights + 1);
  const uint16_t* yf = ct + 3072;
  if constexpr (MODE == NLM_PLAIN) {
    for (int i = tid; i < cols * the; i += 256) {
      const int ey = i / cols, ex = i - ey * cols;
      const uint8_t* p = simg + (int64_t)reflect101(gy0 - b + ey, h) * row_stride +
                         (int64_t)reflect101(gx0 - b + ex, w) * C;
      uint32_t v = p[0];
      if (C == 3) v |= ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
      tile[ey * twe + ex] = v;
    }
  } else {
    for (int i = tid; i < 3072; i += 256) ct[i] = LAB_CBRT_B[i];
    if constexpr (MODE == NLM_LAB_AB)
      for (int i = tid; i < 512; i += 256) ct[3072 + i] = LAB_YF_B[i];
    __syncthreads();
    for (int i = tid; i < cols * the; i += 256) {
      const int ey = i / cols, ex = i - ey * cols;
      const uint8_t* p = simg + (int64_t)reflect101(gy0 - b + ey, h) * row_stride +
                         (int64_t)reflect101(gx0 - b + ex, w) * 3;
      const uint32_t lab = lab_from_bgr<true>(p[0], p[1], p[2], nullptr, ct);
      tile[ey * twe + ex] = MODE == NLM_LAB_L ? (lab & 255u)
                                              : (((lab >> 8) & 255u) | (lab & 0xFF0000u));
    }
  }
  for (int i = tid; i <= n_weights; i += 256) wt[i] = i < n_weights ? (uint32_t)weights[i] : 0u;
  __syncthreads();

  const int lane = tid & 63;
  const int rowbase = (tid >> 6) * NLM_TH;
  if (gy0 + rowbase >= h) return;  // a whole wave below the image (after the only barrier)

  uint32_t wsum[NLM_TH], est[NLM_TH][C];
#pragma unroll
  for (int r = 0; r < NLM_TH; ++r) {
    wsum[r] = 0;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) est[r][ch] = 0;
  }
  // a: the template pixel of this lane's column of differences; ctr: the pixel a weight multiplies
  const uint32_t* pa = tile + (sr + rowbase) * twe + sr + lane;
  const uint32_t* pc = tile + (b + rowbase) * twe + b + min(lane, OW - 1);
  const uint32_t l1 = ((lane + 1) & 63) * 4, l2 = ((lane + 2) & 63) * 4;
  const uint32_t l4 = ((lane + 4) & 63) * 4, l6 = ((lane + 6) & 63) * 4;
  const uint32_t nw = (uint32_t)n_weights;  // wt[nw] = 0 stands for the table's zero tail

  for (int dy = -sr; dy <= sr; ++dy) {
    for (int dx = -sr; dx <= sr; ++dx) {
      const int off = dy * twe + dx;
      // every stage runs over all rows before the next one starts, so that its LDS reads and
      // lane permutes are in flight together instead of one round trip per row
      uint32_t d[STEPS], d1[STEPS], hs[STEPS], ssd[NLM_TH], wgt[NLM_TH], px[NLM_TH];
#pragma unroll
      for (int j = 0; j < STEPS; ++j) {
        const uint32_t a = pa[j * twe], q = pa[j * twe + off];
        d[j] = nlm_dot(q, q, nlm_dot(a, a, 0)) - 2u * nlm_dot(a, q, 0);
      }
#pragma unroll
      for (int j = 0; j < STEPS; ++j) d1[j] = d[j] + nlm_from_lane(l1, d[j]);  // columns +0 .. +1
#pragma unroll
      for (int j = 0; j < STEPS; ++j) {
        if (T == 3) hs[j] = d1[j] + nlm_from_lane(l2, d[j]);
        else hs[j] = d1[j] + nlm_from_lane(l2, d1[j]);                          // +0 .. +3
      }
      if (T == 5) {
#pragma unroll
        for (int j = 0; j < STEPS; ++j) hs[j] += nlm_from_lane(l4, d[j]);
      }
      if (T == 7) {
#pragma unroll
        for (int j = 0; j < STEPS; ++j) hs[j] += nlm_from_lane(l4, d1[j]) + nlm_from_lane(l6, d[j]);
      }
      uint32_t box = 0;
#pragma unroll
      for (int j = 0; j < STEPS; ++j) {
        box += hs[j];
        if (j >= T) box -= hs[j - T];
        if (j >= T - 1) ssd[j - (T - 1)] = box;
      }
#pragma unroll
      for (int r = 0; r < NLM_TH; ++r) {
        wgt[r] = wt[min(ssd[r] >> SHIFT, nw)];
        px[r] = pc[r * twe + off];
      }
#pragma unroll
      for (int r = 0; r < NLM_TH; ++r) {
        wsum[r] += wgt[r];
        est[r][0] += __umul24(wgt[r], px[r] & 255u);
        if (C == 3) {
          est[r][1] += __umul24(wgt[r], (px[r] >> 8) & 255u);
          est[r][2] += __umul24(wgt[r], px[r] >> 16);
        }
        if (C == 2) est[r][1] += __umul24(wgt[r], px[r] >> 16);
      }
    }
  }

  const int gx = gx0 + lane;
  if (lane >= OW || gx >= w) return;
  if constexpr (MODE == NLM_PLAIN) {
    uint8_t* dimg = dst + (int64_t)img * h * row_stride + (int64_t)gx * C;
#pragma unroll
    for (int r = 0; r < NLM_TH; ++r) {
      const int gy = gy0 + rowbase + r;
      if (gy < h) {
        uint8_t* o = dimg + (int64_t)gy * row_stride;
#pragma unroll
        for (int ch = 0; ch < C; ++ch)
          o[ch] = (uint8_t)min(255u, (est[r][ch] + wsum[r] / 2u) / wsum[r]);
      }
    }
  } else {
    const int64_t pimg = (int64_t)img * h * w + gx;  // this column in the compact L' plane
    uint8_t* dimg = dst + (int64_t)img * h * row_stride + (int64_t)gx * 3;
#pragma unroll
    for (int r = 0; r < NLM_TH; ++r) {
      const int gy = gy0 + rowbase + r;
      if (gy < h) {
        uint32_t v[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) v[ch] = min(255u, (est[r][ch] + wsum[r] / 2u) / wsum[r]);
        if constexpr (MODE == NLM_LAB_L) {
          dst[pimg + (int64_t)gy * w] = (uint8_t)v[0];
        } else {
          const uint32_t bgr = bgr_from_lab<true>(lplane[pimg + (int64_t)gy * w], v[0], v[1], yf);
          uint8_t* o = dimg + (int64_t)gy * row_stride;
          o[0] = (uint8_t)bgr;
          o[1] = (uint8_t)(bgr >> 8);
          o[2] = (uint8_t)(bgr >> 16);
        }
      }
    }
  }
}

static int nlm_check_sizes(const char* name, int t, int s) {
  IDN_CHECK_ARG((t & 1) && t >= 3 && t <= 7 && (s & 1) && s >= 5 && s <= 21, "%s: template_size "
                "must be odd in 3..7 and search_size odd in 5..21 (got %d, %d)", name, t, s);
  return IDN_OK;
}

// A launch gets 64 KB of LDS without asking; a longer weight table raises the kernel's limit first
// (up to the CU's 160 KB; one workgroup per CU above 80 KB).  Not a stream operation.
template <int T, int C, int MODE = NLM_PLAIN>
static hipError_t launch_nlm_c(unsigned grid, size_t lds, hipStream_t st, const uint8_t* src,
                               uint8_t* dst, int h, int w, int64_t row_stride, int sr,
                               int tiles_x, int tiles_y, const int32_t* weights, int n_weights,
                               const uint8_t* lplane = nullptr) {
  if (lds > 64 * 1024) {
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&nlmeans_kernel<T, C, MODE>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((nlmeans_kernel<T, C, MODE>), dim3(grid), dim3(256), lds, st, src, dst, h, w,
                     row_stride, sr, tiles_x, tiles_y, weights, n_weights, lplane);
  return hipGetLastError();
}

template <int T>
static hipError_t launch_nlm(int c, unsigned grid, size_t lds, hipStream_t st, const uint8_t* src,
                             uint8_t* dst, int h, int w, int64_t row_stride, int sr, int tiles_x,
                             int tiles_y, const int32_t* weights, int n_weights) {
  return c == 3 ? launch_nlm_c<T, 3>(grid, lds, st, src, dst, h, w, row_stride, sr, tiles_x,
                                     tiles_y, weights, n_weights)
                : launch_nlm_c<T, 1>(grid, lds, st, src, dst, h, w, row_stride, sr, tiles_x,
                                     tiles_y, weights, n_weights);
}

// the L launch into the plane, then the ab launch that reads it: ordered on the stream
template <int T>
static hipError_t launch_nlm_colored(unsigned grid, size_t lds_l, size_t lds_ab, hipStream_t st,
                                     const uint8_t* src, uint8_t* dst, int h, int w,
                                     int64_t row_stride, int sr, int tiles_x, int tiles_y,
                                     const int32_t* wt_l, int n_l, const int32_t* wt_ab, int n_ab,
                                     uint8_t* lplane) {
  const hipError_t e = launch_nlm_c<T, 1, NLM_LAB_L>(grid, lds_l, st, src, lplane, h, w, row_stride,
                                                     sr, tiles_x, tiles_y, wt_l, n_l);
  if (e != hipSuccess) return e;
  return launch_nlm_c<T, 2, NLM_LAB_AB>(grid, lds_ab, st, src, dst, h, w, row_stride, sr, tiles_x,
                                        tiles_y, wt_ab, n_ab, lplane);
}

// the nonzero prefix of the weight table of (h, c, t, s): the first min(cap, length) entries go
// to wt_out; returns the length
static int nlm_fill_weights(double h, int c, int template_size, int search_size, int32_t* wt_out,
                            int cap) {
  const int tt = template_size * template_size;
  const int fpm = INT_MAX / (search_size * search_size * 255);
  const double mult = (double)(1 << nlm_shift(template_size)) / (double)tt;
  const int len = (int)(255.0 * 255.0 * c / mult + 1);
  const double den = h * h * c;
  const double thr = 0.001 * fpm;
  int n = 0;
  for (; n < len; ++n) {  // exp falls monotonically: the first entry below the threshold ends it
    const double wgt = nearbyint(fpm * exp(-(n * mult) / den));
    if (wgt < thr) break;
    if (n < cap) wt_out[n] = (int32_t)wgt;
  }
  return n;
}

}  // namespace idn

extern "C" int idn_nlmeans_weights(double h, int c, int template_size, int search_size,
                                   int32_t* wt_out, int cap, int* n_weights, int* shift,
                                   int* fixed_point_mult) {
  using namespace idn;
  IDN_CHECK_ARG(n_weights && shift && fixed_point_mult && (wt_out || cap == 0),
                "idn_nlmeans_weights: null pointer");
  IDN_CHECK_ARG(cap >= 0, "idn_nlmeans_weights: negative cap %d", cap);
  IDN_CHECK_ARG(h > 0.0 && h < INFINITY, "idn_nlmeans_weights: h must be positive and finite "
                "(got %g)", h);
  if (int e = check_channels_1_or_3("idn_nlmeans_weights", c)) return e;
  if (int e = nlm_check_sizes("idn_nlmeans_weights", template_size, search_size)) return e;
  *n_weights = nlm_fill_weights(h, c, template_size, search_size, wt_out, cap);
  *shift = nlm_shift(template_size);
  *fixed_point_mult = INT_MAX / (search_size * search_size * 255);
  return IDN_OK;
}

extern "C" int idn_nlmeans_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                              int64_t row_stride, int template_size, int search_size,
                              const int32_t* weights_dev, int n_weights, void* stream) {
  using namespace idn;
  const char* const name = "idn_nlmeans_u8";
  IDN_CHECK_ARG(src && dst && weights_dev, "%s: null pointer", name);
  if (int e = check_not_in_place(name, src, dst)) return e;
  if (int e = check_image_1_or_3(name, n, h, w, c, row_stride)) return e;
  if (int e = nlm_check_sizes(name, template_size, search_size)) return e;
  const int sr = search_size / 2, b = template_size / 2 + sr;
  IDN_CHECK_ARG(h > b && w > b, "idn_nlmeans_u8: image %d x %d smaller than the %d pixels the "
                "template and search windows need", h, w, b + 1);
  IDN_CHECK_ARG(n_weights >= 1, "idn_nlmeans_u8: n_weights must be positive (got %d)", n_weights);
  if (n_weights > IDN_NLMEANS_MAX_WEIGHTS)
    return set_error(IDN_EUNSUPPORTED, "idn_nlmeans_u8: a weight table of %d entries exceeds "
                     "IDN_NLMEANS_MAX_WEIGHTS (%d): h is too large", n_weights,
                     IDN_NLMEANS_MAX_WEIGHTS);
  if (n == 0) return IDN_OK;
  const int tiles_x = (w + nlm_ow(template_size) - 1) / nlm_ow(template_size);
  const int tiles_y = (h + NLM_ROWS - 1) / NLM_ROWS;
  if ((int64_t)n * tiles_x * tiles_y > (int64_t)INT_MAX) return batch_too_large(name);
  const unsigned grid = (unsigned)(n * tiles_x * tiles_y);
  const size_t lds = ((size_t)NLM_PITCH * (NLM_ROWS + 2 * b) + (size_t)n_weights + 1) * 4;
  const hipStream_t st = as_stream(stream);
  hipError_t e;
  switch (template_size) {
    case 3: e = launch_nlm<3>(c, grid, lds, st, src, dst, h, w, row_stride, sr, tiles_x, tiles_y, weights_dev, n_weights); break;
    case 5: e = launch_nlm<5>(c, grid, lds, st, src, dst, h, w, row_stride, sr, tiles_x, tiles_y, weights_dev, n_weights); break;
    default: e = launch_nlm<7>(c, grid, lds, st, src, dst, h, w, row_stride, sr, tiles_x, tiles_y, weights_dev, n_weights); break;
  }
  if (e != hipSuccess)
    return set_error(IDN_EHIP, "idn_nlmeans_u8: launch failed (%zu bytes of LDS): %s", lds,
                     hipGetErrorString(e));
  return IDN_OK;
}

extern "C" int idn_nlmeans_colored_weights(double h, double h_color, int template_size,
                                           int search_size, int32_t* wt_l, int cap_l, int* n_l,
                                           int32_t* wt_ab, int cap_ab, int* n_ab, int* shift,
                                           int* fixed_point_mult) {
  using namespace idn;
  IDN_CHECK_ARG(n_l && n_ab && shift && fixed_point_mult && (wt_l || cap_l == 0) &&
                (wt_ab || cap_ab == 0), "idn_nlmeans_colored_weights: null pointer");
  IDN_CHECK_ARG(cap_l >= 0 && cap_ab >= 0, "idn_nlmeans_colored_weights: negative cap %d / %d",
                cap_l, cap_ab);
  IDN_CHECK_ARG(h > 0.0 && h < INFINITY, "idn_nlmeans_colored_weights: h must be positive and "
                "finite (got %g)", h);
  IDN_CHECK_ARG(h_color > 0.0 && h_color < INFINITY, "idn_nlmeans_colored_weights: h_color must "
                "be positive and finite (got %g)", h_color);
  if (int e = nlm_check_sizes("idn_nlmeans_colored_weights", template_size, search_size)) return e;
  *n_l = nlm_fill_weights(h, 1, template_size, search_size, wt_l, cap_l);
  *n_ab = nlm_fill_weights(h_color, 2, template_size, search_size, wt_ab, cap_ab);
  *shift = nlm_shift(template_size);
  *fixed_point_mult = INT_MAX / (search_size * search_size * 255);
  return IDN_OK;
}

extern "C" size_t idn_nlmeans_colored_workspace_size(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return idn::align_up((size_t)n * h * w, 256);
}

extern "C" int idn_nlmeans_colored_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                                      int64_t row_stride, int template_size, int search_size,
                                      const int32_t* wt_l_dev, int n_l, const int32_t* wt_ab_dev,
                                      int n_ab, void* workspace, size_t ws_bytes, void* stream) {
  using namespace idn;
  const char* const name = "idn_nlmeans_colored_u8";
  IDN_CHECK_ARG(src && dst && wt_l_dev && wt_ab_dev, "%s: null pointer", name);
  if (int e = check_not_in_place(name, src, dst)) return e;
  if (int e = check_shape(name, n, h, w)) return e;
  if (int e = check_row_stride(name, row_stride, w, 3, "3")) return e;
  if (int e = nlm_check_sizes(name, template_size, search_size)) return e;
  const int sr = search_size / 2, b = template_size / 2 + sr;
  IDN_CHECK_ARG(h > b && w > b, "%s: image %d x %d smaller than the %d pixels the template and "
                "search windows need", name, h, w, b + 1);
  IDN_CHECK_ARG(n_l >= 1 && n_ab >= 1, "%s: n_weights must be positive (got %d, %d)", name, n_l,
                n_ab);
  if (n_l > IDN_NLMEANS_MAX_WEIGHTS || n_ab > IDN_NLMEANS_MAX_WEIGHTS)
    return set_error(IDN_EUNSUPPORTED, "%s: a weight table of %d / %d entries exceeds "
                     "IDN_NLMEANS_MAX_WEIGHTS (%d): h or h_color is too large", name, n_l, n_ab,
                     IDN_NLMEANS_MAX_WEIGHTS);
  const size_t need = idn_nlmeans_colored_workspace_size(n, h, w);  // reports 0 bytes for NULL
  if (int e = check_workspace_got(name, workspace, workspace ? ws_bytes : 0, need, IDN_EINVAL))
    return e;
  if (n == 0) return IDN_OK;
  const int tiles_x = (w + nlm_ow(template_size) - 1) / nlm_ow(template_size);
  const int tiles_y = (h + NLM_ROWS - 1) / NLM_ROWS;
  if ((int64_t)n * tiles_x * tiles_y > (int64_t)INT_MAX) return batch_too_large(name);
  const unsigned grid = (unsigned)(n * tiles_x * tiles_y);
  const size_t tile = (size_t)NLM_PITCH * (NLM_ROWS + 2 * b);
  const size_t lds_l = (tile + (size_t)n_l + 1) * 4 + NLM_CBRT_BYTES;
  const size_t lds_ab = (tile + (size_t)n_ab + 1) * 4 + NLM_CBRT_BYTES + NLM_YF_BYTES;
  const hipStream_t st = as_stream(stream);
  uint8_t* plane = static_cast<uint8_t*>(workspace);
  hipError_t e;
  switch (template_size) {
    case 3: e = launch_nlm_colored<3>(grid, lds_l, lds_ab, st, src, dst, h, w, row_stride, sr, tiles_x, tiles_y, wt_l_dev, n_l, wt_ab_dev, n_ab, plane); break;
    case 5: e = launch_nlm_colored<5>(grid, lds_l, lds_ab, st, src, dst, h, w, row_stride, sr, tiles_x, tiles_y, wt_l_dev, n_l, wt_ab_dev, n_ab, plane); break;
    default: e = launch_nlm_colored<7>(grid, lds_l, lds_ab, st, src, dst, h, w, row_stride, sr, tiles_x, tiles_y, wt_l_dev, n_l, wt_ab_dev, n_ab, plane); break;
  }
  if (e != hipSuccess)
    return set_error(IDN_EHIP, "%s: launch failed (%zu / %zu bytes of LDS): %s", name, lds_l,
                     lds_ab, hipGetErrorString(e));
  return IDN_OK;
}
