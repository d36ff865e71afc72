// skimage.util.random_noise modes used by the reference's noise closures, on u8 HxWxC batches:
//   gaussian  lib/model/test.py:193-307, minibatch.py:87-201   out = clip(x + N(mean, sd), 0, 1)
//   speckle   lib/model/test.py:476-590, minibatch.py:374-490  out = clip(x + x*N(mean, sd), 0, 1)
//   s&p       lib/model/test.py:357-474, minibatch.py:253-372  out = 1 / 0 / x by two uniforms
//   poisson   lib/model/test.py:309-355, minibatch.py:203-251  out = clip(P(x*vals)/vals, 0, 1)
// with x = v * (1/255) in float64 (img_as_float) and the caller's U8 cast (255*out).astype(uint8).
// The float64 op order is numpy's (file compiled with -ffp-contract=off; explicit _rn ops), so
// with a replayed random field (numpy's own draws) the outputs are bit-exact; with the Philox
// stream they are statistically equivalent (tests/test_noise_gpu.py).
//
// RNG: Philox4x32 keyed by (seed ^ kind tag); counter = (element group, stream tag, image id).
// Gaussian / speckle have two streams (noise_apply.hpp): u8-only outputs draw 16-bit uniforms
// (fp32 Box-Muller, fp32 apply on the 0..255 scale, tag 0, refinement tag 3); float64 outputs
// draw 53-bit uniforms with an fp64 Box-Muller (tag 2) and apply in numpy's float64 order, the
// U8 then being trunc(255 * out) of that value.  s&p (tag 1) and Poisson have one stream each.
// Every layout (flat 16-element kernels for compact rows, element kernels for strided ones) draws
// the same values.  Image id = offset + image index (or an id array), so a rank that owns images
// [a, b) of a batch draws exactly what a single GPU would for those images.
//
// This unit holds gaussian, speckle and s&p and the entry points of all four modes; the Poisson
// sampler is noise_poisson.hip (reached through noise_poisson_launch), the periodic pattern and
// cv2.add(u8, u8) are noise_pattern.hip, the reference's own additive noises noise_add.hip.
#include "noise_common.hpp"
#include "f64_math.hpp"
#include "ycc.hpp"

#include <math.h>

#include <algorithm>
#include <type_traits>

namespace idn {

// two standard normals in float64 from one Philox4x32-10 block (counter (pair, 2, image id)):
// 53-bit uniforms u1 = (a + 1) 2^-53 in (0, 1], u2 = b 2^-53 in [0, 1) (|z| <= 8.57),
// rad = sqrt(-2 ln u1), (cos, sin)(2 pi u2).  ln and (sin, cos) from the integers a + 1, b by the
// table-driven forms of f64_math.hpp (within ~1.4 ulp; the library log / sincospi, ~130 fp64
// operations per pair, made the float64 stream fp64-issue-bound)
// The tables live in LDS (F64mLds, staged once per workgroup): per-lane gathers from the
// __constant__ copies went through the vector L1 at one cache line per lane and cost more than
// the fp64 work they save.
struct F64mLds {
  double ln[f64m::LN_TAB_N];
  double sc[f64m::SC_TAB_N];
};
__device__ __forceinline__ void stage_f64m(F64mLds& t) {
  for (int i = threadIdx.x; i < f64m::LN_TAB_N; i += blockDim.x) t.ln[i] = f64m::LN_TAB[i];
  for (int i = threadIdx.x; i < f64m::SC_TAB_N; i += blockDim.x) t.sc[i] = f64m::SC_TAB[i];
  __syncthreads();
}
__device__ __forceinline__ void normal2_f64(const u32x4& r, const F64mLds& t, double& z0,
                                            double& z1) {
  const uint64_t a = ((uint64_t)r.x << 21) | (r.y >> 11), b = ((uint64_t)r.z << 21) | (r.w >> 11);
  const double rad = sqrt(fmax(-2.0 * f64m::ln_u53(a + 1, t.ln), 0.0));
  double sn, cs;
  f64m::sincos2pi_u53(b, t.sc, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

// element form, one thread per element pair: the noise value n of each element is numpy's own
// draw (SRC_REPLAY: N(mean, sd) field, bit-exact with the reference) or mean + sd * z from the
// float64 stream (SRC_F64); out = clip(x + n) / clip(x + x n) in numpy's op order, U8 = trunc(255
// out).  Any row stride and slot layout.
enum NoiseSrc { SRC_REPLAY = 0, SRC_F64 = 1 };
template <int KIND, int SRC>
__global__ __launch_bounds__(256) void noise_gauss_kernel(NoiseArgs a) {
  __shared__ F64mLds tab;
  if constexpr (SRC == SRC_F64) stage_f64m(tab);
  const int64_t pairs = (a.elems + 1) / 2;
  const int64_t total = pairs * a.n;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(t / pairs);
    const int64_t pr = t - (int64_t)img * pairs;
    double nz[2];
    if constexpr (SRC == SRC_REPLAY) {
      const int64_t e0 = 2 * pr;
      nz[0] = a.replay[(int64_t)img * a.elems + e0];
      nz[1] = (e0 + 1 < a.elems) ? a.replay[(int64_t)img * a.elems + e0 + 1] : 0.0;
    } else {
      const uint64_t gimg = image_id(a, img);
      const u32x4 r = philox4x32(u32x4{(uint32_t)pr, 2u ^ ((uint32_t)(pr >> 32) << 8),
                                       (uint32_t)gimg, (uint32_t)(gimg >> 32)},
                                 a.key);
      double z0, z1;
      normal2_f64(r, tab, z0, z1);
      // np.random.normal(mean, sd): loc + scale * gauss
      nz[0] = __dadd_rn(a.p0, __dmul_rn(a.p1, z0));
      nz[1] = __dadd_rn(a.p0, __dmul_rn(a.p1, z1));
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int64_t e = 2 * pr + s;
      if (e >= a.elems) break;
      const int64_t pix = e / a.c;
      const int ch = (int)(e - pix * a.c);
      const int y = (int)(pix / a.w), x = (int)(pix - (int64_t)y * a.w);
      const int64_t boff = slot_of(a, img) * a.h * a.row_stride + (int64_t)y * a.row_stride +
                           (int64_t)x * a.c + ch;
      const double xv = img_as_float(a.src[boff]);
      double out;
      if (KIND == IDN_NOISE_GAUSSIAN) out = clip01(__dadd_rn(xv, nz[s]));
      else out = clip01(__dadd_rn(xv, __dmul_rn(xv, nz[s])));
      store_out(a, img, e, boff, out);
    }
  }
}

// Float64 gaussian / speckle on compact 3-channel images, with the bior1.5 / Haar wavelet's colour
// range reduced on the fly (the live test path: random_noise's float64 image goes straight to
// denoise_wavelet, lib/model/test.py:1678-1684 -> 1807-1810).  One thread per pixel pair = the
// three element pairs 3q .. 3q+2 of noise_gauss_kernel (the same draws, the same op order: the
// image is bit-identical), plus per image the fp64 min / max of skimage rgb2ycbcr's three dot
// products of the output (ycc_dots, wl_color_minmax's chain), reduced per workgroup and folded
// into ycc[6 img ..] as order-preserving keys with the offsets added after the reduction -- what
// wl_color_minmax would compute from the stored image, without reading its 24 B/pixel back.
template <int KIND, int SRC>
__global__ __launch_bounds__(256) void noise_gauss_ycc_kernel(NoiseArgs a) {
  const int img = blockIdx.y;
  const int64_t npp = a.elems / 6;
  const int64_t slot = slot_of(a, img);
  const uint8_t* s = a.src + slot * a.elems;
  double* of = a.out_f64 + slot * a.elems;
  uint8_t* ou = a.out_u8 ? a.out_u8 + slot * a.elems : nullptr;
  const uint64_t gimg = image_id(a, img);
  __shared__ F64mLds tab;
  if constexpr (SRC == SRC_F64) stage_f64m(tab);
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npp;
       q += (int64_t)gridDim.x * blockDim.x) {
    double nz[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t pr = 3 * q + k;
      if constexpr (SRC == SRC_REPLAY) {
        nz[2 * k] = a.replay[(int64_t)img * a.elems + 2 * pr];
        nz[2 * k + 1] = a.replay[(int64_t)img * a.elems + 2 * pr + 1];
      } else {
        const u32x4 r = philox4x32(u32x4{(uint32_t)pr, 2u ^ ((uint32_t)(pr >> 32) << 8),
                                         (uint32_t)gimg, (uint32_t)(gimg >> 32)},
                                   a.key);
        double z0, z1;
        normal2_f64(r, tab, z0, z1);
        nz[2 * k] = __dadd_rn(a.p0, __dmul_rn(a.p1, z0));
        nz[2 * k + 1] = __dadd_rn(a.p0, __dmul_rn(a.p1, z1));
      }
    }
    const uint16_t* s2 = reinterpret_cast<const uint16_t*>(s + 6 * q);  // 2-byte aligned
    const uint32_t b01 = s2[0], b23 = s2[1], b45 = s2[2];
    const uint32_t bytes[6] = {b01 & 0xFFu, b01 >> 8, b23 & 0xFFu, b23 >> 8, b45 & 0xFFu, b45 >> 8};
    double out[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const double xv = img_as_float(bytes[e]);
      out[e] = KIND == IDN_NOISE_GAUSSIAN ? clip01(__dadd_rn(xv, nz[e]))
                                          : clip01(__dadd_rn(xv, __dmul_rn(xv, nz[e])));
    }
    double2* o2 = reinterpret_cast<double2*>(of + 6 * q);  // 16-byte aligned (48 q bytes)
    o2[0] = make_double2(out[0], out[1]);
    o2[1] = make_double2(out[2], out[3]);
    o2[2] = make_double2(out[4], out[5]);
    if (ou) {
      uint16_t* u2 = reinterpret_cast<uint16_t*>(ou + 6 * q);
      u2[0] = (uint16_t)(u8_of(out[0]) | (u8_of(out[1]) << 8));
      u2[1] = (uint16_t)(u8_of(out[2]) | (u8_of(out[3]) << 8));
      u2[2] = (uint16_t)(u8_of(out[4]) | (u8_of(out[5]) << 8));
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      double d[3];
      ycc_dots(out[3 * p], out[3 * p + 1], out[3 * p + 2], d);
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // finite values: fmin / fmax are plain selects
        mn[c] = fmin(mn[c], d[c]);
        mx[c] = fmax(mx[c], d[c]);
      }
    }
  }
  __shared__ double red[2][3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double da = mn[c], db = mx[c];
    for (int o = 32; o > 0; o >>= 1) {
      da = fmin(da, __shfl_xor(da, o));
      db = fmax(db, __shfl_xor(db, o));
    }
    if (lane == 0) {
      red[0][c][wave] = da;
      red[1][c][wave] = db;
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    double da = red[0][c][0], db = red[1][c][0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
      da = fmin(da, red[0][c][k]);
      db = fmax(db, red[1][c][k]);
    }
    if (da <= db) {  // a workgroup with no pixel leaves the keys alone
      atomicMin(a.ycc + 6 * img + c, dkey(__dadd_rn(da, ycc_offset(c))));
      atomicMax(a.ycc + 6 * img + 3 + c, dkey(__dadd_rn(db, ycc_offset(c))));
    }
  }
}

__global__ void ycc_keys_init(unsigned long long* keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * n) keys[i] = (i % 6) < 3 ? ~0ull : 0ull;
}

// ---- u8 stream, flat form (compact rows): 16 consecutive elements per thread ------------------
// One 16-byte load / store per lane, image = blockIdx.y, no 64-bit index division; the stream is
// noise16_u8 (noise_apply.hpp).
template <int KIND, bool MEAN0 = false>
__global__ __launch_bounds__(256) void noise_flat16_kernel(NoiseArgs a, uint32_t t_flip,
                                                           uint32_t t_salt) {
  const int img = blockIdx.y;
  const uint32_t chunk = blockIdx.x * 256u + threadIdx.x;
  const int64_t e0 = (int64_t)chunk * 16;
  if (e0 >= a.elems) return;
  const uint64_t gimg = image_id(a, img);
  const int64_t base = slot_of(a, img) * a.elems + e0;
  const v4u raw = *reinterpret_cast<const v4u*>(a.src + base);
  const v4u o = noise16_u8<KIND, MEAN0>(raw, chunk, gimg, a.key, a.p0, a.p1, t_flip, t_salt,
                                        a.out_f64 ? a.out_f64 + base : nullptr);
  if (a.out_u8) *reinterpret_cast<v4u*>(a.out_u8 + base) = o;
}

// ---- u8 stream, element form (any layout): the same 16-element chunks gathered byte by byte ---
template <int KIND, bool MEAN0 = false>
__global__ __launch_bounds__(256) void noise_elem16_kernel(NoiseArgs a, uint32_t t_flip,
                                                           uint32_t t_salt) {
  const int64_t chunks = (a.elems + 15) / 16;
  const int64_t total = chunks * a.n;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(t / chunks);
    const uint32_t chunk = (uint32_t)(t - (int64_t)img * chunks);
    const int64_t e0 = (int64_t)chunk * 16;
    int64_t off[16];
    uint32_t in[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t e = e0 + i;
      off[i] = -1;
      if (e < a.elems) {
        const int64_t pix = e / a.c;
        const int ch = (int)(e - pix * a.c);
        const int y = (int)(pix / a.w), x = (int)(pix - (int64_t)y * a.w);
        off[i] = slot_of(a, img) * a.h * a.row_stride + (int64_t)y * a.row_stride +
                 (int64_t)x * a.c + ch;
        in[i >> 2] |= (uint32_t)a.src[off[i]] << (8 * (i & 3));
      }
    }
    double of[16];
    const v4u o = noise16_u8<KIND, MEAN0>(v4u{in[0], in[1], in[2], in[3]}, chunk, image_id(a, img),
                                          a.key, a.p0, a.p1, t_flip, t_salt,
                                          (KIND == IDN_NOISE_SAP && a.out_f64) ? of : nullptr);
    const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (off[i] < 0) continue;
      if (a.out_u8) a.out_u8[off[i]] = (uint8_t)(ow[i >> 2] >> (8 * (i & 3)));
      if (KIND == IDN_NOISE_SAP && a.out_f64) a.out_f64[slot_of(a, img) * a.elems + e0 + i] = of[i];
    }
  }
}

// salt & pepper, replay: flipped = U1 < cdf0(amount), salted = U2 < cdf0(salt_vs_pepper) on
// numpy's own random_sample fields
__global__ __launch_bounds__(256) void noise_sap_kernel(NoiseArgs a) {
  const int64_t total = a.elems * a.n;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(t / a.elems);
    const int64_t e = t - (int64_t)img * a.elems;
    const double u1 = a.replay[t], u2 = a.replay[total + t];
    const int64_t pix = e / a.c;
    const int ch = (int)(e - pix * a.c);
    const int y = (int)(pix / a.w), x = (int)(pix - (int64_t)y * a.w);
    const int64_t boff =
        slot_of(a, img) * a.h * a.row_stride + (int64_t)y * a.row_stride + (int64_t)x * a.c + ch;
    double out = img_as_float(a.src[boff]);
    if (u1 < a.p0) out = (u2 < a.p1) ? 1.0 : 0.0;
    store_out(a, img, e, boff, out);
  }
}

// two runtime flags -> one template instance: f(std::bool_constant<a>, std::bool_constant<b>);
// kind_of / src_of turn the constants into the gaussian / speckle kernels' template arguments
template <class F>
static void with_flags(bool a, bool b, F&& f) {
  if (a && b) f(std::true_type{}, std::true_type{});
  else if (a) f(std::true_type{}, std::false_type{});
  else if (b) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
constexpr int kind_of(bool gauss) { return gauss ? IDN_NOISE_GAUSSIAN : IDN_NOISE_SPECKLE; }
constexpr int src_of(bool replay) { return replay ? SRC_REPLAY : SRC_F64; }

static int noise_u8_impl(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h, int w,
                         int c, int64_t row_stride, int kind, double p0, double p1, uint64_t seed,
                         uint64_t offset, const uint64_t* ids, const int64_t* slots,
                         const double* replay,
                         void* workspace, size_t ws_bytes, void* stream) {
  const int rc = check_noise_shape("idn_noise_u8", src, out_u8, out_f64, n, h, w, c, row_stride,
                                   true);
  if (rc != IDN_OK) return rc;
  IDN_CHECK_ARG(kind >= 0 && kind <= 3, "idn_noise_u8: unknown noise kind %d", kind);
  IDN_CHECK_ARG((const void*)out_u8 != (const void*)src || kind != IDN_NOISE_POISSON,
                "idn_noise_u8: poisson cannot run in place");
  if (n == 0) return IDN_OK;
  hipStream_t st = as_stream(stream);
  NoiseArgs a = make_noise_args(src, out_u8, out_f64, n, h, w, c, row_stride, kind, seed, offset,
                                ids, slots, replay, nullptr);
  // flat form: Philox stream, compact rows, 16-element chunks that never straddle images
  const bool flat = !replay && row_stride == (int64_t)w * c && a.elems % 16 == 0 &&
                    ((uintptr_t)src & 15) == 0 && ((uintptr_t)out_u8 & 15) == 0 &&
                    ((uintptr_t)out_f64 & 7) == 0 && a.elems / 16 < ((int64_t)1 << 31);
  IDN_CHECK_ARG((a.elems + 15) / 16 < ((int64_t)1 << 32), "idn_noise_u8: image too large");
  const unsigned g16 = grid_for((a.elems + 15) / 16 * n);
  switch (kind) {
    case IDN_NOISE_GAUSSIAN:
    case IDN_NOISE_SPECKLE: {
      IDN_CHECK_ARG(p1 >= 0.0, "idn_noise_u8: var must be >= 0");
      a.p0 = p0;             // mean
      a.p1 = pow(p1, 0.5);   // var ** 0.5 (random_noise)
      const int64_t work = (a.elems + 1) / 2 * n;
      const bool g = kind == IDN_NOISE_GAUSSIAN, m0 = a.p0 == 0.0;
      if (replay || out_f64) {  // numpy's field, or the float64 stream: float64 apply
        with_flags(g, replay != nullptr, [&](auto G, auto R) {
          hipLaunchKernelGGL((noise_gauss_kernel<kind_of(G.value), src_of(R.value)>),
                             dim3(grid_for(work)), dim3(256), 0, st, a);
        });
      } else if (flat) {
        const dim3 grid((unsigned)((a.elems / 16 + 255) / 256), (unsigned)n);
        with_flags(g, m0, [&](auto G, auto M0) {
          hipLaunchKernelGGL((noise_flat16_kernel<kind_of(G.value), M0.value>), grid, dim3(256), 0,
                             st, a, 0u, 0u);
        });
      } else {
        with_flags(g, m0, [&](auto G, auto M0) {
          hipLaunchKernelGGL((noise_elem16_kernel<kind_of(G.value), M0.value>), dim3(g16),
                             dim3(256), 0, st, a, 0u, 0u);
        });
      }
      break;
    }
    case IDN_NOISE_SAP: {
      IDN_CHECK_ARG(p0 >= 0.0 && p0 <= 1.0 && p1 >= 0.0 && p1 <= 1.0,
                    "idn_noise_u8: amount / salt_vs_pepper must be in [0, 1]");
      // np.random.choice([True, False], p=[p, 1-p]): True iff random_sample < cdf[0]
      a.p0 = p0 / (p0 + (1.0 - p0));
      a.p1 = p1 / (p1 + (1.0 - p1));
      const uint32_t tf = sap_threshold(a.p0), ts = sap_threshold(a.p1);
      if (replay) {
        hipLaunchKernelGGL(noise_sap_kernel, dim3(grid_for(a.elems * n)), dim3(256), 0, st, a);
      } else if (flat) {
        // 16-bit uniform thresholds: P(u < t / 2^16) within 2^-16 of cdf0
        const dim3 grid((unsigned)((a.elems / 16 + 255) / 256), (unsigned)n);
        hipLaunchKernelGGL(noise_flat16_kernel<IDN_NOISE_SAP>, grid, dim3(256), 0, st, a, tf, ts);
      } else {
        hipLaunchKernelGGL(noise_elem16_kernel<IDN_NOISE_SAP>, dim3(g16), dim3(256), 0, st, a, tf, ts);
      }
      break;
    }
    default: {  // POISSON
      const int prc = noise_poisson_launch(a, flat, workspace, ws_bytes, st);
      if (prc != IDN_OK) return prc;
      break;
    }
  }
  IDN_CHECK_LAUNCH("idn_noise_u8");
  return IDN_OK;
}
}  // namespace idn

extern "C" int idn_noise_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h,
                            int w, int c, int64_t row_stride, int kind, double p0, double p1,
                            uint64_t seed, uint64_t offset, const double* replay, void* workspace,
                            size_t ws_bytes, void* stream) {
  return idn::noise_u8_impl(src, out_u8, out_f64, n, h, w, c, row_stride, kind, p0, p1, seed,
                            offset, nullptr, nullptr, replay, workspace, ws_bytes, stream);
}

extern "C" int idn_noise_ids_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n,
                                int h, int w, int c, int64_t row_stride, int kind, double p0,
                                double p1, uint64_t seed, const uint64_t* image_ids,
                                void* workspace, size_t ws_bytes, void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(image_ids || n == 0, "idn_noise_ids_u8: null image_ids");
  return noise_u8_impl(src, out_u8, out_f64, n, h, w, c, row_stride, kind, p0, p1, seed, 0,
                       image_ids, nullptr, nullptr, workspace, ws_bytes, stream);
}

extern "C" int idn_noise_slots_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n,
                                  int h, int w, int c, int64_t row_stride, int kind, double p0,
                                  double p1, uint64_t seed, const uint64_t* image_ids,
                                  const int64_t* slots, void* workspace, size_t ws_bytes,
                                  void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(image_ids || n == 0, "idn_noise_slots_u8: null image_ids");
  IDN_CHECK_ARG(slots || n == 0, "idn_noise_slots_u8: null slots");
  IDN_CHECK_ARG(row_stride == (int64_t)w * c, "idn_noise_slots_u8: slots need compact rows "
                "(row_stride %lld != w*c)", (long long)row_stride);
  return noise_u8_impl(src, out_u8, out_f64, n, h, w, c, row_stride, kind, p0, p1, seed, 0,
                       image_ids, slots, nullptr, workspace, ws_bytes, stream);
}

extern "C" int idn_noise_ycc_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n,
                                int h, int w, int kind, double p0, double p1, uint64_t seed,
                                uint64_t offset, const uint64_t* image_ids, const double* replay,
                                uint64_t* ycc_keys, void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(src && out_f64 && ycc_keys, "idn_noise_ycc_u8: null src / out_f64 / ycc_keys");
  IDN_CHECK_ARG(kind == IDN_NOISE_GAUSSIAN || kind == IDN_NOISE_SPECKLE,
                "idn_noise_ycc_u8: gaussian or speckle only (got %d)", kind);
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0, "idn_noise_ycc_u8: bad shape");
  IDN_CHECK_ARG(p1 >= 0.0, "idn_noise_ycc_u8: var must be >= 0");
  if (n == 0) return IDN_OK;
  const int64_t elems = (int64_t)h * w * 3;
  if (elems % 6 != 0 || ((uintptr_t)src & 1) || ((uintptr_t)out_f64 & 15) ||
      ((uintptr_t)out_u8 & 1) || n > 65535)
    return set_error(IDN_EUNSUPPORTED, "idn_noise_ycc_u8: needs an even pixel count per image, "
                     "2-byte aligned u8 and 16-byte aligned float64 buffers");
  hipStream_t st = as_stream(stream);
  NoiseArgs a = make_noise_args(src, out_u8, out_f64, n, h, w, 3, (int64_t)w * 3, kind, seed,
                                offset, image_ids, nullptr, replay,
                                reinterpret_cast<unsigned long long*>(ycc_keys));
  a.p0 = p0;
  a.p1 = pow(p1, 0.5);
  hipLaunchKernelGGL(ycc_keys_init, dim3((6 * n + 255) / 256), dim3(256), 0, st, a.ycc, n);
  // about 2048 workgroups in all: one image alone spreads over the chip, a batch keeps the
  // per-workgroup atomics few
  const int64_t npp = elems / 6;
  const unsigned gx = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((npp + 255) / 256, (2048 + n - 1) / n));
  const dim3 grid(gx, (unsigned)n);
  with_flags(kind == IDN_NOISE_GAUSSIAN, replay != nullptr, [&](auto G, auto R) {
    hipLaunchKernelGGL((noise_gauss_ycc_kernel<kind_of(G.value), src_of(R.value)>), grid,
                       dim3(256), 0, st, a);
  });
  IDN_CHECK_LAUNCH("idn_noise_ycc_u8");
  return IDN_OK;
}
