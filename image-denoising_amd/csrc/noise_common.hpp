// What the noise units share: the kernel argument struct of the skimage-mode generators with its
// device accessors (noise.hip, noise_poisson.hip), the host's argument checks and launch helpers
// (those two, noise_pattern.hip, noise_add.hip), and the one seam between units: noise.hip hands a
// Poisson call to noise_poisson.hip through noise_poisson_launch.  The build has no relocatable
// device code, so every kernel is instantiated in the unit that launches it.
#pragma once

#include "idn_common.hpp"
#include "noise_apply.hpp"

namespace idn {

constexpr uint64_t KIND_TAG = 0x9E3779B97F4A7C15ull;

struct NoiseArgs {
  const uint8_t* src;
  uint8_t* out_u8;
  double* out_f64;
  const double* replay;
  const uint32_t* vals;  // poisson: per-image vals (power of two), workspace
  int n, h, w, c;
  int64_t row_stride;
  int64_t elems;  // h*w*c
  double p0, p1;  // mean/sd (gaussian, speckle), sap thresholds
  uint64_t key, offset;
  const uint64_t* ids;  // optional per-image ids (device); else id = offset + image index
  const int64_t* slots;  // optional batch positions (device): image i of the launch reads and
                         // writes image slots[i] of src / out_u8 / out_f64; else slot = i
  unsigned long long* ycc;  // noise_gauss_ycc_kernel: per image the colour range keys (ycc.hpp)
};
__device__ __forceinline__ uint64_t image_id(const NoiseArgs& a, int img) {
  return a.ids ? a.ids[img] : a.offset + (uint64_t)img;
}
__device__ __forceinline__ int64_t slot_of(const NoiseArgs& a, int img) {
  return a.slots ? a.slots[img] : (int64_t)img;
}

__device__ __forceinline__ void store_out(const NoiseArgs& a, int img, int64_t e, int64_t boff,
                                          double out) {
  if (a.out_f64) a.out_f64[slot_of(a, img) * a.elems + e] = out;
  if (a.out_u8) a.out_u8[boff] = u8_of(out);
}

inline unsigned grid_for(int64_t work, int64_t cap = 65536) {
  int64_t b = (work + 255) / 256;
  if (b < 1) b = 1;
  return (unsigned)(b > cap ? cap : b);
}

// every field set: vals (Poisson) and p0 / p1 (the kind's own mapping of the caller's two
// parameters) start at zero and are filled in by the kind's branch
inline NoiseArgs make_noise_args(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n,
                                 int h, int w, int c, int64_t row_stride, int kind, uint64_t seed,
                                 uint64_t offset, const uint64_t* ids, const int64_t* slots,
                                 const double* replay, unsigned long long* ycc) {
  NoiseArgs a{};
  a.src = src;
  a.out_u8 = out_u8;
  a.out_f64 = out_f64;
  a.replay = replay;
  a.vals = nullptr;
  a.n = n;
  a.h = h;
  a.w = w;
  a.c = c;
  a.row_stride = row_stride;
  a.elems = (int64_t)h * w * c;
  a.p0 = 0.0;
  a.p1 = 0.0;
  a.key = seed ^ (KIND_TAG * (uint64_t)(kind + 1));
  a.offset = offset;
  a.ids = ids;
  a.slots = slots;
  a.ycc = ycc;
  return a;
}

// the shape rules of the per-element generators (idn_noise_*_u8, idn_noise_add_*_u8), reported
// under the caller's name.  The two families word the batch limit differently (got_n: with the
// count); error text is part of the ABI's behaviour, so each keeps its own.
inline int check_noise_shape(const char* name, const uint8_t* src, const uint8_t* out_u8,
                             const double* out_f64, int n, int h, int w, int c,
                             int64_t row_stride, bool got_n) {
  IDN_CHECK_ARG(src, "%s: null src", name);
  IDN_CHECK_ARG(out_u8 || out_f64, "%s: at least one of out_u8 / out_f64 is required", name);
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0 && c >= 1 && c <= 4, "%s: bad shape", name);
  // the per-image kernels put the image on gridDim.y
  if (got_n) IDN_CHECK_ARG(n <= 65535, "%s: at most 65535 images per call (got %d)", name, n);
  IDN_CHECK_ARG(n <= 65535, "%s: at most 65535 images per call", name);
  IDN_CHECK_ARG(row_stride >= (int64_t)w * c, "%s: row_stride < w*c", name);
  return IDN_OK;
}

// the Poisson branch of noise_u8_impl (noise_poisson.hip): workspace check, distinct-value masks,
// vals, the tables, then the flat or the element kernel on `st`; the caller checks the launch
int noise_poisson_launch(NoiseArgs a, bool flat, void* workspace, size_t ws_bytes, hipStream_t st);

}  // namespace idn
