// The periodic noise pattern (add_periodic_noise, lib/model/test.py:1128-1298): the pattern
// U8(255 * sin(linspace(-A, A, size))), cv2.add(u8, u8) of a batch and one pattern, and the plain
// slot copy that carries the noise-free members of a mixed batch.
#include "noise_common.hpp"

#include <math.h>

#include <algorithm>

namespace idn {

// cv2.add(u8, u8) on compact rows, 16 bytes per thread: SWAR saturating byte add
__device__ __forceinline__ uint32_t addsat_u8x4(uint32_t a, uint32_t b) {
  const uint32_t low7 = (a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu);  // no carry out of any byte
  const uint32_t sum = low7 ^ ((a ^ b) & 0x80808080u);          // byte sums mod 256
  const uint32_t carry = ((a & b) | ((a | b) & ~sum)) & 0x80808080u;
  return sum | ((carry >> 7) * 0xFFu);
}
__global__ __launch_bounds__(256) void add_pattern_flat_kernel(const uint8_t* __restrict__ src,
                                                               const uint8_t* __restrict__ pat,
                                                               uint8_t* __restrict__ dst,
                                                               int64_t per_img,
                                                               const int64_t* __restrict__ slots) {
  const int img = blockIdx.y;
  const int64_t nq = per_img / 16;
  const int64_t base = (slots ? slots[img] : (int64_t)img) * per_img;
  const v4u* s = reinterpret_cast<const v4u*>(src + base);
  const v4u* p = reinterpret_cast<const v4u*>(pat);
  v4u* d = reinterpret_cast<v4u*>(dst + base);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq;
       q += (int64_t)gridDim.x * blockDim.x) {
    const v4u a = s[q], b = p[q];
    d[q] = v4u{addsat_u8x4(a.x, b.x), addsat_u8x4(a.y, b.y), addsat_u8x4(a.z, b.z),
               addsat_u8x4(a.w, b.w)};
  }
}

// periodic pattern: t_i = i*step + (-A) (numpy linspace op order), t_last = A
__global__ __launch_bounds__(256) void periodic_kernel(uint8_t* __restrict__ pat, int64_t size,
                                                       double amp, double step) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < size;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double t = (i == size - 1) ? amp : __dadd_rn(__dmul_rn((double)i, step), -amp);
    const double y = __dmul_rn(sin(t), 255.0);
    // (uint8)(int32)trunc(y): truncate toward zero, wrap mod 256
    pat[i] = (uint8_t)(int)y;
  }
}

// cv2.add(u8, u8) = min(a + b, 255), 16 bytes per thread where aligned
__global__ __launch_bounds__(256) void add_pattern_kernel(const uint8_t* __restrict__ src,
                                                          const uint8_t* __restrict__ pat,
                                                          uint8_t* __restrict__ dst, int n, int h,
                                                          int rowbytes, int64_t row_stride,
                                                          const int64_t* __restrict__ slots) {
  const int64_t per_img = (int64_t)h * rowbytes;
  const int64_t total = per_img * n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(i / per_img);
    const int64_t e = i - (int64_t)img * per_img;
    const int y = (int)(e / rowbytes);
    const int64_t off = (slots ? slots[img] : (int64_t)img) * h * row_stride +
                        (int64_t)y * row_stride + (e - (int64_t)y * rowbytes);
    const uint32_t s = (uint32_t)src[off] + (uint32_t)pat[e];
    dst[off] = (uint8_t)(s > 255u ? 255u : s);
  }
}

// dst image slots[i] = src image slots[i] (compact images, 16 bytes per thread where aligned)
__global__ __launch_bounds__(256) void copy_slots_kernel(const uint8_t* __restrict__ src,
                                                         uint8_t* __restrict__ dst,
                                                         int64_t per_img,
                                                         const int64_t* __restrict__ slots) {
  const int64_t base = slots[blockIdx.y] * per_img;
  if ((per_img & 15) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const v4u* s = reinterpret_cast<const v4u*>(src + base);
    v4u* d = reinterpret_cast<v4u*>(dst + base);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < per_img / 16;
         q += (int64_t)gridDim.x * blockDim.x)
      d[q] = s[q];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_img;
         i += (int64_t)gridDim.x * blockDim.x)
      dst[base + i] = src[base + i];
  }
}

static int add_pattern_impl(const uint8_t* src, const uint8_t* pattern, uint8_t* dst, int n,
                            int h, int w, int c, int64_t row_stride, const int64_t* slots,
                            void* stream) {
  IDN_CHECK_ARG(src && pattern && dst, "idn_add_pattern_u8: null pointer");
  IDN_CHECK_ARG(n >= 0 && h > 0 && w > 0 && c > 0, "idn_add_pattern_u8: bad shape");
  IDN_CHECK_ARG(row_stride >= (int64_t)w * c, "idn_add_pattern_u8: row_stride < w*c");
  if (n == 0) return IDN_OK;
  const int64_t per_img = (int64_t)h * w * c;
  if (row_stride == (int64_t)w * c && per_img % 16 == 0 && n <= 65535 &&
      (((uintptr_t)src | (uintptr_t)pattern | (uintptr_t)dst) & 15) == 0) {
    const int64_t nq = per_img / 16;
    const unsigned gx = (unsigned)std::min<int64_t>((nq + 255) / 256, 1024);
    hipLaunchKernelGGL(add_pattern_flat_kernel, dim3(gx, (unsigned)n), dim3(256), 0,
                       as_stream(stream), src, pattern, dst, per_img, slots);
  } else {
    hipLaunchKernelGGL(add_pattern_kernel, dim3(grid_for((int64_t)n * h * w * c)), dim3(256), 0,
                       as_stream(stream), src, pattern, dst, n, h, w * c, row_stride, slots);
  }
  IDN_CHECK_LAUNCH("idn_add_pattern_u8");
  return IDN_OK;
}

}  // namespace idn

extern "C" int idn_periodic_pattern_u8(uint8_t* pattern, int h, int w, int c, double amplitude,
                                       void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(pattern, "idn_periodic_pattern_u8: null pattern");
  IDN_CHECK_ARG(h > 0 && w > 0 && c > 0, "idn_periodic_pattern_u8: bad shape");
  const int64_t size = (int64_t)h * w * c;
  // numpy.linspace(-A, A, size): step = (A - (-A)) / (size - 1)
  const double step = size > 1 ? (amplitude - (-amplitude)) / (double)(size - 1) : 0.0;
  hipLaunchKernelGGL(periodic_kernel, dim3(grid_for(size)), dim3(256), 0, as_stream(stream),
                     pattern, size, amplitude, step);
  IDN_CHECK_LAUNCH("idn_periodic_pattern_u8");
  return IDN_OK;
}

extern "C" int idn_add_pattern_u8(const uint8_t* src, const uint8_t* pattern, uint8_t* dst, int n,
                                  int h, int w, int c, int64_t row_stride, void* stream) {
  return idn::add_pattern_impl(src, pattern, dst, n, h, w, c, row_stride, nullptr, stream);
}

extern "C" int idn_add_pattern_slots_u8(const uint8_t* src, const uint8_t* pattern, uint8_t* dst,
                                        int n, int h, int w, int c, const int64_t* slots,
                                        void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(slots || n == 0, "idn_add_pattern_slots_u8: null slots");
  return add_pattern_impl(src, pattern, dst, n, h, w, c, (int64_t)w * c, slots, stream);
}

extern "C" int idn_copy_slots_u8(const uint8_t* src, uint8_t* dst, int n, int64_t per_img,
                                 const int64_t* slots, void* stream) {
  using namespace idn;
  IDN_CHECK_ARG(src && dst && (slots || n == 0), "idn_copy_slots_u8: null pointer");
  IDN_CHECK_ARG(n >= 0 && n <= 65535 && per_img > 0, "idn_copy_slots_u8: bad shape");
  if (n == 0 || src == dst) return IDN_OK;
  const unsigned gx = (unsigned)std::min<int64_t>((per_img / 16 + 255) / 256, 1024);
  hipLaunchKernelGGL(copy_slots_kernel, dim3(gx < 1 ? 1 : gx, (unsigned)n), dim3(256), 0,
                     as_stream(stream), src, dst, per_img, slots);
  IDN_CHECK_LAUNCH("idn_copy_slots_u8");
  return IDN_OK;
}
