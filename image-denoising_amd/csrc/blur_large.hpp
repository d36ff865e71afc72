// blur_large_u8.hip for the stencil entry points (host): the wide smoothers and the Q8 Gaussian taps
#pragma once
#include "idn_common.hpp"

namespace idn {
int gaussian_taps(int ksize, double sigma, uint16_t* taps, const char* name);
int launch_box_large(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                     int64_t row_stride, int k, hipStream_t s, const char* name);
int launch_gauss_large(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                       int64_t row_stride, int ksize, const uint16_t* taps, hipStream_t s,
                       const char* name);
}  // namespace idn
