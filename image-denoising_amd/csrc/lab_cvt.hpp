// 8-bit BGR <-> Lab for one pixel: OpenCV 3.4.2's integer paths (RGB2Lab_b, Lab2RGBinteger) with
// the tables of lab_tables.hpp.  Shared by quant.hip (the sRGB flavour, COLOR_BGR2LAB /
// COLOR_LAB2BGR) and nlmeans.hip (the linear flavour, COLOR_LBGR2Lab / COLOR_Lab2LBGR, which
// fastNlMeansDenoisingColored converts with).  LINEAR replaces the two gamma tables by
// initLabTabs()'s linear ones, which need no storage: linearGammaTab_b[i] = i << 3 on the way in,
// linearInvGammaTab_b[v] = (255 * v) >> 12 on the way out.  Everything else (coefficients, cbrt
// table, descaling, clipping) is common.  oracle/cvlab.py and tests/nlm_colored_model.py are the
// test restatements; parity vs cv2 is unpinned (no cv2 where this is built).
#pragma once
#include "idn_common.hpp"
#include "lab_tables.hpp"

namespace idn {

// RGB2Lab_b::operator() for one BGR pixel with the gamma / cbrt tables at gt / ct (gt is not read
// when LINEAR) -> packed L | a << 8 | b << 16
template <bool LINEAR = false>
__device__ __forceinline__ uint32_t lab_from_bgr(uint32_t b, uint32_t g, uint32_t r,
                                                 const uint16_t* gt, const uint16_t* ct) {
  const int B = LINEAR ? (int)(b << 3) : (int)gt[b];
  const int G = LINEAR ? (int)(g << 3) : (int)gt[g];
  const int R = LINEAR ? (int)(r << 3) : (int)gt[r];
  const int fX = ct[(B * LAB_C_FWD[0] + G * LAB_C_FWD[1] + R * LAB_C_FWD[2] + (1 << 11)) >> 12];
  const int fY = ct[(B * LAB_C_FWD[3] + G * LAB_C_FWD[4] + R * LAB_C_FWD[5] + (1 << 11)) >> 12];
  const int fZ = ct[(B * LAB_C_FWD[6] + G * LAB_C_FWD[7] + R * LAB_C_FWD[8] + (1 << 11)) >> 12];
  constexpr int Lscale = (116 * 255 + 50) / 100;
  constexpr int Lshift = -((16 * 255 * (1 << 15) + 50) / 100);
  const int L = (Lscale * fY + Lshift + (1 << 14)) >> 15;
  const int A = (500 * (fX - fY) + 128 * (1 << 15) + (1 << 14)) >> 15;
  const int Bb = (200 * (fY - fZ) + 128 * (1 << 15) + (1 << 14)) >> 15;
  return (uint32_t)clampi(L, 0, 255) | (uint32_t)clampi(A, 0, 255) << 8 |
         (uint32_t)clampi(Bb, 0, 255) << 16;
}

// abToXZ_b[v - minABvalue] (integer formula of initLabTabs)
__device__ __forceinline__ int lab_ab_to_xz(int v) {
  if (v <= 3390) return v * 108 / 841 - (1 << 14) * 16 / 116 * 108 / 841;
  return v * v / (1 << 14) * v / (1 << 14);
}

// Lab2RGBinteger::process for one 8-bit Lab colour -> packed B | G << 8 | R << 16; yf: LabToYF_b
// (LAB_YF_B or a copy of it in LDS)
template <bool LINEAR = false>
__device__ uint32_t bgr_from_lab(uint32_t L, uint32_t A, uint32_t Bb,
                                 const uint16_t* yf = LAB_YF_B) {
  const int y = yf[2 * L], ify = yf[2 * L + 1];
  constexpr int BASE = 1 << 14;
  const int adiv = (int)A * BASE / 500 - 128 * BASE / 500;
  const int bdiv = (int)Bb * BASE / 200 - 128 * BASE / 200;
  const int x = lab_ab_to_xz(ify + adiv), z = lab_ab_to_xz(ify - bdiv);
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {  // output B, G, R = rows 2, 1, 0 of XYZ -> sRGB
    const int row = 2 - ch;
    int v = (LAB_C_INV[row * 3] * x + LAB_C_INV[row * 3 + 1] * y + LAB_C_INV[row * 3 + 2] * z +
             (1 << 13)) >> 14;
    v = clampi(v, 0, 4095);
    if constexpr (LINEAR) out |= (uint32_t)((255 * v) >> 12) << (8 * ch);
    else out |= (uint32_t)min((int)LAB_INV_GAMMA_B[v], 255) << (8 * ch);
  }
  return out;
}

__device__ __forceinline__ void stage_lab_tables(uint16_t* gt, uint16_t* ct) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) gt[i] = LAB_GAMMA_B[i];
  for (int i = threadIdx.x; i < 3072; i += blockDim.x) ct[i] = LAB_CBRT_B[i];
}

}  // namespace idn
