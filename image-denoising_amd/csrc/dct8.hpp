// The orthonormal 8-point DCT-II and its inverse in fp32, by the even/odd split: Cm[u][i] =
// DCT_Ck[u (2i+1) mod 32] up to sign with c_k = cos(k pi / 16) / 2, and Cm[u][7-i] = (-1)^u Cm[u][i],
// so the even rows work on the sums x_i + x_(7-i) and the odd rows on the differences.
//
// The two rows whose every tap is +-c4 (u = 0 and u = 4) are carried without that factor:
// dct8_fwd returns X0' = X0 / c4 and X4' = X4 / c4, and dct8_inv takes them in that form and
// multiplies by c4^2 = 1/8, an exact scaling.  The DC path of an integer patch therefore has no
// rounding at all (sums of bytes, then powers of two), where the matrix form would round the
// largest coefficient of the patch four times.  A caller that compares such a coefficient with a
// threshold scales the threshold instead (DCT_INV_C4 per direction).
#pragma once

namespace idn {

constexpr float DCT_C1 = 0.49039264020161522f;
constexpr float DCT_C2 = 0.46193976625564337f;
constexpr float DCT_C3 = 0.41573480615127262f;
constexpr float DCT_C5 = 0.27778511650980114f;
constexpr float DCT_C6 = 0.19134171618254492f;
constexpr float DCT_C7 = 0.09754516100806417f;
constexpr float DCT_INV_C4 = 2.8284271247461903f;  // 1 / c4 = 2 sqrt 2

#if defined(__HIPCC__)
#define IDN_DCT_FN __host__ __device__ __forceinline__
#else
#define IDN_DCT_FN inline
#endif

// 34 operations.  X[0] and X[4] come back without their factor c4
IDN_DCT_FN void dct8_fwd(const float (&x)[8], float (&X)[8]) {
  const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
  const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
  const float a0 = s0 + s3, a1 = s1 + s2, b0 = s0 - s3, b1 = s1 - s2;
  X[0] = a0 + a1;
  X[4] = a0 - a1;
  X[2] = __builtin_fmaf(DCT_C6, b1, DCT_C2 * b0);
  X[6] = __builtin_fmaf(-DCT_C2, b1, DCT_C6 * b0);
  X[1] = __builtin_fmaf(DCT_C7, d3, __builtin_fmaf(DCT_C5, d2, __builtin_fmaf(DCT_C3, d1, DCT_C1 * d0)));
  X[3] = __builtin_fmaf(-DCT_C5, d3, __builtin_fmaf(-DCT_C1, d2, __builtin_fmaf(-DCT_C7, d1, DCT_C3 * d0)));
  X[5] = __builtin_fmaf(DCT_C3, d3, __builtin_fmaf(DCT_C7, d2, __builtin_fmaf(-DCT_C1, d1, DCT_C5 * d0)));
  X[7] = __builtin_fmaf(-DCT_C1, d3, __builtin_fmaf(DCT_C3, d2, __builtin_fmaf(-DCT_C5, d1, DCT_C7 * d0)));
}

// 35 operations.  X[0] and X[4] are taken without their factor c4 (as dct8_fwd leaves them)
IDN_DCT_FN void dct8_inv(const float (&X)[8], float (&x)[8]) {
  const float t0 = 0.125f * X[0];
  const float a = __builtin_fmaf(0.125f, X[4], t0), b = __builtin_fmaf(-0.125f, X[4], t0);
  const float p = __builtin_fmaf(DCT_C6, X[6], DCT_C2 * X[2]);
  const float q = __builtin_fmaf(-DCT_C2, X[6], DCT_C6 * X[2]);
  const float e0 = a + p, e1 = b + q, e2 = b - q, e3 = a - p;
  const float o0 = __builtin_fmaf(DCT_C7, X[7], __builtin_fmaf(DCT_C5, X[5], __builtin_fmaf(DCT_C3, X[3], DCT_C1 * X[1])));
  const float o1 = __builtin_fmaf(-DCT_C5, X[7], __builtin_fmaf(-DCT_C1, X[5], __builtin_fmaf(-DCT_C7, X[3], DCT_C3 * X[1])));
  const float o2 = __builtin_fmaf(DCT_C3, X[7], __builtin_fmaf(DCT_C7, X[5], __builtin_fmaf(-DCT_C1, X[3], DCT_C5 * X[1])));
  const float o3 = __builtin_fmaf(-DCT_C1, X[7], __builtin_fmaf(DCT_C3, X[5], __builtin_fmaf(-DCT_C5, X[3], DCT_C7 * X[1])));
  x[0] = e0 + o0;
  x[7] = e0 - o0;
  x[1] = e1 + o1;
  x[6] = e1 - o1;
  x[2] = e2 + o2;
  x[5] = e2 - o2;
  x[3] = e3 + o3;
  x[4] = e3 - o3;
}

}  // namespace idn
