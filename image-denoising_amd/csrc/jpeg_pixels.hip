// JPEG decoder, coefficients to pixels (jpeg.hip has the map of the units): libjpeg 9d's block
// smoothing, dequantisation and the ISLOW integer IDCT (jidctint.c's 8x8, 16x16 and 16x8 forms,
// restated) into u8 component planes, then chroma upsampling, colour conversion and the EXIF turn
// into the batch output.
// This software is based in part on the work of the Independent JPEG Group.
#include "jpeg_device.hpp"

#include <algorithm>

namespace idn {

// ---- device: ISLOW IDCT (jidctint.c) ------------------------------------------------------------
constexpr int JCB = 13, JP1 = 2;  // CONST_BITS, PASS1_BITS
__device__ __forceinline__ int jpg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// libjpeg's IDCT range limit: the descaled value's low 10 bits as a signed number, + 128, clamped
__device__ __forceinline__ uint32_t jpg_range(int x) {
  const int v = ((x & 1023) ^ 512) - 512;
  return (uint32_t)min(max(v + 128, 0), 255);
}

template <bool ROW>
__device__ __forceinline__ void jpg_idct1(int i0, int i1, int i2, int i3, int i4, int i5, int i6,
                                          int i7, int (&o)[8]) {
  // even part
  int z2 = i2, z3 = i6;
  int z1 = (z2 + z3) * 4433;  // FIX_0_541196100
  int tmp2 = z1 + z3 * -15137;  // FIX_1_847759065
  int tmp3 = z1 + z2 * 6270;    // FIX_0_765366865
  int tmp0 = (i0 + i4) * (1 << JCB);
  int tmp1 = (i0 - i4) * (1 << JCB);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  tmp0 = i7;
  tmp1 = i5;
  tmp2 = i3;
  tmp3 = i1;
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;  // FIX_1_175875602
  tmp0 *= 2446;                     // FIX_0_298631336
  tmp1 *= 16819;                    // FIX_2_053119869
  tmp2 *= 25172;                    // FIX_3_072711026
  tmp3 *= 12299;                    // FIX_1_501321110
  z1 *= -7373;                      // FIX_0_899976223
  z2 *= -20995;                     // FIX_2_562915447
  z3 *= -16069;                     // FIX_1_961570560
  z4 *= -3196;                      // FIX_0_390180644
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr int SH = ROW ? JCB + JP1 + 3 : JCB - JP1;
  o[0] = jpg_descale(tmp10 + tmp3, SH);
  o[7] = jpg_descale(tmp10 - tmp3, SH);
  o[1] = jpg_descale(tmp11 + tmp2, SH);
  o[6] = jpg_descale(tmp11 - tmp2, SH);
  o[2] = jpg_descale(tmp12 + tmp1, SH);
  o[5] = jpg_descale(tmp12 - tmp1, SH);
  o[3] = jpg_descale(tmp13 + tmp0, SH);
  o[4] = jpg_descale(tmp13 - tmp0, SH);
}

// 16-point IDCT kernel of jidctint.c's jpeg_idct_16x16 / jpeg_idct_16x8 (libjpeg 9, cK =
// sqrt(2) cos(K pi / 32)): 8 coefficients -> 16 samples.  Pass 1 (columns) descales by
// CONST_BITS - PASS1_BITS, pass 2 (ROW) by CONST_BITS + PASS1_BITS + 3; libjpeg 9 folds the
// rounding fudge (and the range centre) into the DC term, which equals rounding at the end.
template <bool ROW>
__device__ __forceinline__ void jpg_idct16(const int (&x)[8], int (&o)[16]) {
  // even part
  int tmp0 = x[0] * (1 << JCB);
  int z1 = x[4];
  int tmp1 = z1 * 10703;   // FIX(1.306562965)   c4[16] = c2[8]
  int tmp2 = z1 * 4433;    // FIX_0_541196100    c12[16] = c6[8]
  int tmp10 = tmp0 + tmp1, tmp11 = tmp0 - tmp1, tmp12 = tmp0 + tmp2, tmp13 = tmp0 - tmp2;
  z1 = x[2];
  int z2 = x[6];
  int z3 = z1 - z2;
  int z4 = z3 * 2260;      // FIX(0.275899379)   c14[16] = c7[8]
  z3 = z3 * 11363;         // FIX(1.387039845)   c2[16] = c1[8]
  tmp0 = z3 + z2 * 20995;  // FIX_2_562915447    (c6+c2)[16]
  tmp1 = z4 + z1 * 7373;   // FIX_0_899976223    (c6-c14)[16]
  tmp2 = z3 - z1 * 4926;   // FIX(0.601344887)   (c2-c10)[16]
  int tmp3 = z4 - z2 * 4176;  // FIX(0.509795579) (c10-c14)[16]
  const int tmp20 = tmp10 + tmp0, tmp27 = tmp10 - tmp0;
  const int tmp21 = tmp12 + tmp1, tmp26 = tmp12 - tmp1;
  const int tmp22 = tmp13 + tmp2, tmp25 = tmp13 - tmp2;
  const int tmp23 = tmp11 + tmp3, tmp24 = tmp11 - tmp3;
  // odd part
  z1 = x[1];
  z2 = x[3];
  z3 = x[5];
  z4 = x[7];
  tmp11 = z1 + z3;
  tmp1 = (z1 + z2) * 11086;  // FIX(1.353318001) c3
  tmp2 = tmp11 * 10217;      // FIX(1.247225013) c5
  tmp3 = (z1 + z4) * 8956;   // FIX(1.093201867) c7
  tmp10 = (z1 - z4) * 7350;  // FIX(0.897167586) c9
  tmp11 = tmp11 * 5461;      // FIX(0.666655658) c11
  tmp12 = (z1 - z2) * 3363;  // FIX(0.410524528) c13
  tmp0 = tmp1 + tmp2 + tmp3 - z1 * 18730;     // FIX(2.286341144) c7+c5+c3-c1
  tmp13 = tmp10 + tmp11 + tmp12 - z1 * 15038; // FIX(1.835730603) c9+c11+c13-c15
  z1 = (z2 + z3) * 1136;                      // FIX(0.138617169) c15
  tmp1 += z1 + z2 * 589;                      // FIX(0.071888074) c9+c11-c3-c15
  tmp2 += z1 - z3 * 9222;                     // FIX(1.125726048) c5+c7+c15-c3
  z1 = (z3 - z2) * 11529;                     // FIX(1.407403738) c1
  tmp11 += z1 - z3 * 6278;                    // FIX(0.766367282) c1+c11-c9-c13
  tmp12 += z1 + z2 * 16154;                   // FIX(1.971951411) c1+c5+c13-c7
  z2 += z4;
  z1 = z2 * -5461;                            // -c11
  tmp1 += z1;
  tmp3 += z1 + z4 * 8728;                     // FIX(1.065388962) c3+c11+c15-c7
  z2 = z2 * -10217;                           // -c5
  tmp10 += z2 + z4 * 25733;                   // FIX(3.141271809) c1+c5+c9-c13
  tmp12 += z2;
  z2 = (z3 + z4) * -11086;                    // -c3
  tmp2 += z2;
  tmp3 += z2;
  z2 = (z4 - z3) * 3363;                      // c13
  tmp10 += z2;
  tmp11 += z2;
  constexpr int SH = ROW ? JCB + JP1 + 3 : JCB - JP1;
  o[0] = jpg_descale(tmp20 + tmp0, SH);
  o[15] = jpg_descale(tmp20 - tmp0, SH);
  o[1] = jpg_descale(tmp21 + tmp1, SH);
  o[14] = jpg_descale(tmp21 - tmp1, SH);
  o[2] = jpg_descale(tmp22 + tmp2, SH);
  o[13] = jpg_descale(tmp22 - tmp2, SH);
  o[3] = jpg_descale(tmp23 + tmp3, SH);
  o[12] = jpg_descale(tmp23 - tmp3, SH);
  o[4] = jpg_descale(tmp24 + tmp10, SH);
  o[11] = jpg_descale(tmp24 - tmp10, SH);
  o[5] = jpg_descale(tmp25 + tmp11, SH);
  o[10] = jpg_descale(tmp25 - tmp11, SH);
  o[6] = jpg_descale(tmp26 + tmp12, SH);
  o[9] = jpg_descale(tmp26 - tmp12, SH);
  o[7] = jpg_descale(tmp27 + tmp13, SH);
  o[8] = jpg_descale(tmp27 - tmp13, SH);
}

// libjpeg 9d block smoothing (jdcoefct.c decompress_smooth_data) of block (bx, by) of component
// c, on its dequantised coefficients x: a coefficient among AC01 AC10 AC20 AC11 AC02 whose
// coef_bits latch Al != 0 and whose value is still 0 is estimated from the quantised DC values
// DC1..DC9 of the 3x3 blocks around it (rows above / own / below; edge blocks repeat at the
// image's data edges, width_in_blocks x height_in_blocks):
//   num = mult Q00 term,  pred = ((Qk << 7) + |num|) / (Qk << 8), capped at 2^Al - 1 for Al > 0,
//   signed as num, stored as a 16-bit JCOEF; then dequantised like the coded coefficients.
// The estimates never feed a neighbour (libjpeg smooths a copy of each block).
__device__ __forceinline__ void jpg_smooth(const JpegDev& D, int c, const int16_t* cc, int bx,
                                           int by, const uint16_t* q, int (&x)[64]) {
  const int bw = D.bw[c], xl = D.wib[c] - 1, yl = D.hib[c] - 1;
  const int xs[3] = {max(bx - 1, 0), bx, min(bx + 1, xl)};
  const int ys[3] = {max(by - 1, 0), by, min(by + 1, yl)};
  long long dc[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) dc[3 * r + k] = cc[((size_t)ys[r] * bw + xs[k]) * 64];
  const long long q00 = q[0];
  auto est = [&](int z, int pos, long long num) {
    const int al = D.cbits[c][z];
    if (al == 0 || x[pos] != 0) return;  // q[pos] != 0 (smoothing_ok): x == 0 iff the coefficient is
    const long long qk = q[pos];
    long long pred = ((qk << 7) + (num >= 0 ? num : -num)) / (qk << 8);
    if (al > 0 && pred >= (1ll << al)) pred = (1ll << al) - 1;
    if (num < 0) pred = -pred;
    x[pos] = (int)(int16_t)pred * (int)qk;
  };
  est(1, 1, 36 * q00 * (dc[3] - dc[5]));                      // AC01: DC4 - DC6
  est(2, 8, 36 * q00 * (dc[1] - dc[7]));                      // AC10: DC2 - DC8
  est(3, 16, 9 * q00 * (dc[1] + dc[7] - 2 * dc[4]));          // AC20
  est(4, 9, 5 * q00 * (dc[0] - dc[2] - dc[6] + dc[8]));       // AC11
  est(5, 2, 9 * q00 * (dc[3] + dc[5] - 2 * dc[4]));           // AC02
}

// one thread per coefficient block of components whose IDCT output is (8 SV) x (8 SH) samples;
// blocks of all components of all images in one flat index space (blocks of other scales exit)
template <int SV, int SH>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDev* __restrict__ imgs,
                                                        const uint64_t* __restrict__ blk_end,
                                                        int n, uint64_t nblk,
                                                        const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblk) return;
  int img = 0;  // the image holding block b (blk_end: exclusive prefix ends per image)
  {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (blk_end[mid] > b) hi = mid;
      else lo = mid + 1;
    }
    img = lo;
  }
  const JpegDev& D = imgs[img];
  int c = D.ncomp - 1;
  while (c > 0 && b < D.blk_off[c]) --c;
  if (D.sv[c] != SV || D.sh[c] != SH) return;
  const uint64_t lb = b - D.blk_off[c];
  const int by = (int)(lb / D.bw[c]), bx = (int)(lb - (uint64_t)by * D.bw[c]);
  const uint16_t* q = D.q[D.tq[c]];
  const int16_t* in = coef + b * 64;
  int x[64];
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // 8 x 16-byte loads
    const int4 v = reinterpret_cast<const int4*>(in)[k];
    const int w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[8 * k + 2 * j] = (int)(int16_t)(w4[j] & 0xFFFF) * (int)q[8 * k + 2 * j];
      x[8 * k + 2 * j + 1] = (int)(int16_t)((uint32_t)w4[j] >> 16) * (int)q[8 * k + 2 * j + 1];
    }
  }
  if (D.smooth && bx < D.wib[c] && by < D.hib[c])
    jpg_smooth(D, c, coef + D.blk_off[c] * 64, bx, by, q, x);
  constexpr int R = 8 * SV, C = 8 * SH;  // output rows, columns
  int ws[R * 8];
#pragma unroll
  for (int col = 0; col < 8; ++col) {  // pass 1: columns (the all-zero-AC shortcut is exact)
    if constexpr (SV == 1) {
      int o[8];
      jpg_idct1<false>(x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col],
                       x[48 + col], x[56 + col], o);
#pragma unroll
      for (int r = 0; r < 8; ++r) ws[8 * r + col] = o[r];
    } else {
      const int xi[8] = {x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col],
                         x[48 + col], x[56 + col]};
      int o[16];
      jpg_idct16<false>(xi, o);
#pragma unroll
      for (int r = 0; r < 16; ++r) ws[8 * r + col] = o[r];
    }
  }
  const int pw = D.pw[c];
  uint8_t* out = planes + D.pl_off[c] + (uint64_t)(by * R) * pw + bx * C;
#pragma unroll
  for (int r = 0; r < R; ++r) {  // pass 2: rows
    int o[C];
    if constexpr (SH == 1) {
      jpg_idct1<true>(ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4],
                      ws[8 * r + 5], ws[8 * r + 6], ws[8 * r + 7], o);
    } else {
      const int xi[8] = {ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4],
                         ws[8 * r + 5], ws[8 * r + 6], ws[8 * r + 7]};
      jpg_idct16<true>(xi, o);
    }
    uint32_t wd[C / 4];
#pragma unroll
    for (int j = 0; j < C / 4; ++j)
      wd[j] = jpg_range(o[4 * j]) | jpg_range(o[4 * j + 1]) << 8 | jpg_range(o[4 * j + 2]) << 16 |
              jpg_range(o[4 * j + 3]) << 24;
    uint8_t* orow = out + (uint64_t)r * pw;
    if constexpr (SH == 1) {
      reinterpret_cast<uint2*>(orow)[0] = make_uint2(wd[0], wd[1]);
    } else {
      reinterpret_cast<uint4*>(orow)[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
  }
}

// ---- device: upsampling + colour ---------------------------------------------------------------
__device__ __forceinline__ uint32_t jpg_clamp(int v) { return (uint32_t)min(max(v, 0), 255); }

// 8 consecutive pixels of a row per thread from dword loads: Y 2 dwords, each chroma row 2 dwords
// (full-size planes) or 3 dwords (the samples the 8 outputs' fancy upsampling needs, columns
// x0/2 - 1 .. x0/2 + 4 for turbo's h2 forms); jdsample.c's h2v1 / h2v2 formulas on the extracted
// samples, jdcolor.c's integer tables.
__device__ __forceinline__ uint32_t ld_dw(const uint8_t* __restrict__ row, int col4, int pw) {
  return (col4 >= 0 && col4 < pw) ? *reinterpret_cast<const uint32_t*>(row + col4) : 0u;
}
// the 12 samples of chroma row r at columns cb .. cb + 11 (cb = x0/2 - 4, dword aligned)
struct C12 {
  uint32_t d[3];
  __device__ __forceinline__ int at(int k) const { return (int)((d[k >> 2] >> (8 * (k & 3))) & 0xFFu); }
};
template <int HS, int VS>  // chroma subsampling factors (1 or 2)
__device__ __forceinline__ void jpg_chroma8(const uint8_t* __restrict__ P, int pw, int dw, int dh,
                                            int x0, int y, int (&out)[8]) {
  if constexpr (HS == 1) {  // 4:4:4
    const uint8_t* r = P + (int64_t)y * pw;
    const uint32_t a = ld_dw(r, x0, pw), b = ld_dw(r, x0 + 4, pw);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = (int)(((k < 4 ? a : b) >> (8 * (k & 3))) & 0xFFu);
    return;
  }
  const int cb = x0 / 2 - 4;  // x0 % 8 == 0: dword aligned
  const int inrow = VS == 2 ? y >> 1 : y;
  C12 r0, r1;
  const uint8_t* p0 = P + (int64_t)inrow * pw;
#pragma unroll
  for (int j = 0; j < 3; ++j) r0.d[j] = ld_dw(p0, cb + 4 * j, pw);
  if constexpr (VS == 2) {
    const int other = min(max((y & 1) ? inrow + 1 : inrow - 1, 0), dh - 1);
    const uint8_t* p1 = P + (int64_t)other * pw;
#pragma unroll
    for (int j = 0; j < 3; ++j) r1.d[j] = ld_dw(p1, cb + 4 * j, pw);
  }
  // column sum of sample k (k = col - cb): h2v1 the sample, h2v2 3 * nearer + further row
  auto cs = [&](int k) { return VS == 2 ? r0.at(k) * 3 + r1.at(k) : r0.at(k); };
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int col = x0 / 2 + (i >> 1), k = 4 + (i >> 1);
    const int t = cs(k);
    if constexpr (VS == 2) {
      if ((i & 1) == 0) out[i] = col == 0 ? (t * 4 + 8) >> 4 : (t * 3 + cs(k - 1) + 8) >> 4;
      else out[i] = col == dw - 1 ? (t * 4 + 7) >> 4 : (t * 3 + cs(k + 1) + 7) >> 4;
    } else {
      if ((i & 1) == 0) out[i] = col == 0 ? t : (t * 3 + cs(k - 1) + 1) >> 2;
      else out[i] = col == dw - 1 ? t : (t * 3 + cs(k + 1) + 2) >> 2;
    }
  }
}

template <int HS, int VS, bool GRAY>
__device__ __forceinline__ void jpg_color8(const JpegDev& D, const uint8_t* __restrict__ planes,
                                           int x0, int y, uint32_t (&o)[6]) {
  const int pw0 = D.pw[0];
  const uint8_t* yr = planes + D.pl_off[0] + (int64_t)y * pw0;
  const uint32_t ya = ld_dw(yr, x0, pw0), yb = ld_dw(yr, x0 + 4, pw0);
  int cbv[8], crv[8];
  if constexpr (!GRAY) {
    jpg_chroma8<HS, VS>(planes + D.pl_off[1], D.pw[1], D.dw[1], D.dh[1], x0, y, cbv);
    jpg_chroma8<HS, VS>(planes + D.pl_off[2], D.pw[2], D.dw[2], D.dh[2], x0, y, crv);
  }
  uint32_t px[24];
  const int cbg = D.cb_g;  // jdcolor.c build_ycc_rgb_table (SCALEBITS 16)
  uint32_t ka = 0, kb = 0;  // a fourth component (K), sampled as the first
  if (!GRAY && D.ncomp == 4) {
    const int pw3 = D.pw[3];
    const uint8_t* kr = planes + D.pl_off[3] + (int64_t)y * pw3;
    ka = ld_dw(kr, x0, pw3);
    kb = ld_dw(kr, x0 + 4, pw3);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int Y = (int)(((i < 4 ? ya : yb) >> (8 * (i & 3))) & 0xFFu);
    if constexpr (GRAY) {
      px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint32_t)Y;
    } else if (D.rgb == 1) {  // jdcolor.c rgb_convert: a copy (components R, G, B -> BGR)
      px[3 * i + 0] = (uint32_t)crv[i];
      px[3 * i + 1] = (uint32_t)cbv[i];
      px[3 * i + 2] = (uint32_t)Y;
    } else if (D.rgb >= 2) {
      // libjpeg's CMYK output: the components as stored (CMYK), or jdcolor.c ycck_cmyk_convert
      // (YCCK: 255 minus the YCbCr -> RGB conversion, K unchanged); then OpenCV's
      // icvCvt_CMYK2BGR_8u_C4C3R (grfmt_jpeg.cpp: Adobe-inverted CMYK), c' = k - ((255 - c) k >> 8)
      int c0 = Y, c1 = cbv[i], c2 = crv[i];
      if (D.rgb == 3) {
        const int xb = cbv[i] - 128, xr = crv[i] - 128;
        c0 = 255 - (int)jpg_clamp(Y + ((91881 * xr + 32768) >> 16));
        c1 = 255 - (int)jpg_clamp(Y + ((-46802 * xr + (-cbg * xb + 32768)) >> 16));
        c2 = 255 - (int)jpg_clamp(Y + ((116130 * xb + 32768) >> 16));
      }
      const int k = (int)(((i < 4 ? ka : kb) >> (8 * (i & 3))) & 0xFFu);
      px[3 * i + 0] = (uint32_t)(k - (((255 - c2) * k) >> 8));
      px[3 * i + 1] = (uint32_t)(k - (((255 - c1) * k) >> 8));
      px[3 * i + 2] = (uint32_t)(k - (((255 - c0) * k) >> 8));
    } else {
      const int xb = cbv[i] - 128, xr = crv[i] - 128;
      px[3 * i + 0] = jpg_clamp(Y + ((116130 * xb + 32768) >> 16));                  // FIX(1.772)
      px[3 * i + 1] = jpg_clamp(Y + ((-46802 * xr + (-cbg * xb + 32768)) >> 16));  // FIX(0.714136286)
      px[3 * i + 2] = jpg_clamp(Y + ((91881 * xr + 32768) >> 16));                   // FIX(1.402)
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j)
    o[j] = px[4 * j] | px[4 * j + 1] << 8 | px[4 * j + 2] << 16 | px[4 * j + 3] << 24;
}

// grid (tiles of 256 x 8 decoded pixels, n); (h, w) is the batch's output size, which is the
// decoded size turned by each image's EXIF orientation (D.orient, OpenCV 3.4.2 loadsave.cpp
// ApplyExifOrientation: 2 flip(1), 3 flip(-1), 4 flip(0), 5 transpose, 6 transpose + flip(1),
// 7 transpose + flip(-1), 8 transpose + flip(0)).  Decoded pixel (y, x) of an H x W image goes to
// the output position below; orientation 1 keeps the coalesced 24-byte row stores
__global__ __launch_bounds__(256) void jpeg_color8_kernel(const JpegDev* __restrict__ imgs,
                                                          const uint8_t* __restrict__ planes,
                                                          uint8_t* __restrict__ dst, int h, int w,
                                                          int64_t row_stride) {
  const JpegDev& D = imgs[blockIdx.y];
  const int H = D.height, W = D.width;  // as decoded
  const int ow = (W + 7) / 8;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)H * ow) return;
  const int y = (int)(q / ow), x0 = 8 * (int)(q - (int64_t)y * ow);
  uint32_t o[6];
  if (D.ncomp == 1) jpg_color8<1, 1, true>(D, planes, x0, y, o);
  else if (D.up == 0) jpg_color8<1, 1, false>(D, planes, x0, y, o);
  else if (D.up == 1) jpg_color8<2, 1, false>(D, planes, x0, y, o);
  else jpg_color8<2, 2, false>(D, planes, x0, y, o);
  uint8_t* const img = dst + (int64_t)blockIdx.y * h * row_stride;
  if (D.orient > 1) {
    const int t = D.orient;
    for (int k = 0; k < 8 && x0 + k < W; ++k) {
      const int x = x0 + k;
      int oy, ox;
      if (t <= 4) {
        oy = (t == 3 || t == 4) ? H - 1 - y : y;
        ox = (t == 2 || t == 3) ? W - 1 - x : x;
      } else {  // transposed: (x, y), then the flip of the W x H result
        oy = (t == 7 || t == 8) ? W - 1 - x : x;
        ox = (t == 6 || t == 7) ? H - 1 - y : y;
      }
      uint8_t* p = img + (int64_t)oy * row_stride + (int64_t)ox * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * k + c;
        p[c] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
      }
    }
    return;
  }
  uint8_t* p = img + (int64_t)y * row_stride + (int64_t)x0 * 3;
  if (x0 + 8 <= w && ((uintptr_t)p & 7) == 0) {
    uint2* p2 = reinterpret_cast<uint2*>(p);
    p2[0] = make_uint2(o[0], o[1]);
    p2[1] = make_uint2(o[2], o[3]);
    p2[2] = make_uint2(o[4], o[5]);
  } else if (x0 + 8 <= w && ((uintptr_t)p & 3) == 0) {
    uint32_t* p4 = reinterpret_cast<uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 6; ++j) p4[j] = o[j];
  } else {
    for (int k = 0; k < 24 && x0 + k / 3 < w; ++k) p[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
  }
}

// ---- launchers -------------------------------------------------------------------------------------
void jpeg_idct(const JpegCall& C, int sv, int sh, unsigned grid, uint64_t nblk) {
  // the scales the planner makes: 8x8, 8x16 (libjpeg 9's 4:2:2 chroma), 16x16 (its 4:2:0 chroma)
  auto* k = sv == 1 && sh == 1 ? jpeg_idct_kernel<1, 1>
            : sv == 1          ? jpeg_idct_kernel<1, 2>
                               : jpeg_idct_kernel<2, 2>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, C.st, C.imgs, C.blk_end, C.n, nblk, C.coef,
                     C.planes);
}

void jpeg_color8(const JpegCall& C, uint8_t* dst, int h, int w, int64_t row_stride) {
  // decoded 8-pixel groups per image: h x ceil(w / 8), or w x ceil(h / 8) for a transposed one
  const int64_t groups = std::max((int64_t)h * ((w + 7) / 8), (int64_t)w * ((h + 7) / 8));
  const int64_t gx = (groups + 255) / 256;
  hipLaunchKernelGGL(jpeg_color8_kernel, dim3((unsigned)gx, (unsigned)C.n), dim3(256), 0, C.st,
                     C.imgs, C.planes, dst, h, w, row_stride);
}

}  // namespace idn
