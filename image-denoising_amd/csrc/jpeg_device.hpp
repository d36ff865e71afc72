// What the device units of the JPEG decoder share (jpeg.hip has the map of the units): the zigzag
// table, the __device__ __forceinline__ Huffman helpers that both entropy units use, one call's
// workspace regions (JpegCall), and at the end the declarations of the host launchers through which
// jpeg.hip reaches the kernels of the other units.
#pragma once
#include "idn_common.hpp"

#include "jpeg_desc.hpp"

namespace idn {

// jpeg_natural_order: zigzag index -> natural (row-major) index.  The units are linked without
// relocatable device code, so each has its own copy; every kernel only copies it into LDS
static __constant__ uint8_t jpg_natural[64 + 16] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
    63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};  // overrun guard (libjpeg)

__device__ __forceinline__ int jpg_extend(uint32_t v, int s) {  // HUFF_EXTEND
  return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v;
}

// entry i of mca (see JpegLds) from a table's maxcode[18]: the codes longer than the fast table,
// lengths 10 .. 16, so the table must be exactly 9 bits
static_assert(JPG_LUTB == 9, "jpg_mca and jpg_decode's compare-count assume 9-bit fast tables");
__device__ __forceinline__ int32_t jpg_mca(const int32_t* __restrict__ maxcode, int i) {
  int32_t m = -1;
  for (int l = 10; l <= 10 + i && l <= 16; ++l)
    if (maxcode[l] >= 0) m = maxcode[l] << (16 - l) | ((1 << (16 - l)) - 1);
  return i == 7 ? 0x7FFFFFFF : m;
}

// one Huffman symbol (nb >= 32 on entry); returns the symbol and its code length in *len.  A bit
// pattern that is no code: symbol 0, badlen bits, *bad set (see jpeg_write_kernel on badlen)
template <typename TT>
__device__ __forceinline__ int jpg_decode(uint64_t acc, const TT& T, int t, int* len,
                                          int badlen = 17, bool* bad = nullptr) {
  const uint32_t e = T.lut[t][acc >> (64 - JPG_LUTB)];
  if (e) {
    *len = (int)(e >> 8);
    return e & 0xFF;
  }
  const int32_t c16 = (int32_t)(acc >> 48);
  const int4 m0 = *reinterpret_cast<const int4*>(&T.mca[t][0]);
  const int4 m1 = *reinterpret_cast<const int4*>(&T.mca[t][4]);
  const int l = 10 + (c16 > m0.x) + (c16 > m0.y) + (c16 > m0.z) + (c16 > m0.w) + (c16 > m1.x) +
                (c16 > m1.y) + (c16 > m1.z);
  if (l > 16) {  // not a code (a speculative trajectory or a corrupt file): jdhuff.c
    *len = badlen;  // jpeg_huff_decode reads up to length 17, then JWRN_HUFF_BAD_CODE, symbol 0
    if (bad) *bad = true;
    return 0;
  }
  *len = l;
  return T.huffval[t][(T.valoff[t][l] + (c16 >> (16 - l))) & 0xFF];
}

// one call's stream, batch size and workspace regions (device pointers; JpegPlan's off_*)
struct JpegCall {
  hipStream_t st;
  int n;
  const JpegDev* imgs;
  const uint64_t* blk_end;
  const JpegScanDev* scans;
  const uint8_t* scan;  // the entropy-coded segments as staged
  int16_t* coef;
  uint8_t* planes;
  uint8_t* ub;
  uint32_t *ivs, *ive;
  uint2* mk;
  uint32_t *ublen, *ublen_s;
  uint64_t* S[2];
  ChunkOut *cnt, *start;
  uint32_t* flag;
  uint8_t* chg[2];
  uint64_t* ck_st;
  ChunkOut* ck_co;
  uint2* tcnt;
  uint32_t *ck_iv, *iv_ck;
};

// ---- the seams: the launchers jpeg.hip calls, each defined beside its kernels -------------------
// jpeg_entropy.hip: unstuffing of the images' segments (mt: most tiles of one) or of the scan
// path's ns scans, each count / write / final; overflow: see jpeg_unstuff_final
void jpeg_unstuff_images(const JpegCall& C, int mt, uint32_t* overflow);
void jpeg_unstuff_scans(const JpegCall& C, unsigned ns, int mt, uint32_t* overflow);
// ... and the parallel path.  max_items: most chunks of an image (max_items_w: times sub-chunks).
// jpeg_sync_b reads the states S[cur] and writes S[cur ^ 1] (chg alike); changed, all, settled and
// badlen: see jpeg_sync_kernel and jpeg_write_kernel
void jpeg_chunk_map(const JpegCall& C);
void jpeg_sync_a(const JpegCall& C, uint32_t max_items, int badlen);
void jpeg_sync_b(const JpegCall& C, uint32_t max_items, int cur, uint32_t* changed, int all,
                 const uint32_t* settled, int badlen);
void jpeg_prefix(const JpegCall& C);
void jpeg_write(const JpegCall& C, uint32_t max_items_w, int badlen, uint32_t* badseen);
// jpeg_scan.hip: the scan path's Huffman and arithmetic-coded images
void jpeg_prog(const JpegCall& C);
void jpeg_arith(const JpegCall& C);
// jpeg_pixels.hip: the IDCT of the blocks whose output is (8 sv) x (8 sh) samples, grid blocks of
// 256 threads over all nblk blocks; then colour into the h x w batch output
void jpeg_idct(const JpegCall& C, int sv, int sh, unsigned grid, uint64_t nblk);
void jpeg_color8(const JpegCall& C, uint8_t* dst, int h, int w, int64_t row_stride);

}  // namespace idn
