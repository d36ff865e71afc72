// What the host and the device side of the JPEG decoder agree on (jpeg.hip has the map of the
// units): the image and scan descriptors the planner fills and the kernels read, the per-chunk
// counts, and the constants that size the workspace.  No HIP header: the host parser and planner
// (jpeg_host.hpp) compile with a plain C++ compiler, so a stand-alone program can run them under a
// sanitizer (tools/check_jpeg_host.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/idn.h"

#ifdef __HIPCC__
#define JPG_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define JPG_HOST_DEVICE inline
#endif

namespace idn {

#ifndef IDN_JPG_LUTB  // A/B builds set it
#define IDN_JPG_LUTB 9
#endif
constexpr int JPG_LUTB = IDN_JPG_LUTB;  // fast Huffman lookup bits

struct JpegDev {
  uint64_t scan_off;   // entropy-coded bytes in the batch buffer
  uint32_t scan_len;
  int width, height, ncomp, mcux, mcuy, restart;  // restart: MCUs per interval (0: none)
  int hmax, vmax, nintervals;
  int ch[4], cv[4], tq[4], td[4], ta[4];
  int bw[4], bh[4];         // blocks per row / column of each component plane (MCU-padded)
  int sh[4], sv[4];         // IDCT output scale per component: 1 (8 samples) or 2 (16 samples)
  int pw[4];                // component plane row pitch in bytes (bw * 8 * sh)
  int dw[4], dh[4];         // component plane size after the IDCT (libjpeg downsampled_width)
  int up;                   // chroma upsampling: 0 none (full-size planes), 1 h2v1, 2 h2v2 fancy
  int cb_g;                 // jdcolor.c Cb -> G multiplier: libjpeg 9 22553, turbo 22554
  int rgb;                  // jpg_color_space: 0 YCbCr, 1 RGB, 2 CMYK, 3 YCCK
  uint64_t blk_off[4];      // first block of each component in the batch coefficient buffer
  uint64_t pl_off[4];       // component plane byte offset in the batch plane buffer
  uint64_t ub_off;          // unstuffed entropy bytes (workspace), capacity scan_len + 64
  uint32_t iv_off;          // first entry of the image's interval tables (jpeg_unstuff_final)
  uint32_t mk_off, mk_cap;  // the markers found in the segment (jpeg_unstuff_write): first, room
  uint32_t ch_off, nchunks; // the image's chunks in the batch chunk arrays
  uint32_t chunk_bits;
  int bpm;                  // blocks per MCU (1 for a single-component scan)
  uint32_t total_blocks;    // MCUs x bpm
  int wib[4], hib[4];       // blocks with data per component row / column (jdinput.c
                            // width_in_blocks): what a non-interleaved scan codes
  uint32_t scan0, nscan;    // scan path: the image's scans in the batch scan table (0: none)
  int arith;                // arithmetic-coded (the scan path's jpeg_arith_kernel)
  int smooth;               // libjpeg 9d block smoothing (jdcoefct.c decompress_smooth_data)
  int orient;               // the EXIF orientation cv2.imread applies (1: none; jpg_exif_orientation)
  int8_t cbits[4][6];       // its coef_bits latch per component (zigzag 0..5; -1: never coded)
  uint8_t ph_comp[10], ph_dv[10], ph_dh[10];  // block of the MCU -> component, block row, column
  uint16_t q[4][64];        // quantisation tables, natural order
  uint16_t lut[4][1 << JPG_LUTB];  // [DC0, DC1, AC0, AC1]: len << 8 | symbol, 0 = longer code
  int32_t maxcode[4][18];   // libjpeg jdhuff: largest code of each length (-1: none), [17] sentinel
  int32_t valoff[4][18];    // huffval index of the first code of each length, minus that code
  uint8_t huffval[4][256];
};

// one scan of the scan path (progressive / multi-scan files).  Table slots: k = the DC table of
// scan component k, 4 + k = its AC table (only the slots the scan's kind reads are filled).
enum { JPG_SEQ = 0, JPG_DC_FIRST = 1, JPG_DC_REFINE = 2, JPG_AC_FIRST = 3, JPG_AC_REFINE = 4 };
struct JpegScanDev {
  uint64_t scan_off;        // entropy-coded bytes in the batch buffer (unstuffed like JpegDev's)
  uint32_t scan_len;
  uint64_t ub_off;
  uint32_t iv_off;
  uint32_t mk_off, mk_cap;
  int nintervals;
  int img, ns, comp[4], Ss, Se, Ah, Al, restart, kind;
  uint32_t nunits;          // MCUs (interleaved) or the component's blocks (non-interleaved)
  int arith;                // arithmetic-coded: the statistics of tables td / ta per scan component,
  int td[4], ta[4];         // conditioned by aL / aU (DC) and aK (AC); no Huffman tables
  uint8_t aL[4], aU[4], aK[4];
  uint16_t lut[8][1 << JPG_LUTB];
  int32_t maxcode[8][18], valoff[8][18];
  uint8_t huffval[8][256];
};

// bits per sub-chunk of an entropy chunk, one checkpoint each (jpeg_entropy.hip says why 256)
#ifndef IDN_JPG_SUB  // A/B builds set it
#define IDN_JPG_SUB 256
#endif
constexpr uint32_t JPG_SUB = IDN_JPG_SUB;
JPG_HOST_DEVICE uint32_t jpg_nsub(uint32_t chunk_bits) {
  return (chunk_bits + JPG_SUB - 1) / JPG_SUB;
}

// a chunk's (or sub-chunk's) counts: DC symbols, and the sum of the DC differences per component
struct ChunkOut {
  uint32_t nblk;
  int32_t dcsum[3];
};

// unstuffing (jpeg_entropy.hip): 16 KiB tiles of a segment, 1024 threads x 16 bytes
constexpr uint32_t UNS_TILE = 1024 * 16;
constexpr uint32_t JPG_MK_EXTRA = 64;  // marker table room beyond the restart markers
constexpr uint32_t JPG_IV_INHERIT = 0x80000000u;  // interval end flag: see jpeg_unstuff_final
constexpr size_t JPG_MAX_SCAN = ((size_t)1 << 28) - 64;  // bytes: bit positions below the flag

// the kernels index arrays of these in the workspace the planner lays out: the layouts are fixed
static_assert(sizeof(JpegDev) == 6680, "JpegDev layout changed");
static_assert(sizeof(JpegScanDev) == 11536, "JpegScanDev layout changed");
static_assert(sizeof(ChunkOut) == 16, "ChunkOut layout changed");

}  // namespace idn

#undef JPG_HOST_DEVICE
