// The host third of the JPEG decoder (jpeg.hip has the map of the units): the marker parser, the
// restatement of OpenCV's EXIF walk, the Huffman table builder, the colour-space rule and the batch
// planner.  This is the code that reads untrusted bytes -- file contents, length fields, EXIF
// offsets, Huffman specs -- and its plan decides what the staging copy reads out of the caller's
// files.  It calls no HIP function and includes no HIP header, so tools/check_jpeg_host.cpp runs it
// over the fixtures, truncated and mutated, under AddressSanitizer (tests/test_jpeg_host.py).
#pragma once

#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "abi_args.hpp"
#include "jpeg_desc.hpp"

namespace idn {

// jpeg_natural_order (zigzag index -> natural index) for the parser's DQT; the kernels have their
// own copy with libjpeg's overrun guard (jpeg_device.hpp)
static const uint8_t jpg_natural_host[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- host: marker parser ---------------------------------------------------------------------
struct HuffSpec {
  bool present = false;
  uint8_t bits[17] = {};
  uint8_t val[256] = {};
};
// one scan of a progressive / multi-scan file: its components (frame indices), their tables as
// defined when the scan starts, spectral band and successive-approximation bits, restart interval
struct ScanHost {
  int ns = 0, comp[4] = {}, Ss = 0, Se = 63, Ah = 0, Al = 0, restart = 0;
  HuffSpec dc[4], ac[4];  // per scan component
  int td[4] = {}, ta[4] = {};                   // its table numbers
  uint8_t aL[4] = {}, aU[4] = {}, aK[4] = {};  // arithmetic conditioning of those tables (DAC)
  size_t begin = 0, end = 0;
};
struct JpegHost {
  int width = 0, height = 0, ncomp = 0, restart = 0;
  int cid[4] = {}, ch[4] = {}, cv[4] = {}, tq[4] = {}, td[4] = {}, ta[4] = {};
  bool qpresent[4] = {};
  uint16_t q[4][64] = {};  // natural order
  HuffSpec dc[4], ac[4];
  size_t scan_begin = 0, scan_end = 0;
  bool arith = false;       // arithmetic-coded frame (SOF9 / SOF10)
  // arithmetic conditioning per table (DAC; jdmarker.c get_soi's defaults L 0, U 1, K 5)
  uint8_t dacL[16] = {}, dacU[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
          dacK[16] = {5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5};
  bool jfif = false, adobe = false;  // APP0 "JFIF" / APP14 "Adobe" seen (jdmarker.c examine_app0/14)
  int adobe_transform = 0;
  bool progressive = false;
  bool smooth = false;      // libjpeg 9d block-smooths the file (jpg_scans_done)
  int8_t cbits[4][6] = {};  // its coef_bits latch: per component, zigzag 0..5 (-1: never coded)
  std::vector<ScanHost> scans;  // the scan path (progressive or multi-scan); empty: one scan
};

// end of the entropy-coded segment starting at p[i]: the first marker that is neither RSTn nor
// below SOF0 (stuffed 0xFF00 and fill bytes skipped).  A stray marker below SOF0 stays inside: it
// ends the data of its restart interval (jpeg_unstuff_final), as jdmarker.c's resync reads it.
inline size_t jpg_segment_end(const uint8_t* p, size_t n, size_t i) {
  while (i + 1 < n) {
    if (p[i] != 0xFF) {
      ++i;
      continue;
    }
    const uint8_t nb = p[i + 1];
    if (nb < 0xC0 || (nb >= 0xD0 && nb <= 0xD7)) i += 2;  // (0x00: stuffing)
    else if (nb == 0xFF) i += 1;
    else return i;
  }
  return n;
}

inline int jpg_fail(std::string* err, const char* msg) {
  if (err) *err = msg;
  return IDN_EUNSUPPORTED;
}

// ---- host: the EXIF orientation cv2.imread applies ----------------------------------------------
// OpenCV 3.4.2's imread (loadsave.cpp) calls ApplyExifOrientation on the decoded image unless
// IMREAD_IGNORE_ORIENTATION is set; the tag comes from exif.cpp's ExifReader, which walks the
// file's markers two bytes at a time (the 0xFF is not checked) and takes the FIRST APP1 segment
// as EXIF data whatever its identifier.  Restated from the published OpenCV source [recalled: cv2
// is not importable here], including when it gives up (orientation 1, the image as decoded):
//   - the walk skips (by their length field) SOF0, SOF2, DHT, DQT, DRI, SOS, RST0-7, APP0,
//     APP2-15, COM; SOI / EOI have no length; any other code ends the search (no EXIF);
//   - a length below 2, or an APP1 length <= 6, is a parse error (no EXIF); the APP1 data is
//     the length - 6 bytes after the 6-byte identifier slot (zero-filled past the end of file);
//   - the TIFF header: "II" little-endian, "MM" or any other equal pair big-endian, unequal
//     bytes big-endian too; u16 at 2 must be 42, else no entries; IFD0 at the u32 at 4;
//   - every IFD0 entry is parsed, and the tags exif.cpp knows read their values: an offset past
//     the data (getU16 / getU32 bounds, getString's size check) aborts the whole parse, so a
//     broken MAKE string after a good Orientation still leaves the image unrotated; the first
//     entry of a tag wins (std::map insert); Orientation = the u16 at entry + 8.
// 32-bit offset arithmetic wraps as exif.cpp's uint32_t does.
struct CvExifReader {
  const uint8_t* d;
  size_t n;
  bool intel = false, bad = false;
  uint32_t u16(size_t o) {
    if (o + 1 >= n) {
      bad = true;
      return 0;
    }
    return intel ? (uint32_t)d[o] | (uint32_t)d[o + 1] << 8 : (uint32_t)d[o] << 8 | d[o + 1];
  }
  uint32_t u32(size_t o) {
    if (o + 3 >= n) {
      bad = true;
      return 0;
    }
    return intel ? (uint32_t)d[o] | (uint32_t)d[o + 1] << 8 | (uint32_t)d[o + 2] << 16 |
                       (uint32_t)d[o + 3] << 24
                 : (uint32_t)d[o] << 24 | (uint32_t)d[o + 1] << 16 | (uint32_t)d[o + 2] << 8 |
                       d[o + 3];
  }
  void rationals(size_t entry, int count) {  // getResolution / WhitePoint / ... / RefBW
    uint32_t r = u32(entry + 8);
    for (int k = 0; k < count && !bad; ++k, r += 8) {
      (void)u32(r);
      (void)u32((uint32_t)(r + 4));
    }
  }
  void string(size_t entry) {  // getString: the size check only
    const uint32_t size = u32(entry + 4);
    uint32_t off = 8;
    if (!bad && size > 4) off = u32(entry + 8);
    if (!bad && (off > n || (uint32_t)(off + size) > n)) bad = true;
  }
};

// the orientation (1..8 acts, anything else is left as decoded) OpenCV 3.4.2 applies to file p
inline int jpg_exif_orientation(const uint8_t* p, size_t n) {
  size_t i = 0;
  std::vector<uint8_t> data;
  bool found = false;
  while (!found) {
    if (i + 2 > n) break;  // (a short read ends the search)
    const uint8_t m = p[i + 1];
    i += 2;
    auto field = [&]() -> size_t {  // getFieldSize: 0 on a short read
      if (i + 2 > n) {
        i = n;
        return 0;
      }
      const size_t v = (size_t)p[i] << 8 | p[i + 1];
      i += 2;
      return v;
    };
    if (m == 0xC0 || m == 0xC2 || m == 0xC4 || m == 0xDB || m == 0xDD || m == 0xDA ||
        (m >= 0xD0 && m <= 0xD7) || m == 0xE0 || (m >= 0xE2 && m <= 0xEF) || m == 0xFE) {
      const size_t skip = field();
      if (skip < 2) return 1;
      i += skip - 2;
    } else if (m == 0xD8 || m == 0xD9) {
    } else if (m == 0xE1) {
      const size_t len = field();
      if (len <= 6) return 1;
      data.assign(len - 6, 0);
      i += 6;
      if (i < n) memcpy(data.data(), p + i, std::min(len - 6, n - i));
      found = true;
    } else {
      break;
    }
  }
  if (!found) return 1;
  CvExifReader R{data.data(), data.size()};
  // getFormat: unequal first bytes -> NONE (read big-endian), 'I' Intel, 'M' or other -> big-endian
  R.intel = !(data.size() > 1 && data[0] != data[1]) && data[0] == 'I';
  if (R.u16(2) != 0x2A || R.bad) return 1;  // checkTagMark (a short block throws)
  uint32_t off = R.u32(4);
  const uint32_t nent = R.u16(off);
  if (R.bad) return 1;
  off += 2;
  int orient = -1;
  for (uint32_t e = 0; e < nent; ++e, off += 12) {
    const uint32_t tag = R.u16(off);
    switch (tag) {
      case 0x010E: case 0x010F: case 0x0110: case 0x0131: case 0x0132: case 0x8298:
        R.string(off);
        break;  // description, make, model, software, date-time, copyright
      case 0x0112: {
        const uint32_t v = R.u16((size_t)off + 8);
        if (orient < 0) orient = (int)v;
        break;
      }
      case 0x011A: case 0x011B: R.rationals(off, 1); break;  // x / y resolution
      case 0x0128: case 0x0213: (void)R.u16((size_t)off + 8); break;
      case 0x013E: R.rationals(off, 2); break;   // white point
      case 0x013F: R.rationals(off, 6); break;   // primary chromaticities
      case 0x0211: R.rationals(off, 3); break;   // YCbCr coefficients
      case 0x0214: R.rationals(off, 6); break;   // reference black / white
      default: break;                            // EXIF_OFFSET and unknown tags: no value read
    }
    if (R.bad) return 1;
  }
  return orient >= 1 && orient <= 8 ? orient : 1;
}

// the end of a scan-path file (EOI or end of data): at least one scan.  libjpeg block-smooths a
// progressive file (jdcoefct.c smoothing_ok, libjpeg 9d) only when EVERY component has DC data
// (coef_bits[0] >= 0: jdphuff.c sets coef_bits[k] = Al for k in Ss..Se at each scan's start) and
// nonzero quantisers Q00 Q01 Q10 Q20 Q11 Q02, and some component's AC coefficients 1..5 stay
// imprecise after the last scan (coef_bits != 0): J.smooth and the latched coef_bits, applied by
// the IDCT pass (jpg_smooth)
inline int jpg_scans_done(JpegHost& J, std::string* err) {
  if (J.scans.empty()) return jpg_fail(err, "no SOS");
  if (J.progressive) {
    int bits[4][6];
    for (auto& b : bits)
      for (int& v : b) v = -1;
    for (const ScanHost& S : J.scans)
      for (int k = 0; k < S.ns; ++k)
        for (int z = S.Ss; z <= std::min(S.Se, 5); ++z) bits[S.comp[k]][z] = S.Al;
    bool useful = false;
    for (int c = 0; c < J.ncomp; ++c) {
      const uint16_t* q = J.q[J.tq[c]];
      if (bits[c][0] < 0 || q[0] == 0 || q[1] == 0 || q[8] == 0 || q[16] == 0 || q[9] == 0 ||
          q[2] == 0)
        return IDN_OK;  // smoothing_ok() is FALSE for the whole image
      for (int z = 1; z <= 5; ++z) useful |= bits[c][z] != 0;
    }
    J.smooth = useful;
    for (int c = 0; c < J.ncomp; ++c)
      for (int z = 0; z < 6; ++z) J.cbits[c][z] = (int8_t)bits[c][z];
  }
  return IDN_OK;
}

inline int jpeg_parse(const uint8_t* p, size_t n, JpegHost& J, std::string* err) {
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return jpg_fail(err, "not a JPEG (no SOI)");
  size_t i = 2;
  bool sof = false;
  while (i + 4 <= n) {
    if (p[i] != 0xFF) return jpg_fail(err, "corrupt marker stream");
    uint8_t m = p[i + 1];
    if (m == 0xFF) {  // fill byte
      ++i;
      continue;
    }
    i += 2;
    if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;  // no length
    if (m == 0xD9) return jpg_scans_done(J, err);
    const size_t len = ((size_t)p[i] << 8) | p[i + 1];
    if (len < 2 || i + len > n) return jpg_fail(err, "truncated segment");
    const uint8_t* s = p + i + 2;
    const size_t sl = len - 2;
    switch (m) {
      case 0xC0:
      case 0xC1:
      case 0xC2:
      case 0xC9:
      case 0xCA: {  // SOF0 / 1 / 2: baseline / extended sequential / progressive Huffman; SOF9 /
                    // SOF10: sequential / progressive arithmetic
        if (sof) return jpg_fail(err, "second frame header");
        if (sl < 6 || s[0] != 8) return jpg_fail(err, "only 8-bit JPEG");
        J.progressive = m == 0xC2 || m == 0xCA;
        J.arith = m == 0xC9 || m == 0xCA;
        J.height = (s[1] << 8) | s[2];
        J.width = (s[3] << 8) | s[4];
        J.ncomp = s[5];
        if (J.ncomp != 1 && J.ncomp != 3 && J.ncomp != 4)
          return jpg_fail(err, "only 1, 3 or 4 components");
        if (sl < 6 + 3 * (size_t)J.ncomp || J.width <= 0 || J.height <= 0)
          return jpg_fail(err, "bad SOF");
        for (int c = 0; c < J.ncomp; ++c) {
          J.cid[c] = s[6 + 3 * c];
          J.ch[c] = s[7 + 3 * c] >> 4;
          J.cv[c] = s[7 + 3 * c] & 15;
          J.tq[c] = s[8 + 3 * c];
          if (J.ch[c] < 1 || J.cv[c] < 1 || J.tq[c] > 3) return jpg_fail(err, "bad component");
        }
        sof = true;
        break;
      }
      case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
        return jpg_fail(err, "lossless / hierarchical JPEG not supported");
      case 0xCC: {  // DAC (jdmarker.c get_dac): arithmetic conditioning, 2 bytes per table
        if (sl % 2) return jpg_fail(err, "bad DAC length");
        for (size_t k = 0; k + 2 <= sl; k += 2) {
          const int idx = s[k], val = s[k + 1];
          if (idx >= 32) return jpg_fail(err, "bad DAC table index");
          if (idx >= 16) {
            J.dacK[idx - 16] = (uint8_t)val;
          } else {
            J.dacL[idx] = (uint8_t)(val & 15);
            J.dacU[idx] = (uint8_t)(val >> 4);
            if (J.dacL[idx] > J.dacU[idx]) return jpg_fail(err, "bad DAC value");
          }
        }
        break;
      }
      case 0xC4: {  // DHT
        size_t k = 0;
        while (k < sl) {
          if (k + 17 > sl) return jpg_fail(err, "bad DHT");
          const int tc = s[k] >> 4, th = s[k] & 15;
          if (tc > 1 || th > 3) return jpg_fail(err, "bad DHT class");
          HuffSpec& H = tc ? J.ac[th] : J.dc[th];
          int tot = 0;
          for (int l = 1; l <= 16; ++l) {
            H.bits[l] = s[k + l];
            tot += H.bits[l];
          }
          if (tot > 256 || k + 17 + tot > sl) return jpg_fail(err, "bad DHT counts");
          memcpy(H.val, s + k + 17, tot);
          H.present = true;
          k += 17 + tot;
        }
        break;
      }
      case 0xDB: {  // DQT
        size_t k = 0;
        while (k < sl) {
          const int pq = s[k] >> 4, tq = s[k] & 15;
          if (tq > 3) return jpg_fail(err, "bad DQT");
          const size_t need = 1 + 64 * (pq ? 2 : 1);
          if (k + need > sl) return jpg_fail(err, "truncated DQT");
          for (int z = 0; z < 64; ++z)
            J.q[tq][jpg_natural_host[z]] =
                pq ? (uint16_t)((s[k + 1 + 2 * z] << 8) | s[k + 2 + 2 * z]) : s[k + 1 + z];
          J.qpresent[tq] = true;
          k += need;
        }
        break;
      }
      case 0xDD:  // DRI
        if (sl < 2) return jpg_fail(err, "bad DRI");
        J.restart = (s[0] << 8) | s[1];
        break;
      case 0xE0:  // APP0: JFIF (jdmarker.c examine_app0: identifier + at least 14 bytes)
        if (sl >= 14 && memcmp(s, "JFIF", 5) == 0) J.jfif = true;
        break;
      case 0xEE:  // APP14 Adobe (examine_app14: at least 12 bytes): the colour transform flag
        if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
          J.adobe = true;
          J.adobe_transform = s[11];
        }
        break;
      case 0xDE: case 0xDF: case 0xF0: case 0xF1: case 0xF2: case 0xF3: case 0xF4: case 0xF5:
      case 0xF6: case 0xF7: case 0xF8: case 0xF9: case 0xFA: case 0xFB: case 0xFC: case 0xFD:
        // DHP / EXP / JPGn: fatal in libjpeg-turbo (read_markers' reserved-marker error); in libjpeg
        // 9 JPG8 is the LSE colour-transform marker (not restated)
        return jpg_fail(err, "reserved / extension marker (DHP, EXP, JPGn, LSE) not supported");
      case 0xDA: {  // SOS
        if (!sof) return jpg_fail(err, "SOS before SOF");
        if (sl < 1) return jpg_fail(err, "bad SOS");
        const int ns = s[0];
        if (ns < 1 || ns > J.ncomp || sl < 1 + 2 * (size_t)ns + 3) return jpg_fail(err, "bad SOS");
        if (J.ncomp >= 3) {  // (a fourth component, K, sampled as the first)
          const bool s444 = J.ch[0] == 1 && J.cv[0] == 1;
          const bool s422 = J.ch[0] == 2 && J.cv[0] == 1;
          const bool s420 = J.ch[0] == 2 && J.cv[0] == 2;
          if (!(s444 || s422 || s420) || J.ch[1] != 1 || J.cv[1] != 1 || J.ch[2] != 1 ||
              J.cv[2] != 1 || (J.ncomp == 4 && (J.ch[3] != J.ch[0] || J.cv[3] != J.cv[0])))
            return jpg_fail(err, "chroma sampling other than 4:4:4 / 4:2:2 / 4:2:0");
        }
        ScanHost S;
        S.ns = ns;
        S.restart = J.restart;
        for (int k = 0; k < ns; ++k) {
          int c = 0;
          while (c < J.ncomp && J.cid[c] != s[1 + 2 * k]) ++c;
          if (c == J.ncomp) return jpg_fail(err, "scan names an unknown component");
          if (k > 0 && c <= S.comp[k - 1]) return jpg_fail(err, "scan component order differs from the frame");
          S.comp[k] = c;
          const int td = s[2 + 2 * k] >> 4, ta = s[2 + 2 * k] & 15;
          if (td > 3 || ta > 3) return jpg_fail(err, "bad SOS table");
          J.td[c] = td;
          J.ta[c] = ta;
          S.dc[k] = J.dc[td];
          S.ac[k] = J.ac[ta];
          S.td[k] = td;
          S.ta[k] = ta;
          S.aL[k] = J.dacL[td];
          S.aU[k] = J.dacU[td];
          S.aK[k] = J.dacK[ta];
        }
        const uint8_t* ss = s + 1 + 2 * ns;
        S.Ss = ss[0];
        S.Se = ss[1];
        S.Ah = ss[2] >> 4;
        S.Al = ss[2] & 15;
        if (J.progressive) {  // jdinput.c / jdhuff.c start_pass_huff_decoder checks
          const bool dc = S.Ss == 0;
          if ((dc && S.Se != 0) || (!dc && (S.Se < S.Ss || S.Se > 63 || ns != 1)) || S.Ah > 13 ||
              S.Al > 13 || (S.Ah != 0 && S.Al != S.Ah - 1))
            return jpg_fail(err, "bad progressive scan parameters");
        } else if (S.Ss != 0 || S.Se != 63 || ss[2] != 0) {
          return jpg_fail(err, "not a sequential scan");
        }
        for (int k = 0; k < ns; ++k) {
          const int c = S.comp[k];
          if (!J.qpresent[J.tq[c]]) return jpg_fail(err, "missing quantisation table");
          const bool need_dc = S.Ss == 0 && S.Ah == 0, need_ac = S.Se > 0 && !(J.progressive && S.Ah);
          const bool need_ac_ref = J.progressive && S.Ss > 0 && S.Ah;
          if (!J.arith &&
              ((need_dc && !S.dc[k].present) || ((need_ac || need_ac_ref) && !S.ac[k].present)))
            return jpg_fail(err, "missing Huffman table");
        }
        S.begin = i + len;
        if (!J.progressive && !J.arith && J.ncomp <= 3 && J.scans.empty() && ns == J.ncomp) {
          // one interleaved sequential scan: the parallel path.  Its segment runs up to the EOI
          // (scanning back from the end) or the end of data
          for (int c = 0; c < J.ncomp; ++c)
            if (J.td[c] > 1 || J.ta[c] > 1) return jpg_fail(err, "Huffman table id > 1");
          J.scan_begin = S.begin;
          size_t e = n;
          while (e >= J.scan_begin + 2 && !(p[e - 2] == 0xFF && p[e - 1] == 0xD9)) --e;
          J.scan_end = (e >= J.scan_begin + 2) ? e - 2 : n;
          return IDN_OK;
        }
        S.end = jpg_segment_end(p, n, S.begin);
        J.scans.push_back(S);
        if (J.scans.size() > 64) return jpg_fail(err, "too many scans");
        i = S.end;
        continue;  // the next marker
      }
      default:
        if (m < 0xC0) return jpg_fail(err, "corrupt marker");
        break;  // APPn, COM, ...: skip
    }
    i += len;
  }
  return jpg_scans_done(J, err);
}

// jdhuff.c jpeg_make_d_derived_tbl: canonical codes -> fast lookup + maxcode / valoffset
inline int jpeg_build_huff(const HuffSpec& H, bool dc, uint16_t* lut, int32_t* maxcode,
                           int32_t* valoff, uint8_t* huffval, std::string* err) {
  int code = 0, k = 0;
  memset(lut, 0, sizeof(uint16_t) << JPG_LUTB);
  for (int l = 1; l <= 16; ++l) {
    // jdhuff.c jpeg_make_d_derived_tbl: the codes of length l must fit in l bits and none may be
    // all ones (code after the last >= 2^l is JERR_BAD_HUFF_TABLE); checked before any LUT write
    if (code + (int)H.bits[l] >= (1 << l)) return jpg_fail(err, "bad Huffman table");
    if (H.bits[l]) {
      valoff[l] = k - code;
      for (int t = 0; t < H.bits[l]; ++t, ++k, ++code) {
        if (l <= JPG_LUTB) {
          const int lo = code << (JPG_LUTB - l), hi = (code + 1) << (JPG_LUTB - l);
          for (int x = lo; x < hi; ++x) lut[x] = (uint16_t)(l << 8 | H.val[k]);
        }
      }
      maxcode[l] = code - 1;
    } else {
      valoff[l] = 0;
      maxcode[l] = -1;
    }
    code <<= 1;
  }
  maxcode[0] = -1;
  maxcode[17] = 0x7FFFFFFF;  // sentinel: a corrupt stream stops at length 17
  valoff[0] = valoff[17] = 0;
  memcpy(huffval, H.val, 256);
  if (dc)
    for (int t = 0; t < k; ++t)
      if (H.val[t] > 15) return jpg_fail(err, "bad DC Huffman value");
  return IDN_OK;
}

// the colour space libjpeg assigns a file (jdapimin.c default_decompress_parms; the caller asks
// for RGB, or CMYK for 4 components): 0 YCbCr (converted), 1 RGB (copied), 2 CMYK (copied), 3 YCCK
// (converted to CMYK), -1 one that is not restated.
// libjpeg 9 looks at the component IDs first -- (1, 2, 3) YCbCr, (1, 0x22, 0x23) big-gamut YCC,
// 'R' 'G' 'B' RGB, 'r' 'g' 'b' big-gamut RGB -- then a JFIF marker (YCbCr), then Adobe's transform
// (0 RGB, else YCbCr), else YCbCr.  libjpeg-turbo (6b's order) looks at JFIF, then Adobe, then the
// IDs 'R' 'G' 'B', else YCbCr.
inline int jpg_color_space(const JpegHost& J, bool turbo) {
  if (J.ncomp == 4)  // CMYK stored as is, or YCCK: Adobe's transform 0 / 2 (else YCCK; no marker: CMYK)
    return J.adobe && J.adobe_transform != 0 ? 3 : 2;
  if (J.ncomp != 3) return 0;
  const int a = J.cid[0], b = J.cid[1], c = J.cid[2];
  const bool rgb_ids = a == 'R' && b == 'G' && c == 'B';
  const int adobe = J.adobe_transform == 0 ? 1 : 0;
  if (!turbo) {
    if (a == 1 && b == 2 && c == 3) return 0;
    if ((a == 1 && b == 0x22 && c == 0x23) || (a == 'r' && b == 'g' && c == 'b')) return -1;
    if (rgb_ids) return 1;
    if (J.jfif) return 0;
    return J.adobe ? adobe : 0;
  }
  if (J.jfif) return 0;
  if (J.adobe) return adobe;
  return rgb_ids ? 1 : 0;
}

// ---- host: batch plan ---------------------------------------------------------------------------
// the workspace regions are carved by Bump::take, each on a 256-byte boundary
struct JpegPlan : Bump {
  JpegPlan() { align = 256; }
  std::vector<JpegDev> dev;
  std::vector<uint64_t> blk_end;
  std::vector<size_t> scan_begin;
  std::vector<JpegScanDev> scans;   // the scan path's scans, image by image
  std::vector<size_t> scan_src;     // their first byte in the file
  uint64_t scan_bytes = 0, nblk = 0, plane_bytes = 0, ub_bytes = 0;
  uint32_t nintervals = 0, nchunks = 0, max_items = 1, max_items_w = 1, nsub = 1;
  uint64_t nmk = 0;  // marker table entries
  int mt_img = 1, mt_scan = 1;  // most unstuffing tiles of an image / of a scan
  bool any_chunked = false, any_restart = false;
  bool any_huff_scan = false, any_arith = false;  // scan-path images of each coding
  bool scales[2][2] = {};  // IDCT output scales present: [sv - 1][sh - 1]
  // workspace regions, in this order, each 256-byte aligned; the entry point stages
  // [off_imgs, off_coef) through pinned memory in one piece
  size_t off_imgs = 0, off_blkend = 0, off_scans = 0, off_scan = 0, off_coef = 0, off_planes = 0;
  size_t off_ub = 0, off_iv = 0, off_ivend = 0, off_mk = 0, off_ublen = 0, off_ublen_s = 0, off_s0 = 0, off_s1 = 0,
         off_cnt = 0, off_start = 0, off_flag = 0, off_chg0 = 0, off_chg1 = 0, off_ck_st = 0,
         off_ck_co = 0, off_tcnt = 0, off_ck_iv = 0, off_iv_ck = 0;
};

// flags: IDN_JPEG_TURBO selects libjpeg-turbo's decode (else libjpeg 9d's); bits 8..23 = entropy
// chunk size in bits (0: the batch-dependent default; else a multiple of 64, >= 512)
inline int jpeg_plan(const uint8_t* const* files, const size_t* lens, int n, int h, int w,
                     int flags, JpegPlan& P, std::string* err, bool tables = true) {
  const bool turbo = (flags & IDN_JPEG_TURBO) != 0;
  const bool orient = (flags & IDN_JPEG_IGNORE_ORIENTATION) == 0;
  const uint32_t chunk_req = (uint32_t)(flags >> 8) & 0xFFFFu;
  if ((flags & ~(IDN_JPEG_TURBO | IDN_JPEG_IGNORE_ORIENTATION | (0xFFFF << 8))) != 0 ||
      (chunk_req != 0 && (chunk_req < 512 || chunk_req % 64 != 0))) {
    if (err) *err = "bad flags";
    return IDN_EINVAL;
  }
  uint64_t chunked_bits = 0;  // entropy bits of the images the chunked decoder takes
  P.dev.assign(n, JpegDev{});
  P.blk_end.assign(n, 0);
  P.scan_begin.assign(n, 0);
  for (int i = 0; i < n; ++i) {
    JpegHost J;
    if (!files[i]) return jpg_fail(err, "null file pointer");
    int rc = jpeg_parse(files[i], lens[i], J, err);
    if (rc != IDN_OK) return rc;
    const int ori = orient ? jpg_exif_orientation(files[i], lens[i]) : 1;
    const bool tr = ori >= 5;  // the output is the transposed size
    if ((h > 0 && (tr ? J.width : J.height) != h) || (w > 0 && (tr ? J.height : J.width) != w)) {
      if (err) *err = "image size differs from the batch size";
      return IDN_EINVAL;
    }
    JpegDev& D = P.dev[i];
    memset(&D, 0, sizeof(D));
    D.orient = ori;
    D.width = J.width;
    D.height = J.height;
    D.ncomp = J.ncomp;
    D.restart = J.restart;
    D.hmax = D.vmax = 1;
    for (int c = 0; c < J.ncomp; ++c) {
      D.hmax = std::max(D.hmax, J.ch[c]);
      D.vmax = std::max(D.vmax, J.cv[c]);
    }
    if (J.ncomp == 1) {  // non-interleaved single component: MCU = one block of the component
      D.hmax = D.vmax = 1;
      D.ch[0] = D.cv[0] = 1;
      D.mcux = (J.width + 7) / 8;
      D.mcuy = (J.height + 7) / 8;
    } else {
      for (int c = 0; c < J.ncomp; ++c) {
        D.ch[c] = J.ch[c];
        D.cv[c] = J.cv[c];
      }
      D.mcux = (J.width + 8 * D.hmax - 1) / (8 * D.hmax);
      D.mcuy = (J.height + 8 * D.vmax - 1) / (8 * D.vmax);
    }
    const int mcus = D.mcux * D.mcuy;
    D.nintervals = D.restart ? (mcus + D.restart - 1) / D.restart : 1;
    for (int c = 0; c < J.ncomp; ++c) {
      D.tq[c] = J.tq[c];
      D.td[c] = J.td[c];
      D.ta[c] = J.ta[c];
      D.bw[c] = D.mcux * D.ch[c];
      D.bh[c] = D.mcuy * D.cv[c];
      // jdmaster.c (libjpeg >= 7, do_fancy_upsampling): the IDCT size doubles while the doubled
      // component still divides the maximum sampling factor (at most 16 = 2 x DCTSIZE); the two
      // directions never differ by more than 2x, which holds for factors 1 and 2
      D.sh[c] = (!turbo && D.hmax % (2 * D.ch[c]) == 0) ? 2 : 1;
      D.sv[c] = (!turbo && D.vmax % (2 * D.cv[c]) == 0) ? 2 : 1;
      D.pw[c] = D.bw[c] * 8 * D.sh[c];
      // libjpeg: downsampled size = ceil(image size * samp * idct size / (max samp * 8))
      D.dw[c] = (J.width * D.ch[c] * D.sh[c] + D.hmax - 1) / D.hmax;
      D.dh[c] = (J.height * D.cv[c] * D.sv[c] + D.vmax - 1) / D.vmax;
      P.scales[D.sv[c] - 1][D.sh[c] - 1] = true;
      D.blk_off[c] = P.nblk;
      P.nblk += (uint64_t)D.bw[c] * D.bh[c];
      D.pl_off[c] = P.plane_bytes;
      P.plane_bytes += (uint64_t)D.pw[c] * D.bh[c] * 8 * D.sv[c];
    }
    // what the colour pass still has to upsample (the chroma planes' remaining factor)
    D.up = 0;
    if (J.ncomp >= 3) {
      const int fh = D.hmax / (D.ch[1] * D.sh[1]), fv = D.vmax / (D.cv[1] * D.sv[1]);
      if (fh != D.hmax / (D.ch[2] * D.sh[2]) || fv != D.vmax / (D.cv[2] * D.sv[2]) ||
          D.ch[0] * D.sh[0] != D.hmax || D.cv[0] * D.sv[0] != D.vmax ||
          (J.ncomp == 4 && (D.ch[3] * D.sh[3] != D.hmax || D.cv[3] * D.sv[3] != D.vmax)))
        return jpg_fail(err, "unsupported chroma sampling");
      if (fh == 1 && fv == 1) D.up = 0;
      else if (fh == 2 && fv == 1) D.up = 1;
      else if (fh == 2 && fv == 2) D.up = 2;
      else return jpg_fail(err, "unsupported chroma sampling");
    }
    D.cb_g = turbo ? 22554 : 22553;  // FIX(0.34414) / FIX(0.344136286), SCALEBITS 16
    P.blk_end[i] = P.nblk;
    D.bpm = 0;
    for (int c = 0; c < J.ncomp; ++c)
      for (int v = 0; v < D.cv[c]; ++v)
        for (int hh = 0; hh < D.ch[c]; ++hh) {
          D.ph_comp[D.bpm] = (uint8_t)c;
          D.ph_dv[D.bpm] = (uint8_t)v;
          D.ph_dh[D.bpm] = (uint8_t)hh;
          ++D.bpm;
        }
    D.total_blocks = (uint32_t)mcus * D.bpm;
    for (int c = 0; c < J.ncomp; ++c) {  // jdinput.c: ceil(ceil(size * samp / max samp) / 8)
      const int cw = (J.width * D.ch[c] + D.hmax - 1) / D.hmax;
      const int chh = (J.height * D.cv[c] + D.vmax - 1) / D.vmax;
      D.wib[c] = (cw + 7) / 8;
      D.hib[c] = (chh + 7) / 8;
    }
    for (int t = 0; t < 4; ++t) memcpy(D.q[t], J.q[t], sizeof(D.q[t]));
    if (J.smooth && turbo)  // libjpeg-turbo >= 2.1: 9 coefficients from a 5x5 DC neighbourhood
      return jpg_fail(err, "libjpeg-turbo block smoothing (progressive file with imprecise AC) "
                           "not supported");
    D.smooth = J.smooth ? 1 : 0;
    D.arith = J.arith ? 1 : 0;
    D.rgb = jpg_color_space(J, turbo);
    if (D.rgb < 0) return jpg_fail(err, "big-gamut (BG_YCC / BG_RGB) JPEG not supported");
    memcpy(D.cbits, J.cbits, sizeof(D.cbits));
    if (!J.scans.empty()) {  // the scan path: one descriptor per scan, its bytes in this image's
                             // stretch of the batch scan buffer; the parallel path sees no data
      D.scan_off = P.scan_bytes;
      D.scan_len = 0;
      P.scan_begin[i] = 0;
      D.ub_off = P.ub_bytes;
      P.ub_bytes += 64;
      D.iv_off = P.nintervals;
      D.nintervals = 1;
      P.nintervals += 1;
      D.mk_off = P.nmk;
      D.mk_cap = 0;
      D.restart = 0;
      D.nchunks = 0;
      D.scan0 = (uint32_t)P.scans.size();
      D.nscan = (uint32_t)J.scans.size();
      (J.arith ? P.any_arith : P.any_huff_scan) = true;
      for (const ScanHost& S : J.scans) {
        JpegScanDev SD;
        memset(&SD, 0, sizeof(SD));
        SD.img = i;
        SD.ns = S.ns;
        for (int k = 0; k < S.ns; ++k) SD.comp[k] = S.comp[k];
        SD.Ss = S.Ss;
        SD.Se = S.Se;
        SD.Ah = S.Ah;
        SD.Al = S.Al;
        SD.restart = S.restart;
        SD.kind = !J.progressive ? JPG_SEQ
                  : S.Ss == 0     ? (S.Ah ? JPG_DC_REFINE : JPG_DC_FIRST)
                                  : (S.Ah ? JPG_AC_REFINE : JPG_AC_FIRST);
        SD.nunits = S.ns == 1 ? (uint32_t)D.wib[S.comp[0]] * (uint32_t)D.hib[S.comp[0]]
                              : (uint32_t)mcus;
        SD.nintervals = S.restart ? (int)((SD.nunits + S.restart - 1) / S.restart) : 1;
        if (SD.nintervals < 1) SD.nintervals = 1;
        SD.arith = J.arith ? 1 : 0;
        for (int k = 0; k < 4; ++k) {
          SD.td[k] = S.td[k];
          SD.ta[k] = S.ta[k];
          SD.aL[k] = S.aL[k];
          SD.aU[k] = S.aU[k];
          SD.aK[k] = S.aK[k];
        }
        for (int sl = 0; sl < 8; ++sl)
          for (int k = 0; k < 18; ++k) SD.maxcode[sl][k] = -1;
        for (int k = 0; k < S.ns && tables && !J.arith; ++k) {
          const bool dc = SD.kind == JPG_SEQ || SD.kind == JPG_DC_FIRST;
          const bool ac = SD.kind == JPG_SEQ || SD.kind == JPG_AC_FIRST || SD.kind == JPG_AC_REFINE;
          if (dc) {
            rc = jpeg_build_huff(S.dc[k], true, SD.lut[k], SD.maxcode[k], SD.valoff[k], SD.huffval[k], err);
            if (rc != IDN_OK) return rc;
          }
          if (ac) {
            rc = jpeg_build_huff(S.ac[k], false, SD.lut[4 + k], SD.maxcode[4 + k], SD.valoff[4 + k],
                                 SD.huffval[4 + k], err);
            if (rc != IDN_OK) return rc;
          }
        }
        const size_t len = S.end - S.begin;
        if (len >= JPG_MAX_SCAN) return jpg_fail(err, "scan too large");
        SD.scan_off = P.scan_bytes;
        SD.scan_len = (uint32_t)len;
        P.scan_bytes += (len + 15) & ~(size_t)15;
        SD.ub_off = P.ub_bytes;
        P.ub_bytes += (len + 64 + 15) & ~(size_t)15;
        SD.iv_off = P.nintervals;
        P.nintervals += (uint32_t)SD.nintervals;
        SD.mk_off = P.nmk;
        SD.mk_cap = (uint32_t)SD.nintervals + JPG_MK_EXTRA;
        P.nmk += SD.mk_cap;
        P.scans.push_back(SD);
        P.scan_src.push_back(S.begin);
      }
      continue;
    }
    for (int t = 0; t < 4 && tables; ++t) {
      for (int k = 0; k < 18; ++k) D.maxcode[t][k] = -1;
      const HuffSpec& H = t < 2 ? J.dc[t] : J.ac[t - 2];
      if (!H.present) continue;
      rc = jpeg_build_huff(H, t < 2, D.lut[t], D.maxcode[t], D.valoff[t], D.huffval[t], err);
      if (rc != IDN_OK) return rc;
    }
    D.scan_off = P.scan_bytes;
    D.scan_len = (uint32_t)(J.scan_end - J.scan_begin);
    P.scan_begin[i] = J.scan_begin;
    if (J.scan_end - J.scan_begin >= JPG_MAX_SCAN) return jpg_fail(err, "scan too large");
    P.scan_bytes += (D.scan_len + 15) & ~15u;
    D.ub_off = P.ub_bytes;
    P.ub_bytes += (D.scan_len + 64 + 15) & ~15u;
    D.iv_off = P.nintervals;
    P.nintervals += (uint32_t)D.nintervals;
    D.mk_off = P.nmk;
    D.mk_cap = (uint32_t)D.nintervals + JPG_MK_EXTRA;
    P.nmk += D.mk_cap;
    if (!D.restart) chunked_bits += (uint64_t)D.scan_len * 8;
  }
  // entropy chunks (the self-synchronising decoder's threads).  Default size: about 100k chunks
  // in the batch, within [1536, 6144] bits in steps of 512 -- a single 600x1000 q90 file decodes
  // in 1.41 ms at 1536-bit chunks against 1.62 at 4096, a batch of 256 in 7.07 ms at 6144
  // against 7.27 (profiles/r05/jpeg/chunk_sweep.txt): short chunks shorten every pass when the
  // batch cannot fill the chip, long ones need fewer B passes when it can
  const uint32_t chunk_bits =
      chunk_req ? chunk_req
                : (uint32_t)std::min<uint64_t>(
                      6144, std::max<uint64_t>(1536, (chunked_bits / 100000 + 511) / 512 * 512));
  for (int i = 0; i < n; ++i) {
    JpegDev& D = P.dev[i];
    D.ch_off = P.nchunks;
    D.chunk_bits = chunk_bits;
    if (D.nscan) continue;  // the scan path: no chunks
    // (restart intervals: each its own chunks, jpeg_chunk_map_kernel; room for the worst case)
    D.nchunks = (uint32_t)(((uint64_t)D.scan_len * 8 + D.chunk_bits - 1) / D.chunk_bits) +
                (D.restart ? (uint32_t)D.nintervals : 0u);
    if (D.nchunks == 0) D.nchunks = 1;
    P.nchunks += D.nchunks;
    P.any_chunked = true;
    P.any_restart |= D.restart != 0;
    P.max_items = std::max(P.max_items, D.nchunks);
    P.max_items_w = std::max(P.max_items_w, D.nchunks * jpg_nsub(chunk_bits));
  }
  P.nsub = jpg_nsub(chunk_bits);
  for (const JpegDev& D : P.dev)
    P.mt_img = std::max(P.mt_img, (int)((D.scan_len + UNS_TILE - 1) / UNS_TILE));
  for (const JpegScanDev& S : P.scans)
    P.mt_scan = std::max(P.mt_scan, (int)((S.scan_len + UNS_TILE - 1) / UNS_TILE));
  const size_t nch = P.nchunks, niv = P.nintervals, nsc = P.scans.size();
  P.off_imgs = P.take(sizeof(JpegDev) * (size_t)n);
  P.off_blkend = P.take(sizeof(uint64_t) * (size_t)n);
  P.off_scans = P.take(sizeof(JpegScanDev) * nsc);
  P.off_scan = P.take(P.scan_bytes + 16);
  P.off_coef = P.take(P.nblk * 128);
  P.off_planes = P.take(P.plane_bytes);
  P.off_ub = P.take(P.ub_bytes);
  P.off_iv = P.take(sizeof(uint32_t) * niv);
  P.off_ivend = P.take(sizeof(uint32_t) * niv);
  P.off_mk = P.take(sizeof(uint32_t) * 2 * (size_t)P.nmk);  // (offset, code) pairs
  P.off_ublen = P.take(sizeof(uint32_t) * (size_t)n);
  P.off_ublen_s = P.take(sizeof(uint32_t) * (nsc + 1));
  P.off_s0 = P.take(sizeof(uint64_t) * nch);
  P.off_s1 = P.take(sizeof(uint64_t) * nch);
  P.off_cnt = P.take(sizeof(ChunkOut) * nch);
  P.off_start = P.take(sizeof(ChunkOut) * nch);
  P.off_flag = P.take(256);
  P.off_chg0 = P.take(nch);
  P.off_chg1 = P.take(nch);
  P.off_ck_st = P.take(sizeof(uint64_t) * nch * P.nsub);
  P.off_ck_co = P.take(sizeof(ChunkOut) * nch * P.nsub);
  P.off_ck_iv = P.take(sizeof(uint32_t) * nch);
  P.off_iv_ck = P.take(sizeof(uint32_t) * niv);
  // (count, markers) pairs per unstuffing tile; the images' and the scans' passes share them
  P.off_tcnt = P.take(sizeof(uint32_t) * 2 * std::max((size_t)n * P.mt_img, nsc * (size_t)P.mt_scan));
  return IDN_OK;
}

}  // namespace idn
