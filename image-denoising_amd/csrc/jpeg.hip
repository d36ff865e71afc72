// JPEG decode front-end: cv2.imread(path) (IMREAD_COLOR, BGR u8) for the reference's images
// (lib/model/test.py:191, lib/roi_data_layer/minibatch.py:85), decoded on the GPU.
//
// Output = what the reference's pinned decoder produces with its defaults: IJG libjpeg 9d
// (requirements.txt:74, under OpenCV 3.4.2) -- the ISLOW integer IDCT (jidctint.c) for full-size
// components and, since libjpeg 7, a scaled IDCT for subsampled chroma (jdmaster.c: with fancy
// upsampling a component sampled at half the maximum rate gets jpeg_idct_16x16 (4:2:0) or
// jpeg_idct_16x8 (4:2:2), decoding straight to full resolution, no upsampling pass), then the
// integer YCbCr -> RGB tables of libjpeg 9's jdcolor.c (FIX(0.344136286) for Cb -> G).
// IDN_JPEG_TURBO selects libjpeg-turbo's decode instead (8x8 IDCT everywhere, "fancy" triangular
// h2v1 / h2v2 upsampling from jdsample.c, FIX(0.34414)): what PIL 9+ / turbo-linked OpenCV make.
// All restated from the published algorithms; tests check bit-exactness against the real libjpeg
// 9d decode (committed fixtures) and the GPU box's turbo-linked PIL.
//
// The decoder is split into units.  Host, HIP-free headers:
//   jpeg_desc.hpp     what host and device agree on: the image / scan descriptors (JpegDev,
//                     JpegScanDev), ChunkOut, the constants that size the workspace
//   jpeg_host.hpp     the marker parser (SOI .. SOS: DQT / DHT / DAC / SOFn / DRI / APPn), the
//                     EXIF orientation, the Huffman lookup tables per image and scan, the
//                     colour-space rule and the batch planner with the workspace layout (jpeg_plan)
// Device (jpeg_device.hpp: the helpers two units share, one call's regions, the launchers):
//   jpeg_entropy.hip  unstuff, and the parallel path (sync A / B, prefix, write)
//   jpeg_scan.hip     the scan path (jpeg_prog_kernel, jpeg_arith_kernel)
//   jpeg_pixels.hip   idct and color
//   jpeg.hip          this file: the entry points -- one packed host->device copy of the
//                     descriptors and the images' entropy-coded segments through pinned staging,
//                     then the launch sequence with the B-pass loop
// The stages:
//   unstuff        per 16 KiB tile: the segments without stuffing and markers, every marker's code
//                  and offset; per segment each restart interval's data as libjpeg reads it
//                  (jdmarker.c resync on damaged files)
//   the parallel path: single-scan Huffman files of 1 or 3 components (SOF0 / SOF1)
//     sync A / B   self-synchronising chunk decoders (each restart interval its own chunks) with
//                  checkpoints; B passes until no chunk's end state changes
//     prefix       per image: each chunk's first block and DC predictors
//     write        one thread per 256-bit sub-chunk from the checkpoints: coefficient blocks
//   the scan path: progressive (SOF2), multi-scan, arithmetic-coded (SOF9 / SOF10) and
//     4-component files; one wave per image walks the scans in file order, lanes over restart
//     intervals: jpeg_prog_kernel (Huffman: jdhuff.c's decoders) or jpeg_arith_kernel
//     (jdarith.c's QM-coder)
//   idct           one thread per block: libjpeg 9d block smoothing of progressive files whose last
//                  scan leaves AC 1..5 imprecise (jpg_smooth), dequantise, ISLOW IDCT (8x8, or
//                  16x16 / 16x8 for libjpeg 9's scaled chroma) into u8 component planes
//   color          8 output pixels per thread: chroma upsampling (turbo), then YCbCr -> BGR, RGB
//                  copied, gray replicated, or CMYK / YCCK (libjpeg's CMYK output) through OpenCV's
//                  CMYK -> BGR (jpg_color_space: component IDs, JFIF / Adobe markers, per library)
// Supported: 8-bit DCT JPEG (Huffman or arithmetic), 1, 3 or 4 components, sampling 4:4:4 /
// 4:2:2 (h2v1) / 4:2:0 (h2v2) (a fourth component sampled as the first), optional restart
// intervals.  Anything else (lossless, hierarchical, 12-bit, big-gamut colour, extension
// markers) is IDN_EUNSUPPORTED -- as libjpeg 9d (8-bit, DCT) refuses the first three too.
// Damaged entropy-coded data decodes as libjpeg decodes it: past an interval's data the bits are
// 0 and an MCU is decoded only if the data lasted up to its start (jdhuff.c insufficient_data),
// a bit pattern that is no code takes 17 bits and decodes as 0.
#include "jpeg_device.hpp"
#include "jpeg_host.hpp"

#include <atomic>
#include <thread>

using namespace idn;

extern "C" int idn_jpeg_info(const uint8_t* file, size_t len, int* height, int* width,
                             int* components) {
  IDN_CHECK_ARG(file && height && width && components, "idn_jpeg_info: null pointer");
  JpegHost J;
  std::string err;
  const int rc = jpeg_parse(file, len, J, &err);
  if (rc != IDN_OK) return set_error(rc, "idn_jpeg_info: %s", err.c_str());
  const bool tr = jpg_exif_orientation(file, len) >= 5;  // cv2.imread's shape: after the turn
  *height = tr ? J.width : J.height;
  *width = tr ? J.height : J.width;
  *components = J.ncomp;
  return IDN_OK;
}

extern "C" int idn_jpeg_orientation(const uint8_t* file, size_t len, int* orientation) {
  IDN_CHECK_ARG(file && orientation, "idn_jpeg_orientation: null pointer");
  *orientation = jpg_exif_orientation(file, len);
  return IDN_OK;
}

extern "C" size_t idn_jpeg_workspace_size(const uint8_t* const* files, const size_t* lens, int n,
                                          int flags) {
  if (!files || !lens || n <= 0) return 0;
  JpegPlan P;
  if (jpeg_plan(files, lens, n, 0, 0, flags, P, nullptr) != IDN_OK) return 0;  // tables checked
  return P.total;
}

extern "C" int idn_jpeg_decode_u8(const uint8_t* const* files, const size_t* lens, int n,
                                  uint8_t* dst, int h, int w, int64_t row_stride, int flags,
                                  void* workspace, size_t ws_bytes, void* stream) {
  IDN_CHECK_ARG(n >= 0 && (n == 0 || (files && lens && dst)), "idn_jpeg_decode_u8: null pointer");
  IDN_CHECK_ARG(h > 0 && w > 0 && row_stride >= (int64_t)w * 3,
                "idn_jpeg_decode_u8: bad output shape");
  IDN_CHECK_ARG(n <= 65535, "idn_jpeg_decode_u8: batch too large");
  if (n == 0) return IDN_OK;
  JpegPlan P;
  std::string err;
  const int rc = jpeg_plan(files, lens, n, h, w, flags, P, &err);
  if (rc != IDN_OK) return set_error(rc, "idn_jpeg_decode_u8: %s", err.c_str());
  if (int e = check_workspace_got("idn_jpeg_decode_u8", workspace, ws_bytes, P.total,
                                  IDN_EWORKSPACE))
    return e;
  hipStream_t st = as_stream(stream);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  // one pinned host staging buffer (kept per thread, grown as needed; the call is synchronous, so
  // the next call may reuse it) -> one copy: descriptors, block ends, entropy segments
  static thread_local uint8_t* pin = nullptr;
  static thread_local size_t pin_cap = 0;
  if (pin_cap < P.off_coef) {
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    pin_cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&pin), P.off_coef, 0) != hipSuccess)
      return set_error(IDN_EHIP, "idn_jpeg_decode_u8: pinned staging alloc failed");
    pin_cap = P.off_coef;
  }
  uint8_t* host = pin;
  memcpy(host + P.off_imgs, P.dev.data(), sizeof(JpegDev) * (size_t)n);
  memcpy(host + P.off_blkend, P.blk_end.data(), sizeof(uint64_t) * (size_t)n);
  if (!P.scans.empty())
    memcpy(host + P.off_scans, P.scans.data(), sizeof(JpegScanDev) * P.scans.size());
  bool copy_ok = hipMemcpyAsync(ws, host, P.off_scan, hipMemcpyHostToDevice, st) == hipSuccess;
  {
    // the entropy segments, gathered by a few host threads in NPART parts of the batch; each
    // part's host-to-device copy is issued as soon as the part is complete, so the DMA of part
    // k overlaps the gathering of part k + 1
    constexpr int MAXPART = 16;
    const int nt = std::max(1, std::min(8, n / 8));
    const int npart = std::max(1, std::min(std::min(4, MAXPART), n / 16));
    std::atomic<int> done[MAXPART];
    for (int q = 0; q < MAXPART; ++q) done[q].store(0);
    auto first = [&](int q) { return (int)((int64_t)n * q / npart); };
    // image i's entropy bytes: its one segment, or its scans' segments (the scan path)
    auto gather = [&](int i) {
      const JpegDev& D = P.dev[i];
      if (D.nscan == 0) {
        memcpy(host + P.off_scan + D.scan_off, files[i] + P.scan_begin[i], D.scan_len);
        return;
      }
      for (uint32_t k = D.scan0; k < D.scan0 + D.nscan; ++k)
        memcpy(host + P.off_scan + P.scans[k].scan_off, files[i] + P.scan_src[k],
               P.scans[k].scan_len);
    };
    auto worker = [&](int k) {
      for (int q = 0; q < npart; ++q) {
        for (int i = first(q) + k; i < first(q + 1); i += nt) gather(i);
        done[q].fetch_add(1, std::memory_order_release);
      }
    };
    std::vector<std::thread> th;
    for (int k = 1; k < nt; ++k) th.emplace_back(worker, k);
    for (int q = 0; q < npart; ++q) {  // the calling thread: its share, then the part's copy
      for (int i = first(q); i < first(q + 1); i += nt) gather(i);
      done[q].fetch_add(1, std::memory_order_release);
      while (done[q].load(std::memory_order_acquire) < nt) std::this_thread::yield();
      const size_t b0 = P.dev[first(q)].scan_off;
      const size_t b1 = q + 1 < npart ? (size_t)P.dev[first(q + 1)].scan_off : P.scan_bytes;
      if (b1 > b0)
        copy_ok = copy_ok && hipMemcpyAsync(ws + P.off_scan + b0, host + P.off_scan + b0,
                                            b1 - b0, hipMemcpyHostToDevice, st) == hipSuccess;
    }
    for (auto& t : th) t.join();
  }
  if (!copy_ok) return set_error(IDN_EHIP, "idn_jpeg_decode_u8: staging copy failed");
  JpegCall C;
  C.st = st;
  C.n = n;
  auto at = [&](size_t off) { return static_cast<void*>(ws + off); };
  C.imgs = static_cast<const JpegDev*>(at(P.off_imgs));
  C.blk_end = static_cast<const uint64_t*>(at(P.off_blkend));
  C.scans = static_cast<const JpegScanDev*>(at(P.off_scans));
  C.scan = ws + P.off_scan;
  C.coef = static_cast<int16_t*>(at(P.off_coef));
  C.planes = ws + P.off_planes;
  C.ub = ws + P.off_ub;
  C.ivs = static_cast<uint32_t*>(at(P.off_iv));
  C.ive = static_cast<uint32_t*>(at(P.off_ivend));
  C.mk = static_cast<uint2*>(at(P.off_mk));
  C.ublen = static_cast<uint32_t*>(at(P.off_ublen));
  C.ublen_s = static_cast<uint32_t*>(at(P.off_ublen_s));
  C.S[0] = static_cast<uint64_t*>(at(P.off_s0));
  C.S[1] = static_cast<uint64_t*>(at(P.off_s1));
  C.cnt = static_cast<ChunkOut*>(at(P.off_cnt));
  C.start = static_cast<ChunkOut*>(at(P.off_start));
  C.flag = static_cast<uint32_t*>(at(P.off_flag));
  C.chg[0] = ws + P.off_chg0;
  C.chg[1] = ws + P.off_chg1;
  C.ck_st = static_cast<uint64_t*>(at(P.off_ck_st));
  C.ck_co = static_cast<ChunkOut*>(at(P.off_ck_co));
  C.tcnt = static_cast<uint2*>(at(P.off_tcnt));
  C.ck_iv = static_cast<uint32_t*>(at(P.off_ck_iv));
  C.iv_ck = static_cast<uint32_t*>(at(P.off_iv_ck));
  uint32_t* flag = C.flag;
  uint32_t* mk_over = flag + 33;  // marker table overflow (jpeg_unstuff_final)
  if (hipMemsetAsync(mk_over, 0, 4, st) != hipSuccess)
    return set_error(IDN_EHIP, "idn_jpeg_decode_u8: memset failed");
  jpeg_unstuff_images(C, P.mt_img, mk_over);
  if (P.any_restart) jpeg_chunk_map(C);
  // (after the images' unstuffing: the tile counts reuse the same array)
  if (!P.scans.empty()) jpeg_unstuff_scans(C, (unsigned)P.scans.size(), P.mt_scan, mk_over);
  uint32_t* badseen = flag + 32;  // (past the sync passes' flags)
  // entropy decoding to the output; badlen: see jpeg_write_kernel
  auto decode = [&](int badlen) -> int {
    if (hipMemsetAsync(ws + P.off_coef, 0, P.nblk * 128, st) != hipSuccess ||
        hipMemsetAsync(badseen, 0, 4, st) != hipSuccess)
      return set_error(IDN_EHIP, "idn_jpeg_decode_u8: memset failed");
    int cur = 0;
    if (P.any_chunked) {
      // pass A, then pass B until no chunk's end state changes (a batch takes ~4-6 passes, a
      // single large file ~8-9).  The B passes are launched JPG_BROUND at a time with one flag each
      // and one host read per round: the pass after the first one that changed nothing returns at
      // once (its predecessor's flag), so a round costs the passes that work plus a launch each for
      // the rest -- every host round trip (a D2H read and a stream synchronisation, ~30-40 us)
      // was a gap in a single file's decode
      constexpr int JPG_BROUND = 12;
      jpeg_sync_a(C, P.max_items, badlen);
      for (uint32_t it = 0;; it += JPG_BROUND) {
        if (hipMemsetAsync(flag, 0, 4 * JPG_BROUND, st) != hipSuccess)
          return set_error(IDN_EHIP, "idn_jpeg_decode_u8: memset failed");
        for (int k = 0; k < JPG_BROUND; ++k) {
          jpeg_sync_b(C, P.max_items, cur, flag + k, it + k == 0 ? 1 : 0,
                      k > 0 ? flag + k - 1 : nullptr, badlen);
          cur ^= 1;
        }
        uint32_t changed[JPG_BROUND] = {};
        if (hipMemcpyAsync(changed, flag, sizeof(changed), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
          return set_error(IDN_EHIP, "idn_jpeg_decode_u8: sync pass failed");
        if (!changed[JPG_BROUND - 1]) break;  // the round's last pass changed nothing
        if (it > P.max_items + 2)
          return set_error(IDN_EHIP, "idn_jpeg_decode_u8: entropy decoding did not converge");
      }
      jpeg_prefix(C);
    }
    jpeg_write(C, P.max_items_w, badlen, badseen);
    if (P.any_huff_scan) jpeg_prog(C);
    if (P.any_arith) jpeg_arith(C);
    const uint64_t gb = (P.nblk + 255) / 256;
    IDN_CHECK_ARG(gb < 0x7FFFFFFF, "idn_jpeg_decode_u8: batch too large");
    if (P.scales[0][0]) jpeg_idct(C, 1, 1, (unsigned)gb, P.nblk);
    if (P.scales[0][1]) jpeg_idct(C, 1, 2, (unsigned)gb, P.nblk);
    if (P.scales[1][1]) jpeg_idct(C, 2, 2, (unsigned)gb, P.nblk);
    jpeg_color8(C, dst, h, w, row_stride);
    return IDN_OK;
  };
  int drc = decode(P.any_chunked ? 16 : 17);
  if (drc != IDN_OK) return drc;
  uint32_t bad_over[2] = {0u, 0u};  // badseen, mk_over (adjacent words)
  if (hipMemcpyAsync(bad_over, badseen, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return set_error(IDN_EHIP, "idn_jpeg_decode_u8: decode failed");
  if (bad_over[1])
    return set_error(IDN_EUNSUPPORTED, "idn_jpeg_decode_u8: more markers in an entropy-coded "
                                       "segment than restart intervals + %u (damaged file)",
                     JPG_MK_EXTRA);
  // a bad code on a true trajectory: decode again with libjpeg's rule
  if (P.any_chunked && bad_over[0] && (drc = decode(17)) != IDN_OK) return drc;
  // the staging buffer is reused by the next call: finish here
  if (hipStreamSynchronize(st) != hipSuccess)
    return set_error(IDN_EHIP, "idn_jpeg_decode_u8: decode failed");
  IDN_CHECK_LAUNCH("idn_jpeg_decode_u8");
  return IDN_OK;
}
