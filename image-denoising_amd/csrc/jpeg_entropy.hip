// JPEG decoder, entropy stage (jpeg.hip has the map of the units): the unstuffing kernels, which
// serve both paths, and the parallel path's self-synchronising Huffman decoder (sync A / B, prefix,
// write).
#include "jpeg_device.hpp"

namespace idn {

// ---- device: entropy decoding -----------------------------------------------------------------
// Stage 1, jpeg_unstuff_count / _write / _final (16 KiB tiles): the entropy-coded segment without its
// stuffed 0x00 bytes, fill bytes and RST markers, and the bit offset where each restart interval
// starts.  The decoders then read a plain big-endian bit string.
//
// Stage 2, images without restart markers: the scan is cut into chunk_bits-bit chunks, one thread
// each, decoded in parallel by self-synchronisation (Huffman codes and the block structure
// resynchronise: from an arbitrary start state a trajectory joins the true one after ~0.8 kbit
// median, 9 kbit max on the test images).  A decoder state is (bit position, block of the MCU,
// coefficient index z; z = 0: a DC symbol is next).
//   pass A   every chunk from (its first bit, block 0, z 0)              -> end state
//   pass B   every chunk from its predecessor's end state, repeated until no end state changes
//            (chunk 0 starts from the true state, so the chain is then exact by induction); the
//            final pass also counts the chunk's DC symbols and per-component DC differences
//   prefix   per image: each chunk's first block index and DC predictors
//   write    every chunk again from its exact start state, writing coefficient blocks
// Images with restart markers: each interval is cut into its own chunks (jpeg_chunk_map_kernel);
// an interval's first chunk starts from its known state, the prefix restarts at each interval.
// Chunk size: the ABI's flags may set one; the default depends on the batch (jpeg_plan)
// Checkpoints (round 5): every pass records, per chunk and JPG_SUB-bit sub-chunk, the decoder state
// at the first symbol that starts at or after the sub-chunk's first bit and the counts (blocks, DC
// sums) from the chunk start to it.  A later pass that decodes the chunk from a new start state
// stops at the first checkpoint where its state equals the recorded one -- from there the
// trajectory is the recorded one, so the end state is and the counts shift by the difference at
// that checkpoint (a chunk's trajectories typically join within ~1 kbit, so the B passes no
// longer decode whole chunks) -- and the write pass runs one thread per sub-chunk from the final
// checkpoints: many times the threads of one per chunk, each as much shorter (a single image's
// write pass was 0.76 ms of serial decoding per thread).  256 bits measured best against 128, 512
// and 1024 (profiles/r05/jpeg/sub_ab_sweep.txt: a joining trajectory stops sooner).

// mca[t][l - 10] (l = 10..16): the largest code of length <= l, left-aligned to 16 bits with
// ones below (-1 while there is none; a length without codes repeats the one before), so that
// "code16 <= mca" is monotone in l and a longer-than-LUT code's length is 10 + the number of
// lengths it exceeds -- seven compares on two 16-byte LDS reads instead of a walk of dependent
// maxcode reads (one per length) that every wave took whenever one of its 64 lanes missed the LUT
struct JpegLds {
  alignas(16) int32_t mca[4][8];
  uint8_t natural[80];  // jpg_natural (the write pass's coefficient positions)
  uint16_t lut[4][1 << JPG_LUTB];
  int32_t maxcode[4][18], valoff[4][18];
  uint8_t huffval[4][256];
};

__device__ __forceinline__ void jpg_load_tables(JpegLds& T, const JpegDev& D) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&D.lut[0][0]);
  uint32_t* d = reinterpret_cast<uint32_t*>(&T.lut[0][0]);
  for (int k = threadIdx.x; k < (int)(sizeof(T.lut) / 4); k += blockDim.x) d[k] = s[k];
  for (int k = threadIdx.x; k < 4 * 18; k += blockDim.x) {
    (&T.maxcode[0][0])[k] = (&D.maxcode[0][0])[k];
    (&T.valoff[0][0])[k] = (&D.valoff[0][0])[k];
  }
  for (int k = threadIdx.x; k < 4 * 256; k += blockDim.x) (&T.huffval[0][0])[k] = (&D.huffval[0][0])[k];
  for (int k = threadIdx.x; k < 4 * 8; k += blockDim.x) T.mca[k >> 3][k & 7] = jpg_mca(D.maxcode[k >> 3], k & 7);
  for (int k = threadIdx.x; k < 80; k += blockDim.x) T.natural[k] = jpg_natural[k];
}

// decoder state packed in 64 bits: bit position | block of the MCU << 32 | z << 40
__device__ __forceinline__ uint64_t jpg_state(uint32_t pos, uint32_t ph, uint32_t z) {
  return (uint64_t)pos | (uint64_t)ph << 32 | (uint64_t)z << 40;
}

// the per-image constants jpg_run needs, loaded once into (scalar) registers: inside the symbol
// loop a lane-indexed read of JpegDev (phase -> component -> tables) was a global load on the
// critical path of every symbol
struct JpgConst {
  uint64_t phase_info;  // per block of the MCU, 6 bits: component | DC table << 2 | AC table << 4
  uint64_t phase_pos;   // per block of the MCU, 6 bits: block row | block column << 3
  // per-component values packed into integers and picked by shifts: selecting among fields of a
  // local struct was turned into a lane-indexed load from a stack copy (scratch)
  uint32_t bo0;          // first block of component 0
  uint64_t bo12;         // first blocks of components 1, 2 relative to component 0 (32 bits each)
  uint64_t bw;           // blocks per row, 16 bits per component
  uint32_t vshs;         // per component 4 bits: vertical | horizontal blocks per MCU << 2
  int mcux, bpm;
  uint32_t total_blocks;
};

__device__ __forceinline__ JpgConst jpg_const(const JpegDev& D) {
  JpgConst K;
  K.phase_info = 0;
  K.phase_pos = 0;
  for (int p = 0; p < D.bpm; ++p) {
    const int c = D.ph_comp[p];
    K.phase_info |= (uint64_t)(c | D.td[c] << 2 | (2 + D.ta[c]) << 4) << (6 * p);
    K.phase_pos |= (uint64_t)(D.ph_dv[p] | D.ph_dh[p] << 3) << (6 * p);
  }
  const bool one = D.ncomp == 1;
  K.bo0 = (uint32_t)D.blk_off[0];
  K.bo12 = (uint64_t)(uint32_t)(D.blk_off[1] - D.blk_off[0]) |
           (uint64_t)(uint32_t)(D.blk_off[2] - D.blk_off[0]) << 32;
  K.bw = (uint64_t)(D.bw[0] & 0xFFFF) | (uint64_t)(D.bw[1] & 0xFFFF) << 16 |
         (uint64_t)(D.bw[2] & 0xFFFF) << 32;
  K.vshs = 0;
  for (int c = 0; c < 3; ++c)
    K.vshs |= (uint32_t)((one ? 1 : D.cv[c]) | (one ? 1 : D.ch[c]) << 2) << (4 * c);
  K.mcux = D.mcux;
  K.bpm = D.bpm;
  K.total_blocks = D.total_blocks;
  return K;
}

__device__ __forceinline__ int16_t* jpg_block(const JpgConst& K, int16_t* coef, int32_t blk,
                                              uint32_t ph, int c) {
  if (blk < 0 || (uint32_t)blk >= K.total_blocks) return nullptr;
  const int mcu = blk / K.bpm;
  const int my = mcu / K.mcux, mx = mcu - my * K.mcux;
  const uint32_t pp = (uint32_t)(K.phase_pos >> (6 * ph));
  const uint32_t vh = K.vshs >> (4 * c);
  const int vs = (int)(vh & 3), hs = (int)((vh >> 2) & 3);
  const int bw = (int)((K.bw >> (16 * c)) & 0xFFFF);
  const uint64_t bo = (uint64_t)K.bo0 + (c ? (uint32_t)(K.bo12 >> (32 * (c - 1))) : 0u);
  const int by = my * vs + (int)(pp & 7), bx = mx * hs + (int)((pp >> 3) & 7);
  return coef + (bo + (uint64_t)by * bw + bx) * 64;
}

// The chunk decoders' bit source: a per-lane ring of JRG 16-byte groups of the (byte-swapped)
// stream in LDS, refilled one group ahead from a range-checked buffer load held in registers.
// The 64 lanes of a wave sit at unrelated bit positions, so any per-lane branch in the symbol loop
// is taken by some lane on most iterations and the wave executes it every time; here the refill
// is branch-free (the next word is read from the ring every iteration, one iteration before it
// is needed) and only a group change (every 4 words of a lane) branches.
constexpr int JRG = 4;                 // ring groups per lane
constexpr int JRING_W = JRG * 4 + 4;   // ring words per lane (one pad group: lane stride 80 bytes)

// Decode symbols from state st while the next symbol starts before end_bit (and at most dc_limit
// DC symbols).  WRITE: coefficient blocks (blk = the block in progress; a DC symbol starts blk + 1)
// with DC predictors pred[]; else count DC symbols and DC differences.  Returns the end state.
// One symbol per iteration, DC or AC through the same decode (a DC symbol is a size 0..15, i.e. a
// run/size byte with run 0) and the block bookkeeping by selects.
// Where the data ends, libjpeg (jdhuff.c: jpeg_fill_bit_buffer's zero bits, insufficient_data)
// decodes an MCU only if the data lasted up to its start, reading 0 past the end:
//   tail  (chunked decoder, WRITE) end_bit is the end of the data: complete the MCU in progress,
//         and one that starts exactly at the end, never past the image's last block
//   MASK  (a restart interval, whose data the next one's follows) bits from end_bit on read as 0;
//         stop at dc_limit DC symbols or at an MCU that starts past end_bit
//   CLAMP (any other piece of a restart interval: the sync passes, the write pass's inner pieces)
//         bits from zero_bit (the interval's end) on read as 0, the stop rule unchanged: a symbol
//         that starts in the piece and runs past the interval's data reads libjpeg's zero fill,
//         not the next interval's bits
template <bool WRITE, bool MASK = false, bool CLAMP = false>
__device__ __forceinline__ uint64_t jpg_run(const JpgConst& K, const JpegLds& T, rsrc_t rs,
                                            uint32_t* __restrict__ ring, uint64_t st,
                                            uint32_t end_bit, ChunkOut* cnt, int32_t blk,
                                            int (&pred)[3], int16_t* __restrict__ coef,
                                            uint32_t dc_limit = 0xFFFFFFFFu, bool tail = false,
                                            int badlen = 17, uint32_t* badseen = nullptr,
                                            uint32_t zero_bit = 0xFFFFFFFFu) {
  static_assert(!(MASK && CLAMP), "MASK already zeroes the bits past end_bit");
  uint32_t ndc = 0;
  bool bad_real = false;  // WRITE: a bad code inside the image's blocks
  uint32_t pos = (uint32_t)st, ph = (uint32_t)(st >> 32) & 0xFF, z = (uint32_t)(st >> 40) & 0xFF;
  // ring: words wi .. of groups (wi >> 2) .. (wi >> 2) + JRG - 1 at ring[w & (4 JRG - 1)]; pend =
  // group (wi >> 2) + JRG, raw
  uint32_t wi = pos >> 5;
  {
    const uint32_t g0 = wi >> 2;
#pragma unroll
    for (int k = 0; k < JRG; ++k) {
      const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, (g0 + k) * 16u, 0, 0);
      *reinterpret_cast<v4u*>(ring + ((g0 + k) & (JRG - 1)) * 4) =
          v4u{__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z),
              __builtin_bswap32(v.w)};
    }
  }
  v4u pend = __builtin_amdgcn_raw_buffer_load_b128(rs, ((wi >> 2) + JRG) * 16u, 0, 0);
  uint64_t acc = 0;
  int nb = 0;
  // word wix of the stream (MASK: its bits from end_bit on cleared; CLAMP: from zero_bit on)
  auto fetch = [&](uint32_t wix) -> uint32_t {
    const uint32_t v = ring[wix & (4 * JRG - 1)];
    if (!MASK && !CLAMP) return v;
    const int64_t r = (int64_t)(MASK ? end_bit : zero_bit) - 32 * (int64_t)wix;
    return r >= 32 ? v : r <= 0 ? 0u : v & ~(0xFFFFFFFFu >> (uint32_t)r);
  };
  uint32_t nxt = fetch(wi);
  // append word wi (nxt) to acc; a new group retires its predecessor's slot to pend
  auto append = [&](bool need) {
    acc |= need ? (uint64_t)nxt << (32 - nb) : 0ull;
    nb += need ? 32 : 0;
    wi += need ? 1u : 0u;
    if (need && (wi & 3) == 0) {
      *reinterpret_cast<v4u*>(ring + (((wi >> 2) + JRG - 1) & (JRG - 1)) * 4) =
          v4u{__builtin_bswap32(pend.x), __builtin_bswap32(pend.y), __builtin_bswap32(pend.z),
              __builtin_bswap32(pend.w)};
      pend = __builtin_amdgcn_raw_buffer_load_b128(rs, ((wi >> 2) + JRG) * 16u, 0, 0);
    }
    nxt = fetch(wi);
  };
  append(true);
  append(true);
  acc <<= (pos & 31);
  nb -= (int)(pos & 31);
  int16_t* bp = nullptr;
  if (WRITE && z != 0) bp = jpg_block(K, coef, blk, ph, (int)(K.phase_info >> (6 * ph)) & 3);
  int32_t s0 = 0, s1 = 0, s2 = 0, nblk = 0;
  int p0 = pred[0], p1 = pred[1], p2 = pred[2];
  for (;;) {
    const bool dc = z == 0;
    if (MASK) {
      if (dc && ph == 0 && (ndc == dc_limit || pos > end_bit)) break;
    } else {
      if (pos >= end_bit) {
        if (!WRITE || !tail) break;
        const bool go = dc && ph == 0 ? pos == end_bit && (uint32_t)(blk + 1) < K.total_blocks
                                      : (uint32_t)blk < K.total_blocks;
        if (!go) break;
      }
      if (dc && ndc == dc_limit) break;
    }
    append(nb < 32);
    const uint32_t info = (uint32_t)(K.phase_info >> (6 * ph));
    const int c = info & 3;
    int len;
    bool bad = false;
    const int rs8 = jpg_decode(acc, T, dc ? (info >> 2) & 3 : (info >> 4) & 3, &len, badlen, &bad);
    if (WRITE) bad_real |= bad && (uint32_t)(dc ? blk + 1 : blk) < K.total_blocks;
    const int r = rs8 >> 4, s = rs8 & 15;
    const int val = s ? jpg_extend((uint32_t)((acc << len) >> 32) >> (32 - s), s) : 0;
    acc <<= len + s;
    nb -= len + s;
    pos += len + s;
    ndc += dc ? 1u : 0u;
    if (WRITE) {
      if (dc) {
        ++blk;
        const int p = (c == 0 ? p0 : c == 1 ? p1 : p2) + val;
        p0 = c == 0 ? p : p0;
        p1 = c == 1 ? p : p1;
        p2 = c == 2 ? p : p2;
        bp = jpg_block(K, coef, blk, ph, c);
        if (bp) bp[0] = (int16_t)p;
      } else if (s && bp) {
        bp[T.natural[min(z + r, 79u)]] = (int16_t)val;  // libjpeg's overrun guard
      }
    } else {
      nblk += dc ? 1 : 0;
      s0 += dc && c == 0 ? val : 0;
      s1 += dc && c == 1 ? val : 0;
      s2 += dc && c == 2 ? val : 0;
    }
    // next coefficient index: DC -> 1; AC: value r + 1 on, ZRL 16 on, EOB the block's end
    const uint32_t za = s ? z + r + 1 : (r == 15 ? z + 16 : 64u);
    const uint32_t zn = dc ? 1u : za;
    const bool wrap = zn >= 64;
    z = wrap ? 0u : zn;
    ph = wrap ? (ph + 1 == (uint32_t)K.bpm ? 0u : ph + 1) : ph;
  }
  pred[0] = p0;
  pred[1] = p1;
  pred[2] = p2;
  if (WRITE && badseen && bad_real) *badseen = 1u;
  if (!WRITE) {
    cnt->nblk += nblk;
    cnt->dcsum[0] += s0;
    cnt->dcsum[1] += s1;
    cnt->dcsum[2] += s2;
  }
  return jpg_state(pos, ph, z);
}

// stage 1: unstuff, in 16 KiB tiles of the segment (1024 threads x 16 bytes), every tile its own
// workgroup (one workgroup per image walked its tiles in sequence: 0.28 ms for a single 600x1000
// file): count the tile's kept bytes and markers, then each tile writes from the sum of the tiles
// before it (the kept bytes, and every marker's code and unstuffed offset), then per segment the
// length, the zero padding and the restart intervals (jpeg_unstuff_final).
// (DESC: a JpegDev per image, or a JpegScanDev per scan of the scan path: the same fields)

// the thread's 16 bytes [i0, i0 + 16): bit k of keep = byte i0 + k is data, of mkm = byte i0 + k is
// a marker's code (0xFF followed by neither 0x00 nor 0xFF: RSTn or any other marker)
// (the segment starts 16-byte aligned and its buffer is padded to whole 16-byte groups: one
// 16-byte load per thread, plus the bytes either side)
__device__ __forceinline__ void unstuff_masks(const uint8_t* __restrict__ in, uint32_t n,
                                              uint32_t i0, uint32_t& keep, uint32_t& mkm,
                                              uint32_t (&w)[4]) {
  keep = 0;
  mkm = 0;
  const uint4 v = *reinterpret_cast<const uint4*>(in + i0);
  w[0] = v.x;
  w[1] = v.y;
  w[2] = v.z;
  w[3] = v.w;
  uint32_t pv = i0 > 0 ? in[i0 - 1] : 0u;
  const uint32_t after = i0 + 16 < n ? in[i0 + 16] : 0u;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t i = i0 + k;
    const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    const uint32_t nx = k < 15 ? (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu : after;
    bool kp;
    if (pv == 0xFF && b == 0x00) {
      kp = false;  // stuffing
    } else if (pv == 0xFF && b != 0xFF) {
      kp = false;  // a marker code
      if (i < n) mkm |= 1u << k;
    } else if (b == 0xFF) {
      kp = i + 1 < n && nx == 0x00;  // data 0xFF (stuffed); else fill / marker prefix
    } else {
      kp = true;
    }
    if (kp && i < n) keep |= 1u << k;
    pv = b;
  }
}

template <typename DESC>
__global__ __launch_bounds__(1024) void jpeg_unstuff_count(const DESC* __restrict__ imgs,
                                                           const uint8_t* __restrict__ scans,
                                                           uint2* __restrict__ tcnt, int mt) {
  const DESC& D = imgs[blockIdx.y];
  const uint32_t base = blockIdx.x * UNS_TILE;
  if (base >= D.scan_len) return;  // uniform
  uint32_t keep = 0, mkm = 0, w[4];
  if (base + threadIdx.x * 16 < D.scan_len)
    unstuff_masks(scans + D.scan_off, D.scan_len, base + threadIdx.x * 16, keep, mkm, w);
  uint32_t a = __popc(keep), r = __popc(mkm);
  for (int o = 32; o > 0; o >>= 1) {
    a += (uint32_t)__shfl_xor((int)a, o);
    r += (uint32_t)__shfl_xor((int)r, o);
  }
  __shared__ uint32_t wa[16], wr[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    wa[wv] = a;
    wr[wv] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t ta = 0, tr = 0;
    for (int k = 0; k < 16; ++k) {
      ta += wa[k];
      tr += wr[k];
    }
    tcnt[(size_t)blockIdx.y * mt + blockIdx.x] = make_uint2(ta, tr);
  }
}

template <typename DESC>
__global__ __launch_bounds__(1024) void jpeg_unstuff_write(const DESC* __restrict__ imgs,
                                                           const uint8_t* __restrict__ scans,
                                                           const uint2* __restrict__ tcnt, int mt,
                                                           uint8_t* __restrict__ ub,
                                                           uint2* __restrict__ mk) {
  const DESC& D = imgs[blockIdx.y];
  const uint32_t base = blockIdx.x * UNS_TILE;
  if (base >= D.scan_len) return;  // uniform
  __shared__ uint32_t wsum[16], wrst[16], base_s[2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // kept bytes and markers of the tiles before this one
  if (wv == 0) {
    uint32_t a = 0, r = 0;
    for (int k = lane; k < (int)blockIdx.x; k += 64) {
      const uint2 c = tcnt[(size_t)blockIdx.y * mt + k];
      a += c.x;
      r += c.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
      a += (uint32_t)__shfl_xor((int)a, o);
      r += (uint32_t)__shfl_xor((int)r, o);
    }
    if (lane == 0) {
      base_s[0] = a;
      base_s[1] = r;
    }
  }
  const uint8_t* in = scans + D.scan_off;
  const uint32_t i0 = base + threadIdx.x * 16;
  uint32_t keep = 0, mkm = 0, w[4] = {0u, 0u, 0u, 0u};
  if (i0 < D.scan_len) unstuff_masks(in, D.scan_len, i0, keep, mkm, w);
  // block-wide exclusive scans of the kept-byte and marker counts
  const uint32_t cntk = __popc(keep), nr = __popc(mkm);
  uint32_t inc = cntk, rinc = nr;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, o), q = (uint32_t)__shfl_up((int)rinc, o);
    if (lane >= o) {
      inc += t;
      rinc += q;
    }
  }
  if (lane == 63) {
    wsum[wv] = inc;
    wrst[wv] = rinc;
  }
  __syncthreads();
  uint32_t wbase = 0, rbase = 0;
  for (int k = 0; k < wv; ++k) {
    wbase += wsum[k];
    rbase += wrst[k];
  }
  uint32_t o = base_s[0] + wbase + inc - cntk;
  uint32_t orank = base_s[1] + rbase + rinc - nr;
  uint8_t* out = ub + D.ub_off;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    if (keep >> k & 1u) out[o++] = (uint8_t)b;
    // a marker: its code and the unstuffed offset where the data before it ends (the table's room
    // holds every restart marker of an intact file plus JPG_MK_EXTRA others)
    if (mkm >> k & 1u) {
      if (orank < D.mk_cap) mk[D.mk_off + orank] = make_uint2(o, b);
      ++orank;
    }
  }
}

// Per segment (one workgroup): its length, the zero padding behind it, and where each restart
// interval's data begins and ends (bits) -- as libjpeg reads them (jdhuff.c process_restart ->
// jdmarker.c read_restart_marker / jpeg_resync_to_restart).  The markers split the data into
// segments; interval 0 reads segment 0.  At each restart the marker ending the current segment is
// the expected RSTn (taken: the interval reads the next segment), or resync decides: action 1
// (the expected RST or one too far away) take it; action 2 (a marker below SOF0 or one of the two
// RSTs before the expected one) skip to the marker after the next segment and decide again;
// action 3 (any other marker, one of the next two RSTs, or none left: the data ended) leave it --
// the interval reads nothing and inherits the out-of-data state (JPG_IV_INHERIT in its end entry).
// An intact file takes the parallel fast path: marker r is RST(r mod 8).  Without restart
// intervals the data simply ends at the first marker: for the chunked decoder ublen says so.
template <typename DESC>
__global__ __launch_bounds__(256) void jpeg_unstuff_final(const DESC* __restrict__ imgs,
                                                          const uint2* __restrict__ tcnt, int mt,
                                                          uint8_t* __restrict__ ub,
                                                          const uint2* __restrict__ mk,
                                                          uint32_t* __restrict__ ivstart,
                                                          uint32_t* __restrict__ ivend,
                                                          uint32_t* __restrict__ ublen,
                                                          uint32_t* __restrict__ overflow) {
  const DESC& D = imgs[blockIdx.x];
  __shared__ uint32_t len_s, nmk_s, bad_s;
  if (threadIdx.x < 64) {
    const int ntiles = (int)((D.scan_len + UNS_TILE - 1) / UNS_TILE);
    uint32_t a = 0, r = 0;
    for (int k = threadIdx.x; k < ntiles; k += 64) {
      const uint2 c = tcnt[(size_t)blockIdx.x * mt + k];
      a += c.x;
      r += c.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
      a += (uint32_t)__shfl_xor((int)a, o);
      r += (uint32_t)__shfl_xor((int)r, o);
    }
    if (threadIdx.x == 0) {
      len_s = a;
      nmk_s = min(r, D.mk_cap);
      bad_s = 0;
      // more markers than the table holds (nintervals + JPG_MK_EXTRA: a damaged file full of
      // stray markers): the dropped ones would resynchronise differently -- the host reports it
      if (r > D.mk_cap) *overflow = 1u;
    }
  }
  __syncthreads();
  const uint32_t len = len_s, M = nmk_s, n = (uint32_t)D.nintervals;
  const uint2* m = mk + D.mk_off;
  // segment s: [start, end) bytes and the marker that ends it (after the last one: EOI)
  auto seg_start = [&](uint32_t s) { return s == 0 ? 0u : m[s - 1].x; };
  auto seg_end = [&](uint32_t s) { return s < M ? m[s].x : len; };
  auto seg_mark = [&](uint32_t s) { return s < M ? m[s].y : 0xD9u; };
  if (n == 1) {  // no restart intervals: the data ends at the first marker
    const uint32_t e = seg_end(0);
    if (threadIdx.x < 64) ub[D.ub_off + e + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
      ublen[blockIdx.x] = e;
      ivstart[D.iv_off] = 0;
      ivend[D.iv_off] = e * 8u;
    }
    return;
  }
  if (threadIdx.x < 64) ub[D.ub_off + len + threadIdx.x] = 0;
  if (threadIdx.x == 0) ublen[blockIdx.x] = len;
  // fast path: every marker is the next RSTn, no more of them than restarts
  for (uint32_t r = threadIdx.x; r < M; r += blockDim.x)
    if (m[r].y != 0xD0u + (r & 7u)) bad_s = 1;
  __syncthreads();
  if (!bad_s && M < n) {
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
      const bool has = k <= M;  // interval k reads segment k; past the data's end: nothing
      ivstart[D.iv_off + k] = has ? seg_start(k) * 8u : len * 8u;
      ivend[D.iv_off + k] = has ? seg_end(k) * 8u : len * 8u | JPG_IV_INHERIT;
    }
    return;
  }
  if (threadIdx.x != 0) return;
  // a damaged file: libjpeg's restart processing, serially
  uint32_t j = 0, want = 0;
  ivstart[D.iv_off] = 0;
  ivend[D.iv_off] = seg_end(0) * 8u;
  for (uint32_t k = 1; k < n; ++k) {
    uint32_t mc = seg_mark(j);
    int act;
    for (;;) {
      const uint32_t w0 = 0xD0u + want;
      if (mc == w0) act = 1;
      else if (mc < 0xC0u) act = 2;
      else if (mc < 0xD0u || mc > 0xD7u) act = 3;
      else if (mc == 0xD0u + ((want + 1) & 7u) || mc == 0xD0u + ((want + 2) & 7u)) act = 3;
      else if (mc == 0xD0u + ((want - 1) & 7u) || mc == 0xD0u + ((want - 2) & 7u)) act = 2;
      else act = 1;
      if (act == 2 && j < M) {
        ++j;
        mc = seg_mark(j);
        continue;
      }
      break;
    }
    want = (want + 1) & 7u;
    if (act == 1 && j < M) {
      ++j;
      ivstart[D.iv_off + k] = seg_start(j) * 8u;
      ivend[D.iv_off + k] = seg_end(j) * 8u;
    } else {
      ivstart[D.iv_off + k] = len * 8u;
      ivend[D.iv_off + k] = len * 8u | JPG_IV_INHERIT;
    }
  }
}

// Restart intervals go through the same chunked decoder: each interval is cut into its own chunks
// (its first chunk starts at the interval's known state, DC predictors 0; the others synchronise
// as a scan's do), so a file with a few long intervals is not decoded one thread per interval.
// jpeg_chunk_map_kernel (per image with restart intervals, after unstuffing): interval k gets
// max(1, ceil(bits / chunk_bits)) chunks from slot iv_ck[k] on (none if it reads nothing and
// inherits: its first MCU is its predecessor's, see jpeg_write_kernel); ck_iv[slot] names the
// interval (~0: an unused slot).  The host sized the slots for the worst case.
__global__ __launch_bounds__(256) void jpeg_chunk_map_kernel(const JpegDev* __restrict__ imgs,
                                                             const uint32_t* __restrict__ ivstart,
                                                             const uint32_t* __restrict__ ivend,
                                                             uint32_t* __restrict__ iv_ck,
                                                             uint32_t* __restrict__ ck_iv) {
  const JpegDev& D = imgs[blockIdx.x];
  if (!D.restart || D.nscan) return;  // uniform
  __shared__ uint32_t wsum[4], carry_s;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const uint32_t n = (uint32_t)D.nintervals, cb = D.chunk_bits;
  for (uint32_t k0 = 0; k0 < n; k0 += 256) {
    const uint32_t k = k0 + threadIdx.x;
    uint32_t c = 0;
    if (k < n) {
      const uint32_t ie = ivend[D.iv_off + k];
      if (!(ie & JPG_IV_INHERIT)) c = max(1u, (ie - ivstart[D.iv_off + k] + cb - 1) / cb);
    }
    uint32_t inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t off = carry_s + inc - c;
    for (int w = 0; w < wv; ++w) off += wsum[w];
    if (k < n) {
      iv_ck[D.iv_off + k] = off;
      for (uint32_t q = 0; q < c && off + q < D.nchunks; ++q) ck_iv[D.ch_off + off + q] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) carry_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  for (uint32_t t = carry_s + threadIdx.x; t < D.nchunks; t += 256) ck_iv[D.ch_off + t] = ~0u;
}

// chunk t of image D: its bit range [b0, b1), whether it starts a restart interval (or the image's
// data: a known state) and the interval k; live = false for an unused slot
struct ChunkPos {
  bool live, first;
  uint32_t k, b0, b1, end;  // end: where the interval's (or the image's) data ends
};
__device__ __forceinline__ ChunkPos jpg_chunk_pos(const JpegDev& D, uint32_t t, uint32_t nbits,
                                                  const uint32_t* __restrict__ ck_iv,
                                                  const uint32_t* __restrict__ iv_ck,
                                                  const uint32_t* __restrict__ ivstart,
                                                  const uint32_t* __restrict__ ivend) {
  ChunkPos c;
  if (!D.restart) {
    c.live = t < D.nchunks;
    c.first = t == 0;
    c.k = 0;
    c.end = nbits;
    c.b0 = min(t * D.chunk_bits, nbits);
    c.b1 = min(c.b0 + D.chunk_bits, nbits);
    return c;
  }
  c.k = t < D.nchunks ? ck_iv[D.ch_off + t] : ~0u;
  c.live = c.k != ~0u;
  if (!c.live) {
    c.first = false;
    c.b0 = c.b1 = c.end = 0;
    return c;
  }
  const uint32_t j = t - iv_ck[D.iv_off + c.k];
  c.first = j == 0;
  c.end = ivend[D.iv_off + c.k] & ~JPG_IV_INHERIT;
  c.b0 = min(ivstart[D.iv_off + c.k] + j * D.chunk_bits, c.end);
  c.b1 = min(c.b0 + D.chunk_bits, c.end);
  return c;
}

// stage 2a/2b: sync passes.  grid (max chunks per image, n).  PASS_A: start from the chunk's
// own first bit; else from the predecessor's end state in `prev` (chunk 0: the true start).
// chg_prev / chg_next: per chunk, did its end state change in the previous / this pass.  After
// the first B pass (`all`) a chunk is decoded again only if its predecessor's end state -- its
// start -- changed; otherwise its end state and counts are those of the previous pass.  Only the
// chains still converging cost anything in the later passes.
template <bool PASS_A>
__global__ __launch_bounds__(64) void jpeg_sync_kernel(const JpegDev* __restrict__ imgs,
                                                       const uint8_t* __restrict__ ub,
                                                       const uint32_t* __restrict__ ublen,
                                                       const uint64_t* __restrict__ prev,
                                                       uint64_t* __restrict__ next,
                                                       ChunkOut* __restrict__ cnt,
                                                       uint32_t* __restrict__ changed,
                                                       const uint8_t* __restrict__ chg_prev,
                                                       uint8_t* __restrict__ chg_next, int all,
                                                       uint64_t* __restrict__ ck_st,
                                                       ChunkOut* __restrict__ ck_co,
                                                       const uint32_t* __restrict__ settled,
                                                       int badlen,
                                                       const uint32_t* __restrict__ ck_iv,
                                                       const uint32_t* __restrict__ iv_ck,
                                                       const uint32_t* __restrict__ ivstart,
                                                       const uint32_t* __restrict__ ivend) {
  __shared__ JpegLds T;
  __shared__ __attribute__((aligned(16))) uint32_t ring[64 * JRING_W];
  // the previous pass of this launch round changed nothing: the decode has converged and both
  // state buffers hold the same states (that pass copied every one through), so there is nothing
  // to do -- the host queues a round of passes without reading a flag between them
  if (!PASS_A && settled && *settled == 0u) return;
  const JpegDev& D = imgs[blockIdx.y];
  if (D.nscan || blockIdx.x * 64 >= D.nchunks) return;  // uniform per workgroup
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  const uint32_t nbits = ublen[blockIdx.y] * 8u;
  const ChunkPos cp = jpg_chunk_pos(D, t, nbits, ck_iv, iv_ck, ivstart, ivend);
  bool redo = cp.live;
  if (!PASS_A && !all) {
    redo = cp.live && !cp.first && chg_prev[D.ch_off + t - 1];
    if (cp.live && !redo) {
      next[D.ch_off + t] = prev[D.ch_off + t];
      chg_next[D.ch_off + t] = 0;
    }
    if (__ballot(redo) == 0) return;  // the whole workgroup (one wave) is settled
  }
  jpg_load_tables(T, D);
  __syncthreads();
  if (!redo) return;
  const uint32_t b0 = cp.b0, b1 = cp.b1;
  const uint64_t st = PASS_A || cp.first ? jpg_state(b0, 0, 0) : prev[D.ch_off + t - 1];
  const uint32_t nsub = jpg_nsub(D.chunk_bits);
  uint64_t* cks = ck_st + (size_t)(D.ch_off + t) * nsub;
  ChunkOut* ckc = ck_co + (size_t)(D.ch_off + t) * nsub;
  ChunkOut co{0u, {0, 0, 0}};
  int pred[3] = {0, 0, 0};
  const JpgConst K = jpg_const(D);
  const rsrc_t rs = make_rsrc(ub + D.ub_off, nbits / 8u + 64u);  // past the padding: zeros
  uint64_t e = st;
  for (uint32_t j = 0; j < nsub; ++j) {
    if (!PASS_A && e == cks[j]) {
      // joined the trajectory recorded by this chunk's last decode: its end state stands, the
      // counts from here on shift by the difference at this checkpoint
      const ChunkOut old = ckc[j];
      const int32_t dn = (int32_t)(co.nblk - old.nblk);
      const int32_t d0 = co.dcsum[0] - old.dcsum[0], d1 = co.dcsum[1] - old.dcsum[1],
                    d2 = co.dcsum[2] - old.dcsum[2];
      for (uint32_t k = j; k < nsub; ++k) {
        ChunkOut c = ckc[k];
        c.nblk += (uint32_t)dn;
        c.dcsum[0] += d0;
        c.dcsum[1] += d1;
        c.dcsum[2] += d2;
        ckc[k] = c;
      }
      const ChunkOut tot = cnt[D.ch_off + t];
      co.nblk = tot.nblk + (uint32_t)dn;
      co.dcsum[0] = tot.dcsum[0] + d0;
      co.dcsum[1] = tot.dcsum[1] + d1;
      co.dcsum[2] = tot.dcsum[2] + d2;
      e = prev[D.ch_off + t];
      break;
    }
    cks[j] = e;
    ckc[j] = co;
    const uint32_t sub_end = min(b0 + (j + 1) * JPG_SUB, b1);
    // a state past the sub-chunk (the predecessor ran over it) ends where it starts
    if ((uint32_t)e < sub_end) {
      if (D.restart)  // (uniform per workgroup) the interval's end reads as zero bits
        e = jpg_run<false, false, true>(K, T, rs, ring + threadIdx.x * JRING_W, e, sub_end, &co, 0,
                                        pred, nullptr, 0xFFFFFFFFu, false, badlen, nullptr, cp.end);
      else
        e = jpg_run<false>(K, T, rs, ring + threadIdx.x * JRING_W, e, sub_end, &co, 0, pred,
                           nullptr, 0xFFFFFFFFu, false, badlen);
    }
  }
  next[D.ch_off + t] = e;
  cnt[D.ch_off + t] = co;
  if (PASS_A) {
    chg_next[D.ch_off + t] = 1;
  } else {
    const bool ch = e != prev[D.ch_off + t];
    chg_next[D.ch_off + t] = ch ? 1 : 0;
    if (ch) changed[0] = 1u;
  }
}

// stage 2c: per image, the first block index and DC predictors of every chunk
// one 256-thread workgroup per image: exclusive scan of the chunk counts (block counts and DC
// sums add), 256 chunks per round (a serial walk per image was a ~300-step latency chain),
// segmented at the chunks that start a restart interval (DC sums from 0, blocks from the
// interval's first block)
__global__ __launch_bounds__(256) void jpeg_prefix_kernel(const JpegDev* __restrict__ imgs,
                                                          const ChunkOut* __restrict__ cnt,
                                                          ChunkOut* __restrict__ start, int n,
                                                          const uint32_t* __restrict__ ck_iv,
                                                          const uint32_t* __restrict__ iv_ck) {
  const JpegDev& D = imgs[blockIdx.x];
  if (D.nscan) return;
  __shared__ int32_t sv[4][256];
  __shared__ uint8_t sf[256];
  __shared__ int32_t carry[4];
  if (threadIdx.x < 4) carry[threadIdx.x] = 0;
  for (uint32_t t0 = 0; t0 < D.nchunks; t0 += 256) {
    const uint32_t t = t0 + threadIdx.x;
    ChunkOut c{0u, {0, 0, 0}};
    bool first = t == 0;
    uint32_t k = 0;
    if (t < D.nchunks) {
      c = cnt[D.ch_off + t];
      if (D.restart) {
        k = ck_iv[D.ch_off + t];
        first = k != ~0u && iv_ck[D.iv_off + k] == t;
        if (k == ~0u) c = ChunkOut{0u, {0, 0, 0}};
      }
    }
    const int32_t v[4] = {(int32_t)c.nblk, c.dcsum[0], c.dcsum[1], c.dcsum[2]};
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) sv[q][threadIdx.x] = v[q];
    sf[threadIdx.x] = first ? 1 : 0;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // segmented Hillis-Steele inclusive scan
      int32_t u[4] = {0, 0, 0, 0};
      uint8_t fu = 0;
      if (threadIdx.x >= (unsigned)o) {
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = sv[q][threadIdx.x - o];
        fu = sf[threadIdx.x - o];
      }
      const uint8_t fo = sf[threadIdx.x];
      __syncthreads();
      if (!fo)
#pragma unroll
        for (int q = 0; q < 4; ++q) sv[q][threadIdx.x] += u[q];
      sf[threadIdx.x] = fo | fu;
      __syncthreads();
    }
    if (t < D.nchunks) {
      // exclusive = inclusive - own, plus the carry unless a segment started in this round
      const bool seg = sf[threadIdx.x] != 0;
      ChunkOut e;
      e.nblk = (uint32_t)((seg ? 0 : carry[0]) + sv[0][threadIdx.x] - v[0]);
#pragma unroll
      for (int q = 0; q < 3; ++q) e.dcsum[q] = (seg ? 0 : carry[q + 1]) + sv[q + 1][threadIdx.x] - v[q + 1];
      if (D.restart && k != ~0u) {
        // blocks from the interval's first one; the chunks before the interval's own start in
        // this round add nothing (the scan restarted at the interval's first chunk)
        e.nblk += k * (uint32_t)D.restart * (uint32_t)D.bpm;
      }
      start[D.ch_off + t] = e;
    }
    __syncthreads();
    if (threadIdx.x < 4)
      carry[threadIdx.x] = (sf[255] ? 0 : carry[threadIdx.x]) + sv[threadIdx.x][255];
    __syncthreads();
  }
}

// stage 2d: write pass.  Sub-chunks (grid.x over chunks x sub-chunks, from the final
// checkpoints) of images without restart markers and of each restart interval.
__global__ __launch_bounds__(64) void jpeg_write_kernel(const JpegDev* __restrict__ imgs,
                                                        const uint8_t* __restrict__ ub,
                                                        const uint32_t* __restrict__ ublen,
                                                        const uint32_t* __restrict__ ivstart,
                                                        const uint32_t* __restrict__ ivend,
                                                        const uint64_t* __restrict__ ck_st,
                                                        const ChunkOut* __restrict__ ck_co,
                                                        const ChunkOut* __restrict__ start,
                                                        int16_t* __restrict__ coef, int badlen,
                                                        uint32_t* __restrict__ badseen,
                                                        const uint32_t* __restrict__ ck_iv,
                                                        const uint32_t* __restrict__ iv_ck) {
  __shared__ JpegLds T;
  __shared__ __attribute__((aligned(16))) uint32_t ring[64 * JRING_W];
  const JpegDev& D = imgs[blockIdx.y];
  const uint32_t nsub = jpg_nsub(D.chunk_bits);
  const uint32_t nitems = D.nscan ? 0u : D.nchunks * nsub;
  if (blockIdx.x * 64 >= nitems) return;  // uniform per workgroup
  jpg_load_tables(T, D);
  __syncthreads();
  const uint32_t u = blockIdx.x * 64 + threadIdx.x;
  if (u >= nitems) return;
  const uint32_t nbits = ublen[blockIdx.y] * 8u;
  // sub-chunk j of chunk t from its checkpoint: state, first block, DC predictors.  badlen: the
  // bits a bad code takes.  libjpeg's is 17, but the sync passes converge a pass sooner with 16
  // (1.21 against 1.31 ms for a 600x1000 file: bad codes are frequent on the speculative
  // trajectories), so the host decodes with 16 first; the trajectories agree up to the first bad
  // code on the true one, which the write pass then reports (badseen) and the host decodes again
  // with 17 -- only files with a bad code in their data pay for the exact rule
  const uint32_t t = u / nsub, j = u - t * nsub;
  const ChunkPos cp = jpg_chunk_pos(D, t, nbits, ck_iv, iv_ck, ivstart, ivend);
  if (!cp.live) return;
  const uint32_t b1 = min(cp.b1, cp.b0 + (j + 1) * JPG_SUB);
  // the sub-chunk holding the last bit of the data (of the image, or of the restart interval), or
  // the first one without data, finishes the decode where the data ends
  const bool tail = cp.b0 < cp.end ? cp.b1 == cp.end && (cp.end - 1 - cp.b0) / JPG_SUB == j
                                    : cp.first && j == 0;
  const size_t k = (size_t)(D.ch_off + t) * nsub + j;
  const uint64_t st = ck_st[k];
  const ChunkOut c = ck_co[k], s0 = start[D.ch_off + t];
  int pred[3] = {s0.dcsum[0] + c.dcsum[0], s0.dcsum[1] + c.dcsum[1], s0.dcsum[2] + c.dcsum[2]};
  const int32_t blk = (int32_t)(s0.nblk + c.nblk) - 1;
  if ((uint32_t)st >= b1 && !tail) return;
  ChunkOut dummy{0u, {0, 0, 0}};
  JpgConst K = jpg_const(D);
  uint32_t* myring = ring + threadIdx.x * JRING_W;
  const rsrc_t rs = make_rsrc(ub + D.ub_off, nbits / 8u + 64u);
  if (!D.restart) {
    jpg_run<true>(K, T, rs, myring, st, b1, &dummy, blk, pred, coef, 0xFFFFFFFFu, tail, badlen,
                  badseen);
    return;
  }
  // a restart interval: its blocks only (the bits after its last MCU are padding)
  const uint32_t mcus = (uint32_t)(D.mcux * D.mcuy), R = (uint32_t)D.restart;
  const uint32_t bhi = min((cp.k + 1) * R, mcus) * (uint32_t)D.bpm;
  K.total_blocks = bhi;
  if (!tail) {
    jpg_run<true, false, true>(K, T, rs, myring, st, b1, &dummy, blk, pred, coef, 0xFFFFFFFFu,
                               false, badlen, badseen, cp.end);
    return;
  }
  // the interval's end: its MCUs to the last one, the bits past its data 0, an MCU decoded only if
  // the data lasted up to its start; then, if the next interval reads nothing and inherits the
  // out-of-data state and this one did not run out, libjpeg decodes the next one's first MCU from
  // zero bits
  const uint64_t e = jpg_run<true, true>(K, T, rs, myring, st, cp.end, &dummy, blk, pred, coef,
                                         bhi - (uint32_t)(blk + 1), false, badlen, badseen);
  if (cp.k + 1 < (uint32_t)D.nintervals && (ivend[D.iv_off + cp.k + 1] & JPG_IV_INHERIT) &&
      (uint32_t)e <= cp.end && bhi < mcus * (uint32_t)D.bpm) {
    int pz[3] = {0, 0, 0};
    K.total_blocks = min(bhi + R * (uint32_t)D.bpm, mcus * (uint32_t)D.bpm);
    jpg_run<true, true>(K, T, rs, myring, jpg_state(cp.end, 0, 0), cp.end, &dummy,
                        (int32_t)bhi - 1, pz, coef, (uint32_t)D.bpm, false, badlen, badseen);
  }
}

// ---- launchers -------------------------------------------------------------------------------------
template <typename DESC>
static void jpeg_unstuff(const JpegCall& C, const DESC* descs, unsigned nd, int mt,
                         uint32_t* ublen, uint32_t* overflow) {
  const dim3 g((unsigned)mt, nd);
  hipLaunchKernelGGL(jpeg_unstuff_count<DESC>, g, dim3(1024), 0, C.st, descs, C.scan, C.tcnt, mt);
  hipLaunchKernelGGL(jpeg_unstuff_write<DESC>, g, dim3(1024), 0, C.st, descs, C.scan, C.tcnt, mt,
                     C.ub, C.mk);
  hipLaunchKernelGGL(jpeg_unstuff_final<DESC>, dim3(nd), dim3(256), 0, C.st, descs, C.tcnt, mt,
                     C.ub, C.mk, C.ivs, C.ive, ublen, overflow);
}
void jpeg_unstuff_images(const JpegCall& C, int mt, uint32_t* overflow) {
  jpeg_unstuff(C, C.imgs, (unsigned)C.n, mt, C.ublen, overflow);
}
void jpeg_unstuff_scans(const JpegCall& C, unsigned ns, int mt, uint32_t* overflow) {
  jpeg_unstuff(C, C.scans, ns, mt, C.ublen_s, overflow);
}

void jpeg_chunk_map(const JpegCall& C) {
  hipLaunchKernelGGL(jpeg_chunk_map_kernel, dim3(C.n), dim3(256), 0, C.st, C.imgs, C.ivs, C.ive,
                     C.iv_ck, C.ck_iv);
}

void jpeg_sync_a(const JpegCall& C, uint32_t max_items, int badlen) {
  hipLaunchKernelGGL(jpeg_sync_kernel<true>, dim3((max_items + 63) / 64, C.n), dim3(64), 0, C.st,
                     C.imgs, C.ub, C.ublen, C.S[1], C.S[0], C.cnt, C.flag, C.chg[1], C.chg[0], 1,
                     C.ck_st, C.ck_co, nullptr, badlen, C.ck_iv, C.iv_ck, C.ivs, C.ive);
}

void jpeg_sync_b(const JpegCall& C, uint32_t max_items, int cur, uint32_t* changed, int all,
                 const uint32_t* settled, int badlen) {
  hipLaunchKernelGGL(jpeg_sync_kernel<false>, dim3((max_items + 63) / 64, C.n), dim3(64), 0, C.st,
                     C.imgs, C.ub, C.ublen, C.S[cur], C.S[cur ^ 1], C.cnt, changed, C.chg[cur],
                     C.chg[cur ^ 1], all, C.ck_st, C.ck_co, settled, badlen, C.ck_iv, C.iv_ck,
                     C.ivs, C.ive);
}

void jpeg_prefix(const JpegCall& C) {
  hipLaunchKernelGGL(jpeg_prefix_kernel, dim3(C.n), dim3(256), 0, C.st, C.imgs, C.cnt, C.start,
                     C.n, C.ck_iv, C.iv_ck);
}

void jpeg_write(const JpegCall& C, uint32_t max_items_w, int badlen, uint32_t* badseen) {
  hipLaunchKernelGGL(jpeg_write_kernel, dim3((max_items_w + 63) / 64, C.n), dim3(64), 0, C.st,
                     C.imgs, C.ub, C.ublen, C.ivs, C.ive, C.ck_st, C.ck_co, C.start, C.coef, badlen,
                     badseen, C.ck_iv, C.iv_ck);
}

}  // namespace idn
