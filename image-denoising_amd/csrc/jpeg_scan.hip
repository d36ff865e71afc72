// JPEG decoder, the scan path (jpeg.hip has the map of the units): progressive, multi-scan,
// arithmetic-coded and 4-component files, one wave per image walking the scans in file order --
// jpeg_prog_kernel (jdhuff.c's sequential and progressive decoders, restated) and jpeg_arith_kernel
// (jdarith.c's QM-coder, restated).
// This software is based in part on the work of the Independent JPEG Group.
#include "jpeg_device.hpp"

namespace idn {

// reads one restart interval of a plain big-endian bit string through a range-checked buffer
// resource, through a per-lane ring of JRG_S byte-swapped 16-byte groups in LDS refilled one group
// ahead from a load held in a register (as the chunk decoders' jpg_run): a register queue of
// groups in flight made every group change wait for the youngest load (moving a register whose
// load is pending waits for it).  Bits from `end` on read as 0 (jdhuff.c jpeg_fill_bit_buffer past
// a marker); `pos` counts the bits taken, so pos > end says the data ran out (insufficient_data).
constexpr int JRG_S = 4;
constexpr int JRING_S = JRG_S * 4 + 4;  // ring words per lane (a pad group)
struct BitStream {
  rsrc_t rs;
  uint32_t* ring;
  uint64_t acc;    // left-aligned
  int nb;
  uint32_t wi, pos, end;  // wi: the next word to append
  v4u pend;               // group (wi >> 2) + JRG_S, raw
  __device__ __forceinline__ void put(uint32_t g, const v4u v) {
    *reinterpret_cast<v4u*>(ring + (g & (JRG_S - 1)) * 4) =
        v4u{__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z),
            __builtin_bswap32(v.w)};
  }
  __device__ __forceinline__ uint32_t word() {
    uint32_t w = ring[wi & (4 * JRG_S - 1)];
    const uint32_t wbit = wi * 32u;  // (bit positions are below 2^31: 32-bit arithmetic)
    w = wbit + 32u <= end ? w : wbit >= end ? 0u : w & ~(0xFFFFFFFFu >> (end - wbit));
    if ((++wi & 3) == 0) {  // group (wi >> 2) - 1 retired: its slot takes the pending group
      put((wi >> 2) + JRG_S - 1, pend);
      pend = __builtin_amdgcn_raw_buffer_load_b128(rs, ((wi >> 2) + JRG_S) * 16u, 0, 0);
    }
    return w;
  }
  __device__ __forceinline__ void start(rsrc_t r, uint32_t* rg, uint32_t p, uint32_t e) {
    rs = r;
    ring = rg;
    end = e;
    pos = p;
    wi = p >> 5;
    const uint32_t g0 = wi >> 2;
#pragma unroll
    for (int k = 0; k < JRG_S; ++k)
      put(g0 + k, __builtin_amdgcn_raw_buffer_load_b128(rs, (g0 + k) * 16u, 0, 0));
    pend = __builtin_amdgcn_raw_buffer_load_b128(rs, (g0 + JRG_S) * 16u, 0, 0);
    const uint32_t w0 = word(), w1 = word();
    acc = ((uint64_t)w0 << 32 | w1) << (p & 31);
    nb = 64 - (int)(p & 31);
  }
  __device__ __forceinline__ void refill() {
    if (nb < 32) {
      acc |= (uint64_t)word() << (32 - nb);
      nb += 32;
    }
  }
  __device__ __forceinline__ uint32_t bits(int s) {
    const uint32_t r = s ? (uint32_t)(acc >> (64 - s)) : 0u;
    acc <<= s;
    nb -= s;
    pos += (uint32_t)s;
    return r;
  }
};

// the scan path's tables (JpegScanDev slots)
struct JpegLdsScan {
  alignas(16) int32_t mca[8][8];
  uint8_t natural[80];  // jpg_natural: a __constant__ read at a computed index is a vector load
  uint16_t lut[8][1 << JPG_LUTB];
  int32_t maxcode[8][18], valoff[8][18];
  uint8_t huffval[8][256];
};

// ---- device: the scan path (progressive / multi-scan files) --------------------------------------
// jdhuff.c's decode_mcu (sequential), decode_mcu_DC_first / _AC_first / _DC_refine / _AC_refine
// (progressive: spectral selection, successive approximation, EOB runs), restated.  One wave per
// image walks the image's scans in file order (a refinement scan reads what the earlier scans
// left in the coefficient blocks); within a scan the lanes take the restart intervals (without
// restart markers lane 0 decodes the scan).  Throughput is not the goal of this path: it makes
// cv2.imread's progressive files decodable bit-exactly (the parallel path is the baseline one).
__device__ __forceinline__ void jpg_load_scan_tables(JpegLdsScan& T, const JpegScanDev& S) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&S.lut[0][0]);
  uint32_t* d = reinterpret_cast<uint32_t*>(&T.lut[0][0]);
  for (int k = threadIdx.x; k < (int)(sizeof(T.lut) / 4); k += blockDim.x) d[k] = s[k];
  for (int k = threadIdx.x; k < 8 * 18; k += blockDim.x) {
    (&T.maxcode[0][0])[k] = (&S.maxcode[0][0])[k];
    (&T.valoff[0][0])[k] = (&S.valoff[0][0])[k];
  }
  for (int k = threadIdx.x; k < 8 * 256; k += blockDim.x) (&T.huffval[0][0])[k] = (&S.huffval[0][0])[k];
  for (int k = threadIdx.x; k < 8 * 8; k += blockDim.x) T.mca[k >> 3][k & 7] = jpg_mca(S.maxcode[k >> 3], k & 7);
  for (int k = threadIdx.x; k < 80; k += blockDim.x) T.natural[k] = jpg_natural[k];
}

__device__ __forceinline__ uint32_t jpg_get(BitStream& br, int s) {  // s <= 16
  br.refill();
  return br.bits(s);
}
__device__ __forceinline__ int jpg_huff(BitStream& br, const JpegLdsScan& T, int t) {
  br.refill();
  int len;
  const int sym = jpg_decode(br.acc, T, t, &len);
  br.bits(len);
  return sym;
}
__device__ __forceinline__ int16_t jpg_lshift(int v, int al) { return (int16_t)(int)((uint32_t)v << al); }

// one block of scan component k (slot k: DC table, 4 + k: AC table); eobrun / pred per interval
template <typename SK>
__device__ __forceinline__ void jpg_scan_block(BitStream& br, const JpegLdsScan& T, const SK& S,
                                               int k, int16_t* __restrict__ blk, int& pred,
                                               uint32_t& eobrun) {
  switch (S.kind) {
    case JPG_SEQ: {
      const int s = jpg_huff(br, T, k);
      pred += s ? jpg_extend(jpg_get(br, s), s) : 0;
      blk[0] = (int16_t)pred;
      for (int z = 1; z < 64;) {
        const int rs = jpg_huff(br, T, 4 + k);
        const int r = rs >> 4, sz = rs & 15;
        if (sz) {
          z += r;
          blk[T.natural[min(z, 79)]] = (int16_t)jpg_extend(jpg_get(br, sz), sz);
          ++z;
        } else if (r == 15) {
          z += 16;
        } else {
          break;
        }
      }
      break;
    }
    case JPG_DC_FIRST: {
      const int s = jpg_huff(br, T, k);
      pred += s ? jpg_extend(jpg_get(br, s), s) : 0;
      blk[0] = jpg_lshift(pred, S.Al);
      break;
    }
    case JPG_DC_REFINE:  // OR the bit into the low half of the block's first dword: no load to
                         // wait for (blk is 128-byte aligned, Al <= 13)
      if (jpg_get(br, 1)) atomicOr(reinterpret_cast<unsigned int*>(blk), 1u << S.Al);
      break;
    case JPG_AC_FIRST: {
      if (eobrun) {
        --eobrun;
        break;
      }
      for (int z = S.Ss; z <= S.Se; ++z) {
        const int rs = jpg_huff(br, T, 4);
        const int r = rs >> 4, sz = rs & 15;
        if (sz) {
          z += r;
          blk[T.natural[min(z, 79)]] = jpg_lshift(jpg_extend(jpg_get(br, sz), sz), S.Al);
        } else if (r != 15) {
          eobrun = 1u << r;
          if (r) eobrun += jpg_get(br, r);
          --eobrun;
          break;
        } else {
          z += 15;
        }
      }
      break;
    }
    default: {  // JPG_AC_REFINE
      const int p1 = 1 << S.Al, m1 = -(1 << S.Al);
      int z = S.Ss;
      if (eobrun == 0) {
        for (; z <= S.Se; ++z) {
          const int rs = jpg_huff(br, T, 4);
          int r = rs >> 4, sz = rs & 15;
          if (sz) {
            sz = jpg_get(br, 1) ? p1 : m1;
          } else if (r != 15) {
            eobrun = 1u << r;
            if (r) eobrun += jpg_get(br, r);
            break;
          }
          do {  // refine the nonzero coefficients up to the target zero (r zeros skipped)
            int16_t* c = blk + T.natural[min(z, 79)];
            if (*c != 0) {
              if (jpg_get(br, 1) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c + m1);
            } else if (--r < 0) {
              break;
            }
            ++z;
          } while (z <= S.Se);
          if (sz) blk[T.natural[min(z, 79)]] = (int16_t)sz;
        }
      }
      if (eobrun > 0) {  // the band of this block is in an EOB run: refine its nonzeros
        for (; z <= S.Se; ++z) {
          int16_t* c = blk + T.natural[min(z, 79)];
          if (*c != 0 && jpg_get(br, 1) && (*c & p1) == 0) *c = (int16_t)(*c >= 0 ? *c + p1 : *c + m1);
        }
        --eobrun;
      }
    }
  }
}

// a scan's constants, read once per scan: inside the unit loop a read of JpegDev / JpegScanDev
// (component fields at a computed index) was a vector load waited for at every unit
struct ScanK {
  int kind, Ss, Se, Al, ns;
  uint32_t mcux;
  uint32_t wib[4], bw[4], cv[4], ch[4];  // per scan component k
  uint64_t boff[4];                      // its first block
};
__device__ __forceinline__ ScanK jpg_scan_k(const JpegDev& D, const JpegScanDev& S) {
  ScanK K;
  K.kind = S.kind;
  K.Ss = S.Ss;
  K.Se = S.Se;
  K.Al = S.Al;
  K.ns = S.ns;
  K.mcux = (uint32_t)D.mcux;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = k < S.ns ? S.comp[k] : 0;
    K.wib[k] = (uint32_t)D.wib[c];
    K.bw[k] = (uint32_t)D.bw[c];
    K.cv[k] = (uint32_t)D.cv[c];
    K.ch[k] = (uint32_t)D.ch[c];
    K.boff[k] = D.blk_off[c];
  }
  return K;
}
template <typename A>
__device__ __forceinline__ A jpg_pick(const A (&a)[4], int k) {  // (no dynamic register index)
  return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3];
}

// the scan path's unit u of scan S: an MCU (interleaved) or one block of the scan's component
__device__ __forceinline__ void jpg_scan_unit(BitStream& br, const JpegLdsScan& T, const ScanK& S,
                                              uint32_t u, int16_t* __restrict__ coef,
                                              int (&pred)[4], uint32_t& eobrun) {
  if (S.ns == 1) {  // non-interleaved: the component's own blocks, raster order
    const uint32_t by = u / S.wib[0], bx = u - by * S.wib[0];
    int16_t* blk = coef + (S.boff[0] + (uint64_t)by * S.bw[0] + bx) * 64;
    jpg_scan_block(br, T, S, 0, blk, pred[0], eobrun);
  } else {  // interleaved MCU (sequential, or a progressive DC scan)
    const uint32_t my = u / S.mcux, mx = u - my * S.mcux;
    for (int k = 0; k < S.ns; ++k) {
      const uint32_t cv = jpg_pick(S.cv, k), ch = jpg_pick(S.ch, k), bw = jpg_pick(S.bw, k);
      const uint64_t bo = jpg_pick(S.boff, k);
      for (uint32_t dv = 0; dv < cv; ++dv)
        for (uint32_t dh = 0; dh < ch; ++dh) {
          const uint64_t by = (uint64_t)my * cv + dv, bx = (uint64_t)mx * ch + dh;
          jpg_scan_block(br, T, S, k, coef + (bo + by * bw + bx) * 64, pred[k], eobrun);
        }
    }
  }
}

// One block of an AC refinement scan (jdhuff.c decode_mcu_AC_refine) from its nonzero history h
// (zigzag positions in the band Ss..Se, before this scan) alone: what the decoder reads never
// depends on the coefficient values, only on which are nonzero, and a new coefficient is never
// passed again in its block.  Every history position of the band gets one correction bit, in
// zigzag order (corr: the K = popcount(h) bits, the first read highest); newp / newn: the
// positions that become +-2^Al (newn: negative).  libjpeg's overrun guard writes a value past
// position 63 at 63.  The caller applies it.
struct RefineOut {
  uint64_t corr, newp, newn;
};
__device__ __forceinline__ void jpg_refine_block(BitStream& br, const JpegLdsScan& T, int Ss, int Se,
                                                 uint64_t h, uint32_t& eobrun, RefineOut& out) {
  uint64_t corr = 0, newp = 0, newn = 0;
  auto take = [&](uint64_t nz) {  // the correction bits of the history positions in nz
    for (int k = __popcll(nz); k > 0;) {
      const int s = min(k, 24);
      corr = corr << s | jpg_get(br, s);
      k -= s;
    }
  };
  int z = Ss;
  if (eobrun == 0) {
    while (z <= Se) {
      const int rs = jpg_huff(br, T, 4);
      const int r = rs >> 4, sz = rs & 15;
      bool neg = false;
      if (sz) {
        neg = jpg_get(br, 1) == 0;
      } else if (r != 15) {
        eobrun = 1u << r;
        if (r) eobrun += jpg_get(br, r);
        break;
      }
      // the (r + 1)-th position without history from z on (Se + 1 if the band runs out first)
      uint64_t zs = ~h & (~0ull << z) & (Se == 63 ? ~0ull : (1ull << (Se + 1)) - 1);
      for (int i = 0; i < r && zs; ++i) zs &= zs - 1;
      const int t = zs ? __builtin_ctzll(zs) : Se + 1;
      take(h & (~0ull << z) & (t >= 64 ? ~0ull : (1ull << t) - 1));
      if (sz) {
        const int zt = min(t, 63);
        newp |= 1ull << zt;
        newn |= (uint64_t)neg << zt;
      }
      z = t + 1;
    }
  }
  if (eobrun > 0) {
    if (z <= Se) take(h & (~0ull << z));
    --eobrun;
  }
  out = RefineOut{corr, newp, newn};
}

// Out of data (jdhuff.c insufficient_data): a unit is decoded only while the interval's data lasted
// up to its start (a skipped unit keeps what the earlier scans left); an interval that reads
// nothing and inherits the out-of-data state is the predecessor's lane's: it decodes the first unit
// from zero bits if the predecessor did not run out (see jpeg_unstuff_final).
// A non-interleaved scan without restart intervals (every AC scan) decodes on one lane into blocks
// the wave stages JPG_PT at a time in LDS (loaded, decoded into, written back): an AC refinement
// read every block's earlier coefficients as it went, a dependent HBM round trip each, and on gfx9
// the bit reader's waits for its loads (vmcnt) also waited for every coefficient store before.
constexpr uint32_t JPG_PT = 256;
__global__ __launch_bounds__(64) void jpeg_prog_kernel(const JpegDev* __restrict__ imgs,
                                                       const JpegScanDev* __restrict__ scans,
                                                       const uint8_t* __restrict__ ub,
                                                       const uint32_t* __restrict__ ivstart,
                                                       const uint32_t* __restrict__ ivend,
                                                       const uint32_t* __restrict__ ublen_s,
                                                       int16_t* __restrict__ coef) {
  __shared__ JpegLdsScan T;
  __shared__ uint4 tile[JPG_PT * 8];  // JPG_PT blocks of 64 coefficients
  __shared__ uint64_t ref_hist[JPG_PT];
  __shared__ RefineOut ref_out[JPG_PT];
  __shared__ __attribute__((aligned(16))) uint32_t bring[64 * JRING_S];
  uint32_t* myring = bring + threadIdx.x * JRING_S;
  const JpegDev& D = imgs[blockIdx.x];
  const uint32_t nscan = D.nscan;
  if (nscan == 0 || D.arith) return;  // uniform: a parallel-path or arithmetic-coded image
  for (uint32_t si = 0; si < nscan; ++si) {
    const JpegScanDev& S = scans[D.scan0 + si];
    // the previous scan's coefficient stores visible to every lane, its table reads done
    __threadfence();
    __syncthreads();
    jpg_load_scan_tables(T, S);
    __syncthreads();
    const rsrc_t rs = make_rsrc(ub + S.ub_off, ublen_s[D.scan0 + si] + 64u);
    const ScanK K = jpg_scan_k(D, S);
    if (S.ns == 1 && S.nintervals == 1) {  // (interval 0 never inherits)
      const uint32_t ie = ivend[S.iv_off];
      const int c = S.comp[0];
      const uint32_t wib = (uint32_t)D.wib[c], bw = (uint32_t)D.bw[c];
      int16_t* cb = coef + D.blk_off[c] * 64;
      const uint64_t band = (S.Se == 63 ? ~0ull : (1ull << (S.Se + 1)) - 1) & (~0ull << S.Ss);
      const int p1 = 1 << S.Al, m1 = -(1 << S.Al);
      const bool refine = S.kind == JPG_AC_REFINE;
      BitStream br;
      if (threadIdx.x == 0) br.start(rs, myring, ivstart[S.iv_off], ie);
      uint32_t eobrun = 0;
      int pred = 0;
      for (uint32_t t0 = 0; t0 < S.nunits; t0 += JPG_PT) {
        const uint32_t nt = min(JPG_PT, S.nunits - t0);
        // 16-byte piece k of the tile: part k % 8 of its block k / 8
        for (uint32_t k = threadIdx.x; k < nt * 8; k += 64) {
          const uint32_t u = t0 + k / 8, by = u / wib, bx = u - by * wib;
          tile[k] = reinterpret_cast<const uint4*>(cb + ((uint64_t)by * bw + bx) * 64)[k % 8];
        }
        __syncthreads();
        if (!refine) {  // the other kinds read nothing back: the blocks in LDS, one lane
          if (threadIdx.x == 0)
            for (uint32_t u = 0; u < nt && br.pos <= ie; ++u)
              jpg_scan_block(br, T, K, 0, reinterpret_cast<int16_t*>(tile + 8 * u), pred, eobrun);
        }
        const int16_t* tb = reinterpret_cast<const int16_t*>(tile);
        for (uint32_t u = threadIdx.x; u < nt && refine; u += 64) {  // nonzero history, zigzag
          uint64_t h = 0;
          for (int zz = 0; zz < 64; ++zz) h |= (uint64_t)(tb[u * 64 + T.natural[zz]] != 0) << zz;
          ref_hist[u] = h & band;
        }
        __syncthreads();
        if (threadIdx.x == 0 && refine) {
          uint32_t u = 0;
          for (; u < nt && br.pos <= ie; ++u)
            jpg_refine_block(br, T, S.Ss, S.Se, ref_hist[u], eobrun, ref_out[u]);
          for (; u < nt; ++u) ref_out[u] = RefineOut{0ull, 0ull, 0ull};  // out of data: unchanged
        }
        __syncthreads();
        for (uint32_t u = threadIdx.x; u < nt && refine; u += 64) {  // corrections, then new ones
          int16_t* blk = reinterpret_cast<int16_t*>(tile + 8 * u);
          const RefineOut o = ref_out[u];
          uint64_t h = ref_hist[u];
          for (int j = __popcll(h) - 1; h; h &= h - 1, --j) {
            if (!((o.corr >> j) & 1u)) continue;
            int16_t* cp = blk + T.natural[__builtin_ctzll(h)];
            if ((*cp & p1) == 0) *cp = (int16_t)(*cp >= 0 ? *cp + p1 : *cp + m1);
          }
          for (uint64_t nw = o.newp; nw; nw &= nw - 1) {
            const int zz = __builtin_ctzll(nw);
            blk[T.natural[zz]] = (int16_t)((o.newn >> zz) & 1u ? m1 : p1);
          }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nt * 8; k += 64) {
          const uint32_t u = t0 + k / 8, by = u / wib, bx = u - by * wib;
          reinterpret_cast<uint4*>(cb + ((uint64_t)by * bw + bx) * 64)[k % 8] = tile[k];
        }
        __syncthreads();
      }
      continue;
    }
    for (int t = threadIdx.x; t < S.nintervals; t += 64) {
      const uint32_t ie = ivend[S.iv_off + t];
      if (ie & JPG_IV_INHERIT) continue;
      const uint32_t u0 = S.restart ? (uint32_t)t * (uint32_t)S.restart : 0u;
      const uint32_t u1 = S.restart ? min(u0 + (uint32_t)S.restart, S.nunits) : S.nunits;
      BitStream br;
      br.start(rs, myring, ivstart[S.iv_off + t], ie);
      int pred[4] = {0, 0, 0, 0};
      uint32_t eobrun = 0;
      for (uint32_t u = u0; u < u1 && br.pos <= ie; ++u) jpg_scan_unit(br, T, K, u, coef, pred, eobrun);
      if (t + 1 < S.nintervals && (ivend[S.iv_off + t + 1] & JPG_IV_INHERIT) && br.pos <= ie &&
          u1 < S.nunits) {
        int pz[4] = {0, 0, 0, 0};
        uint32_t ez = 0;
        br.start(rs, myring, ie, ie);
        jpg_scan_unit(br, T, K, u1, coef, pz, ez);
      }
    }
  }
}

// ---- device: arithmetic-coded scans (jdarith.c, libjpeg 9d) ------------------------------------
// The QM-coder (ITU-T T.81 Annex D) over each restart interval's unstuffed bytes, with libjpeg's
// statistics per table (DC: 64 bins, AC: 256) reset at every interval, the DC conditioning of
// the DAC parameters (L, U) and the AC split K, restated: decode_mcu (sequential) and
// decode_mcu_DC_first / _AC_first / _DC_refine / _AC_refine.  The structure is the scan path's:
// one wave per image, scans in file order, lanes over restart intervals (one lane without them:
// an arithmetic-coded file decodes serially -- correct, not fast; such files are rare).
#include "jpeg_aritab.inc"  // jpg_aritab[114]: T.81 Table D.2 + the fixed 0.5 state 113

constexpr int JAR_DC = 64, JAR_AC = 256, JAR_LANE = 4 * JAR_DC + 4 * JAR_AC;  // stats bytes per lane

struct ArithDec {
  const uint8_t* p;
  uint32_t i, end;  // byte cursor and the interval's end (past it libjpeg reads 0)
  long long c;      // libjpeg's INT32 registers (long)
  int a, ct;
  bool bad;         // JWRN_ARITH_BAD_CODE: the rest of the interval decodes nothing
};

__device__ __forceinline__ int jar_decode(ArithDec& e, uint8_t* st) {
  while (e.a < 0x8000) {  // renormalisation and data input (D.2.6)
    if (--e.ct < 0) {
      const int data = e.i < e.end ? (int)e.p[e.i] : 0;
      ++e.i;
      e.c = (e.c << 8) | data;
      if ((e.ct += 8) < 0 && ++e.ct == 0) e.a = 0x8000;  // 2 initial bytes: a = 0x10000 below
    }
    e.a <<= 1;
  }
  int sv = *st;
  const uint32_t qv = jpg_aritab[sv & 0x7F];
  const int nl = (int)(qv & 0xFF), nm = (int)((qv >> 8) & 0xFF), qe = (int)(qv >> 16);
  const int temp = e.a - qe;
  e.a = temp;
  const long long t2 = (long long)temp << e.ct;
  if (e.c >= t2) {  // LPS path, with the conditional exchange (D.2.4 / D.2.5)
    e.c -= t2;
    if (e.a < qe) {
      e.a = qe;
      *st = (uint8_t)((sv & 0x80) ^ nm);
    } else {
      e.a = qe;
      *st = (uint8_t)((sv & 0x80) ^ nl);
      sv ^= 0x80;
    }
  } else if (e.a < 0x8000) {  // MPS path, conditional exchange
    if (e.a < qe) {
      *st = (uint8_t)((sv & 0x80) ^ nl);
      sv ^= 0x80;
    } else {
      *st = (uint8_t)((sv & 0x80) ^ nm);
    }
  }
  return sv >> 7;
}

// a DC difference (Figures F.19, F.21-F.24), updating the component's conditioning ctx
__device__ int jar_dc_diff(ArithDec& e, uint8_t* dcs, int& ctx, int L, int U) {
  uint8_t* st = dcs + ctx;
  if (jar_decode(e, st) == 0) {
    ctx = 0;
    return 0;
  }
  const int sign = jar_decode(e, st + 1);
  st += 2 + sign;
  int m = jar_decode(e, st);
  if (m) {
    st = dcs + 20;  // X1
    while (jar_decode(e, st)) {
      if ((m <<= 1) == 0x8000) {
        e.bad = true;
        return 0;
      }
      ++st;
    }
  }
  if (m < ((1 << L) >> 1)) ctx = 0;
  else if (m > ((1 << U) >> 1)) ctx = 12 + sign * 4;
  else ctx = 4 + sign * 4;
  int v = m;
  st += 14;
  while (m >>= 1)
    if (jar_decode(e, st)) v |= m;
  v += 1;
  return sign ? -v : v;
}

// an AC coefficient's value once its position k is known (st: the bins of its run, 3 (k - 1))
__device__ int jar_ac_value(ArithDec& e, uint8_t* acs, uint8_t* st, int k, int K, uint8_t* fixed) {
  const int sign = jar_decode(e, fixed);
  st += 2;
  int m = jar_decode(e, st);
  if (m && jar_decode(e, st)) {
    m <<= 1;
    st = acs + (k <= K ? 189 : 217);
    while (jar_decode(e, st)) {
      if ((m <<= 1) == 0x8000) {
        e.bad = true;
        return 0;
      }
      ++st;
    }
  }
  int v = m;
  st += 14;
  while (m >>= 1)
    if (jar_decode(e, st)) v |= m;
  v += 1;
  return sign ? -v : v;
}

// one block of scan component k
__device__ void jar_block(ArithDec& e, const JpegScanDev& S, int k, uint8_t* dcs, uint8_t* acs,
                          uint8_t* fixed, int16_t* __restrict__ blk, int& last, int& ctx,
                          const uint8_t* nat) {
  const bool prog = S.kind != JPG_SEQ;
  if (S.kind == JPG_SEQ || S.kind == JPG_DC_FIRST) {
    last += jar_dc_diff(e, dcs, ctx, S.aL[k], S.aU[k]);
    if (e.bad) return;
    blk[0] = jpg_lshift(last, prog ? S.Al : 0);
    if (prog) return;
    int z = 0;  // sequential: AC 1..63
    while (z < 63) {
      uint8_t* st = acs + 3 * z;
      if (jar_decode(e, st)) break;  // EOB
      for (;;) {
        ++z;
        if (jar_decode(e, st + 1)) break;
        st += 3;
        if (z >= 63) {
          e.bad = true;
          return;
        }
      }
      const int v = jar_ac_value(e, acs, st, z, S.aK[k], fixed);
      if (e.bad) return;
      blk[nat[z]] = (int16_t)v;
    }
  } else if (S.kind == JPG_DC_REFINE) {
    if (jar_decode(e, fixed)) blk[0] = (int16_t)(blk[0] | (1 << S.Al));
  } else if (S.kind == JPG_AC_FIRST) {
    int z = S.Ss - 1;
    while (z < S.Se) {
      uint8_t* st = acs + 3 * z;
      if (jar_decode(e, st)) break;
      for (;;) {
        ++z;
        if (jar_decode(e, st + 1)) break;
        st += 3;
        if (z >= S.Se) {
          e.bad = true;
          return;
        }
      }
      const int v = jar_ac_value(e, acs, st, z, S.aK[k], fixed);
      if (e.bad) return;
      blk[nat[z]] = jpg_lshift(v, S.Al);
    }
  } else {  // AC refine
    const int p1 = 1 << S.Al, m1 = -(1 << S.Al);
    int kex = S.Se;  // the previous stage's end of block
    while (kex > 0 && blk[nat[kex]] == 0) --kex;
    int z = S.Ss - 1;
    while (z < S.Se) {
      uint8_t* st = acs + 3 * z;
      if (z >= kex && jar_decode(e, st)) break;
      for (;;) {
        int16_t* c = blk + nat[++z];
        if (*c) {  // previously nonzero: a correction bit
          if (jar_decode(e, st + 2)) *c = (int16_t)(*c < 0 ? *c + m1 : *c + p1);
          break;
        }
        if (jar_decode(e, st + 1)) {  // newly nonzero
          *c = (int16_t)(jar_decode(e, fixed) ? m1 : p1);
          break;
        }
        st += 3;
        if (z >= S.Se) {
          e.bad = true;
          return;
        }
      }
    }
  }
}

__global__ __launch_bounds__(64) void jpeg_arith_kernel(const JpegDev* __restrict__ imgs,
                                                        const JpegScanDev* __restrict__ scans,
                                                        const uint8_t* __restrict__ ub,
                                                        const uint32_t* __restrict__ ivstart,
                                                        const uint32_t* __restrict__ ivend,
                                                        int16_t* __restrict__ coef) {
  __shared__ uint8_t stats[64 * JAR_LANE];
  __shared__ uint8_t nat[80];  // jpg_natural in LDS
  for (int k = threadIdx.x; k < 80; k += 64) nat[k] = jpg_natural[k];
  const JpegDev& D = imgs[blockIdx.x];
  const uint32_t nscan = D.nscan;
  if (nscan == 0 || !D.arith) return;  // uniform
  uint8_t* mine = stats + threadIdx.x * JAR_LANE;
  for (uint32_t si = 0; si < nscan; ++si) {
    const JpegScanDev& S = scans[D.scan0 + si];
    // the previous scan's coefficient stores visible to every lane
    __threadfence();
    __syncthreads();
    for (int t = threadIdx.x; t < S.nintervals; t += 64) {
      const uint32_t u0 = S.restart ? (uint32_t)t * (uint32_t)S.restart : 0u;
      const uint32_t u1 = S.restart ? min(u0 + (uint32_t)S.restart, S.nunits) : S.nunits;
      for (int k = 0; k < JAR_LANE; k += 16) *reinterpret_cast<uint4*>(mine + k) = make_uint4(0, 0, 0, 0);
      ArithDec e;
      e.p = ub + S.ub_off;
      // (jdarith.c has no out-of-data state: past its data an interval decodes zeros)
      e.i = ivstart[S.iv_off + t] >> 3;
      e.end = (ivend[S.iv_off + t] & ~JPG_IV_INHERIT) >> 3;
      e.c = 0;
      e.a = 0;
      e.ct = -16;
      e.bad = false;
      uint8_t fixed = 113;
      int last[4] = {0, 0, 0, 0}, ctx[4] = {0, 0, 0, 0};
      for (uint32_t u = u0; u < u1 && !e.bad; ++u) {
        if (S.ns == 1) {
          const int c = S.comp[0];
          const uint32_t by = u / (uint32_t)D.wib[c], bx = u - by * (uint32_t)D.wib[c];
          int16_t* blk = coef + (D.blk_off[c] + (uint64_t)by * D.bw[c] + bx) * 64;
          jar_block(e, S, 0, mine + S.td[0] * JAR_DC, mine + 4 * JAR_DC + S.ta[0] * JAR_AC, &fixed,
                    blk, last[0], ctx[0], nat);
        } else {
          const uint32_t my = u / (uint32_t)D.mcux, mx = u - my * (uint32_t)D.mcux;
          for (int k = 0; k < S.ns && !e.bad; ++k) {
            const int c = S.comp[k];
            for (int dv = 0; dv < D.cv[c]; ++dv)
              for (int dh = 0; dh < D.ch[c] && !e.bad; ++dh) {
                const uint64_t by = (uint64_t)my * D.cv[c] + dv, bx = (uint64_t)mx * D.ch[c] + dh;
                int16_t* blk = coef + (D.blk_off[c] + by * D.bw[c] + bx) * 64;
                jar_block(e, S, k, mine + S.td[k] * JAR_DC, mine + 4 * JAR_DC + S.ta[k] * JAR_AC,
                          &fixed, blk, last[k], ctx[k], nat);
              }
          }
        }
      }
    }
  }
}

// ---- launchers -------------------------------------------------------------------------------------
void jpeg_prog(const JpegCall& C) {
  hipLaunchKernelGGL(jpeg_prog_kernel, dim3(C.n), dim3(64), 0, C.st, C.imgs, C.scans, C.ub, C.ivs,
                     C.ive, C.ublen_s, C.coef);
}

void jpeg_arith(const JpegCall& C) {
  hipLaunchKernelGGL(jpeg_arith_kernel, dim3(C.n), dim3(64), 0, C.st, C.imgs, C.scans, C.ub, C.ivs,
                     C.ive, C.coef);
}

}  // namespace idn
