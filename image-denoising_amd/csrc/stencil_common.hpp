// Shared pieces of the separable 8-bit stencils (stencil_u8.hip has the overview and the dispatch
// rule): the ops, the vertical-first SWAR arithmetic on the stripe lane layout (stripe.hpp), the
// per-row body of the stripe form and the flat tile, the fused blob epilogue's row store, and the
// seams between the units.
#pragma once

#include "stripe.hpp"

namespace idn {

// OP_IDENT5: tuning-build probe -- the pitched tile's data movement with the taps reduced to a copy
// of the centre byte
enum StencilOp { OP_GAUSS3 = 0, OP_GAUSS5 = 1, OP_BOX3 = 2, OP_IDENT5 = 3 };

template <int OP> struct Stencil;
template <> struct Stencil<OP_GAUSS3> { static constexpr int K = 3; };
template <> struct Stencil<OP_GAUSS5> { static constexpr int K = 5; };
template <> struct Stencil<OP_BOX3> { static constexpr int K = 3; };

// ---- vertical-first fast path --------------------------------------------------------------
// Halo rows of a band cost only their unpack (8 ops); the horizontal pass runs per output row.
// Borders: the lead lane's reflected bytes are rebuilt on the raw row (lead_fix) before the
// unpack; the tail reflections are rebuilt on the u16 vertical sums (reflection commutes with the
// separable sums).

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_mad16(uint32_t a, uint32_t k, uint32_t c) {
  const u16x2 r = __builtin_bit_cast(u16x2, a) * __builtin_bit_cast(u16x2, k) +
                  __builtin_bit_cast(u16x2, c);
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t k, uint32_t c) {
  return __umul24(a, k) + c;
}

// vertical taps over ring rows r0..r(K-1) (oldest first); raw u16 lanes <= 255
template <int OP>
__device__ __forceinline__ uint32_t vtap(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3,
                                         uint32_t r4) {
  if constexpr (OP == OP_GAUSS5) {
    // [1 4 6 4 1] + 8 per lane (x16 horizontal weight = the +128 rounding bias): <= 4088
    const uint32_t t = ((r1 + r3) << 2) + 0x00080008u;
    return r0 + r4 + mad24(r2, 6u, t);
  } else if constexpr (OP == OP_GAUSS3) {
    return r0 + r2 + (r1 << 1);  // [1 2 1]: <= 1020
  } else {
    return r0 + r1 + r2;  // <= 765
  }
}

// horizontal taps at window byte P of the vertical sums, finished to the output byte:
// GAUSS: result in the high byte of each u16 lane; BOX: the rounded mean in byte 2 of each of
// two dwords (lo lane, hi lane)
template <int C, int OP>
__device__ __forceinline__ uint32_t htap(const VWin& V, int P) {
  if constexpr (OP == OP_GAUSS5) {
    const uint32_t t = (V.at(P - C) + V.at(P + C)) << 2;
    return V.at(P - 2 * C) + V.at(P + 2 * C) + pk_mad16(V.at(P), 0x00060006u, t);
  } else if constexpr (OP == OP_GAUSS3) {
    // 16 * [1 2 1] + 128: (16 S + 128) >> 8 == (S + 8) >> 4
    const uint32_t x = V.at(P - C) + V.at(P + C) + (V.at(P) << 1);
    return (x << 4) + 0x00800080u;
  } else {
    return V.at(P - C) + V.at(P) + V.at(P + C);  // <= 2295
  }
}

template <int OP>
__device__ __forceinline__ v4u finish(const uint32_t (&A)[8]) {
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if constexpr (OP == OP_BOX3) {
      // round(S/9) == (S*455 + 2075) >> 12 == (S*7280 + 33200) >> 16 (byte 2), S <= 2295
      const uint32_t e = A[2 * k], od = A[2 * k + 1];
      const uint32_t el = mad24(e & 0xFFFFu, 7280u, 33200u), eh = mad24(e >> 16, 7280u, 33200u);
      const uint32_t ol = mad24(od & 0xFFFFu, 7280u, 33200u), oh = mad24(od >> 16, 7280u, 33200u);
      // bytes: (el.b2, ol.b2, eh.b2, oh.b2)
      const uint32_t lo = __builtin_amdgcn_perm(ol, el, 0x0C0C0602u);  // el.b2 | ol.b2 << 8
      const uint32_t hi = __builtin_amdgcn_perm(oh, eh, 0x06020C0Cu);  // eh.b2 << 16 | oh.b2 << 24
      o[k] = lo | hi;
    } else {
      o[k] = __builtin_amdgcn_perm(A[2 * k + 1], A[2 * k], 0x07030501u);
    }
  }
  v4u r = {o[0], o[1], o[2], o[3]};
  return r;
}

// ---- shared per-row body of the stripe form and the flat tile ----------------------------------
// One output row from the register ring of K unpacked input rows whose newest row sits in slot
// `nw`: vertical taps, DPP halos, tail reflections, horizontal taps, pack, store.
template <int C, int OP>
__device__ __forceinline__ v4u ring_row(const uint32_t (&Rg)[Stencil<OP>::K][8], int nw,
                                        const StripeGeom& g) {
  constexpr int K = Stencil<OP>::K;
  constexpr int R = K / 2;
  uint32_t Vs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (K == 5) {
      Vs[j] = vtap<OP>(Rg[(nw + 1) % K][j], Rg[(nw + 2) % K][j], Rg[(nw + 3) % K][j],
                       Rg[(nw + 4) % K][j], Rg[nw][j]);
    } else {
      Vs[j] = vtap<OP>(Rg[(nw + 1) % K][j], Rg[(nw + 2) % K][j], Rg[nw][j], 0u, 0u);
    }
  }
  VWin V;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    V.SE[2 + j] = Vs[j];
    V.SO[2 + j] = Vs[4 + j];
  }
  if constexpr (R * C > 4) {
    V.SE[0] = from_prev_lane(Vs[2]);
    V.SO[0] = from_prev_lane(Vs[6]);
    V.SE[7] = from_next_lane(Vs[1]);
    V.SO[7] = from_next_lane(Vs[5]);
  } else {
    V.SE[0] = V.SO[0] = V.SE[7] = V.SO[7] = 0u;
  }
  V.SE[1] = from_prev_lane(Vs[3]);
  V.SO[1] = from_prev_lane(Vs[7]);
  V.SE[6] = from_next_lane(Vs[0]);
  V.SO[6] = from_next_lane(Vs[4]);
  if (g.tail) {  // scalar branch: the other segments' waves skip the masked tail fix-ups
    if (g.fix_t0) vwin_tail_fix<C>(V, 24);
    if (g.fix_t8) vwin_tail_fix<C>(V, 16);
  }
  uint32_t A[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    A[2 * k] = htap<C, OP>(V, 4 * k + 8);
    A[2 * k + 1] = htap<C, OP>(V, 4 * k + 9);
  }
  return finish<OP>(A);
}
template <int C, int OP, int NT>
__device__ __forceinline__ void ring_out_row(const uint32_t (&Rg)[Stencil<OP>::K][8], int nw,
                                             const StripeGeom& g, rsrc_t rd, const StoreOffs& so,
                                             uint32_t row_off) {
  stripe_store_nb<NT>(ring_row<C, OP>(Rg, nw, g), rd, so, row_off);
}

// the lane's 16-byte chunk of one row staged in LDS at byte `o`, lead lane rebuilt, unpacked
template <int C>
__device__ __forceinline__ void lds_take_row(const uint8_t* tile, uint32_t o, bool lead,
                                             uint32_t (&U)[8]) {
  const v2u a = *reinterpret_cast<const v2u*>(&tile[o]);
  const v2u b = *reinterpret_cast<const v2u*>(&tile[o + 8]);
  v4u Lv = v4u{a.x, a.y, b.x, b.y};
  if (lead) {
    const uint32_t L[4] = {Lv.x, Lv.y, Lv.z, Lv.w};
    Lv = v4u{lead_fix<C, BORDER_REFLECT101>(L, -8), lead_fix<C, BORDER_REFLECT101>(L, -4), L[0],
             L[1]};
  }
  unpack_row(Lv, U);
}

enum TileEpi { EPI_U8 = 0, EPI_BLOB = 1 };

// Blob epilogue (EPI_BLOB): blob = float32(float64(v) - PIXEL_MEANS[ch]) (lib/utils/blob.py:35-36:
// numpy's float64 subtract, then the float32 store) is a 3 x 256 table, held in LDS interleaved as
// lut[3 v + ch] (lanes reading the same byte value of different channels hit different banks).
// The filtered row segment is staged in LDS (one 16-byte write per lane) and re-read as dwords, so
// store k of a lane writes the four floats of row bytes seg_start + 256 k + 4 lane .. + 3: every
// 16-byte store instruction of a wave writes 1 KiB of contiguous blob (the last 960 B), with no
// partial-chunk stores.
constexpr int BLOB_LUT = 768;          // floats
constexpr int BLOB_STAGE = 3 * 1024;   // bytes: one 1 KiB row-segment stage per wave
template <int AUX = 0>
__device__ __forceinline__ void blob_row_store(const v4u& o, uint32_t* __restrict__ stage,
                                               const float* __restrict__ lut, int lane,
                                               const StripeGeom& g, const uint32_t (&c4)[3],
                                               rsrc_t rd, bool row_ok, uint32_t row_byte) {
  // WAR: the previous row's reads of this wave's stage are issued before this write
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  reinterpret_cast<v4u*>(stage)[lane] = o;  // stage byte 16 lane = row byte q
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = g.seg_start + 256 * k + 4 * lane;  // row byte of the store's first float
    const bool ok = row_ok && e < g.seg_end;         // seg_end - seg_start is a multiple of 8
    const uint32_t w = stage[min(2 + 64 * k + lane, 255)];
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t v = (w >> (8 * j)) & 0xFFu;
      f[j] = *reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(lut) +
                                             (v * 12u + c4[(k + j) % 3]));
    }
    __builtin_amdgcn_raw_buffer_store_b128(
        v4u{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
            __float_as_uint(f[3])},
        rd, ok ? 4u * (row_byte + (uint32_t)e) : OOB_OFF, 0, AUX);
  }
}

// ---- the seams: host functions defined in one unit and called from stencil_u8.hip ---------------
// Each launches (no launch check: the caller's IDN_CHECK_LAUNCH follows) or refuses with
// "batch too large"; each kernel is instantiated in the unit that defines its launcher.
constexpr int TILE_RBMAX = 3024;  // widest row of both tiles: 3 segments of 1008 bytes

// one call of a tiled form on compact rows of rb bytes: u8 -> u8 into dst, or, with blob set, the
// fused blob epilogue (float32(float64(v) - mean[ch]) into blob; dst unused; Gaussian only)
struct TileCall {
  const uint8_t* src;
  uint8_t* dst;
  float* blob;
  const double* mean;
  int n, h, rb;
  hipStream_t st;
  const char* name;
};
// stencil_pitched.hpp (compiled by stencil_tile.hip): rows of 16 k + 8 bytes
int stencil_pitched(StencilOp op, const TileCall& c);
// stencil_tile.hip: the other compact rows
int stencil_tile(StencilOp op, const TileCall& c);
// stencil_stripe.hip: strided or wider rows from HBM (burst bands for rows of <= 4 segments)
int stencil_stripe(StencilOp op, const uint8_t* src, uint8_t* dst, int n, int h, int64_t rb,
                   int64_t row_stride, hipStream_t st, const char* name);

}  // namespace idn
