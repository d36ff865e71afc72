// The stripe form of the separable 8-bit stencils (stencil_u8.hip has the overview): strided rows
// and rows wider than the tiles' 3024 bytes.  The arithmetic of stencil_common.hpp with each row
// segment loaded from HBM: a wave owns one segment of a band of rows, lane l its 16-byte chunk.
#include "stencil_common.hpp"

namespace idn {

// NB > 0: burst form.  The band is exactly NB rows (the launcher sizes it so), all NB + 2R input
// rows are loaded up front (PF = NB + 2R) and the body is straight-line code.  NB == 0: long
// bands, a PF-deep load queue and a U-row unrolled loop (U a multiple of K and PF).
template <int C, int OP, int PF, int NB>
__global__ __launch_bounds__(256) void stencil_u8_vf(const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst, int h, int rb,
                                                     uint32_t row_stride, int nseg, int seg_len,
                                                     int bands, int band_rows, int total_items,
                                                     int map) {
  constexpr int K = Stencil<OP>::K;
  constexpr int R = K / 2;
  constexpr int U = NB ? NB : (K == 5) ? 5 : 6;
  static_assert(NB ? PF == NB + 2 * R : (U % K == 0 && U % PF == 0), "queue / unroll shape");
  static_assert(R * C <= 8, "one-side halo must fit in two neighbour dwords");

  const int lane = threadIdx.x & 63;
  const int item = stripe_item(map, nseg);
  if (item >= total_items) return;
  const StripeGeom g = stripe_geom(item, lane, rb, nseg, seg_len, bands);

  const uint32_t img_bytes = (uint32_t)h * row_stride;
  const rsrc_t rs = make_rsrc(src + (size_t)g.img * img_bytes, img_bytes);
  const rsrc_t rd = make_rsrc(dst + (size_t)g.img * img_bytes, img_bytes);
  const uint32_t ld_off = g.lead ? 0u : (uint32_t)g.q;

  const int y0 = g.band * band_rows;
  const int y1 = min(y0 + band_rows, h);
  if (y0 >= y1) return;
  const int nin = (y1 - y0) + 2 * R;
  auto load_row = [&](int r) -> v4u {
    const int y = reflect101_1(y0 - R + min(r, nin - 1), h);
    return __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)y * row_stride + ld_off, 0, 0);
  };
  const StoreOffs so = store_offs(g);

  v4u Lq[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) Lq[i] = load_row(i);

  uint32_t Rg[K][8];  // ring of unpacked input rows; row r lives in slot r % K

  // input row r: take it from the queue, refill the queue, rebuild the lead lane, unpack
  auto take_row = [&](int r, int slot_q, int slot_k, bool refill) {
    v4u Lv = Lq[slot_q];
    if (refill) Lq[slot_q] = load_row(r + PF);
    if (g.lead) {  // chunk = row bytes -8..7: rebuild the reflected 8 bytes
      const uint32_t L[4] = {Lv.x, Lv.y, Lv.z, Lv.w};
      Lv = v4u{lead_fix<C, BORDER_REFLECT101>(L, -8), lead_fix<C, BORDER_REFLECT101>(L, -4),
               L[0], L[1]};
    }
    unpack_row(Lv, Rg[slot_k]);
  };
  // output row from the ring whose newest row sits in slot `nw`.  A copy of ring_out_row without
  // the g.tail guard (same bytes): calling ring_out_row here made the burst 5x5 Gaussian 2 %
  // slower (profiles/stencil_split/README.md)
  auto out_row = [&](int nw, uint32_t row_off) {
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
    if constexpr (R * C > 4) {  // halos: R*C bytes each side
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
    if (g.fix_t0) vwin_tail_fix<C>(V, 24);
    if (g.fix_t8) vwin_tail_fix<C>(V, 16);
    uint32_t A[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      A[2 * k] = htap<C, OP>(V, 4 * k + 8);
      A[2 * k + 1] = htap<C, OP>(V, 4 * k + 9);
    }
    stripe_store_nb<0>(finish<OP>(A), rd, so, row_off);
  };

  // prologue: the 2R rows above the band only fill the ring
#pragma unroll
  for (int r = 0; r < 2 * R; ++r) take_row(r, r % PF, r % K, !NB);

  if constexpr (NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int r = 2 * R + u;
      take_row(r, r % PF, r % K, false);
      const int y = y0 + u;
      out_row(r % K, y < y1 ? (uint32_t)y * row_stride : OOB_OFF);
    }
  } else {
    const int nout = y1 - y0;
    const int ngroups = (nout + U - 1) / U;
    for (int gi = 0; gi < ngroups; ++gi) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = 2 * R + gi * U + u;  // slots (2R + u) % K / % PF are static
        take_row(r, (2 * R + u) % PF, (2 * R + u) % K, true);
        const int y = y0 + gi * U + u;
        out_row((2 * R + u) % K, y < y1 ? (uint32_t)y * row_stride : OOB_OFF);
      }
    }
  }
}

// Rows of <= 4 segments: short bands, one workgroup per band, all band rows loaded up front
// (burst); wider rows: long bands of independent waves.
template <int OP>
static int launch_stripe(const uint8_t* src, uint8_t* dst, int n, int h, int64_t rb,
                         int64_t row_stride, hipStream_t st, const char* name) {
  constexpr int K = Stencil<OP>::K;
  constexpr int PF = (K == 5) ? 5 : 6;
  constexpr int NBS = 6;
  const bool burst = (rb + 1007) / 1008 <= 4;
  const StripePlan p = plan_stripe(n, h, rb, K, burst ? 1 : PF, 5120, burst ? 1 : 0, NBS,
                                   burst ? NBS : 0);
  IDN_CHECK_ARG(p.total < (int64_t)0x7FFFFFFF, "%s: batch too large", name);
  const auto kernel = burst ? stencil_u8_vf<3, OP, NBS + K - 1, NBS> : stencil_u8_vf<3, OP, PF, 0>;
  hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), 0, st, src, dst, h, (int)rb,
                     (uint32_t)row_stride, p.nseg, p.seg_len, p.bands, p.band_rows, (int)p.total,
                     p.map);
  return IDN_OK;
}

int stencil_stripe(StencilOp op, const uint8_t* src, uint8_t* dst, int n, int h, int64_t rb,
                   int64_t row_stride, hipStream_t st, const char* name) {
  if (op == OP_GAUSS3) return launch_stripe<OP_GAUSS3>(src, dst, n, h, rb, row_stride, st, name);
  if (op == OP_GAUSS5) return launch_stripe<OP_GAUSS5>(src, dst, n, h, rb, row_stride, st, name);
  return launch_stripe<OP_BOX3>(src, dst, n, h, rb, row_stride, st, name);
}

}  // namespace idn
