// The flat LDS tile of the separable 8-bit stencils (stencil_u8.hip has the overview): compact
// rows of <= 3024 bytes that are not 16 k + 8 bytes long (those take stencil_pitched.hpp), for the
// u8 filters and the fused blob epilogue.  The unit also compiles the pitched tile
// (stencil_pitched.hpp says why).
#include "stencil_common.hpp"
#include "stencil_pitched.hpp"

namespace idn {

// ---- LDS-tiled form --------------------------------------------------------------------------
// One workgroup = one band of NB output rows of one image, nseg waves (<= 3: rows <= 3024 bytes).
// The band's NB + 2R input rows are contiguous in HBM (row_stride == row bytes), so the whole
// tile is fetched flat -- 16 B per lane, consecutive lanes on consecutive addresses, all loads in
// flight at once -- and staged in LDS; the waves then walk their row segments out of LDS with
// the vertical-first arithmetic (ring_row) and store their output rows directly.  Measured on this
// chip the flat tile fetch sustains ~5.8 TB/s copy-equivalent where per-segment row loads stop
// near 5.2 (tools/membench3.hip).
#ifndef IDN_STENCIL_NB  // band height of the u8 stencils' LDS tile (A/B builds set it)
#define IDN_STENCIL_NB 6
#endif
constexpr int TILE_WGT = 192;     // 3 waves
template <int NB, int K>
struct TileShape {
  static constexpr int ROWS = NB + K - 1;
  static constexpr int BYTES = ROWS * TILE_RBMAX + 16;           // + alignment shift
  static constexpr int NL = (BYTES + 16 * TILE_WGT - 1) / (16 * TILE_WGT);
  // exact footprint (the fetch never writes past the tile's bytes): one more resident
  // workgroup per CU for some band heights than a whole number of fetch rounds would allow
  static constexpr int LDS = (BYTES + 15) / 16 * 16;
};

template <int C, int OP, int NB, int EPI = EPI_U8, int NTS = 0, int DMA = 0>
__global__ __launch_bounds__(TILE_WGT) void stencil_u8_lds(const uint8_t* __restrict__ src,
                                                          uint8_t* __restrict__ dst, int h, int rb,
                                                          int nseg, int seg_len, int bands,
                                                          int total_items,
                                                          float* __restrict__ blob = nullptr,
                                                          double mb = 0.0, double mg = 0.0,
                                                          double mr = 0.0) {
  constexpr int K = Stencil<OP>::K;
  constexpr int R = K / 2;
  using TS = TileShape<NB, K>;
  constexpr int EXTRA = EPI == EPI_BLOB ? BLOB_LUT * 4 + BLOB_STAGE : 0;
  __shared__ __attribute__((aligned(16))) uint8_t smem[TS::LDS + EXTRA];
  uint8_t* const tile = smem;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-contiguous block order: a band's neighbours (which fetch its halo rows) run on the same
  // XCD, so the halo re-reads hit that XCD's L2
  const int blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
  // waves beyond nseg (rows narrower than 3 segments) only help fetch the tile
  const int item = blk * nseg + min(wave, nseg - 1);
  const StripeGeom g = stripe_geom(item, lane, rb, nseg, seg_len, bands);
  const uint32_t img_bytes = (uint32_t)h * (uint32_t)rb;
  const rsrc_t rs = make_rsrc(src + (size_t)g.img * img_bytes, img_bytes);
  const rsrc_t rd = EPI != EPI_BLOB ? make_rsrc(dst + (size_t)g.img * img_bytes, img_bytes)
                                  : make_rsrc(blob + (size_t)g.img * img_bytes, 4u * img_bytes);

  const int y0 = g.band * NB;
  const int y1 = min(y0 + NB, h);
  const int ys = max(y0 - R, 0), ye = min(y1 + R, h);
  const uint32_t base = (uint32_t)ys * (uint32_t)rb;
  const uint32_t base_al = base & ~15u, shift = base - base_al;
  const uint32_t nbytes = (uint32_t)ye * (uint32_t)rb - base_al;
  if constexpr (EPI == EPI_BLOB) {  // the blob table (published by the tile's barrier)
    float* lut = reinterpret_cast<float*>(smem + TS::LDS);
    for (int i = threadIdx.x; i < BLOB_LUT; i += TILE_WGT) {
      const int v = i / 3, ch = i - 3 * v;
      lut[i] = (float)__dsub_rn((double)v, ch == 0 ? mb : ch == 1 ? mg : mr);
    }
  }

  // flat fetch of the tile into LDS (out-of-image lanes read 0 and are not written).  Full bands
  // (every chunk but the last round's inside the tile): one lane offset, the round in the scalar
  // offset, no per-load compare / select and no guarded LDS stores but the last round's (~30
  // fewer VALU per band: the filter runs at the power cap, so VALU is time)
  {
    v4u v[TS::NL];
    const bool full = __builtin_amdgcn_readfirstlane(
        (int)(nbytes >= (uint32_t)(16 * TILE_WGT * (TS::NL - 1))));
    if (DMA && full) {  // (full: every chunk but the last round's inside the tile)
      // LDS-DMA: global_load_lds_dwordx4 writes each wave's 1 KiB straight into the tile (the
      // destination is wave base + 16 lane, as the flat layout wants), no VGPR round trip and no
      // ds_write.  Every wave must see every other wave's rows after the barrier, so each wave
      // waits for its own DMA (vmcnt(0)) before it: the workgroup fence does not promise that
      // wait on gfx9 (LLVM emits it here today, s_waitcnt vmcnt(0) lgkmcnt(0) before s_barrier;
      // stated explicitly so it cannot silently go away)
      const uint8_t* gsrc = src + (size_t)g.img * img_bytes + base_al + 16u * threadIdx.x;
      const int wv64 = 64 * wave;
#pragma unroll
      for (int i = 0; i < TS::NL - 1; ++i)
        __builtin_amdgcn_global_load_lds(
            (const void*)(gsrc + 16 * TILE_WGT * i),
            (__attribute__((address_space(3))) void*)(tile + 16 * (TILE_WGT * i + wv64)), 16, 0, 0);
      const uint32_t o = 16u * (uint32_t)(TILE_WGT * (TS::NL - 1) + threadIdx.x);
      if (o < nbytes)
        __builtin_amdgcn_global_load_lds(
            (const void*)(gsrc + 16 * TILE_WGT * (TS::NL - 1)),
            (__attribute__((address_space(3))) void*)(tile + 16 * (TILE_WGT * (TS::NL - 1) + wv64)),
            16, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (full) {
      const uint32_t vo = base_al + 16u * threadIdx.x;
#pragma unroll
      for (int i = 0; i < TS::NL - 1; ++i)
        v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 16 * TILE_WGT * i, 0);
      const uint32_t o = 16u * (uint32_t)(TILE_WGT * (TS::NL - 1) + threadIdx.x);
      v[TS::NL - 1] = __builtin_amdgcn_raw_buffer_load_b128(rs, o < nbytes ? base_al + o : OOB_OFF,
                                                            0, 0);
#pragma unroll
      for (int i = 0; i < TS::NL - 1; ++i)
        *reinterpret_cast<v4u*>(&tile[16u * (uint32_t)(TILE_WGT * i + threadIdx.x)]) = v[i];
      if (o < nbytes) *reinterpret_cast<v4u*>(&tile[o]) = v[TS::NL - 1];
    } else {
#pragma unroll
      for (int i = 0; i < TS::NL; ++i) {
        const uint32_t o = 16u * (uint32_t)(TILE_WGT * i + threadIdx.x);
        v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, o < nbytes ? base_al + o : OOB_OFF, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < TS::NL; ++i) {
        const uint32_t o = 16u * (uint32_t)(TILE_WGT * i + threadIdx.x);
        if (o < nbytes) *reinterpret_cast<v4u*>(&tile[o]) = v[i];
      }
    }
  }
  __syncthreads();
  const bool active = !(wave >= nseg || item >= total_items || y0 >= y1);  // wave-uniform
  if (!active) return;

  const uint32_t ld_off = g.lead ? 0u : (uint32_t)g.q;
  const int nin = (y1 - y0) + 2 * R;
  const StoreOffs so = store_offs(g);
  uint32_t Rg[K][8];
  auto take_row = [&](int r) {
    const int y = reflect101_1(y0 - R + min(r, nin - 1), h);
    lds_take_row<C>(tile, (uint32_t)(y - ys) * (uint32_t)rb + shift + ld_off, g.lead, Rg[r % K]);
  };
  // blob: byte offsets into lut[3 v + ch] of the channels of this lane's store bytes
  // (row byte seg_start + 256 k + 4 lane + j has channel (c0 + k + j) % 3: 256 = 1 mod 3)
  uint32_t c4[3] = {0u, 0u, 0u};
  if constexpr (EPI == EPI_BLOB) {
    const int c0 = (g.seg_start + 4 * lane) % 3;
#pragma unroll
    for (int t = 0; t < 3; ++t) c4[t] = 4u * (uint32_t)((c0 + t) % 3);
  }
#pragma unroll
  for (int r = 0; r < 2 * R; ++r) take_row(r);
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int r = 2 * R + u;
    take_row(r);
    const int y = y0 + u;
    const uint32_t row_off = y < y1 ? (uint32_t)y * (uint32_t)rb : OOB_OFF;
    if constexpr (EPI == EPI_BLOB) {
      blob_row_store(ring_row<C, OP>(Rg, r % K, g),
                     reinterpret_cast<uint32_t*>(smem + TS::LDS + BLOB_LUT * 4 + 1024 * wave),
                     reinterpret_cast<const float*>(smem + TS::LDS), lane, g, c4, rd, y < y1,
                     (uint32_t)y * (uint32_t)rb);
    } else {
      ring_out_row<C, OP, NTS ? 2 : 0>(Rg, r % K, g, rd, so, row_off);
    }
  }
}

// ---- host launcher ---------------------------------------------------------------------------
// The flat tile's LDS-DMA fetch issues 16-byte global_load_lds from the image base + 16 k: it is
// used only from a 16-byte-aligned base (compact rows of 16 k bytes keep every image of the batch
// there); a base at 8 mod 16 fetches the same tile through registers (16-byte buffer loads, which
// the stripe form issues at such addresses for strided rows).
static inline bool tile_dma_ok(const uint8_t* src) { return ((uintptr_t)src & 15) == 0; }

// 6-row bands (10 / 8 input rows in LDS, 30 / 24 KB per workgroup, up to 5-6 workgroups per CU;
// band heights 4-11 measured, tools/sweep_stencil.py)
struct TilePlan {
  int nseg, seg_len, bands, total;
  unsigned grid;
};
static int plan_tile(int n, int h, int rb, int NB, const char* name, TilePlan* p) {
  p->nseg = (rb + 1007) / 1008;
  p->seg_len = ((rb + p->nseg - 1) / p->nseg + 7) / 8 * 8;
  p->bands = (h + NB - 1) / NB;
  const int64_t total = (int64_t)n * p->bands * p->nseg;
  IDN_CHECK_ARG(total < (int64_t)0x7FFFFFFF, "%s: batch too large", name);
  p->total = (int)total;
  p->grid = (unsigned)((int64_t)n * p->bands);
  return IDN_OK;
}

// the blob epilogue keeps 6-row bands whatever an A/B build sets for the u8 filters
template <int OP, int EPI>
static int launch_tile(const TileCall& c) {
  constexpr int NB = EPI == EPI_BLOB ? 6 : IDN_STENCIL_NB;
  TilePlan p;
  if (int e = plan_tile(c.n, c.h, c.rb, NB, c.name, &p)) return e;
  const double zero[3] = {0.0, 0.0, 0.0};
  const double* m = EPI == EPI_BLOB ? c.mean : zero;
#define IDN_TILE(NTS, DMA)                                                                    \
  hipLaunchKernelGGL((stencil_u8_lds<3, OP, NB, EPI, NTS, DMA>), dim3(p.grid), dim3(TILE_WGT), 0, \
                     c.st, c.src, c.dst, c.h, c.rb, p.nseg, p.seg_len, p.bands, p.total, c.blob,  \
                     m[0], m[1], m[2])
#ifdef IDN_TUNING_BUILD
  // A/B: nontemporal stores of the u8 filters (IDN_STENCIL_NTS, measured slower)
  if constexpr (EPI == EPI_U8) {
    if (knob("IDN_STENCIL_NTS", 0)) {
      IDN_TILE(1, 0);
      return IDN_OK;
    }
  }
#endif
  // the tile is fetched by LDS-DMA; the register-staged fetch serves a base at 8 mod 16 and the
  // tuning build's A/B (IDN_STENCIL_GLDS=0)
  if (knob("IDN_STENCIL_GLDS", 1) && tile_dma_ok(c.src))
    IDN_TILE(0, 1);
  else
    IDN_TILE(0, 0);
#undef IDN_TILE
  return IDN_OK;
}

int stencil_tile(StencilOp op, const TileCall& c) {
  if (c.blob)
    return op == OP_GAUSS5 ? launch_tile<OP_GAUSS5, EPI_BLOB>(c)
                           : launch_tile<OP_GAUSS3, EPI_BLOB>(c);
  if (op == OP_GAUSS3) return launch_tile<OP_GAUSS3, EPI_U8>(c);
  if (op == OP_GAUSS5) return launch_tile<OP_GAUSS5, EPI_U8>(c);
  return launch_tile<OP_BOX3, EPI_U8>(c);
}

}  // namespace idn
