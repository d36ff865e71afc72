// Exposure correction on u8 images that already live on the device: COLOR_BGR2YUV / COLOR_YUV2BGR,
// cv2.equalizeHist, cv2.createCLAHE(clip, grid).apply, and the tone part of Automold's
// exposure_process (BGR -> YUV, luma * 0.85 above 150, CLAHE, equalizeHist, CLAHE, YUV -> BGR), whose
// last step, fastNlMeansDenoisingColored, is idn_nlmeans_colored_u8.  The arithmetic is OpenCV 3.4's
// 8-bit code as recalled (include/idn.h restates it); tests/exposure_model.py is the definition.
//
// Everything between the bytes is integer or a fixed sequence of fp32 operations, and the only
// cross-workgroup communication is integer atomicAdd into zeroed counters, whose order cannot change
// a sum: an image gives the same bytes alone, in any batch and on every run.
//
// exp_hist_kernel    one 256-thread workgroup counts up to EXP_HR rows of one CLAHE tile (or of the
//                    whole image: a 1 x 1 grid without padding) into four per-wave LDS histograms
//                    of u32 counters, adds them and flushes the non-zero bins with atomicAdd into
//                    the (n, tiles, 256) u32 array.  The tile grid covers the image extended by
//                    BORDER_REFLECT_101 at the bottom and the right; the extension is counted by
//                    reading the reflected source pixels.
// exp_clahe_lut_kernel  one wave per (image, tile), four bins per lane: clip, wave reduction of the
//                    excess, even share, residual rule, inclusive scan, 256-byte table.
// exp_equalize_lut_kernel  one wave per image: first non-zero bin, scale, scan, table.
// exp_apply_kernel   one workgroup owns EXP_AR rows of one image and holds the tables of the tile
//                    rows those image rows blend in LDS; per pixel four byte look-ups and the fp32
//                    blend.  Its forms read the luma from a byte plane or compute it from BGR (with
//                    the tone step), send it through a per-image table first (equalizeHist folded
//                    in), count their output into the image's histogram, and write a byte plane
//                    or, with U and V recomputed from the source, BGR.
//
// idn_correct_exposure_u8 is seven launches and stores no YUV image; per pixel of the batch
//   1  exp_hist  <BGR+tone>           reads 3       tile histograms of the toned luma
//   2  exp_clahe_lut
//   3  exp_apply <BGR+tone -> plane>  reads 3, writes 1; counts the plane's histogram
//   4  exp_equalize_lut
//   5  exp_hist  <plane, through the equalize table>  reads 1
//   6  exp_clahe_lut
//   7  exp_apply <plane, through the equalize table -> BGR>  reads 1 + 3, writes 3
// 15 bytes, where the seven separate steps (two conversions, the tone step, two CLAHE, equalizeHist)
// would move 23.
#include "idn_common.hpp"
#include "abi_args.hpp"

#include <limits.h>
#include <math.h>

namespace idn {

constexpr int EXP_HR = 32;       // rows of a tile per histogram workgroup
constexpr int EXP_AR = 16;       // image rows per apply workgroup
constexpr int EXP_HU = 8;        // byte loads a histogram (or map) lane issues together
constexpr int EXP_AU = 4;        // columns of a row an apply lane owns (the next row's are in flight)
constexpr int EXP_MAX_TILES = 16;  // per axis
constexpr uint32_t EXP_TONE_ABOVE = 150;

enum { EXP_SRC_PLANE = 0, EXP_SRC_BGR_TONE = 1 };
enum { EXP_OUT_PLANE = 0, EXP_OUT_BGR = 1 };

// ---- colour ---------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ int exp_descale(int v) { return (v + 8192) >> 14; }
__host__ __device__ __forceinline__ int exp_sat(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__host__ __device__ __forceinline__ int exp_luma(int b, int g, int r) {
  return exp_descale(1868 * b + 9617 * g + 4899 * r);  // <= 255: the weights add up to 1 << 14
}
__host__ __device__ __forceinline__ int exp_u(int b, int y) {
  return exp_sat(exp_descale((b - y) * 8061 + (128 << 14)));
}
__host__ __device__ __forceinline__ int exp_v(int r, int y) {
  return exp_sat(exp_descale((r - y) * 14369 + (128 << 14)));
}
__host__ __device__ __forceinline__ void exp_yuv2bgr(int y, int u, int v, uint8_t* o) {
  u -= 128;
  v -= 128;
  o[0] = (uint8_t)exp_sat(y + exp_descale(33292 * u));
  o[1] = (uint8_t)exp_sat(y + exp_descale(-6472 * u - 9519 * v));
  o[2] = (uint8_t)exp_sat(y + exp_descale(18678 * v));
}
// trunc(y * 0.85) in float64 for every byte y (tests/test_exposure.py)
__host__ __device__ __forceinline__ uint32_t exp_tone(uint32_t y) {
  return y > EXP_TONE_ABOVE ? (17u * y) / 20u : y;
}

template <int SRC>
__device__ __forceinline__ uint32_t exp_luma_at(const uint8_t* row, int x) {
  if (SRC == EXP_SRC_PLANE) return row[x];
  const uint8_t* p = row + 3 * (int64_t)x;
  return exp_tone((uint32_t)exp_luma(p[0], p[1], p[2]));
}

template <bool TO_YUV>
__global__ __launch_bounds__(256) void exp_cvt_kernel(const uint8_t* __restrict__ src,
                                                      uint8_t* __restrict__ dst, int w,
                                                      int64_t row_stride, int xblocks) {
  const int64_t row = blockIdx.x / xblocks;
  const int x = (int)(blockIdx.x - row * xblocks) * 256 + (int)threadIdx.x;
  if (x >= w) return;
  const uint8_t* p = src + row * row_stride + 3 * (int64_t)x;
  uint8_t* q = dst + row * row_stride + 3 * (int64_t)x;
  const int a = p[0], b = p[1], c = p[2];
  if (TO_YUV) {
    const int y = exp_luma(a, b, c);
    q[0] = (uint8_t)exp_sat(y);
    q[1] = (uint8_t)exp_u(a, y);
    q[2] = (uint8_t)exp_v(c, y);
  } else {
    exp_yuv2bgr(a, b, c, q);
  }
}

// ---- histograms -----------------------------------------------------------------------------------

struct ExpGeom {
  int h, w, tiles_x, tiles_y, th, tw;  // th x tw: the tile, tiles_y*th x tiles_x*tw the extension
};

// Four per-wave sub-histograms: a constant region makes every lane of a wave hit one bin, but the
// four waves of the workgroup do not also queue behind each other.
__device__ __forceinline__ void exp_hist_flush(uint32_t (*sh)[256], int t, uint32_t* out) {
  __syncthreads();
  const uint32_t s = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
  if (s) atomicAdd(out + t, s);
}

template <int SRC, bool PRELUT>
__global__ __launch_bounds__(256) void exp_hist_kernel(const uint8_t* __restrict__ src,
                                                       int64_t row_stride, int64_t img_pitch,
                                                       ExpGeom g, int chunks,
                                                       const uint8_t* __restrict__ prelut,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[4][256];
  __shared__ uint8_t pl[256];
  const int t = threadIdx.x;
  const int tiles = g.tiles_x * g.tiles_y;
  const int per_img = tiles * chunks;
  const int img = blockIdx.x / per_img;
  const int rem = blockIdx.x - img * per_img;
  const int tile = rem / chunks;
  const int chunk = rem - tile * chunks;
  const int tyi = tile / g.tiles_x, txi = tile - tyi * g.tiles_x;
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[k][t] = 0;
  if (PRELUT) pl[t] = prelut[(int64_t)img * 256 + t];
  __syncthreads();

  const int r0 = chunk * EXP_HR;
  const int rows = min(EXP_HR, g.th - r0);
  const uint8_t* base = src + (int64_t)img * img_pitch;
  uint32_t* my = sh[t >> 6];
  // A lane owns a column of the tile and walks down it EXP_HU rows at a step, their loads issued
  // together, and nothing in the loop divides: with a flat pixel index and a division per pixel
  // equalize_hist took 0.28 ms instead of 0.18 (profiles/exposure/README.md).  A row past the chunk's end
  // loads the chunk's last row again (a valid address) and is not counted.
  // BORDER_REFLECT_101, once: the pads are at most tiles_y < h rows and tiles_x < w columns.
  for (int cx = t; cx < g.tw; cx += 256) {
    const int ex = txi * g.tw + cx;
    const int sx = ex < g.w ? ex : 2 * g.w - 2 - ex;
    for (int r = 0; r < rows; r += EXP_HU) {
      uint32_t v[EXP_HU];
#pragma unroll
      for (int k = 0; k < EXP_HU; ++k) {
        const int ey = tyi * g.th + r0 + min(r + k, rows - 1);
        const int sy = ey < g.h ? ey : 2 * g.h - 2 - ey;
        v[k] = exp_luma_at<SRC>(base + (int64_t)sy * row_stride, sx);
      }
#pragma unroll
      for (int k = 0; k < EXP_HU; ++k) {
        if (r + k < rows) atomicAdd(&my[PRELUT ? (uint32_t)pl[v[k]] : v[k]], 1u);
      }
    }
  }
  exp_hist_flush(sh, t, hist + ((int64_t)img * tiles + tile) * 256);
}

// ---- tables ---------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor(v, m, 64));
  return v;
}
// exclusive prefix of the lanes' values
__device__ __forceinline__ uint32_t wave_scan_excl(uint32_t v, int lane) {
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  return inc - v;
}
__device__ __forceinline__ uint32_t exp_scaled(uint32_t sum, float scale) {
  const float r = rintf((float)sum * scale);  // round half to even
  return (uint32_t)exp_sat((int)fminf(r, 255.0f));
}

// one wave per (image, tile); lane l owns bins 4l .. 4l+3
__global__ __launch_bounds__(64) void exp_clahe_lut_kernel(const uint32_t* __restrict__ hist,
                                                           uint32_t clip, float scale,
                                                           uint8_t* __restrict__ luts) {
  const int lane = threadIdx.x;
  const uint32_t* hp = hist + (int64_t)blockIdx.x * 256 + 4 * lane;
  uint32_t hv[4] = {hp[0], hp[1], hp[2], hp[3]};
  if (clip > 0) {
    uint32_t over = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (hv[k] > clip) {
        over += hv[k] - clip;
        hv[k] = clip;
      }
    }
    const uint32_t excess = wave_sum(over);
    const uint32_t share = excess >> 8, resid = excess & 255u;
    const uint32_t step = resid ? max(256u / resid, 1u) : 1u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t i = 4u * lane + k;
      // bins 0, step, 2 step, ... while the residual lasts: (resid - 1) * step < 256
      hv[k] += share + ((resid && i % step == 0 && i / step < resid) ? 1u : 0u);
    }
  }
  const uint32_t own = (hv[0] + hv[1]) + (hv[2] + hv[3]);
  uint32_t run = wave_scan_excl(own, lane);
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    run += hv[k];
    packed |= exp_scaled(run, scale) << (8 * k);
  }
  reinterpret_cast<uint32_t*>(luts + (int64_t)blockIdx.x * 256)[lane] = packed;
}

// one wave per image
__global__ __launch_bounds__(64) void exp_equalize_lut_kernel(const uint32_t* __restrict__ hist,
                                                              uint32_t total,
                                                              uint8_t* __restrict__ luts) {
  const int lane = threadIdx.x;
  const uint32_t* hp = hist + (int64_t)blockIdx.x * 256 + 4 * lane;
  const uint32_t hv[4] = {hp[0], hp[1], hp[2], hp[3]};
  uint32_t first = 256;
#pragma unroll
  for (int k = 3; k >= 0; --k)
    if (hv[k]) first = 4u * lane + k;
  const uint32_t i0 = wave_min(first);  // total > 0: some bin is not empty
  const uint32_t h0 = hist[(int64_t)blockIdx.x * 256 + i0];
  const uint32_t own = (hv[0] + hv[1]) + (hv[2] + hv[3]);
  uint32_t run = wave_scan_excl(own, lane);
  uint32_t packed = 0;
  if (h0 == total) {
    packed = i0 * 0x01010101u;
  } else {
    const float scale = 255.0f / (float)(total - h0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      run += hv[k];
      const uint32_t i = 4u * lane + k;
      if (i > i0) packed |= exp_scaled(run - h0, scale) << (8 * k);
    }
  }
  reinterpret_cast<uint32_t*>(luts + (int64_t)blockIdx.x * 256)[lane] = packed;
}

// dst = table of the image [src]; one workgroup owns EXP_AR rows of one image
__global__ __launch_bounds__(256) void exp_map_kernel(const uint8_t* __restrict__ src,
                                                      uint8_t* __restrict__ dst, int h, int w,
                                                      int64_t row_stride, int bands,
                                                      const uint8_t* __restrict__ luts) {
  __shared__ uint8_t pl[256];
  const int t = threadIdx.x;
  const int img = blockIdx.x / bands;
  const int band = blockIdx.x - img * bands;
  const int y0 = band * EXP_AR, y1 = min(y0 + EXP_AR, h);
  pl[t] = luts[(int64_t)img * 256 + t];
  __syncthreads();
  const int64_t base = (int64_t)img * h * row_stride;
  for (int y = y0; y < y1; ++y) {
    const uint8_t* srow = src + base + (int64_t)y * row_stride;
    uint8_t* drow = dst + base + (int64_t)y * row_stride;
    for (int xb = t; xb < w; xb += 256 * EXP_HU) {
      uint32_t v[EXP_HU];
#pragma unroll
      for (int k = 0; k < EXP_HU; ++k) v[k] = srow[min(xb + 256 * k, w - 1)];
#pragma unroll
      for (int k = 0; k < EXP_HU; ++k)
        if (xb + 256 * k < w) drow[xb + 256 * k] = pl[v[k]];
    }
  }
}

// ---- CLAHE apply ----------------------------------------------------------------------------------

struct ExpApply {
  const uint8_t* src;   // the luma's source: a byte plane, or BGR (EXP_SRC_BGR_TONE)
  int64_t src_stride, src_pitch;
  const uint8_t* bgr;   // EXP_OUT_BGR: the image U and V are taken from
  int64_t bgr_stride, bgr_pitch;
  uint8_t* dst;
  int64_t dst_stride, dst_pitch;
  const uint8_t* luts;    // (n, tiles_y, tiles_x, 256)
  const uint8_t* prelut;  // (n, 256), PRELUT
  uint32_t* ihist;        // (n, 256), HIST: the histogram of the bytes written
  float inv_th, inv_tw;
  int bands, lds_rows;
};

template <int SRC, int OUT, bool PRELUT, bool HIST>
__global__ __launch_bounds__(256) void exp_apply_kernel(ExpApply a, ExpGeom g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tab[];  // lds_rows * tiles_x * 256
  __shared__ uint32_t sh[HIST ? 4 : 1][256];
  __shared__ uint8_t pl[256];
  const int t = threadIdx.x;
  const int img = blockIdx.x / a.bands;
  const int band = blockIdx.x - img * a.bands;
  const int y0 = band * EXP_AR, y1 = min(y0 + EXP_AR, g.h) - 1;
  // the tile rows that rows y0..y1 blend: at most EXP_AR / th + 3 = lds_rows of them
  const int lo = max((int)floorf((float)y0 * a.inv_th - 0.5f), 0);
  int hi = min((int)floorf((float)y1 * a.inv_th - 0.5f) + 1, g.tiles_y - 1);
  hi = min(hi, lo + a.lds_rows - 1);
  {
    const int words = (hi - lo + 1) * g.tiles_x * 64;
    const uint32_t* from = reinterpret_cast<const uint32_t*>(
        a.luts + ((int64_t)img * g.tiles_y + lo) * g.tiles_x * 256);
    uint32_t* to = reinterpret_cast<uint32_t*>(tab);
    for (int i = t; i < words; i += 256) to[i] = from[i];
  }
  if (HIST) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[k][t] = 0;
  }
  if (PRELUT) pl[t] = a.prelut[(int64_t)img * 256 + t];
  __syncthreads();

  uint32_t* my = sh[HIST ? (t >> 6) : 0];
  const uint8_t* sbase = a.src + (int64_t)img * a.src_pitch;
  const uint8_t* cbase = OUT == EXP_OUT_BGR ? a.bgr + (int64_t)img * a.bgr_pitch : nullptr;
  uint8_t* dbase = a.dst + (int64_t)img * a.dst_pitch;
  // A lane owns EXP_AU columns, 256 apart, and walks down the band: the columns' tile indices and
  // weights are computed once, a row's loads are issued together and the next row's before this
  // row's arithmetic.  A column past the row's end loads the row's last pixel again (a valid
  // address) and is not written.
  for (int xb = t; xb < g.w; xb += 256 * EXP_AU) {
    float xa[EXP_AU], xa1[EXP_AU];
    int o1[EXP_AU], o2[EXP_AU], xc[EXP_AU];
#pragma unroll
    for (int k = 0; k < EXP_AU; ++k) {
      xc[k] = min(xb + 256 * k, g.w - 1);
      const float txf = (float)xc[k] * a.inv_tw - 0.5f;
      const float fx = floorf(txf);
      xa[k] = txf - fx;
      xa1[k] = 1.0f - xa[k];
      const int tx1 = (int)fx;
      o2[k] = min(tx1 + 1, g.tiles_x - 1) * 256;
      o1[k] = max(tx1, 0) * 256;
    }
    uint32_t lum[EXP_AU], col[EXP_AU], lum_n[EXP_AU], col_n[EXP_AU];
    auto fetch = [&](int y, uint32_t* l, uint32_t* c) {
      const uint8_t* srow = sbase + (int64_t)y * a.src_stride;
#pragma unroll
      for (int k = 0; k < EXP_AU; ++k) {
        l[k] = exp_luma_at<SRC>(srow, xc[k]);
        if (OUT == EXP_OUT_BGR) {
          const uint8_t* p = cbase + (int64_t)y * a.bgr_stride + 3 * (int64_t)xc[k];
          c[k] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
      }
    };
    fetch(y0, lum, col);
    for (int y = y0; y <= y1; ++y) {
      if (y < y1) fetch(y + 1, lum_n, col_n);
      const float tyf = (float)y * a.inv_th - 0.5f;
      const float fy = floorf(tyf);
      const float ya = tyf - fy, ya1 = 1.0f - ya;
      const int ty1 = (int)fy;
      const int ty2 = min(min(ty1 + 1, g.tiles_y - 1), hi);
      const uint8_t* T1 = tab + (min(max(ty1, 0), hi) - lo) * g.tiles_x * 256;
      const uint8_t* T2 = tab + (ty2 - lo) * g.tiles_x * 256;
#pragma unroll
      for (int k = 0; k < EXP_AU; ++k) {
        const int x = xb + 256 * k;
        if (x >= g.w) break;
        const uint32_t v = PRELUT ? (uint32_t)pl[lum[k]] : lum[k];
        const float l11 = (float)T1[o1[k] + v], l12 = (float)T1[o2[k] + v];
        const float l21 = (float)T2[o1[k] + v], l22 = (float)T2[o2[k] + v];
        // every product and sum rounds to fp32 (the build has -ffp-contract=off)
        const float res = (l11 * xa1[k] + l12 * xa[k]) * ya1 + (l21 * xa1[k] + l22 * xa[k]) * ya;
        const uint32_t o = (uint32_t)exp_sat((int)rintf(res));
        if (HIST) atomicAdd(&my[o], 1u);
        if (OUT == EXP_OUT_PLANE) {
          dbase[(int64_t)y * a.dst_stride + x] = (uint8_t)o;
        } else {
          const int b = col[k] & 255u, gg = (col[k] >> 8) & 255u, r = col[k] >> 16;
          const int yy = exp_luma(b, gg, r);
          exp_yuv2bgr((int)o, exp_u(b, yy), exp_v(r, yy),
                      dbase + (int64_t)y * a.dst_stride + 3 * (int64_t)x);
        }
      }
#pragma unroll
      for (int k = 0; k < EXP_AU; ++k) {
        lum[k] = lum_n[k];
        col[k] = col_n[k];
      }
    }
  }
  if (HIST) exp_hist_flush(sh, t, a.ihist + (int64_t)img * 256);
}

// ---- host side ------------------------------------------------------------------------------------

static bool exp_grid_ok(int tiles_x, int tiles_y) {
  return tiles_x >= 1 && tiles_x <= EXP_MAX_TILES && tiles_y >= 1 && tiles_y <= EXP_MAX_TILES;
}

static ExpGeom exp_geom(int h, int w, int tiles_x, int tiles_y) {
  ExpGeom g;
  g.h = h;
  g.w = w;
  g.tiles_x = tiles_x;
  g.tiles_y = tiles_y;
  int hext = h, wext = w;
  if (w % tiles_x != 0 || h % tiles_y != 0) {  // both pads whenever either fails to divide
    hext = h + (tiles_y - h % tiles_y);
    wext = w + (tiles_x - w % tiles_x);
  }
  g.th = hext / tiles_y;
  g.tw = wext / tiles_x;
  return g;
}

struct ExpLayout {
  size_t hist, ihist, luts, eq, plane, total;
};

static ExpLayout exp_layout(int n, int h, int w, int tiles) {
  ExpLayout l;
  Bump ws;
  l.hist = ws.take((size_t)n * tiles * 256 * sizeof(uint32_t));
  l.ihist = ws.take((size_t)n * 256 * sizeof(uint32_t));
  l.luts = ws.take((size_t)n * tiles * 256);
  l.eq = ws.take((size_t)n * 256);
  l.plane = ws.take((size_t)n * h * w);
  l.total = align_up(ws.total, 256);
  return l;
}

// what one launch can index: a histogram workgroup per EXP_HR tile rows, pixels of a tile in int
static int exp_check_size(int n, const ExpGeom& g, const char* name) {
  const int64_t tiles = (int64_t)g.tiles_x * g.tiles_y;
  const int64_t chunks = (g.th + EXP_HR - 1) / EXP_HR;
  const int64_t bands = (g.h + EXP_AR - 1) / EXP_AR;
  if ((int64_t)g.th * g.tw * tiles > (int64_t)INT_MAX || n * tiles * chunks > (int64_t)INT_MAX ||
      n * bands > (int64_t)INT_MAX)
    return set_error(IDN_EUNSUPPORTED, "%s: image or batch too large for one launch", name);
  return IDN_OK;
}

static int exp_clip(double clip_limit, int area) {
  if (clip_limit == 0.0) return 0;
  const double v = clip_limit * (double)area / 256.0;
  if (v >= (double)INT_MAX) return INT_MAX;  // above every count: clips nothing either way
  const int c = (int)v;
  return c > 1 ? c : 1;
}

template <int SRC, bool PRELUT>
static void exp_launch_hist(hipStream_t st, const uint8_t* src, int64_t stride, int64_t pitch,
                            int n, const ExpGeom& g, const uint8_t* prelut, uint32_t* hist) {
  const int chunks = (g.th + EXP_HR - 1) / EXP_HR;
  const unsigned grid = (unsigned)(n * g.tiles_x * g.tiles_y * chunks);
  hipLaunchKernelGGL((exp_hist_kernel<SRC, PRELUT>), dim3(grid), dim3(256), 0, st, src, stride,
                     pitch, g, chunks, prelut, hist);
}

template <int SRC, int OUT, bool PRELUT, bool HIST>
static void exp_launch_apply(hipStream_t st, ExpApply a, int n, const ExpGeom& g) {
  a.inv_th = 1.0f / (float)g.th;
  a.inv_tw = 1.0f / (float)g.tw;
  a.bands = (g.h + EXP_AR - 1) / EXP_AR;
  a.lds_rows = g.tiles_y < EXP_AR / g.th + 3 ? g.tiles_y : EXP_AR / g.th + 3;
  const size_t lds = (size_t)a.lds_rows * g.tiles_x * 256;  // th >= 2: at most 11 * 16 * 256
  hipLaunchKernelGGL((exp_apply_kernel<SRC, OUT, PRELUT, HIST>), dim3((unsigned)(n * a.bands)),
                     dim3(256), lds, st, a, g);
}

template <bool TO_YUV>
static int exp_cvt(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                   void* stream, const char* name) {
  if (int e = check_src_dst(name, src, dst, n, h, w, "operation")) return e;
  if (int e = check_row_stride(name, row_stride, w, 3, "3")) return e;
  if (n == 0) return IDN_OK;
  const int xblocks = (w + 255) / 256;
  if ((int64_t)n * h * xblocks > (int64_t)INT_MAX) return batch_too_large(name);
  hipLaunchKernelGGL((exp_cvt_kernel<TO_YUV>), dim3((unsigned)(n * h * xblocks)), dim3(256), 0,
                     as_stream(stream), src, dst, w, row_stride, xblocks);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

}  // namespace idn

extern "C" int idn_bgr2yuv_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                              int64_t row_stride, void* stream) {
  return idn::exp_cvt<true>(src, dst, n, h, w, row_stride, stream, "idn_bgr2yuv_u8");
}

extern "C" int idn_yuv2bgr_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                              int64_t row_stride, void* stream) {
  return idn::exp_cvt<false>(src, dst, n, h, w, row_stride, stream, "idn_yuv2bgr_u8");
}

extern "C" size_t idn_exposure_workspace_size(int n, int h, int w, int tiles_x, int tiles_y) {
  using namespace idn;
  if (n <= 0 || h <= 0 || w <= 0 || !exp_grid_ok(tiles_x, tiles_y)) return 0;
  return exp_layout(n, h, w, tiles_x * tiles_y).total;
}

extern "C" int idn_equalize_hist_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                                    int64_t row_stride, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  using namespace idn;
  const char* const name = "idn_equalize_hist_u8";
  if (int e = check_src_dst(name, src, dst, n, h, w, "operation")) return e;
  if (int e = check_row_stride(name, row_stride, w, 1, "1")) return e;
  if (n == 0) return IDN_OK;
  const ExpLayout l = exp_layout(n, h, w, 1);
  if (int e = check_workspace(name, workspace, workspace_bytes, l.total)) return e;
  const ExpGeom g = exp_geom(h, w, 1, 1);
  if (int e = exp_check_size(n, g, name)) return e;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* ihist = reinterpret_cast<uint32_t*>(ws + l.ihist);
  const hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(ihist, 0, (size_t)n * 256 * sizeof(uint32_t), st) != hipSuccess)
    return set_error(IDN_EHIP, "%s: clearing the histograms failed", name);
  exp_launch_hist<EXP_SRC_PLANE, false>(st, src, row_stride, (int64_t)h * row_stride, n, g, nullptr,
                                        ihist);
  IDN_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(exp_equalize_lut_kernel, dim3((unsigned)n), dim3(64), 0, st, ihist,
                     (uint32_t)(h * w), ws + l.eq);
  IDN_CHECK_LAUNCH(name);
  const int bands = (h + EXP_AR - 1) / EXP_AR;
  hipLaunchKernelGGL(exp_map_kernel, dim3((unsigned)(n * bands)), dim3(256), 0, st, src, dst, h, w,
                     row_stride, bands, ws + l.eq);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

extern "C" int idn_clahe_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                            int64_t row_stride, double clip_limit, int tiles_x, int tiles_y,
                            void* workspace, size_t workspace_bytes, void* stream) {
  using namespace idn;
  const char* const name = "idn_clahe_u8";
  if (int e = check_src_dst(name, src, dst, n, h, w, "operation")) return e;
  if (int e = check_row_stride(name, row_stride, w, 1, "1")) return e;
  IDN_CHECK_ARG(exp_grid_ok(tiles_x, tiles_y), "%s: tiles_x and tiles_y must be in 1..%d (got %d, "
                "%d)", name, EXP_MAX_TILES, tiles_x, tiles_y);
  IDN_CHECK_ARG(h > tiles_y && w > tiles_x, "%s: image %d x %d needs more rows and columns than "
                "the %d x %d tile grid", name, h, w, tiles_y, tiles_x);
  IDN_CHECK_ARG(clip_limit >= 0.0 && clip_limit < INFINITY, "%s: clip_limit must be finite and "
                "not negative (got %g)", name, clip_limit);
  const int tiles = tiles_x * tiles_y;
  if (n == 0) return IDN_OK;
  const ExpLayout l = exp_layout(n, h, w, tiles);
  if (int e = check_workspace(name, workspace, workspace_bytes, l.total)) return e;
  const ExpGeom g = exp_geom(h, w, tiles_x, tiles_y);
  if (int e = exp_check_size(n, g, name)) return e;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + l.hist);
  const hipStream_t st = as_stream(stream);
  const int area = g.th * g.tw;
  if (hipMemsetAsync(hist, 0, (size_t)n * tiles * 256 * sizeof(uint32_t), st) != hipSuccess)
    return set_error(IDN_EHIP, "%s: clearing the histograms failed", name);
  exp_launch_hist<EXP_SRC_PLANE, false>(st, src, row_stride, (int64_t)h * row_stride, n, g, nullptr,
                                        hist);
  IDN_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(exp_clahe_lut_kernel, dim3((unsigned)(n * tiles)), dim3(64), 0, st, hist,
                     (uint32_t)exp_clip(clip_limit, area), 255.0f / (float)area, ws + l.luts);
  IDN_CHECK_LAUNCH(name);
  ExpApply a = {};
  a.src = src;
  a.src_stride = row_stride;
  a.src_pitch = (int64_t)h * row_stride;
  a.dst = dst;
  a.dst_stride = row_stride;
  a.dst_pitch = (int64_t)h * row_stride;
  a.luts = ws + l.luts;
  exp_launch_apply<EXP_SRC_PLANE, EXP_OUT_PLANE, false, false>(st, a, n, g);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}

extern "C" int idn_correct_exposure_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                                       int64_t row_stride, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  using namespace idn;
  const char* const name = "idn_correct_exposure_u8";
  constexpr int TX = 4, TY = 4, TILES = TX * TY;  // createCLAHE(clipLimit=2.0, tileGridSize=(4,4))
  constexpr double CLIP_LIMIT = 2.0;
  if (int e = check_src_dst(name, src, dst, n, h, w, "operation")) return e;
  if (int e = check_row_stride(name, row_stride, w, 3, "3")) return e;
  IDN_CHECK_ARG(h > TY && w > TX, "%s: image %d x %d needs more rows and columns than the %d x %d "
                "tile grid", name, h, w, TY, TX);
  if (n == 0) return IDN_OK;
  const ExpLayout l = exp_layout(n, h, w, TILES);
  if (int e = check_workspace(name, workspace, workspace_bytes, l.total)) return e;
  const ExpGeom g = exp_geom(h, w, TX, TY);
  if (int e = exp_check_size(n, g, name)) return e;
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + l.hist);
  uint32_t* ihist = reinterpret_cast<uint32_t*>(ws + l.ihist);
  uint8_t* plane = ws + l.plane;
  const hipStream_t st = as_stream(stream);
  const int area = g.th * g.tw;
  const uint32_t clip = (uint32_t)exp_clip(CLIP_LIMIT, area);
  const float scale = 255.0f / (float)area;
  const int64_t pitch = (int64_t)h * row_stride;
  const size_t hist_bytes = (size_t)n * TILES * 256 * sizeof(uint32_t);

  // tile and image histograms are adjacent: one clear
  if (hipMemsetAsync(hist, 0, hist_bytes + (size_t)n * 256 * sizeof(uint32_t), st) != hipSuccess)
    return set_error(IDN_EHIP, "%s: clearing the histograms failed", name);
  exp_launch_hist<EXP_SRC_BGR_TONE, false>(st, src, row_stride, pitch, n, g, nullptr, hist);
  IDN_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(exp_clahe_lut_kernel, dim3((unsigned)(n * TILES)), dim3(64), 0, st, hist, clip,
                     scale, ws + l.luts);
  IDN_CHECK_LAUNCH(name);
  ExpApply a = {};
  a.src = src;
  a.src_stride = row_stride;
  a.src_pitch = pitch;
  a.dst = plane;
  a.dst_stride = w;
  a.dst_pitch = (int64_t)h * w;
  a.luts = ws + l.luts;
  a.ihist = ihist;
  exp_launch_apply<EXP_SRC_BGR_TONE, EXP_OUT_PLANE, false, true>(st, a, n, g);
  IDN_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(exp_equalize_lut_kernel, dim3((unsigned)n), dim3(64), 0, st, ihist,
                     (uint32_t)(h * w), ws + l.eq);
  IDN_CHECK_LAUNCH(name);
  // the second CLAHE sees the equalised plane: its histograms and its blend go through the table
  if (hipMemsetAsync(hist, 0, hist_bytes, st) != hipSuccess)
    return set_error(IDN_EHIP, "%s: clearing the histograms failed", name);
  exp_launch_hist<EXP_SRC_PLANE, true>(st, plane, w, (int64_t)h * w, n, g, ws + l.eq, hist);
  IDN_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(exp_clahe_lut_kernel, dim3((unsigned)(n * TILES)), dim3(64), 0, st, hist, clip,
                     scale, ws + l.luts);
  IDN_CHECK_LAUNCH(name);
  ExpApply f = {};
  f.src = plane;
  f.src_stride = w;
  f.src_pitch = (int64_t)h * w;
  f.bgr = src;
  f.bgr_stride = row_stride;
  f.bgr_pitch = pitch;
  f.dst = dst;
  f.dst_stride = row_stride;
  f.dst_pitch = pitch;
  f.luts = ws + l.luts;
  f.prelut = ws + l.eq;
  exp_launch_apply<EXP_SRC_PLANE, EXP_OUT_BGR, true, false>(st, f, n, g);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}
