// Total-variation denoising: skimage 0.14.2's restoration.denoise_tv_chambolle(x, weight, eps,
// n_iter_max, multichannel=True) on u8 images (Chambolle's projection algorithm on the dual).  Not
// on the reference's preprocessing path: the edge-preserving member of the bank between the
// bilateral filter and non-local means.  tests/tv_model.py restates the algorithm in float64 and
// defines the result.
//
// Every (image, channel) is a plane of its own with its own stopping iteration.  A plane's state is
// the dual field P = (p0, p1), one float2 per pixel, in two buffers; iteration i reads the buffer
// of parity i - 1 and writes the buffer of parity i (the Jacobi update needs the old neighbours, and
// a plane that stops at i returns the image formed from the duals before i's update: the buffer it
// read, which nothing overwrites afterwards).  im = byte / 255 is not stored: it is read from the
// interleaved source bytes through a 256-entry table.  Per iteration a pixel reads 8 B of duals
// and 1 B of image and writes 8 B; the neighbours' duals come out of L1 / L2.
//
// tv_iter_kernel<FIRST>: one launch per iteration.  A 256-thread workgroup owns TV_TW columns x
// TV_TH rows of one plane; a lane owns a column and walks down it, carrying the row above in
// registers, so per row it loads P(y+1, x), p1(y+1, x-1), P(y, x+1) and two image bytes.  No LDS
// tile and no barrier in the walk: the right neighbour's `out` is recomputed by the lane itself.
// The loads run a row ahead of their use (row y + 2 is asked for while row y is worked on), which
// keeps two rows per lane in flight.
// In one pass it forms d (the divergence of the old duals) and out = im + d at (y, x), (y+1, x)
// and (y, x+1), the gradient, the dual update and the pixel's two energy terms d^2 and |g|.  The
// state is fp32 and the update is fp32 arithmetic in the model's operation order; the energy
// terms are added in fp64: a lane's in row order, the lanes' in a fixed butterfly, the waves' in
// order.  The workgroup stores its pair of sums as one partial (two buffers by parity).  FIRST is
// iteration 0: the duals are zero and are not read, so the workspace may be dirty.
//
// The stopping rule runs on the device without atomics, without a grid-wide barrier and without a
// launch of its own: at the start of launch i every workgroup adds its plane's partials of
// iteration i - 1 in a fixed order (wave 0, tv_energy), so all of them obtain the same bits, and
// evaluates |E_prev - E| < eps * E_init against the plane's state record written during launch
// i - 1.  Workgroup 0 of the plane writes the new record (two records by parity: the others still
// read the old one).  A plane that is done exits at once, in this launch after the decision and
// in every later one on reading its record, before anything else.
// tv_final_kernel takes the same decision once more after the last launch and leaves iters and
// the surviving buffer in the record; tv_out_kernel forms out = im + d from that buffer and writes
// f32 and / or u8 = clip(rint(255 out)).  Nothing depends on timing or on the other planes of the
// batch: a plane gives the same bits, iters included, on every call and in every batch.
#include "idn_common.hpp"
#include "abi_args.hpp"

#include <limits.h>
#include <math.h>

namespace idn {

constexpr int TV_TW = 256;  // columns per workgroup: one per lane
constexpr int TV_TH = 64;   // rows per workgroup: the walk of a lane (tuning build: IDN_TV_ROWS)

struct TvState {
  double e_prev, e_init;
  int32_t done, iters;
  int32_t sel, pad;  // sel: the dual buffer `out` is formed from, -1 = none (out = im)
};
static_assert(sizeof(TvState) == 32, "TvState layout");

struct TvLayout {
  size_t state, part, dual, total;  // byte offsets of state[2], part[2], dual[2]
  int tiles_x, tiles_y, rows;
};

static TvLayout tv_layout(int n, int h, int w, int c) {
  TvLayout L;
  L.rows = knob("IDN_TV_ROWS", TV_TH);
  if (L.rows < 1) L.rows = TV_TH;
  L.tiles_x = (w + TV_TW - 1) / TV_TW;
  L.tiles_y = (h + L.rows - 1) / L.rows;
  const size_t planes = (size_t)n * c;
  const size_t tpp = (size_t)L.tiles_x * L.tiles_y;
  Bump ws;
  L.state = ws.take(2 * planes * sizeof(TvState));
  L.part = ws.take(2 * planes * tpp * 2 * sizeof(double));
  L.dual = ws.take(2 * planes * (size_t)h * w * sizeof(float2));
  L.total = ws.total;
  return L;
}

// the 64 lanes' values added in a fixed butterfly: every lane returns the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// E of one iteration from a plane's partials (wave-wide, every lane returns the same bits)
__device__ __forceinline__ double tv_energy(const double* __restrict__ part, int npart,
                                            double weight, double npix) {
  const int l = threadIdx.x & 63;
  double s2 = 0.0, sn = 0.0;
  for (int k = l; k < npart; k += 64) {
    s2 += part[2 * k];
    sn += part[2 * k + 1];
  }
  s2 = wave_sum(s2);
  sn = wave_sum(sn);
  double e = s2;
  e += weight * sn;
  return e / npix;
}

// The decision taken at the start of launch i (i >= 1) from iteration i - 1's partials and the
// record written during launch i - 1 (records exist from launch 1 on).  Wave-wide, same bits in
// every lane and in every workgroup of the plane.
__device__ __forceinline__ TvState tv_decide(int i, const TvState* __restrict__ prev,
                                             const double* __restrict__ part, int npart,
                                             double weight, double eps, double npix) {
  TvState s;
  if (i >= 2) {
    s = *prev;
    if (s.done) return s;
  }
  const double e = tv_energy(part, npart, weight, npix);
  if (i == 1) {
    s.e_prev = s.e_init = e;
    s.done = 0;
    s.iters = 0;
    s.sel = -1;
    s.pad = 0;
  } else if (fabs(s.e_prev - e) < eps * s.e_init) {
    s.done = 1;
    s.iters = i - 1;   // iteration i - 1 breaks: it read the buffer of parity i - 2
    s.sel = i & 1;
  } else {
    s.e_prev = e;
  }
  return s;
}

__device__ __forceinline__ void tv_fill_lut(float* lut) {
  lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
}

template <bool FIRST>
__global__ __launch_bounds__(256) void tv_iter_kernel(
    const uint8_t* __restrict__ src, int h, int w, int c, int64_t row_stride, int tiles_x,
    int tiles_y, int rows, int iter, float quarter_over_weight, double weight, double eps,
    const TvState* __restrict__ st_prev, TvState* __restrict__ st_new,
    const double* __restrict__ part_prev, double* __restrict__ part_new,
    const float2* __restrict__ dual_old, float2* __restrict__ dual_new) {
  __shared__ float lut[256];
  __shared__ double wsum[4][2];
  __shared__ int skip;

  const int t = threadIdx.x;
  const int tpp = tiles_x * tiles_y;
  const int plane = blockIdx.x / tpp;
  const int tile = blockIdx.x - plane * tpp;
  const int tyi = tile / tiles_x;
  const int txi = tile - tyi * tiles_x;

  if (!FIRST && iter >= 2) {  // a finished plane: pass its record on and leave
    const TvState* rec = st_prev + plane;
    if (rec->done) {
      if (tile == 0 && t == 0) st_new[plane] = *rec;
      return;
    }
  }
  tv_fill_lut(lut);
  if (!FIRST) {
    if (t < 64) {
      const TvState s = tv_decide(iter, st_prev + plane, part_prev + (int64_t)plane * tpp * 2, tpp,
                                  weight, eps, (double)h * (double)w);
      if (tile == 0 && t == 0) st_new[plane] = s;
      if (t == 0) skip = s.done;
    }
  }
  __syncthreads();
  if (!FIRST && skip) return;

  const int img = plane / c;
  const int ch = plane - img * c;
  const int x = txi * TV_TW + t;
  const int y0 = tyi * rows;
  const int y1 = min(y0 + rows, h);
  const bool col = x < w;
  const bool right = x + 1 < w;
  const bool left = col && x > 0;

  const int64_t hw = (int64_t)h * w;
  const uint8_t* sp = src + (int64_t)img * h * row_stride + (int64_t)x * c + ch;
  const float2* po = dual_old + (int64_t)plane * hw;
  float2* pn = dual_new + (int64_t)plane * hw;

  double s2 = 0.0, sn = 0.0;
  if (col) {
    // row y0: own pixel, the pixel to the right, and p0 of the row above both
    int64_t idx = (int64_t)y0 * w + x;
    float2 pc = make_float2(0.f, 0.f), pr = make_float2(0.f, 0.f);
    float up_c = 0.f, up_r = 0.f, p1l = 0.f;
    if (!FIRST) {
      pc = po[idx];
      if (left) p1l = po[idx - 1].y;
      if (right) pr = po[idx + 1];
      if (y0 > 0) {
        up_c = po[idx - w].x;
        if (right) up_r = po[idx - w + 1].x;
      }
    }
    float im_c = lut[sp[(int64_t)y0 * row_stride]];
    float d_c = -(pc.x + pc.y);
    if (y0 > 0) d_c += up_c;
    if (x > 0) d_c += p1l;
    float o_c = im_c + d_c;

    // two rows of loads in flight: the row below was loaded a step ago, row y + 2 is asked for now
    float2 pb = make_float2(0.f, 0.f);
    float p1lb = 0.f;
    uint32_t bb = 0, br = 0;
    if (y0 + 1 < h) {
      if (!FIRST) {
        pb = po[idx + w];
        if (left) p1lb = po[idx + w - 1].y;
      }
      bb = sp[(int64_t)(y0 + 1) * row_stride];
    }
    if (right) br = sp[(int64_t)y0 * row_stride + c];
    for (int y = y0; y < y1; ++y, idx += w) {
      const bool below = y + 1 < h;
      float2 pb2 = make_float2(0.f, 0.f), pr2 = make_float2(0.f, 0.f);
      float p1lb2 = 0.f;
      uint32_t bb2 = 0, br2 = 0;
      if (y + 1 < y1) {  // this workgroup also owns row y + 1 (so y + 1 < h)
        if (y + 2 < h) {
          if (!FIRST) {
            pb2 = po[idx + 2 * (int64_t)w];
            if (left) p1lb2 = po[idx + 2 * (int64_t)w - 1].y;
          }
          bb2 = sp[(int64_t)(y + 2) * row_stride];
        }
        if (right) {
          if (!FIRST) pr2 = po[idx + w + 1];
          br2 = sp[(int64_t)(y + 1) * row_stride + c];
        }
      }
      float o_b = 0.f, d_b = 0.f;
      if (below) {
        d_b = -(pb.x + pb.y);
        d_b += pc.x;
        if (x > 0) d_b += p1lb;
        o_b = lut[bb] + d_b;
      }
      float g1 = 0.f;
      if (right) {
        float d_r = -(pr.x + pr.y);
        if (y > 0) d_r += up_r;
        d_r += pc.y;
        const float o_r = lut[br] + d_r;
        g1 = o_r - o_c;
      }
      const float g0 = below ? o_b - o_c : 0.f;
      const float nrm = sqrtf(g0 * g0 + g1 * g1);
      s2 += (double)d_c * (double)d_c;
      sn += (double)nrm;
      const float den = nrm * quarter_over_weight + 1.0f;
      float2 q;
      q.x = (pc.x - 0.25f * g0) / den;
      q.y = (pc.y - 0.25f * g1) / den;
      pn[idx] = q;
      up_r = pr.x;
      pr = pr2;
      br = br2;
      pc = pb;
      d_c = d_b;
      o_c = o_b;
      pb = pb2;
      p1lb = p1lb2;
      bb = bb2;
    }
  }

  s2 = wave_sum(s2);
  sn = wave_sum(sn);
  if ((t & 63) == 0) {
    wsum[t >> 6][0] = s2;
    wsum[t >> 6][1] = sn;
  }
  __syncthreads();
  if (t == 0) {
    double* q = part_new + ((int64_t)plane * tpp + tile) * 2;
    q[0] = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
    q[1] = ((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1];
  }
}

// one wave per plane: the decision after the last launch, iters, and the buffer `out` comes from
__global__ __launch_bounds__(64) void tv_final_kernel(int n_iter_max, int tpp, double weight,
                                                      double eps, double npix,
                                                      const TvState* __restrict__ st_prev,
                                                      TvState* __restrict__ st_new,
                                                      const double* __restrict__ part_prev,
                                                      int32_t* __restrict__ iters_out) {
  const int plane = blockIdx.x;
  TvState s;
  if (n_iter_max == 1) {
    s.e_prev = s.e_init = 0.0;
    s.done = 1;
    s.iters = 1;
    s.sel = -1;
    s.pad = 0;
  } else {
    s = tv_decide(n_iter_max, st_prev + plane, part_prev + (int64_t)plane * tpp * 2, tpp, weight,
                  eps, npix);
    if (!s.done) {  // exhausted: out is the one iteration n_iter_max - 1 formed
      s.done = 1;
      s.iters = n_iter_max;
      s.sel = n_iter_max & 1;
    }
  }
  if (threadIdx.x == 0) {
    st_new[plane] = s;
    if (iters_out) iters_out[plane] = s.iters;
  }
}

// out = im + d from the surviving buffer; a lane owns one interleaved byte column of one row
__global__ __launch_bounds__(256) void tv_out_kernel(const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst_u8,
                                                     float* __restrict__ dst_f32, int h, int w,
                                                     int c, int64_t row_stride, int tiles,
                                                     const TvState* __restrict__ st,
                                                     const float2* __restrict__ dual0,
                                                     const float2* __restrict__ dual1) {
  __shared__ float lut[256];
  tv_fill_lut(lut);
  __syncthreads();
  const int wb = w * c;
  const int rows = blockIdx.x / tiles;  // image * h + y
  const int tile = blockIdx.x - rows * tiles;
  const int img = rows / h;
  const int y = rows - img * h;
  const int xb = tile * 256 + threadIdx.x;
  if (xb >= wb) return;
  const int x = xb / c;
  const int ch = xb - x * c;
  const int plane = img * c + ch;
  const int sel = st[plane].sel;
  float o = lut[src[(int64_t)rows * row_stride + xb]];
  if (sel >= 0) {
    const int64_t hw = (int64_t)h * w;
    const float2* p = (sel ? dual1 : dual0) + (int64_t)plane * hw;
    const int64_t idx = (int64_t)y * w + x;
    const float2 pc = p[idx];
    float d = -(pc.x + pc.y);
    if (y > 0) d += p[idx - w].x;
    if (x > 0) d += p[idx - 1].y;
    o += d;
  }
  if (dst_f32) dst_f32[(int64_t)rows * wb + xb] = o;
  if (dst_u8) {
    double v = rint(255.0 * (double)o);
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
    dst_u8[(int64_t)rows * row_stride + xb] = (uint8_t)(int)v;
  }
}

static bool tv_shape_ok(int n, int h, int w, int c) {
  return n >= 0 && h >= 1 && w >= 1 && (c == 1 || c == 3);
}

}  // namespace idn

extern "C" size_t idn_tv_chambolle_workspace_size(int n, int h, int w, int c) {
  using namespace idn;
  if (!tv_shape_ok(n, h, w, c) || n == 0) return 0;
  return tv_layout(n, h, w, c).total;
}

extern "C" int idn_tv_chambolle_u8(const uint8_t* src, uint8_t* dst_u8, float* dst_f32,
                                   int32_t* iters, int n, int h, int w, int c, int64_t row_stride,
                                   double weight, double eps, int n_iter_max, void* workspace,
                                   size_t ws_bytes, void* stream) {
  using namespace idn;
  const char* name = "idn_tv_chambolle_u8";
  IDN_CHECK_ARG(src, "%s: null pointer (src)", name);
  IDN_CHECK_ARG(dst_u8 || dst_f32, "%s: no destination (dst_u8 and dst_f32 are both null)", name);
  if (int e = check_not_in_place(name, src, dst_u8, "dst_u8 is src")) return e;
  if (int e = check_image_1_or_3(name, n, h, w, c, row_stride)) return e;
  IDN_CHECK_ARG(isfinite(weight) && weight > 0.0, "%s: weight must be positive and finite", name);
  IDN_CHECK_ARG(isfinite(eps) && eps >= 0.0, "%s: eps must be finite and not negative", name);
  IDN_CHECK_ARG(n_iter_max >= 1 && n_iter_max <= IDN_TV_MAX_ITER,
                "%s: n_iter_max must be in 1..%d (got %d)", name, IDN_TV_MAX_ITER, n_iter_max);
  if (n == 0) return IDN_OK;
  const TvLayout L = tv_layout(n, h, w, c);
  const int64_t planes = (int64_t)n * c;
  const int64_t tpp = (int64_t)L.tiles_x * L.tiles_y;
  const int64_t out_tiles = ((int64_t)w * c + 255) / 256;
  if ((int64_t)w * c > INT_MAX || planes * tpp > INT_MAX || (int64_t)n * h * out_tiles > INT_MAX)
    return batch_too_large(name);
  if (int e = check_workspace(name, workspace, ws_bytes, L.total)) return e;

  char* base = static_cast<char*>(workspace);
  TvState* state[2];
  double* part[2];
  float2* dual[2];
  for (int k = 0; k < 2; ++k) {
    state[k] = reinterpret_cast<TvState*>(base + L.state) + k * planes;
    part[k] = reinterpret_cast<double*>(base + L.part) + k * planes * tpp * 2;
    dual[k] = reinterpret_cast<float2*>(base + L.dual) + k * planes * (int64_t)h * w;
  }
  const hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)(planes * tpp);
  const float qow = (float)(0.25 / weight);
  const double npix = (double)h * (double)w;
  if (n_iter_max > 1) {
    hipLaunchKernelGGL((tv_iter_kernel<true>), dim3(grid), dim3(256), 0, st, src, h, w, c,
                       row_stride, L.tiles_x, L.tiles_y, L.rows, 0, qow, weight, eps,
                       (const TvState*)nullptr, (TvState*)nullptr, (const double*)nullptr, part[0],
                       (const float2*)nullptr, dual[0]);
    IDN_CHECK_LAUNCH(name);
    for (int i = 1; i < n_iter_max; ++i) {
      const int a = i & 1, b = a ^ 1;  // reads parity i - 1 (b), writes parity i (a)
      hipLaunchKernelGGL((tv_iter_kernel<false>), dim3(grid), dim3(256), 0, st, src, h, w, c,
                         row_stride, L.tiles_x, L.tiles_y, L.rows, i, qow, weight, eps,
                         (const TvState*)state[b], state[a], (const double*)part[b], part[a],
                         (const float2*)dual[b], dual[a]);
      IDN_CHECK_LAUNCH(name);
    }
  }
  const int fa = n_iter_max & 1, fb = fa ^ 1;
  hipLaunchKernelGGL(tv_final_kernel, dim3((unsigned)planes), dim3(64), 0, st, n_iter_max,
                     (int)tpp, weight, eps, npix, (const TvState*)state[fb], state[fa],
                     (const double*)part[fb], iters);
  IDN_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(tv_out_kernel, dim3((unsigned)((int64_t)n * h * out_tiles)), dim3(256), 0, st,
                     src, dst_u8, dst_f32, h, w, c, row_stride, (int)out_tiles,
                     (const TvState*)state[fa], (const float2*)dual[0], (const float2*)dual[1]);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}
