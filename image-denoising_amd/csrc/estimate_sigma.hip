// idn_estimate_sigma: skimage.restoration.estimate_sigma per (image, channel) plane, the median
// absolute finest diagonal db2 coefficient over Phi^-1(0.75), bit-equal to tests/sigma_model.py.
//
// The fp64 band is never stored.  Every pass recomputes the keys |d| from the image: a lane walks
// down one (extended) column and forms the vertical high-pass of an output row from a sliding
// window of four input rows, the 256 column results of the row go through LDS, and 127 lanes form
// the horizontal high-pass over four neighbouring columns.  The arithmetic is pywt's, in pywt's
// order (multiply, then add, no FMA: the unit is built with -ffp-contract=off), because which
// coefficients are exactly zero and where the ~1e-31 keys of a flat region rank is part of the
// result; an fp32 or reordered form changes the ranks, not the last bits.  (The model's leading
// `0.0 +` is left out: it can only turn a -0.0 into +0.0, and zeros of either sign are dropped.)
//
// The median is an exact rank selection on the key bits (non-negative doubles order like their bit
// patterns), most significant digit first, for the two ranks (m - 1) / 2 and m / 2 of the m
// nonzero keys.  A pass at `level` looks at the keys that share the digits selected so far:
//   * more than SIG_CAP of them: it counts their next 11-bit digit (8 bits at the last level) in an
//     LDS histogram per workgroup, added into the plane's histogram with integer atomics;
//   * at most SIG_CAP: it appends them to the plane's list, and the scan that follows every pass
//     finishes the selection in LDS.
// Noise-like keys finish in three passes (exponent digit, 11 mantissa bits, list); keys with more
// than SIG_CAP ties on the median go through all six digits, after which the digits are the key.
// A plane of at most SIG_CAP keys is listed by the first pass.  Planes that have finished leave
// the later passes at once.  Counts are integers and the list is ranked by value, so no result
// depends on the order of execution; one workgroup never straddles two planes.
#include "idn_common.hpp"
#include "abi_args.hpp"

#include <limits.h>

namespace idn {

constexpr int SIG_CAP = 1024;     // keys a plane lists for the in-LDS finish
constexpr int SIG_BINS = 2048;    // 11-bit digits
constexpr int SIG_LEVELS = 6;     // 11 + 11 + 11 + 11 + 11 + 8 = 63 key bits
constexpr int SIG_TW = 127;       // output columns per workgroup: 2 * 127 + 2 = 256 input columns
constexpr int SIG_TH = 64;        // output rows per workgroup
constexpr int SIG_ROWS = 2;       // of them per step of the walk
constexpr uint64_t SIG_ABS = 0x7FFFFFFFFFFFFFFFull;

// db2 decomposition high-pass (pywt.Wavelet('db2').dec_hi)
#define SIG_G0 (-0.48296291314453416)
#define SIG_G1 (0.8365163037378079)
#define SIG_G2 (-0.2241438680420134)
#define SIG_G3 (-0.12940952255126037)

// per selected rank r in {0, 1} (the lower and the upper median rank) of one plane
struct SigState {
  uint64_t prefix[2];  // the digits selected so far, in place
  uint64_t value[2];   // the selected key's bits once done
  uint32_t rank[2];    // rank among the keys that share the prefix
  uint32_t cnt[2];     // how many keys share the prefix (an upper bound before the first pass)
  uint32_t done[2];
  uint32_t same;       // both ranks still follow the same prefix: slot 0 counts for both
  uint32_t pad;
};
static_assert(sizeof(SigState) == 64, "SigState layout");

struct SigLayout {
  size_t state, lcnt, hist, list, total;
};

static SigLayout sig_layout(int64_t planes) {
  SigLayout L;
  Bump ws;
  L.state = ws.take((size_t)planes * sizeof(SigState));
  L.lcnt = ws.take((size_t)planes * 2 * sizeof(uint32_t));
  L.hist = ws.take((size_t)planes * 2 * SIG_BINS * sizeof(uint32_t));
  L.list = ws.take((size_t)planes * 2 * SIG_CAP * sizeof(uint64_t));
  L.total = ws.total;
  return L;
}

// digit of `level`: bits [shift, shift + 11) (8 bits at the last level); the prefix is what lies
// above them
__host__ __device__ __forceinline__ int sig_shift(int level) {
  return level == 5 ? 0 : 52 - 11 * level;
}
__host__ __device__ __forceinline__ int sig_above(int level) {
  return level == 0 ? 63 : 63 - 11 * level;
}

__global__ __launch_bounds__(256) void sig_init_kernel(SigState* __restrict__ st,
                                                       uint32_t* __restrict__ lcnt,
                                                       uint32_t* __restrict__ hist,
                                                       uint32_t keys_per_plane) {
  const int plane = blockIdx.x;
  uint32_t* h = hist + (size_t)plane * 2 * SIG_BINS;
  for (int b = threadIdx.x; b < 2 * SIG_BINS; b += 256) h[b] = 0;
  if (threadIdx.x < 2) lcnt[plane * 2 + threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    SigState s;
    for (int r = 0; r < 2; ++r) {
      s.prefix[r] = 0;
      s.value[r] = 0;
      s.rank[r] = 0;
      s.cnt[r] = keys_per_plane;
      s.done[r] = 0;
    }
    s.same = 1;
    s.pad = 0;
    st[plane] = s;
  }
}

// index into a length-n axis of the half-sample symmetric extension, for -n <= i < 2 n
__device__ __forceinline__ int sig_reflect(int i, int n) {
  return i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i);
}

// sum_j g[j] X(i - j) from the window a = X(i-3), b = X(i-2), c = X(i-1), d = X(i): taps 0..3 in
// ascending order, or 2, 1, 0, 3 at i = n + 2 (the model's right-overhang order; at i = n and
// i = n + 1 that order gives the ascending order's value)
__device__ __forceinline__ double sig_taps(double a, double b, double c, double d, bool last_odd) {
  double s;
  if (last_odd) {
    s = SIG_G2 * b;
    s = s + SIG_G1 * c;
    s = s + SIG_G0 * d;
  } else {
    s = SIG_G0 * d;
    s = s + SIG_G1 * c;
    s = s + SIG_G2 * b;
  }
  return s + SIG_G3 * a;
}

// R output rows per step: a lane has the 2 R input rows of a step in flight at once and asks for
// the next step's before it works on this one's; two barriers per step
template <typename T, int R>
__global__ __launch_bounds__(256) void sig_pass_kernel(const T* __restrict__ src, int h, int w,
                                                       int c, int64_t row_stride, int tiles_x,
                                                       int tiles_y, int th, int level,
                                                       const SigState* __restrict__ st,
                                                       uint32_t* __restrict__ lcnt,
                                                       uint32_t* __restrict__ hist,
                                                       uint64_t* __restrict__ list) {
  static_assert(R == 1 || R % 2 == 0, "rows per step");
  __shared__ uint32_t lh[2][SIG_BINS];
  __shared__ __attribute__((aligned(16))) double vrow[R][256];

  // the channels of a tile, then the tiles of an image, are neighbours on one XCD
  int b = xcd_contiguous_block(blockIdx.x, gridDim.x);
  const int ch = b % c;
  b /= c;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  const int img = b / tiles_y;
  const int plane = img * c + ch;

  const SigState S = st[plane];
  if (S.done[0] && S.done[1]) return;
  const int tid = threadIdx.x;
  const int above = sig_above(level), shift = sig_shift(level);
  const uint32_t mask = level == 5 ? 0xFFu : (uint32_t)(SIG_BINS - 1);
  const int nsel = S.same ? 1 : 2;
  bool live[2], listed[2];
  uint64_t want[2];
  for (int r = 0; r < 2; ++r) {
    live[r] = r < nsel && !S.done[r];
    listed[r] = S.cnt[r] <= (uint32_t)SIG_CAP;
    want[r] = S.prefix[r] >> above;
  }
  for (int i = tid; i < 2 * SIG_BINS; i += 256) (&lh[0][0])[i] = 0;

  const int oh = (h + 3) >> 1, ow = (w + 3) >> 1;
  const int oy0 = ty * th, oy1 = min(oy0 + th, oh);
  const int ox0 = tx * SIG_TW;
  // extended column of this lane; lanes past the last column an output reads (its centre, column
  // 2 ow - 1) load column 0 and nobody reads what they make of it.  Every load is unconditional
  // and stays in the image's own type until it is used, so that a step's loads are in flight
  // together: a select or a conversion behind each load would wait for it on the spot
  const int e = 2 * ox0 - 2 + tid;
  const uint32_t loff = (e <= 2 * ow - 1 ? (uint32_t)sig_reflect(e, w) * (uint32_t)c : 0u) + ch;
  const T* base = src + (int64_t)img * h * row_stride;
  const int rmax = 2 * oh - 1;  // the last extended row any output reads
  auto ld = [&](int r) -> T {
    return base[(int64_t)sig_reflect(min(r, rmax), h) * row_stride + loff];
  };
  // the horizontal step: the two halves of the workgroup take two rows of the step at once
  constexpr int HALF = R == 1 ? 256 : 128, ROUNDS = R == 1 ? 1 : R / 2;
  const int hl = tid & (HALF - 1), hk = R == 1 ? 0 : tid >> 7;
  const int ox = ox0 + hl;
  const bool outl = hl < SIG_TW && ox < ow;
  const bool h_last_odd = 2 * ox + 1 == w + 2;

  // rows i - 3, i - 2 of the step's first output (i = 2 oy + 1), then the 2 R rows i - 1 ...
  T nx[2 * R];
  const T ta = ld(2 * oy0 - 2), tb = ld(2 * oy0 - 1);
#pragma unroll
  for (int q = 0; q < 2 * R; ++q) nx[q] = ld(2 * oy0 + q);
  double ra = (double)ta, rb = (double)tb;
  for (int oy = oy0; oy < oy1; oy += R) {
    double cur[2 * R];
#pragma unroll
    for (int q = 0; q < 2 * R; ++q) cur[q] = (double)nx[q];
    if (oy + R < oy1) {  // the next step's rows, asked for before this step's work
#pragma unroll
      for (int q = 0; q < 2 * R; ++q) nx[q] = ld(2 * (oy + R) + q);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      vrow[k][tid] = sig_taps(ra, rb, cur[2 * k], cur[2 * k + 1], 2 * (oy + k) + 1 == h + 2);
      ra = cur[2 * k];
      rb = cur[2 * k + 1];
    }
    __syncthreads();
#pragma unroll
    for (int round = 0; round < ROUNDS; ++round) {
      const int k = 2 * round + hk;
      if (outl && oy + k < oy1) {
        const double* v = &vrow[k][2 * hl];
        const double d = sig_taps(v[0], v[1], v[2], v[3], h_last_odd);
        const uint64_t key = (uint64_t)__double_as_longlong(d) & SIG_ABS;
        if (key != 0) {
          for (int r = 0; r < 2; ++r) {
            if (!live[r] || (key >> above) != want[r]) continue;
            if (listed[r]) {
              const uint32_t at = atomicAdd(&lcnt[plane * 2 + r], 1u);
              if (at < (uint32_t)SIG_CAP) list[((size_t)plane * 2 + r) * SIG_CAP + at] = key;
            } else {
              atomicAdd(&lh[r][(uint32_t)(key >> shift) & mask], 1u);
            }
          }
        }
      }
    }
    __syncthreads();
  }
  for (int r = 0; r < 2; ++r) {
    if (!live[r] || listed[r]) continue;
    uint32_t* g = hist + ((size_t)plane * 2 + r) * SIG_BINS;
    for (int i = tid; i < SIG_BINS; i += 256) {
      const uint32_t v = lh[r][i];
      if (v) atomicAdd(&g[i], v);
    }
  }
}

// one workgroup per plane after every pass: picks each rank's digit from the histogram, or the
// key itself from the list; writes sigma once both ranks are known; clears the counters
__global__ __launch_bounds__(256) void sig_scan_kernel(int level, SigState* __restrict__ st,
                                                       uint32_t* __restrict__ lcnt,
                                                       uint32_t* __restrict__ hist,
                                                       const uint64_t* __restrict__ list,
                                                       double* __restrict__ dst) {
  __shared__ uint64_t keys[SIG_CAP];
  __shared__ uint32_t tsum[256];
  __shared__ SigState ns;
  const int plane = blockIdx.x, tid = threadIdx.x;
  const SigState S = st[plane];
  if (S.done[0] && S.done[1]) return;
  if (tid == 0) ns = S;
  __syncthreads();
  uint32_t* H = hist + (size_t)plane * 2 * SIG_BINS;
  const int shift = sig_shift(level);
  const uint64_t nan_bits = 0x7FF8000000000000ull;

  for (int r = 0; r < 2; ++r) {
    if (S.done[r]) continue;
    const int from = S.same ? 0 : r;
    if (S.cnt[r] <= (uint32_t)SIG_CAP) {
      const uint32_t n = min(lcnt[plane * 2 + from], (uint32_t)SIG_CAP);
      for (uint32_t i = tid; i < n; i += 256)
        keys[i] = list[((size_t)plane * 2 + from) * SIG_CAP + i];
      __syncthreads();
      // before the first pass the ranks are not known: n is the count of nonzero keys
      const uint32_t rank = level == 0 ? (r == 0 ? (n - 1) / 2 : n / 2) : S.rank[r];
      if (n == 0) {
        if (tid == 0) {
          ns.value[r] = nan_bits;
          ns.done[r] = 1;
        }
      } else {
        for (uint32_t i = tid; i < n; i += 256) {
          const uint64_t ki = keys[i];
          uint32_t less = 0, eq = 0;
          for (uint32_t j = 0; j < n; ++j) {
            const uint64_t kj = keys[j];
            less += kj < ki;
            eq += kj == ki;
          }
          if (less <= rank && rank < less + eq) {  // ties write the same bits
            ns.value[r] = ki;
            ns.done[r] = 1;
          }
        }
      }
      __syncthreads();
    } else {
      uint32_t local[8], sum = 0;
      for (int q = 0; q < 8; ++q) {
        local[q] = H[from * SIG_BINS + tid * 8 + q];
        sum += local[q];
      }
      tsum[tid] = sum;
      __syncthreads();
      uint32_t excl = 0, total = 0;
      for (int u = 0; u < 256; ++u) {
        const uint32_t t = tsum[u];
        excl += u < tid ? t : 0;
        total += t;
      }
      const uint32_t rank = level == 0 ? (r == 0 ? (total - 1) / 2 : total / 2) : S.rank[r];
      if (total == 0) {
        if (tid == 0) {
          ns.value[r] = nan_bits;
          ns.done[r] = 1;
        }
      } else if (excl <= rank && rank < excl + sum) {
        uint32_t acc = excl;
        for (int q = 0; q < 8; ++q) {
          if (rank < acc + local[q]) {
            const uint64_t pre = S.prefix[r] | ((uint64_t)(tid * 8 + q) << shift);
            ns.prefix[r] = pre;
            ns.rank[r] = rank - acc;
            ns.cnt[r] = local[q];
            if (level == SIG_LEVELS - 1) {
              ns.value[r] = pre;
              ns.done[r] = 1;
            }
            break;
          }
          acc += local[q];
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    ns.same = !ns.done[0] && !ns.done[1] && ns.prefix[0] == ns.prefix[1];
    st[plane] = ns;
    if (ns.done[0] && ns.done[1]) {
      const double a = __longlong_as_double((long long)ns.value[0]);
      const double b = __longlong_as_double((long long)ns.value[1]);
      dst[plane] = ((a + b) / 2.0) / 0.6744897501960817;  // numpy's median, then norm.ppf(0.75)
    }
  }
  for (int i = tid; i < 2 * SIG_BINS; i += 256) H[i] = 0;
  if (tid < 2) lcnt[plane * 2 + tid] = 0;
}

// IDN_SIG_ROWS (tuning build only): output rows per step of the pass, 1 / 2 / 4 / 8;
// IDN_SIG_TH: output rows per workgroup
template <typename T>
static void sig_launch_pass(int rows, unsigned grid, hipStream_t s, const T* src, int h, int w,
                            int c, int64_t row_stride, int tiles_x, int tiles_y, int th,
                            int level, const SigState* st, uint32_t* lcnt, uint32_t* hist,
                            uint64_t* list) {
#define SIG_LAUNCH(R)                                                                          \
  hipLaunchKernelGGL((sig_pass_kernel<T, R>), dim3(grid), dim3(256), 0, s, src, h, w, c,       \
                     row_stride, tiles_x, tiles_y, th, level, st, lcnt, hist, list)
#ifdef IDN_TUNING_BUILD
  if (rows == 1) {
    SIG_LAUNCH(1);
    return;
  }
  if (rows == 2) {
    SIG_LAUNCH(2);
    return;
  }
  if (rows == 8) {
    SIG_LAUNCH(8);
    return;
  }
#endif
  (void)rows;
  SIG_LAUNCH(SIG_ROWS);
#undef SIG_LAUNCH
}

static bool sig_shape_ok(int n, int h, int w, int c) {
  return n > 0 && h >= 4 && w >= 4 && (c == 1 || c == 3);
}

}  // namespace idn

extern "C" size_t idn_estimate_sigma_workspace_size(int n, int h, int w, int c, int is_f64) {
  using namespace idn;
  (void)is_f64;  // both source types recompute their keys: the scratch holds counters only
  if (!sig_shape_ok(n, h, w, c)) return 0;
  return sig_layout((int64_t)n * c).total;
}

extern "C" int idn_estimate_sigma(const uint8_t* src_u8, const double* src_f64, double* dst, int n,
                                  int h, int w, int c, int64_t row_stride, void* workspace,
                                  size_t ws_bytes, void* stream) {
  using namespace idn;
  const char* name = "idn_estimate_sigma";
  IDN_CHECK_ARG((src_u8 != nullptr) != (src_f64 != nullptr),
                "%s: exactly one of src_u8 and src_f64 must be given (null pointer otherwise)", name);
  IDN_CHECK_ARG(dst, "%s: null pointer (dst)", name);
  if (int e = check_image_1_or_3(name, n, h, w, c, row_stride)) return e;
  IDN_CHECK_ARG(!src_f64 || ((uintptr_t)src_f64 & 7) == 0, "%s: src_f64 must be 8-byte aligned",
                name);
  IDN_CHECK_ARG(((uintptr_t)dst & 7) == 0, "%s: dst must be 8-byte aligned", name);
  if (h < 4 || w < 4)
    return set_error(IDN_EUNSUPPORTED, "%s: h and w must be at least 4 (got %d x %d): the db2 "
                     "symmetric extension reflects once", name, h, w);
  if (n == 0) return IDN_OK;
  const int64_t planes = (int64_t)n * c;
  const int oh = (h + 3) / 2, ow = (w + 3) / 2;
  const int th_knob = knob("IDN_SIG_TH", SIG_TH);
  const int th = th_knob < 1 ? 1 : th_knob;
  const int tiles_x = (ow + SIG_TW - 1) / SIG_TW, tiles_y = (oh + th - 1) / th;
  if ((int64_t)w * c > INT_MAX || planes * tiles_x * tiles_y > INT_MAX ||
      (int64_t)oh * ow > (int64_t)UINT_MAX)
    return batch_too_large(name);
  const SigLayout L = sig_layout(planes);
  if (int e = check_workspace(name, workspace, ws_bytes, L.total)) return e;

  char* base = static_cast<char*>(workspace);
  SigState* st = reinterpret_cast<SigState*>(base + L.state);
  uint32_t* lcnt = reinterpret_cast<uint32_t*>(base + L.lcnt);
  uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
  uint64_t* list = reinterpret_cast<uint64_t*>(base + L.list);
  const hipStream_t s = as_stream(stream);
  const unsigned grid = (unsigned)(planes * tiles_x * tiles_y);
  const int rows = knob("IDN_SIG_ROWS", SIG_ROWS);

  hipLaunchKernelGGL(sig_init_kernel, dim3((unsigned)planes), dim3(256), 0, s, st, lcnt, hist,
                     (uint32_t)((int64_t)oh * ow));
  IDN_CHECK_LAUNCH(name);
  for (int level = 0; level < SIG_LEVELS; ++level) {
    if (src_u8)
      sig_launch_pass<uint8_t>(rows, grid, s, src_u8, h, w, c, row_stride, tiles_x, tiles_y, th,
                               level, st, lcnt, hist, list);
    else
      sig_launch_pass<double>(rows, grid, s, src_f64, h, w, c, row_stride, tiles_x, tiles_y, th,
                              level, st, lcnt, hist, list);
    IDN_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(sig_scan_kernel, dim3((unsigned)planes), dim3(256), 0, s, level, st, lcnt,
                       hist, (const uint64_t*)list, dst);
    IDN_CHECK_LAUNCH(name);
  }
  return IDN_OK;
}
