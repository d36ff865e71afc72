// The adaptive median filter (Hwang & Haddad 1995; Gonzalez & Woods §5.3) on interleaved u8
// HxWxC images, BORDER_REPLICATE, per channel plane, bit-exact to tests/adaptive_median_model.py:
//   for k = 3, 5, .., K:  mn, mx, md = min, max, median (rank k*k/2) of the k x k window
//     if mn < md < mx:  out = (mn < z < mx) ? z : md;  ksize = k;  stop
//   no k passed:        out = md of the K x K window;  ksize = 0
//
// One launch, no workspace.  A workgroup of four waves stages a tile of AMED_ROWS + K - 1 rows by
// AMED_SEG + 2 (K/2) C bytes in LDS (byte loads: any pointer alignment, any row_stride, any C; the
// replicated rows and columns are resolved while staging, so the filter itself never clamps).  Wave
// v then owns the 64 adjacent output bytes v*64.. of the tile's rows, a byte per lane (channels
// interleaved: the window neighbours of byte b are b +- j*C), and marches down the rows.  The level
// loop is wave-uniform: a wave leaves it when none of its lanes is undecided.
//
// Level 3 runs by its definition on nine registers: the column-sort network gives mn, md and mx in
// about 30 min / max.  Most waves end there.
// From 5 on stage A needs no median.  With n = k*k, md == mn exactly when at least (n+1)/2 samples
// equal mn, likewise for mx, so  mn < md < mx  <=>  mn != mx && count(== mn) <= (n-1)/2 &&
// count(== mx) <= (n-1)/2  (tests/test_adaptive_median.py proves it on the model).  The exact
// median is computed only when a lane of the wave passed A with z itself the extreme, at that
// level: an 8-step bisection on the value, the largest t with count(< t) <= rank.  The
// fall-through needs none: stage A failed at K, so the median at K is mn (its count exceeds
// (n-1)/2, or mn == mx) or mx.
// Levels 5 and 7 keep the window in registers, four samples to a dword, and count with v_sad_u8:
// f(t) = sum |v - t| has the slope f(t) - f(t-1) = 2 count(v < t) - N, so a count over the whole
// window is two chains of N/4 sad instructions; count(== mn) is count(< mn + 1) and count(== mx)
// is n - count(< mx).  Beyond 7 the windows nest: a lane carries mn, mx and the two counts from k
// to k + 2 through the 4 (k + 1) samples of the new ring in the staged tile, O(k) per level, and
// the bisection counts over the tile.
#include "idn_common.hpp"
#include "abi_args.hpp"

namespace idn {

constexpr int AMED_SEG = 256;   // output bytes of a row per workgroup (64 per wave)
constexpr int AMED_ROWS = 32;   // output rows per workgroup at most
constexpr int AMED_NS = (AMED_SEG + 2 * 15 * 4 + 63) / 64;  // staged bytes per lane and row (C <= 4)

__device__ __forceinline__ uint32_t amed_med3(uint32_t a, uint32_t b, uint32_t c) {
  return max(min(a, b), min(max(a, b), c));
}

// NS samples packed four to a dword in p[NR], the 4 NR - NS spare bytes 0
template <int NR, int NS>
struct AmedPacked {
  // sum |v - t| over the 4 NR bytes, t in 0..255
  static __device__ __forceinline__ uint32_t l1(const uint32_t (&p)[NR], uint32_t t) {
    const uint32_t t4 = t * 0x01010101u;
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < NR; ++i) s = __builtin_amdgcn_sad_u8(p[i], t4, s);
    return s;
  }
  // count(v < t) over the samples, t in 1..255: a byte below t adds 1 to f(t) - f(t-1), any other
  // takes 1 off, and the spare bytes are below every t
  static __device__ __forceinline__ uint32_t count_lt(const uint32_t (&p)[NR], uint32_t t) {
    return (l1(p, t) + 4u * NR - l1(p, t - 1u)) / 2u - (4u * NR - NS);
  }
  // rank NS / 2 of the sorted samples
  static __device__ __forceinline__ uint32_t median(const uint32_t (&p)[NR]) {
    uint32_t lo = 0;
#pragma unroll
    for (int bit = 7; bit >= 0; --bit) {
      const uint32_t t = lo | (1u << bit);
      lo = count_lt(p, t) <= (uint32_t)(NS / 2) ? t : lo;
    }
    return lo;
  }
  // count(== mn) and count(== mx) of the window's extremes
  static __device__ __forceinline__ void extreme_counts(const uint32_t (&p)[NR], uint32_t mn,
                                                        uint32_t mx, uint32_t& cmn, uint32_t& cmx) {
    const bool flat = mn == mx;  // then mn + 1 may be 256 and mx may be 0: not for count_lt
    const uint32_t a = count_lt(p, flat ? 1u : mn + 1u);
    const uint32_t b = count_lt(p, flat ? 1u : mx);
    cmn = flat ? (uint32_t)NS : a;
    cmx = flat ? (uint32_t)NS : (uint32_t)NS - b;
  }
};

// the median of the (2 r + 1)^2 window around tp, counting over the staged tile
__device__ __forceinline__ uint32_t amed_median_tile(const uint8_t* tp, int pitch, int c, int r) {
  const int k = 2 * r + 1;
  const uint32_t rank = (uint32_t)(k * k / 2);
  uint32_t lo = 0;
  for (int bit = 7; bit >= 0; --bit) {
    const uint32_t t = lo | (1u << bit);
    uint32_t cnt = 0;
    for (int dy = -r; dy <= r; ++dy) {
      const uint8_t* rp = tp + dy * pitch - r * c;
      for (int j = 0; j < k; ++j) cnt += (uint32_t)rp[j * c] < t;
    }
    lo = cnt <= rank ? t : lo;
  }
  return lo;
}

__global__ __launch_bounds__(256) void adaptive_median_u8_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint8_t* __restrict__ kmap, int h,
    int w, int c, int rb, int64_t row_stride, int nseg, int bands, int band_rows, int R, int pw,
    int pitch) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tile[];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int item = blockIdx.x;
  const int seg = item % nseg, tq = item / nseg;
  const int band = tq % bands, img = tq / bands;
  const int y0 = band * band_rows;
  const int y1 = min(y0 + band_rows, h);
  if (y0 >= y1) return;
  const int b0 = seg * AMED_SEG;

  const uint8_t* s = src + (int64_t)img * h * row_stride;
  const int64_t obase = (int64_t)img * h * row_stride;

  // staged byte i of a row is row byte b0 - R*c + i with its pixel clamped into the image
  int coff[AMED_NS];
#pragma unroll
  for (int i = 0; i < AMED_NS; ++i) {
    const int p = b0 - R * c + lane + 64 * i;
    const int ch = (p + 64 * c) % c;
    const int px = clampi((p - ch) / c, 0, w - 1);
    coff[i] = px * c + ch;
  }
  const int nrows = (y1 - y0) + 2 * R;
  for (int t = wv; t < nrows; t += 4) {
    const uint8_t* row = s + (int64_t)clampi(y0 - R + t, 0, h - 1) * row_stride;
    uint32_t v[AMED_NS];
#pragma unroll
    for (int i = 0; i < AMED_NS; ++i) v[i] = lane + 64 * i < pw ? row[coff[i]] : 0u;
#pragma unroll
    for (int i = 0; i < AMED_NS; ++i)
      if (lane + 64 * i < pw) tile[t * pitch + lane + 64 * i] = (uint8_t)v[i];
  }
  __syncthreads();

  const int b = b0 + 64 * wv + lane;  // this lane's byte of the row
  if (b0 + 64 * wv >= rb) return;     // the whole wave lies past the row's end
  const bool active = b < rb;

  for (int y = y0; y < y1; ++y) {
    const uint8_t* tp = tile + (y - y0 + R) * pitch + R * c + 64 * wv + lane;
    const int64_t o = obase + (int64_t)y * row_stride + b;
    // level 3 by its definition, from registers: sort the window's three columns, then
    // mn = min of their minima, mx = max of their maxima and
    // md = med3(max of the minima, med3 of the medians, min of the maxima)
    uint32_t a[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = tp[(i / 3 - 1) * pitch + (i % 3 - 1) * c];
    const uint32_t z = a[4];
    uint32_t lo[3], me[3], hi[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      lo[j] = min(min(a[j], a[3 + j]), a[6 + j]);
      hi[j] = max(max(a[j], a[3 + j]), a[6 + j]);
      me[j] = a[j] + a[3 + j] + a[6 + j] - lo[j] - hi[j];
    }
    uint32_t mn = min(min(lo[0], lo[1]), lo[2]), mx = max(max(hi[0], hi[1]), hi[2]);
    const uint32_t md3 = amed_med3(max(max(lo[0], lo[1]), lo[2]), amed_med3(me[0], me[1], me[2]),
                                   min(min(hi[0], hi[1]), hi[2]));
    const bool pass3 = active && mn < md3 && md3 < mx;
    uint32_t out = pass3 ? (mn < z && z < mx ? z : md3) : z;
    uint32_t ks = pass3 ? 3u : 0u;
    bool undecided = active && !pass3;
    if (R == 1) out = undecided ? md3 : out;  // the fall-through at K = 3
    if (R == 1 || __builtin_amdgcn_ballot_w64(undecided) == 0) {  // wave-uniform
      if (active) {
        dst[o] = (uint8_t)out;
        if (kmap) kmap[o] = (uint8_t)ks;
      }
      continue;
    }

    // stages A and B at radius r from mn, mx and their counts; true when the wave is done
    uint32_t cmn, cmx;
    auto stage = [&](int r, auto&& median) -> bool {
      const uint32_t half = (uint32_t)(2 * r * (r + 1));  // (k*k - 1) / 2
      const bool pass = undecided && mn != mx && cmn <= half && cmx <= half;
      const bool need = pass && !(mn < z && z < mx);
      if (__builtin_amdgcn_ballot_w64(need) != 0) {  // wave-uniform
        const uint32_t md = median();
        out = need ? md : out;
      }
      ks = pass ? (uint32_t)(2 * r + 1) : ks;
      undecided = undecided && !pass;
      if (r == R) {  // stage A failed at K: the median there is one of the extremes
        const bool is_mn = mn == mx || cmn > half;
        out = undecided ? (is_mn ? mn : mx) : out;
        return true;
      }
      return __builtin_amdgcn_ballot_w64(undecided) == 0;
    };

    // level 5: the ring's top and bottom rows, then its two columns, packed behind the 3 x 3
    uint32_t g[16];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      g[j] = tp[-2 * pitch + (j - 2) * c];
      g[5 + j] = tp[2 * pitch + (j - 2) * c];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      g[10 + j] = tp[(j - 1) * pitch - 2 * c];
      g[13 + j] = tp[(j - 1) * pitch + 2 * c];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      mn = min(mn, g[i]);
      mx = max(mx, g[i]);
    }
    uint32_t p[13];  // 25 samples in p[0..6] (3 spare bytes), 49 in p[0..12] (3 spare bytes)
    p[0] = a[0] | a[1] << 8 | a[2] << 16 | a[3] << 24;
    p[1] = a[4] | a[5] << 8 | a[6] << 16 | a[7] << 24;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      p[2 + i] = g[4 * i] | g[4 * i + 1] << 8 | g[4 * i + 2] << 16 | g[4 * i + 3] << 24;
    p[6] = a[8];
    typedef AmedPacked<7, 25> P5;
    {
      const uint32_t(&p5)[7] = reinterpret_cast<const uint32_t(&)[7]>(p);
      P5::extreme_counts(p5, mn, mx, cmn, cmx);
      if (stage(2, [&] { return P5::median(p5); })) {
        if (active) {
          dst[o] = (uint8_t)out;
          if (kmap) kmap[o] = (uint8_t)ks;
        }
        continue;
      }
    }

    // level 7 the same way: 24 more samples
    uint32_t q[24];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      q[j] = tp[-3 * pitch + (j - 3) * c];
      q[7 + j] = tp[3 * pitch + (j - 3) * c];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      q[14 + j] = tp[(j - 2) * pitch - 3 * c];
      q[19 + j] = tp[(j - 2) * pitch + 3 * c];
    }
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      mn = min(mn, q[i]);
      mx = max(mx, q[i]);
    }
    p[6] |= q[0] << 8 | q[1] << 16 | q[2] << 24;
#pragma unroll
    for (int i = 0; i < 5; ++i)
      p[7 + i] = q[3 + 4 * i] | q[4 + 4 * i] << 8 | q[5 + 4 * i] << 16 | q[6 + 4 * i] << 24;
    p[12] = q[23];
    typedef AmedPacked<13, 49> P7;
    P7::extreme_counts(p, mn, mx, cmn, cmx);
    bool done = stage(3, [&] { return P7::median(p); });

    // 9 and beyond: mn, mx and the counts are carried through the ring at radius r in the tile
    auto visit = [&](uint32_t v) {
      cmn = v < mn ? 1u : cmn + (v == mn);
      cmx = v > mx ? 1u : cmx + (v == mx);
      mn = min(mn, v);
      mx = max(mx, v);
    };
    for (int r = 4; !done; ++r) {
      const uint8_t* top = tp - r * pitch - r * c;
      const uint8_t* bot = tp + r * pitch - r * c;
      for (int j = 0; j <= 2 * r; ++j) {
        visit(top[j * c]);
        visit(bot[j * c]);
      }
      const uint8_t* lft = tp - (r - 1) * pitch - r * c;
      const uint8_t* rgt = tp - (r - 1) * pitch + r * c;
      for (int j = 0; j < 2 * r - 1; ++j) {
        visit(lft[j * pitch]);
        visit(rgt[j * pitch]);
      }
      done = stage(r, [&] { return amed_median_tile(tp, pitch, c, r); });
    }
    if (active) {
      dst[o] = (uint8_t)out;
      if (kmap) kmap[o] = (uint8_t)ks;
    }
  }
}

}  // namespace idn

extern "C" int idn_adaptive_median_u8(const uint8_t* src, uint8_t* dst, uint8_t* ksize_map, int n,
                                      int h, int w, int c, int64_t row_stride, int max_ksize,
                                      void* stream) {
  using namespace idn;
  const char* name = "idn_adaptive_median_u8";
  if (int e = check_filter_args(src, dst, n, h, w, c, row_stride, name)) return e;
  IDN_CHECK_ARG(ksize_map != src && ksize_map != dst, "%s: ksize_map aliases src or dst", name);
  if (max_ksize < 3 || max_ksize > 31 || !(max_ksize & 1))
    return set_error(IDN_EUNSUPPORTED, "%s: max_ksize %d not supported (odd, 3..31)", name,
                     max_ksize);
  if (n == 0) return IDN_OK;
  const int64_t rb = (int64_t)w * c;
  IDN_CHECK_ARG(rb < (int64_t)0x7FFFFF00, "%s: row too long", name);
  const int R = max_ksize / 2;
  const int nseg = (int)((rb + AMED_SEG - 1) / AMED_SEG);
  int bands = (h + AMED_ROWS - 1) / AMED_ROWS;
  const int band_rows = (h + bands - 1) / bands;  // equal bands
  bands = (h + band_rows - 1) / band_rows;
  const int64_t total = (int64_t)n * bands * nseg;
  IDN_CHECK_ARG(total < (int64_t)0x7FFFFFFF, "%s: batch too large", name);
  const int pw = AMED_SEG + 2 * R * c;
  const int pitch = (pw + 15) & ~15;
  const size_t lds = (size_t)(band_rows + 2 * R) * pitch;  // at most 62 * 384 bytes
  hipLaunchKernelGGL(adaptive_median_u8_kernel, dim3((unsigned)total), dim3(256), lds,
                     as_stream(stream), src, dst, ksize_map, h, w, c, (int)rb, row_stride, nseg,
                     bands, band_rows, R, pw, pitch);
  IDN_CHECK_LAUNCH(name);
  return IDN_OK;
}
