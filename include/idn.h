/*
 * idn.h — C-ABI of the MI355X-native noise-injection + denoising filter bank.
 *
 * One shared library (image-denoising_amd/idn/libidn_hip.so, hipcc --offload-arch=gfx950)
 * exports every function below with C linkage.  No torch types cross this boundary:
 * plain device pointers, sizes and a hipStream_t passed as `void*`.
 *
 * Conventions (all entry points)
 *   - Images are uint8 HxWxC, channel-interleaved (cv2.imread layout: BGR, C=3), row pitch
 *     `row_stride` bytes (>= W*C), a batch of `n` images laid back to back with image pitch
 *     h*row_stride.  f64 arrays use the same element order with pitch W*C elements.
 *   - Pointers are DEVICE pointers owned by the caller; nothing is allocated inside a call.
 *     Calls that need scratch take (workspace, ws_bytes) and expose idn_*_workspace_size().
 *   - Workspaces (every entry point that takes one).  What the workspace holds on entry does not
 *     matter: a call initialises what it reads, on `stream`, and gives the same bits on a zeroed
 *     buffer, on one full of 0xFF and on what any earlier call left.  Nothing outside
 *     [workspace, workspace + idn_*_workspace_size()) is written, whatever ws_bytes says beyond
 *     it.  Consecutive calls on one stream, of one entry point or of different ones, may share
 *     one buffer of the largest size; calls on two streams need a buffer each.  What a call
 *     leaves in its workspace is unspecified but for the diagnostics documented below
 *     (tests/test_workspace_gpu.py: exact-size guarded workspaces under three fills, the ops one
 *     after the other on one buffer, every op on a side stream).
 *   - Every call is stream-ordered on `stream` (NULL = default stream) and capture-safe
 *     (no sync, no malloc; idn_jpeg_decode_u8 and the one-time Poisson table build are the
 *     documented exceptions).  The RNG position is explicit: Philox4x32 keyed by (seed ^ a per-
 *     mode tag), counter = (element group, stream tag, image id) with image id = offset + i (or
 *     an explicit id array), so results do not depend on how a batch is split across launches,
 *     ranks or memory layouts.  Streams (csrc/noise.hip, noise_poisson.hip,
 *     noise_apply.hpp):
 *       gaussian / speckle, u8-only output  Philox4x32-7, one block per 8 elements: 16-bit
 *         uniforms, fp32 Box-Muller (the extreme radius cell refined to 32 bits from a second
 *         block, |z| <= 6.66), U8 computed as floor(clip(v + 255 n)) / floor(clip(v + v n)) in
 *         fp32 on the 0..255 scale
 *       gaussian / speckle, float64 output  Philox4x32-10, one block per 2 elements: 53-bit
 *         uniforms, fp64 Box-Muller, numpy's float64 apply; U8 = trunc(255 * out) of it
 *       s&p      Philox4x32-7, one block per 4 elements: 16-bit `flipped` / `salted` uniforms
 *                against integer thresholds (|P - p| < 2^-16)
 *       poisson  Philox4x32-7, one block per 4 elements, 32-bit words inverted through the
 *                exact CDF of Poisson(img_as_float(v) * vals)
 *     The host model tests/philox_model.py is the definition of these streams: the kernels are
 *     tested against it draw for draw (tests/test_noise_streams_gpu.py).
 *     The tuning knobs of the kernels are compile-time constants: this library reads no
 *     environment variable.
 *   - Alignment.  A uint8 image pointer (source, destination, pattern, labels) may have any byte
 *     alignment, a float32 / float64 pointer needs only its natural alignment (4 / 8 bytes), and
 *     neither changes a result: the launchers pick their vector forms by the pointers they are
 *     given and fall back to narrower accesses elsewhere (tests/test_alignment_gpu.py).  The
 *     exceptions, each refused with a message: idn_copy_u8 (16-byte pointers and size,
 *     IDN_EINVAL); idn_noise_ycc_u8 (2-byte u8 pointers, 16-byte out_f64, IDN_EUNSUPPORTED: use
 *     idn_noise_u8); idn_gaussian_blob_f32 fuses only a source at 0 mod 8 with a blob at 0 mod
 *     16 (IDN_EUNSUPPORTED otherwise: idn_gaussian_blur_u8 + idn_blob_f32 give the same blob);
 *     the workspaces of idn_mse_u8, idn_ssim_u8, idn_tv_chambolle_u8, idn_estimate_sigma,
 *     idn_equalize_hist_u8, idn_clahe_u8 and idn_correct_exposure_u8 are 8-byte aligned
 *     (IDN_EINVAL).  The other workspaces are taken from the base of a device allocation.
 *   - Return IDN_OK (0) or a negative idn_status; idn_last_error() returns a thread-local
 *     message for the last failing call on the calling thread.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   cv2.GaussianBlur / cv2.blur / cv2.medianBlur / cv2.bilateralFilter calls inside the noise
 *   closures and the post-dispatch denoise hook: lib/model/test.py:193-1607,1787-1831 and
 *   lib/roi_data_layer/minibatch.py:87-1516,1636-1673; skimage random_noise calls at the same
 *   sites; lib/utils/blob.py:17-47 (prep_im_for_blob / im_list_to_blob).
 */
#ifndef IDN_H_
#define IDN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum idn_status {
  IDN_OK = 0,
  IDN_EINVAL = -1,        /* bad shape / stride / parameter                         */
  IDN_EUNSUPPORTED = -2,  /* valid but unsupported combination (e.g. ksize 7)        */
  IDN_EHIP = -3,          /* HIP runtime error (launch failure, ...)                */
  IDN_EWORKSPACE = -4     /* workspace missing or too small                         */
} idn_status;

/* noise kinds for idn_noise_u8 (skimage.util.random_noise modes used on the path) */
typedef enum idn_noise_kind {
  IDN_NOISE_GAUSSIAN = 0, /* out = clip(x + N(mean, sqrt(var)), 0, 1)                */
  IDN_NOISE_SPECKLE = 1,  /* out = clip(x + x*N(mean, sqrt(var)), 0, 1)              */
  IDN_NOISE_SAP = 2,      /* salt & pepper, amount = p0, salt_vs_pepper = p1          */
  IDN_NOISE_POISSON = 3   /* out = clip(Poisson(x*vals)/vals, 0, 1), vals per image    */
} idn_noise_kind;

/* wavelet families: idn_wavelet_denoise_u8 / _ycc take the first two, idn_wavelet_denoise_general
 * all five */
typedef enum idn_wavelet {
  IDN_WAVELET_DB1 = 0,    /* Haar ('db1', skimage default)                           */
  IDN_WAVELET_BIOR15 = 1, /* 'bior1.5' (the reference's in-branch choice)             */
  IDN_WAVELET_DB2 = 2,    /* 'db2'   (F = 4; the wavelet of idn_estimate_sigma)       */
  IDN_WAVELET_SYM4 = 3,   /* 'sym4'  (F = 8)                                          */
  IDN_WAVELET_COIF5 = 4   /* 'coif5' (F = 30; the reference's older recipe)           */
} idn_wavelet;
/* threshold selection and shrinkage of idn_wavelet_denoise_general */
typedef enum idn_wavelet_method {
  IDN_WAVELET_BAYES = 0,  /* per band t = var / sqrt(max(mean(d^2) - var, eps))       */
  IDN_WAVELET_VISU = 1    /* one threshold sigma sqrt(2 log(h w))                      */
} idn_wavelet_method;
typedef enum idn_wavelet_mode {
  IDN_WAVELET_SOFT = 0,   /* pywt.threshold(d, t, 'soft')                             */
  IDN_WAVELET_HARD = 1    /* d where |d| >= t, else 0                                 */
} idn_wavelet_mode;

/* ---- library ------------------------------------------------------------------------- */
/* ABI version of this header; idn_abi_version() returns the library's.  A caller (the ctypes
 * binding idn/_lib.py) refuses a library whose number differs.  History:
 *   3  idn_jpeg_workspace_size / idn_jpeg_decode_u8 gained `flags` before `workspace`
 *      (IDN_JPEG_TURBO); the default decode became IJG libjpeg 9d's; idn_noise_filter_u8
 *      (the fused noise -> 3x3 / 5x5 filter) was removed: compose idn_noise_u8 and the filter
 *   4  idn_abi_version added (no signature changed)
 *   5  idn_noise_ycc_u8 and idn_wavelet_denoise_ycc added (no signature changed)
 *   6  cv2.imread's EXIF orientation: idn_jpeg_decode_u8 turns each image by it (flag
 *      IDN_JPEG_IGNORE_ORIENTATION keeps the decoded layout), idn_jpeg_info reports the turned
 *      size, idn_jpeg_orientation added
 *   7  quality metrics: idn_metrics_workspace_size, idn_mse_u8 and idn_ssim_u8 added (no
 *      signature changed)
 *   8  non-local means: idn_nlmeans_weights and idn_nlmeans_u8 added (no signature changed)
 *   9  colour non-local means: idn_lbgr2lab_u8, idn_lab2lbgr_u8, idn_nlmeans_colored_weights,
 *      idn_nlmeans_colored_workspace_size and idn_nlmeans_colored_u8 added (no signature
 *      changed)
 *  10  total-variation denoising: idn_tv_chambolle_workspace_size and idn_tv_chambolle_u8 added
 *      (no signature changed); later, under the same number, the noise-level estimate:
 *      idn_estimate_sigma_workspace_size and idn_estimate_sigma added (no signature changed);
 *      and the wavelet denoiser's options: idn_wavelet_general_workspace_size and
 *      idn_wavelet_denoise_general added, with IDN_WAVELET_DB2 / SYM4 / COIF5 and the enums
 *      idn_wavelet_method and idn_wavelet_mode (no signature changed; the earlier wavelet entry
 *      points reject the new wavelets)
 *  11  idn_quant_runs_offset added: where each restart of the quant fit leaves its centres and
 *      its inertia in the workspace (no signature changed); later, under the same number,
 *      exposure correction: idn_bgr2yuv_u8, idn_yuv2bgr_u8, idn_equalize_hist_u8, idn_clahe_u8,
 *      idn_exposure_workspace_size and idn_correct_exposure_u8 added (no signature changed);
 *      later, under the same number, the adaptive Wiener filter: idn_wiener_workspace_size and
 *      idn_wiener_u8 added, with the enum idn_wiener_border (no signature changed); later, under
 *      the same number, the wide smoothers: idn_gaussian_taps and idn_gaussian_blur_sigma_u8
 *      added, idn_gaussian_blur_u8 and idn_box_blur_u8 accept every odd ksize 3..31 (no
 *      signature changed); later,
 *      under the same number, the adaptive median filter: idn_adaptive_median_u8 added (no
 *      signature changed); later, under the
 *      same number, the sliding DCT denoiser: idn_dct_denoise_workspace_size and
 *      idn_dct_denoise_u8 added (no signature changed) */
#define IDN_ABI_VERSION 11
int idn_abi_version(void);
const char* idn_version(void);
const char* idn_last_error(void);
/* Test hook, not part of the ABI (exported, deliberately undeclared): the bilateral output
 * step's reciprocal, idn_internal_bl_recip_check, used by tests/test_filters_gpu.py only. */

/* ---- denoising filters (u8 -> u8, src != dst) ------------------------------------------ */

/* The Gaussian smoother, odd ksize in 3..31, BORDER_REFLECT_101 (repeated, so images smaller than
 * the radius are legal): Q8 taps t[0..ksize-1] that sum to 256 (idn_gaussian_taps) and
 *   dst = (sum_i sum_j t[i] t[j] src[y+i-r, x+j-r] + 32768) >> 16.
 * At 3, 5 and 7 this is cv2.GaussianBlur(img, (ksize, ksize), 0) bit for bit (the dyadic kernels);
 * 3 and 5 replace e.g. lib/model/test.py:224, lib/roi_data_layer/minibatch.py:1636-1639 and run the
 * stencil kernels.  Beyond the dyadic kernels tests/blur_model.py is the definition and parity
 * with cv2 is unpinned: OpenCV rounds the taps the same way but, as far as is known, does not
 * renormalise them to 256 (its sum at 29 would be 252 and darken a flat 255 to 247); here a
 * constant image always comes back unchanged.  7..31 run a separable LDS kernel whose cost grows
 * with ksize, not ksize^2: measured on an MI355X, 256 x 600x1000x3, 1.01 / 1.06 / 1.41 / 1.62 /
 * 2.11 ms at 7 / 9 / 15 / 21 / 31 (the copy of the batch: 0.165 ms; 5 on the stencil kernel:
 * 0.166 ms).  Any other ksize: IDN_EUNSUPPORTED. */
int idn_gaussian_blur_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                         int64_t row_stride, int ksize, void* stream);

/* The same with a given sigma (cv2.GaussianBlur(img, (ksize, ksize), sigma) up to the caveat
 * above).  sigma = 0 is idn_gaussian_blur_u8; a negative, NaN or infinite sigma: IDN_EINVAL.
 * Only (3, 0) and (5, 0) run the stencil kernels. */
int idn_gaussian_blur_sigma_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                               int64_t row_stride, int ksize, double sigma, void* stream);

/* Host only, no HIP call: the ksize Q8 taps the two entries above use.  sigma = 0 at 3, 5, 7:
 * [64,128,64], [16,64,96,64,16], [8,28,56,72,56,28,8].  Otherwise s = sigma, or
 * 0.3*((ksize-1)*0.5 - 1) + 0.8 for sigma = 0; g[i] = exp(-(i - ksize/2)^2 / (2 s^2)) in double,
 * t[i] = rint(256 g[i] / sum g), and 256 - sum t is added to the centre tap.  A tap can be 0
 * (the outer ones at 29 and 31) or 256 (the identity, e.g. (3, 0.1)). */
int idn_gaussian_taps(int ksize, double sigma, uint16_t* taps);

/* cv2.blur(img, (ksize, ksize)), odd ksize in 3..31, BORDER_REFLECT_101 (repeated): with S the
 * window's sum, dst = (2 S + ksize^2) / (2 ksize^2); ksize^2 is odd, so S / ksize^2 is never a
 * tie and this is cv2's result under either rounding.  Bit-exact.  3 replaces
 * lib/model/test.py:241,1767, lib/roi_data_layer/minibatch.py:1640-1643 and runs the stencil
 * kernel; 5..31 run running column sums whose cost does not grow with the window's area: measured
 * on an MI355X, 256 x 600x1000x3, 1.12 / 1.25 / 1.48 / 1.70 ms at 5 / 7 / 15 / 31 (idn_wiener_u8
 * with the noise given, same run: 1.29 / 1.35 / 1.54 / 1.79).  Any other ksize: IDN_EUNSUPPORTED. */
int idn_box_blur_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                    int64_t row_stride, int ksize, void* stream);

/* cv2.medianBlur(img, ksize), odd ksize in 3..31, BORDER_REPLICATE: the exact median (rank
 * ksize*ksize/2) of the window per channel, for any h, w >= 1.  3 and 5 run sorting networks,
 * 7..31 a per-lane LDS histogram (no workspace).  Any other ksize: IDN_EUNSUPPORTED.
 * Replaces lib/model/test.py:259, lib/roi_data_layer/minibatch.py:1644-1648. Bit-exact. */
int idn_median_blur_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                       int64_t row_stride, int ksize, void* stream);

/* The adaptive median filter for salt & pepper (Hwang & Haddad 1995; Gonzalez & Woods, "Digital
 * Image Processing", section 5.3), per channel plane of every image, BORDER_REPLICATE, any
 * h, w >= 1 (replicated samples count with their multiplicity).  K = max_ksize is odd, in 3..31.
 * For a sample z at (y, x):
 *   for k = 3, 5, ..., K:
 *     mn, mx = min, max of the k x k window;  md = its median (rank k*k/2 of the sorted window)
 *     if mn < md < mx:                      stage A: the median is not an extreme
 *       dst = (mn < z < mx) ? z : md        stage B, with the mn / mx of this same k
 *       ksize = k;  stop
 *   if no k passed:  dst = md of the K x K window;  ksize = 0
 * The fall-through (no level passes) outputs the median at K, the rule of the 3rd and later
 * editions of Gonzalez & Woods (the 2nd edition outputs z there).  A constant image comes back
 * unchanged with ksize 0 everywhere.  There is no parameter other than K, which caps the window
 * and is no strength: the window grows only where the impulses are dense.
 * ksize_map (nullable) receives ksize per sample, 3..K or 0, in dst's layout with the same
 * row_stride.  No workspace, one launch; any pointer alignment and any row_stride >= w*c, padding
 * bytes of dst and ksize_map are never written.  Bit-equal to tests/adaptive_median_model.py.
 * Any other max_ksize (even, 1, above 31, negative): IDN_EUNSUPPORTED, before any HIP call. */
int idn_adaptive_median_u8(const uint8_t* src, uint8_t* dst, uint8_t* ksize_map /* nullable */,
                           int n, int h, int w, int c, int64_t row_stride, int max_ksize,
                           void* stream);

/* cv2.bilateralFilter(img, d, sigma_color, sigma_space, borderType=BORDER_CONSTANT), c = 3
 * (or 1).  Replaces lib/model/test.py:278, lib/roi_data_layer/minibatch.py:1658-1663.
 * <= 1 LSB vs OpenCV (fp32 summation order). */
int idn_bilateral_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                     int64_t row_stride, int d, double sigma_color, double sigma_space,
                     void* stream);

/* ---- noise generators (skimage.util.random_noise, as called on the path) --------------- */

/* Apply one random_noise mode to a batch of u8 images.
 *   out_u8  (nullable): U8(255*out)  == (255*out).astype(np.uint8), the denoise-branch input
 *   out_f64 (nullable): out itself (float64 in [0,1]), what the "plain" branches return
 *   p0, p1: GAUSSIAN/SPECKLE: mean, var; SAP: amount, salt_vs_pepper; POISSON: unused
 *   replay  (nullable): caller-provided random field, which makes the result bit-exact with
 *     numpy's legacy stream:  GAUSSIAN/SPECKLE: f64 N(mean,sqrt(var)) field (n*h*w*c);
 *     SAP: f64 [2][n*h*w*c] = (random_sample for `flipped`, random_sample for `salted`);
 *     POISSON: f64 per-element Poisson draws (n*h*w*c).  NULL = Philox stream (seed, offset).
 *   workspace: POISSON needs idn_noise_workspace_size() bytes (per-image `vals`); else unused.
 *     (POISSON's CDF / level tables are built once per device by the library and kept.)
 * Replaces skimage random_noise at lib/model/test.py:193-590, minibatch.py:87-490. */
int idn_noise_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h, int w,
                 int c, int64_t row_stride, int kind, double p0, double p1, uint64_t seed,
                 uint64_t offset, const double* replay, void* workspace, size_t ws_bytes,
                 void* stream);
size_t idn_noise_workspace_size(int kind, int n);
/* Diagnostics for the POISSON flat kernel: builds (once per device) the per-vals level tables
 * (vals = 1 .. 256) and copies to ntab_out[9] the thresholds each level holds; a value above
 * cap_out[0] (the LDS capacity) means that level's draws would bisect the global CDF rows
 * instead of the LDS tables.  Synchronous on `stream`. */
int idn_poisson_levels(uint32_t* ntab_out, uint32_t* cap_out, void* stream);
/* As idn_noise_u8 (Philox stream only) with an explicit device array of n image ids instead of
 * offset + i: a mixed batch's images of one noise type (any ids) run as one launch and draw
 * exactly what per-image calls with offset = id would.  Replaces the per-image dispatch of the
 * mix lists (test.py:1611-1677, minibatch.py:1518-1574). */
int idn_noise_ids_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h, int w,
                     int c, int64_t row_stride, int kind, double p0, double p1, uint64_t seed,
                     const uint64_t* image_ids, void* workspace, size_t ws_bytes, void* stream);
/* As idn_noise_ids_u8, addressing the batch through a device array of n slots (int64): image i
 * of the launch reads src image slots[i] and writes out_u8 / out_f64 image slots[i] (compact
 * h*w*c images; row_stride must be w*c).  A mixed batch's per-type group then runs in place in
 * the full batch with no gather / scatter of its images. */
int idn_noise_slots_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h, int w,
                       int c, int64_t row_stride, int kind, double p0, double p1, uint64_t seed,
                       const uint64_t* image_ids, const int64_t* slots, void* workspace,
                       size_t ws_bytes, void* stream);

/* The live test path's float64 gaussian / speckle noise (random_noise(..., 'gaussian') returned as
 * float64 straight into denoise_wavelet: lib/model/test.py:1678-1684 -> 1807-1810), fused with
 * the wavelet's colour range: as idn_noise_u8 (kind GAUSSIAN or SPECKLE, c = 3, compact rows,
 * out_f64 required, out_u8 nullable; the float64 Philox stream, or numpy's field in `replay`;
 * image ids offset + i, or image_ids[i] when image_ids is non-NULL) -- the same bytes -- and per
 * image i the fp64 min and max of skimage rgb2ycbcr's Y, Cb, Cr over out_f64, as order-preserving
 * u64 keys in ycc_keys[6 i .. 6 i + 2] (min) and [6 i + 3 .. 6 i + 5] (max), written whole by the
 * call, for idn_wavelet_denoise_ycc: the wavelet then does not read the float64 image an extra
 * time for its colour range.  IDN_EUNSUPPORTED for an odd pixel count or misaligned buffers
 * (u8 2-byte, float64 16-byte aligned). */
int idn_noise_ycc_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h, int w,
                     int kind, double p0, double p1, uint64_t seed, uint64_t offset,
                     const uint64_t* image_ids, const double* replay, uint64_t* ycc_keys,
                     void* stream);

/* The reference's own additive noises (not skimage), SURVEY §8f:
 *   IDN_NOISE_UNIFORM   p0 = high   out = img_as_float(x) + U(0, high)         (test.py:767-903)
 *   IDN_NOISE_GAMMA     p0 = shape, p1 = scale: out = x + gamma.rvs(shape, scale) (1300-1437)
 *   IDN_NOISE_RAYLEIGH  p0 = scale  out = x + rayleigh.rvs(scale)               (1439-1572)
 *   IDN_NOISE_BROWNIAN  p0 = dt     out_u8 = sat(img + U8(255 * B)),
 *                       B = concat([0], cumsum(sqrt(dt) * N(0,1)[h*w*c - 1]))  (905-1126)
 * cv2.add(float64, float64) is a plain add, so out is unclipped; out_u8 = U8(255*out) wraps
 * modulo 256 ((uint8)(int32)trunc, |y| >= 2^31 -> 0); out_f64 = out (brownian: the walk B).
 * replay (float64, N*h*w*c, optional): numpy's unit draws -- random_sample, standard_gamma(shape),
 * sqrt(chisquare(2)), or for brownian the normals with element e holding z[e-1] (element 0
 * unused).  Brownian needs idn_noise_add_workspace_size() bytes of workspace. */
typedef enum idn_noise_add_kind {
  IDN_NOISE_UNIFORM = 4,
  IDN_NOISE_GAMMA = 5,
  IDN_NOISE_RAYLEIGH = 6,
  IDN_NOISE_BROWNIAN = 7
} idn_noise_add_kind;
int idn_noise_add_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h, int w,
                     int c, int64_t row_stride, int kind, double p0, double p1, uint64_t seed,
                     uint64_t offset, const double* replay, void* workspace, size_t ws_bytes,
                     void* stream);
size_t idn_noise_add_workspace_size(int kind, int n, int h, int w, int c);
/* As idn_noise_add_u8 (Philox stream only) with a device array of n image ids (see
 * idn_noise_ids_u8). */
int idn_noise_add_ids_u8(const uint8_t* src, uint8_t* out_u8, double* out_f64, int n, int h,
                         int w, int c, int64_t row_stride, int kind, double p0, double p1,
                         uint64_t seed, const uint64_t* image_ids, void* workspace,
                         size_t ws_bytes, void* stream);

/* Periodic noise pattern of add_periodic_noise (lib/model/test.py:1128-1298):
 * pattern[i] = U8(255*sin(t_i)), t = np.linspace(-A, A, h*w*c), written as u8 HxWxC (pitch w*c).
 * Image independent: build once per (h, w, c, A) and reuse. */
int idn_periodic_pattern_u8(uint8_t* pattern, int h, int w, int c, double amplitude,
                            void* stream);

/* cv2.add(img, pattern) on u8 (saturating), pattern broadcast over the batch. */
int idn_add_pattern_u8(const uint8_t* src, const uint8_t* pattern, uint8_t* dst, int n, int h,
                       int w, int c, int64_t row_stride, void* stream);
/* idn_add_pattern_u8 on the batch images slots[0..n) (compact h*w*c images, see
 * idn_noise_slots_u8). */
int idn_add_pattern_slots_u8(const uint8_t* src, const uint8_t* pattern, uint8_t* dst, int n,
                             int h, int w, int c, const int64_t* slots, void* stream);
/* dst image slots[i] = src image slots[i] for i < n (per_img bytes per image): the noise-free
 * ("original") members of a mixed batch. */
int idn_copy_slots_u8(const uint8_t* src, uint8_t* dst, int n, int64_t per_img,
                      const int64_t* slots, void* stream);

/* ---- quant noise (colour quantisation by k-means in 8-bit Lab) ---------------------------- */

/* Per image: lab = cv2.cvtColor(img, COLOR_BGR2LAB); k-means with k clusters on the Lab pixels;
 * out = cv2.cvtColor(centres.astype(uint8)[labels], COLOR_LAB2BGR).  Replaces the
 * MiniBatchKMeans(n_clusters=k).fit_predict blocks of lib/model/test.py:592-765 and
 * lib/roi_data_layer/minibatch.py:492-667.  C = 3 (BGR), 1 <= k <= 16, h*w >= k.
 *   centers_in == NULL: device fit -- greedy k-means++ seeding + Lloyd to a fixed point on up to
 *     8192 Lab samples of the image (all pixels when h*w <= 8192, else Philox draws keyed by
 *     (seed, image id = offset + i or image_ids[i])), best of 3 restarts by sample inertia
 *     (sklearn's n_init = 3; the restarts run as separate workgroups).
 *   centers_in != NULL: replay -- the caller's fitted centres (double [n][k][3], e.g. sklearn's
 *     cluster_centers_): labels = argmin_j ||c_j||^2 - 2 x.c_j in float64 (sklearn's
 *     _labels_inertia), bit-exact given the centres.
 * labels_out (nullable): uint8 [n][h][w] cluster index per pixel.  centers_out (nullable):
 * double [n][k][3], the centres used.  8-bit Lab follows OpenCV's integer RGB2Lab_b /
 * Lab2RGBinteger paths (parity vs cv2 unpinned: no cv2 in the build container). */
int idn_quant_u8(const uint8_t* src, uint8_t* dst, uint8_t* labels_out, int n, int h, int w,
                 int64_t row_stride, int k, uint64_t seed, uint64_t offset,
                 const uint64_t* image_ids, const double* centers_in, double* centers_out,
                 void* workspace, size_t ws_bytes, void* stream);
size_t idn_quant_workspace_size(int n, int k);
/* diagnostics: byte offset in the workspace, after a device fit, of each restart's result:
 * run_cen, double [n][3][k][3], every restart's centres (a nonempty cluster's is the exact mean of
 * its samples, an empty one's the fp32 centre it kept), followed at
 *   idn_quant_runs_offset(n, k) + round_up(n * 3 * k * 3 * sizeof(double), 256)
 * by run_inert, double [n][3], the restarts' inertias over the fit's samples.  The centres the
 * call used are those of the restart with the lowest inertia (the earliest on ties).  A replay
 * call (centers_in != NULL) leaves both untouched.  tests/quant_fit_model.py restates the fit. */
size_t idn_quant_runs_offset(int n, int k);
/* cv2.cvtColor(img, COLOR_BGR2LAB) / (lab, COLOR_LAB2BGR) on 8-bit 3-channel images. */
int idn_bgr2lab_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                   void* stream);
int idn_lab2bgr_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                   void* stream);
/* cv2.cvtColor(img, COLOR_LBGR2Lab) / (lab, COLOR_Lab2LBGR): the same integer paths with OpenCV's
 * linear gamma tables (linearGammaTab_b[i] = i << 3 in, linearInvGammaTab_b[v] = (255 * v) >> 12
 * out) in place of the sRGB ones; what fastNlMeansDenoisingColored converts with.  At 8 bits the
 * round trip is not the identity (it moves B, G, R by up to 4, 2, 5).  Parity vs cv2 unpinned. */
int idn_lbgr2lab_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                    void* stream);
int idn_lab2lbgr_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                    void* stream);

/* ---- fused steps (one pass over HBM instead of two) ------------------------------------------ */

/* cv2.GaussianBlur(img, (ksize, ksize), 0) then prep_im_for_blob at scale 1.0
 * (lib/utils/blob.py:33-47): blob = float32(float64(v) - mean[ch]), dense (n, h, w, c) float32
 * written by the filter kernel (the filtered u8 image never reaches HBM).  mean: host double[3].
 * IDN_EUNSUPPORTED unless C = 3, ksize 3 or 5 and compact rows of 8k <= 3024 bytes (compose
 * idn_gaussian_blur_u8 and idn_blob_f32 then). */
int idn_gaussian_blob_f32(const uint8_t* src, float* blob, int n, int h, int w, int c,
                          int64_t row_stride, int ksize, const double* mean, void* stream);

/* Flat copy of nbytes (multiple of 16, 16-byte aligned pointers).  policy 0 = default cache
 * policy, 1 = nontemporal loads and stores.  Not a reference interface: the bench's same-run
 * copy ceiling (SURVEY §8d "also report a measured copy-kernel peak"). */
int idn_copy_u8(const uint8_t* src, uint8_t* dst, int64_t nbytes, int policy, void* stream);

/* ---- wavelet denoise (skimage 0.14.2 denoise_wavelet, BayesShrink, soft, YCbCr) -------- */

/* out_u8 = (255*denoise_wavelet(img, method='BayesShrink', mode='soft', wavelet=wavelet,
 *           multichannel=True, convert2ycbcr=True, wavelet_levels=levels)).astype(uint8),
 * c = 3.  levels <= 0 selects skimage's default max(dwt_max_level - 3, 1).  in_f64 (nullable)
 * replaces src when the caller holds a float image in [0,1] (the reference's f64 branches, dense
 * n*h*w*3).  out_f32 (nullable) receives the float result before the U8 cast (dense n*h*w*3).
 * Precision: Haar computes its statistics exactly (integer moments / fp64) and, on the fused
 * path, its level-1 synthesis stage in fp32.  bior1.5 keeps pywt's fp64 op order where an exact
 * value matters -- the normalisation (exact quotient), the level-1 column highpass and the finest
 * dd (whose exact zeros and median give sigma, bit-identical to an all-fp64 run: the median
 * recomputes its candidates' exact dd from the input), and the sums of squares -- and runs the
 * lowpass outputs (aa / ad / da), the deeper levels and the synthesis in fp32; intermediate bands
 * live in the workspace as fp32 (the coarsest aa as fp64): |out - reference| <= 1e-5 before the
 * cast (tests: <= 2e-6 from the all-fp64 form).
 * Replaces lib/model/test.py:197-201,1807-1810, minibatch.py:1653-1656,
 * minibatch_before_curvelet.py:85-87. */
int idn_wavelet_denoise_u8(const uint8_t* src, const double* in_f64, uint8_t* out_u8,
                           float* out_f32, int n, int h, int w, int64_t row_stride, int wavelet,
                           int levels, void* workspace, size_t ws_bytes, void* stream);
/* As idn_wavelet_denoise_u8 on float64 input (dense n*h*w*3) whose colour range idn_noise_ycc_u8
 * already reduced into ycc_keys: the same outputs bit for bit, one pass over the input fewer. */
int idn_wavelet_denoise_ycc(const double* in_f64, const uint64_t* ycc_keys, uint8_t* out_u8,
                            float* out_f32, int n, int h, int w, int wavelet, int levels,
                            void* workspace, size_t ws_bytes, void* stream);
size_t idn_wavelet_workspace_size(int n, int h, int w, int wavelet, int levels);
/* diagnostics: byte offset in the workspace of the per-image statistics blocks (256 doubles per
 * image: channel sums of squared details, sigma medians, thresholds) after a call */
size_t idn_wavelet_stats_offset(int n, int h, int w, int wavelet, int levels);

/* The denoiser with every option: per image skimage 0.14.2's
 *   denoise_wavelet(img, sigma, wavelet, mode, wavelet_levels=levels, multichannel=True,
 *                   convert2ycbcr=convert2ycbcr, method=method)
 * (c = 1 with convert2ycbcr = 0: multichannel=False on the 2-D image), then the u8 cast.
 * Exactly one of src (u8, rows of row_stride >= w*c bytes) and in_f64 (dense n*h*w*c, values in
 * [0, 1]) is given; out_u8 (rows of row_stride bytes) and / or out_f32 (dense) receive the result.
 * c is 1 or 3; convert2ycbcr needs c = 3.  wavelet: any idn_wavelet, extension 'symmetric';
 * levels <= 0 selects max(dwt_max_level - 3, 1), at most 10 levels.  method: idn_wavelet_method,
 * mode: idn_wavelet_mode.  sigma_dev: null (sigma = median(|dd_1| != 0) / 0.6745 per channel) or
 * n*c doubles in device memory, sigma of image i channel k at [i*c + k], read on the device; with
 * convert2ycbcr it applies to the normalised Y / Cb / Cr channel.  convert2ycbcr = 0 transforms
 * each channel of the float image as it is and clips once to [0, 1].  A channel without a finite
 * sigma (no nonzero dd_1) gives 0.  Every band is fp64 and the analysis keeps pywt's operation
 * order; |out - reference| <= 1e-5 before the cast.  With the options of idn_wavelet_denoise_u8
 * (BAYES, SOFT, no sigma, convert2ycbcr) it computes what that function computes, on kernels of
 * its own, slower.  No allocation, stream-ordered. */
size_t idn_wavelet_general_workspace_size(int n, int h, int w, int c, int wavelet, int levels);
int idn_wavelet_denoise_general(const uint8_t* src, const double* in_f64, uint8_t* out_u8,
                                float* out_f32, int n, int h, int w, int c, int64_t row_stride,
                                int wavelet, int levels, int method, int mode, int convert2ycbcr,
                                const double* sigma_dev, void* workspace, size_t ws_bytes,
                                void* stream);

/* ---- float64 filters (the reference's quirk branches blur random_noise's float64 output) -- */

/* cv2.GaussianBlur / cv2.blur on CV_64F images (dense n*h*w*c doubles), BORDER_REFLECT_101.
 * Reached by train_v0 post hooks after a "plain" noise branch (minibatch.py:1636-1643) and by
 * test_v0's default branch (test.py:1757-1768).  Within 1e-12 of the double reference. */
int idn_gaussian_blur_f64(const double* src, double* dst, int n, int h, int w, int c, int ksize,
                          void* stream);
int idn_box_blur_f64(const double* src, double* dst, int n, int h, int w, int c, int ksize,
                     void* stream);

/* ---- non-local means (cv2.fastNlMeansDenoising, OpenCV 3.4's 8-bit integer scheme) ---------- */

/* Not a reference interface: the denoiser a cv2-flavoured bank is expected to have.  The scheme
 * (fast_nlmeans_denoising_invoker.hpp, DistSquared, IT = int, WT = int) is pure integer
 * arithmetic; tests/nlm_model.py restates it in numpy and the kernel matches that model bit for
 * bit.  cv2 is not importable where this project is built, so parity with cv2 itself is unpinned.
 * With t = template_size (odd, 3..7), s = search_size (odd, 5..21), b = t/2 + s/2:
 *   fpm = INT_MAX / (s*s*255), shift = ceil(log2(t*t)), mult = 2^shift / (t*t)
 *   wt[a] = rint(fpm * exp(-(a*mult) / (h*h*c))), 0 where below 0.001 * fpm
 *   per pixel p and each of the s*s offsets o, on the image reflected (BORDER_REFLECT_101) by b:
 *     ssd = sum over the t x t template and the channels of (E[p+q] - E[p+o+q])^2
 *     w = wt[ssd >> shift];  wsum += w;  est[ch] += w * E[p+o][ch]
 *   dst[ch] = min(255, (est[ch] + wsum/2) / wsum)
 * h must be of the order of the noise's standard deviation on the 0..255 scale.
 *
 * idn_nlmeans_weights (host only, no HIP call): the table is a nonzero prefix followed by zeros;
 *   writes the first min(cap, prefix length) entries to wt_out and reports the full prefix length
 *   in *n_weights (a cap that is too small is not an error: call again with a larger buffer),
 *   shift and fpm.  IDN_EINVAL: null pointer (wt_out may be null when cap is 0), cap < 0, h not
 *   positive and finite, c not 1 or 3, sizes even or out of range.
 * idn_nlmeans_u8: weights_dev is that prefix on the device (n_weights entries; built once per
 *   (h, c, t, s) and kept by the caller); shift and fpm follow from the sizes.  Stream-ordered and
 *   capture-safe: no allocation, copy or synchronisation inside.  src and dst share row_stride.
 *   IDN_EINVAL: null pointer, src == dst, row_stride < w*c, c not 1 or 3, sizes even or out of
 *   range, min(h, w) < b + 1, n_weights < 1.  IDN_EUNSUPPORTED: n_weights above
 *   IDN_NLMEANS_MAX_WEIGHTS (the prefix lives in LDS next to the 30 KB tile; 24576 is h ~ 39 at
 *   c = 3, t = 7.  Up to 8800 entries, h ~ 23, the launch stays within the 64 KB every launch
 *   gets; above, the kernel's LDS limit is raised first, and above 12900 entries, h ~ 28, only
 *   one workgroup fits a CU instead of two).  Every argument check runs before any HIP call. */
#define IDN_NLMEANS_MAX_WEIGHTS 24576
int idn_nlmeans_weights(double h, int c, int template_size, int search_size, int32_t* wt_out,
                        int cap, int* n_weights, int* shift, int* fixed_point_mult);
int idn_nlmeans_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                   int64_t row_stride, int template_size, int search_size,
                   const int32_t* weights_dev, int n_weights, void* stream);

/* cv2.fastNlMeansDenoisingColored(src, None, h, hColor, t, s) on 8-bit BGR images (c = 3), OpenCV
 * 3.4's definition restated:
 *   lab = cvtColor(src, COLOR_LBGR2Lab)                        (idn_lbgr2lab_u8)
 *   L'  = fastNlMeansDenoising(lab[..., 0:1], h, t, s)         (the scheme above with c = 1)
 *   ab' = fastNlMeansDenoising(lab[..., 1:3], hColor, t, s)    (c = 2: a and b denoised jointly)
 *   dst = cvtColor(merge(L', ab'), COLOR_Lab2LBGR)             (idn_lab2lbgr_u8)
 * tests/nlm_colored_model.py restates it in numpy and the kernels match that model bit for bit;
 * parity with cv2 itself is unpinned (cv2 is not importable where this project is built; the two
 * linear gamma tables are recalled from initLabTabs()).  Because the 8-bit Lab round trip is not
 * the identity, a constant image comes back as lab2lbgr(lbgr2lab(x)), not as x.
 *
 * idn_nlmeans_colored_weights (host only): both tables at once, as two idn_nlmeans_weights calls
 *   with (h, c = 1) and (h_color, c = 2) would give them if c = 2 were accepted there; caps and
 *   lengths per table, a short cap is not an error.  IDN_EINVAL: null pointer (a table pointer may
 *   be null when its cap is 0), a negative cap, h or h_color not positive and finite, bad sizes.
 * idn_nlmeans_colored_workspace_size: bytes of the L' plane (at least n*h*w); 0 for a bad shape.
 * idn_nlmeans_colored_u8: two launches ordered on the stream, no Lab image in memory: the first
 *   converts while staging, denoises L and writes L' to the workspace (compact, w bytes per row);
 *   the second converts while staging, denoises (a, b), reads L', converts back and writes BGR.
 *   Stream-ordered and capture-safe: no allocation, copy or synchronisation inside.  src and dst
 *   share row_stride; src == dst is rejected (the second launch still reads src).
 *   IDN_EINVAL: null pointer, src == dst, row_stride < 3w, bad shape or sizes, min(h, w) < b + 1,
 *   a table length below 1, workspace missing or below idn_nlmeans_colored_workspace_size.
 *   IDN_EUNSUPPORTED: either table above IDN_NLMEANS_MAX_WEIGHTS (at t = 7, s = 21: h up to 68,
 *   h_color up to 48).  n == 0 returns IDN_OK without a launch.  Every argument check runs before
 *   any HIP call. */
int idn_nlmeans_colored_weights(double h, double h_color, int template_size, int search_size,
                                int32_t* wt_l, int cap_l, int* n_l, int32_t* wt_ab, int cap_ab,
                                int* n_ab, int* shift, int* fixed_point_mult);
size_t idn_nlmeans_colored_workspace_size(int n, int h, int w);
int idn_nlmeans_colored_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                           int64_t row_stride, int template_size, int search_size,
                           const int32_t* wt_l_dev, int n_l, const int32_t* wt_ab_dev, int n_ab,
                           void* workspace, size_t ws_bytes, void* stream);

/* ---- total-variation denoising (skimage 0.14.2 restoration.denoise_tv_chambolle) ------------- */

/* Not a reference interface: the edge-preserving denoiser of the module the reference takes its
 * wavelet denoiser from.  denoise_tv_chambolle(x, weight, eps, n_iter_max, multichannel=True) on
 * u8 images: every channel of every image is denoised on its own as im = x[..., ch] / 255 by
 * Chambolle's projection iteration on the dual field (p0, p1), and stops on its own when the
 * energy E of an iteration differs from the previous one's by less than eps * E(iteration 0), or
 * after n_iter_max iterations.  tests/tv_model.py restates the algorithm in numpy float64 and is
 * the definition; skimage is not importable where this project is built, so parity with skimage
 * itself is unpinned.  The kernels keep the duals in fp32 and add the energies in fp64 in a fixed
 * order: a channel's result, its iteration count included, is the same bits on every call and in
 * every batch, and lies within 1e-5 of the model.
 *   dst_f32 (nullable): out, float32, dense n*h*w*c, not clipped
 *   dst_u8  (nullable): clip(rint(255 * out), 0, 255), row pitch row_stride as src
 *   iters   (nullable): n*c int32, the iteration each (image, channel) stopped at: the index of the
 *     iteration that met the rule (out is then the image formed from the duals before that
 *     iteration's update), or n_iter_max.  A constant channel never meets the rule; eps = 0 gives
 *     a fixed count.
 * One launch per iteration plus two at the end; the stopping rule is evaluated on the device and
 * the workgroups of a finished (image, channel) exit at once.  Stream-ordered and capture-safe: no
 * allocation, copy or synchronisation inside.  src is read by every launch and must not be dst_u8.
 * workspace: idn_tv_chambolle_workspace_size(n, h, w, c) bytes (0 for a shape the call does not
 *   accept), 8-byte aligned, contents irrelevant on entry: two buffers of fp32 dual pairs, 16 bytes
 *   per pixel and channel (48 bytes per pixel at c = 3: 7.4 GB for 256 images of 600 x 1000 x 3),
 *   plus 32 bytes per 256 x 64 pixel tile and 64 bytes per (image, channel).
 * IDN_EINVAL: null src, both destinations null, dst_u8 == src, h or w < 1, c not 1 or 3,
 *   row_stride < w*c, weight not positive and finite, eps negative or not finite, n_iter_max
 *   outside 1..IDN_TV_MAX_ITER.  IDN_EWORKSPACE: workspace missing or too small.  n == 0 returns
 *   IDN_OK without a launch.  Every argument check runs before any HIP call. */
#define IDN_TV_MAX_ITER 1000
size_t idn_tv_chambolle_workspace_size(int n, int h, int w, int c);
int idn_tv_chambolle_u8(const uint8_t* src, uint8_t* dst_u8, float* dst_f32, int32_t* iters, int n,
                        int h, int w, int c, int64_t row_stride, double weight, double eps,
                        int n_iter_max, void* workspace, size_t ws_bytes, void* stream);

/* ---- noise level (skimage restoration.estimate_sigma, unchanged 0.14.2 .. 0.18.3) ------------ */

/* Not a reference interface: measures the noise of the batch a pipeline is handed, so that the
 * strengths of the denoisers above need not be guessed.  dst[i*c + ch] =
 * estimate_sigma(x[i][..., ch]): the median of |d| over the coefficients d != 0 of the finest
 * diagonal db2 detail band (pywt.dwtn(plane, 'db2')['dd'], symmetric extension), divided by
 * norm.ppf(0.75) = 0.6744897501960817.  Exactly one of src_u8 / src_f64 is given, the other is
 * NULL; the plane is taken as float64 as it is (no division by 255), so the result is on the
 * input's scale.  row_stride counts elements of the source (bytes / doubles), >= w*c.
 * tests/sigma_model.py restates pywt's arithmetic in numpy float64, tap order included, and is
 * the definition; tests/golden/sigma.npz pins it bit for bit to the real skimage and pywt.  The
 * kernels compute every coefficient in fp64 in that order and select the median exactly on the
 * key bits: dst is bit-equal to the model, the same bits on every call and in every batch.  A
 * plane without a nonzero coefficient gives NaN.  A flat region of a nonzero value gives
 * coefficients of about 1e-31, not zeros, and they count (as in pywt).  Non-finite float64 input
 * gives an unspecified value; no access leaves the buffers.
 * The band is not stored: up to six passes recompute it from the image (three for noise-like
 * images), each followed by one small launch per plane.  Stream-ordered and capture-safe: no
 * allocation, copy or synchronisation inside.
 * workspace: idn_estimate_sigma_workspace_size(n, h, w, c, is_f64) bytes (0 for n <= 0, h or
 *   w < 4, c not 1 or 3; additive in n), 8-byte aligned, contents irrelevant on entry: counters
 *   and a short key list, 32840 bytes per (image, channel), whatever the image size.
 * IDN_EINVAL: both or neither source given, null dst, src_f64 or dst not 8-byte aligned, n < 0,
 *   h or w < 1, c not 1 or 3, row_stride < w*c, workspace not 8-byte aligned.  IDN_EUNSUPPORTED:
 *   h or w < 4 (the extension would reflect twice).  IDN_EWORKSPACE: workspace missing or too
 *   small.  n == 0 returns IDN_OK without a launch.  Every argument check runs before any HIP
 *   call. */
size_t idn_estimate_sigma_workspace_size(int n, int h, int w, int c, int is_f64);
int idn_estimate_sigma(const uint8_t* src_u8, const double* src_f64, double* dst, int n, int h,
                       int w, int c, int64_t row_stride, void* workspace, size_t ws_bytes,
                       void* stream);

/* ---- wiener (scipy.signal.wiener per channel plane: the adaptive local-statistics filter) ---- */

/* Not a reference interface: the adaptive linear denoiser of the bank (Lee / Matlab wiener2),
 * the natural consumer of idn_estimate_sigma's number, squared.  Every channel plane of every
 * image is filtered on its own, as scipy.signal.wiener(plane.astype(float64), (kh, kw), noise).
 * With S1 = sum t and S2 = sum t^2 over the kh x kw window of a sample x, as integers, and
 * n = kh*kw:
 *   m = double(S1) / n,  v = double(S2) / n - m*m  (the product rounds, then the difference),
 *   r = v == 0 ? m : (v < noise ? m : (x - m) * (1 - noise / v) + m).
 * border: IDN_WIENER_ZERO takes a tap outside the image as 0 (scipy's correlate 'same'; it dims
 * the rim), IDN_WIENER_REFLECT101 as the mirrored sample (cv2's default border, numpy's
 * pad mode 'reflect'; needs kh/2 < h and kw/2 < w).  kh, kw: odd, 1..31, each on its own.
 * noise: device array on the 0..255 scale squared, read at noise[i*noise_image_stride + ch]
 * (noise_image_stride c, or 0 when one row of c values serves every image), not validated; NULL
 * estimates it per (image, channel) as scipy does, the mean of v over the plane, here as
 * double(Q) / double(n*n*h*w) with the exact integer Q = sum (n*S2 - S1*S1): within 3.3e-16
 * relative of scipy's mean, which rounds per sample.  On a structured image that mean counts
 * the signal and overestimates.  noise_out (nullable): the n*c values used.
 * v == 0 returns m: the one departure from scipy, which gives NaN there when noise is 0 too
 * (an all-zero image with no noise given).
 * dst_f64 (n*h*w*c doubles, compact) receives r, dst_u8 (src's layout) clip(rint(r), 0, 255),
 * round half to even; either may be NULL, not both.  tests/wiener_model.py is the definition and
 * tests/golden/wiener.npz pins it to scipy 1.15.3; both outputs are bit-equal to the model, the
 * same bits on every call and in every batch.  The cost per sample does not grow with kh*kw:
 * running column sums and at most about 20 LDS reads (wide windows are summed in two levels).
 * Given noise: one launch, the image read once and written once.  noise NULL: a first pass forms Q with integer atomics and the filter pass recomputes
 * the sums.  Stream-ordered and capture-safe: no allocation, host copy or synchronisation.
 * workspace: idn_wiener_workspace_size(n, c) bytes (8 per (image, channel); 0 for n <= 0 or c not
 *   1 or 3), 8-byte aligned, needed only when noise is NULL.
 * IDN_EINVAL: null src, both destinations null, dst_u8 == src, n < 0, h or w < 1, c not 1 or 3,
 *   row_stride < w*c, kh or kw even or outside 1..31, unknown border, reflect101 with kh/2 >= h
 *   or kw/2 >= w, a double pointer not 8-byte aligned, noise_image_stride neither 0 nor c.
 *   IDN_EWORKSPACE: noise NULL and the workspace missing or too small.  IDN_EUNSUPPORTED: noise
 *   NULL and h*w above 2^28 (Q would leave 64 bits).  n == 0 returns IDN_OK without a launch.
 *   Every argument check runs before any HIP call. */
typedef enum idn_wiener_border {
  IDN_WIENER_ZERO = 0,
  IDN_WIENER_REFLECT101 = 1
} idn_wiener_border;
size_t idn_wiener_workspace_size(int n, int c);
int idn_wiener_u8(const uint8_t* src, uint8_t* dst_u8, double* dst_f64, int n, int h, int w, int c,
                  int64_t row_stride, int kh, int kw, int border, const double* noise,
                  int64_t noise_image_stride, double* noise_out, void* workspace, size_t ws_bytes,
                  void* stream);

/* ---- sliding DCT denoiser (Yu & Sapiro, IPOL 2011: 8x8 DCT, hard threshold, aggregation) ---- */

/* Not a reference interface: the transform-domain denoiser of the bank, the self-contained form
 * of "keep the strong coefficients of a redundant transform and invert".  For every plane k of
 * every image and every patch P with the top-left corner (i, j), 0 <= i <= h-8, 0 <= j <= w-8:
 *   D = Cm P Cm^T            (Cm: the orthonormal 8-point DCT-II matrix)
 *   D'[u][v] = D[u][v] if (u, v) == (0, 0) or |D[u][v]| >= T_k, else 0
 *   R = Cm^T D' Cm
 * and r_k[y][x] is the sum of R at (y, x) over the patches that contain it, divided by their
 * number, (min(y,h-8) - max(y-7,0) + 1) * (min(x,w-8) - max(x-7,0) + 1).  Nothing is decimated.
 * color = 0: the planes are the channels, T_k = factor * sigma_k.  color = 1 (c = 3 only): the
 * planes are g_k = sum_j M[k][j] x_j with M the orthonormal 3-point DCT on the channels as stored
 * (rows [1,1,1]/sqrt3, [1,0,-1]/sqrt2, [1,-2,1]/sqrt6), T_k = factor * sqrt(sum_j M[k][j]^2
 * sigma_j^2), the exact propagation of the noise, and the result is r_j = sum_k M[k][j] r_k.
 * sigma: device array of doubles on the 0..255 scale (what idn_estimate_sigma writes), read at
 * sigma[i*sigma_image_stride + ch] (sigma_image_stride c, or 0 when one row of c values serves
 * every image), not validated: a NaN keeps the DC terms only.  sigma 0 returns the input.
 * dst_f32 (n*h*w*c floats, compact) receives r, dst_u8 (src's layout) clip(rint(r), 0, 255),
 * round half to even; either may be NULL, not both.
 * fp32 arithmetic.  tests/dct_model.py (numpy float64) is the definition; the device result lies
 * within a few 1e-4 of it wherever no coefficient is within rounding of its threshold (a flipped
 * coefficient moves a sample by up to about 0.6), and has the same bits on every call and in
 * every batch: every sum has a fixed order, nothing is an atomic.  Parity with
 * cv2.xphoto.dctDenoising and the IPOL code is unpinned: here the DC term always stays, the patch
 * is 8, the colour transform is fixed and there is no PCA.
 * One launch; each lane walks a patch column down the image with the row transforms in a
 * register ring, 18 one-dimensional transforms per patch (csrc/dct_denoise.hip).
 * Stream-ordered and capture-safe: no allocation, host copy or synchronisation.
 * workspace: idn_dct_denoise_workspace_size(n, h, w, c) bytes, which is 0 (the thresholds are
 *   formed in the kernel's prologue): workspace may be NULL, and IDN_EWORKSPACE cannot occur.
 * IDN_EINVAL: null src or sigma, both destinations null, dst_u8 == src, n < 0, h or w < 1, c not
 *   1 or 3, row_stride < w*c, color not 0 or 1, color 1 with c 1, dst_f32 not 4-byte or sigma
 *   not 8-byte aligned, sigma_image_stride neither 0 nor c, factor negative, NaN or infinite.
 *   IDN_EUNSUPPORTED: patch other than 8 (16 is not built), h or w below 8.  n == 0 returns
 *   IDN_OK without a launch.  Every argument check runs before any HIP call. */
size_t idn_dct_denoise_workspace_size(int n, int h, int w, int c);
int idn_dct_denoise_u8(const uint8_t* src, uint8_t* dst_u8, float* dst_f32, int n, int h, int w,
                       int c, int64_t row_stride, int patch, int color, const double* sigma,
                       int64_t sigma_image_stride, double factor, void* workspace,
                       size_t ws_bytes, void* stream);

/* ---- quality metrics (skimage 0.14.2 measure.compare_mse / compare_psnr / compare_ssim) ---- */

/* Score a batch against another (a denoiser's output against the clean images) without leaving
 * the device: one float64 per image pair.  a, b: u8 batches of the same shape, c in {1, 3}, each
 * with its own row pitch.  Not a reference interface: the reference never scores its filters.
 *
 * idn_mse_u8: mse_out[i] = compare_mse(a[i], b[i]) = sum((a - b)^2) / (h*w*c).  The sum is
 *   carried in integers and divided once, so the value is bit-equal to numpy's float64 mean.
 *   compare_psnr is 10 log10(255^2 / mse) of it (idn.ops.psnr; +inf for equal images).
 * idn_ssim_u8: ssim_out[i] = compare_ssim(a[i], b[i], win_size=win_size, multichannel=True)
 *   (data_range 255, uniform window, sample covariance, K1 0.01, K2 0.03): per channel the mean
 *   of S over the (h - win_size + 1) * (w - win_size + 1) windows that lie inside the image,
 *   then the mean over channels.  win_size odd, 3..11, <= min(h, w).  The window moments are
 *   exact integers, S and the sums are float64, and the sums run in a fixed order: a pair gives
 *   the same bits on every call and in every batch, and a == b gives exactly 1.0.
 *   ssim_ch_out (nullable): the n*c per-channel values.  mse_out (nullable): idn_mse_u8's
 *   values, from the same pass over the bytes.
 * workspace: idn_metrics_workspace_size(n, h, w, c, win_size) bytes, 8-byte aligned, for either
 *   call (win_size outside 3..11: idn_mse_u8's need alone); 0 for a shape neither call accepts.
 * IDN_EINVAL: null image or result pointer, row pitch < w*c, c not 1 or 3, win_size even or
 *   outside 3..11 or above min(h, w).  IDN_EWORKSPACE: workspace missing or too small.
 *   IDN_EUNSUPPORTED: idn_mse_u8 on images above 1 GiB. */
size_t idn_metrics_workspace_size(int n, int h, int w, int c, int win_size);
int idn_mse_u8(const uint8_t* a, const uint8_t* b, double* mse_out, int n, int h, int w, int c,
               int64_t row_stride_a, int64_t row_stride_b, void* workspace,
               size_t workspace_bytes, void* stream);
int idn_ssim_u8(const uint8_t* a, const uint8_t* b, double* ssim_out, double* ssim_ch_out,
                double* mse_out, int n, int h, int w, int c, int64_t row_stride_a,
                int64_t row_stride_b, int win_size, void* workspace, size_t workspace_bytes,
                void* stream);

/* ---- exposure correction (Automold correct_exposure: tools/Automold.py:817-842) -------------- */

/* OpenCV 3.4's 8-bit code as recalled; cv2 is not available to the tests, so parity with cv2
 * itself is unpinned and the numpy model tests/exposure_model.py, written from the text below,
 * defines the result.  The kernels are bit-equal to it, and an image gives the same bytes alone
 * and in any batch: all that crosses workgroups is integer atomic addition.
 * descale(v) = (v + 8192) >> 14 (arithmetic), sat clips to 0..255, rne rounds an fp32 value half to
 * even.
 *
 * idn_bgr2yuv_u8 (COLOR_BGR2YUV, c = 3):  Y = descale(1868 B + 9617 G + 4899 R),
 *   U = sat(descale((B - Y) 8061 + (128 << 14))),  V = sat(descale((R - Y) 14369 + (128 << 14))).
 * idn_yuv2bgr_u8 (COLOR_YUV2BGR, c = 3):  u = U - 128, v = V - 128,  B = sat(Y + descale(33292 u)),
 *   G = sat(Y + descale(-6472 u - 9519 v)),  R = sat(Y + descale(18678 v)).  The round trip is
 *   not the identity.
 * idn_equalize_hist_u8 (cv2.equalizeHist per image, c = 1): with hist over the image and i0 its
 *   first non-zero bin, a constant image comes back; otherwise scale = 255.f / (h w - hist[i0]),
 *   lut[i0] = 0 and lut[i] = sat(rne((float)sum(hist[i0+1 .. i]) scale)).
 * idn_clahe_u8 (cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply per image, c = 1):
 *   if tiles_x divides w and tiles_y divides h the tiles cut the image; otherwise the image is
 *   extended by BORDER_REFLECT_101, by tiles_y - h % tiles_y rows at the bottom and
 *   tiles_x - w % tiles_x columns at the right, BOTH whenever either fails to divide (a dimension
 *   that divides then grows by a whole tiles_y or tiles_x).  Per tile of area pixels:
 *   clip = clip_limit == 0 ? 0 : max((int)(clip_limit area / 256), 1); if clip > 0 the bins are
 *   cut at clip, every bin gains excess / 256, and bins 0, step, 2 step, ... gain one more while
 *   r = excess % 256 lasts (step = max(256 / r, 1)); lut[i] = sat(rne((float)cumsum[i] 255.f /
 *   area)).  Each pixel blends the tables of the four nearest tile centres bilinearly in fp32:
 *   txf = x (1.f / tile_w) - 0.5f, tx1 = floor(txf), xa = txf - tx1, tx2 = min(tx1 + 1, tiles_x -
 *   1), tx1 = max(tx1, 0), the same in y, out = sat(rne((L11 (1 - xa) + L12 xa)(1 - ya) +
 *   (L21 (1 - xa) + L22 xa) ya)), every product and sum rounded to fp32.
 *   tiles_x, tiles_y in 1..16, h > tiles_y and w > tiles_x (one reflection is enough),
 *   clip_limit >= 0 and finite (0: no clipping).
 * idn_correct_exposure_u8 (c = 3, BGR): the tone part of exposure_process: BGR -> YUV, Y <-
 *   (17 Y) / 20 where Y > 150 (trunc(0.85 Y) for every byte), CLAHE(2.0, (4, 4)), equalizeHist,
 *   CLAHE(2.0, (4, 4)), YUV -> BGR with the source's U and V.  Byte for byte the composition of the
 *   entry points above, in seven launches that store no YUV image (csrc/exposure.hip).  It does NOT
 *   run exposure_process's last step, fastNlMeansDenoisingColored(., 3, 3, 7, 21): the caller (the
 *   binding idn.ops.correct_exposure) runs idn_nlmeans_colored_u8 on the result.  h, w > 4.
 * workspace: idn_exposure_workspace_size(n, h, w, tiles_x, tiles_y) bytes, 8-byte aligned;
 *   (1, 1) for idn_equalize_hist_u8, (4, 4) for idn_correct_exposure_u8; 0 for n, h or w < 1 or a
 *   grid outside 1..16.  Histograms (u32), tables and one byte plane of luma.
 * IDN_EINVAL: null image pointer, src == dst, n < 0, h or w < 1, row_stride < w*c, a parameter
 *   outside the ranges above, workspace not 8-byte aligned.  IDN_EWORKSPACE: workspace missing or
 *   too small.  IDN_EUNSUPPORTED: an image of 2^31 pixels or more.  n == 0 returns IDN_OK without
 *   a launch.  Every argument check runs before any HIP call. */
int idn_bgr2yuv_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                   void* stream);
int idn_yuv2bgr_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                   void* stream);
size_t idn_exposure_workspace_size(int n, int h, int w, int tiles_x, int tiles_y);
int idn_equalize_hist_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                         int64_t row_stride, void* workspace, size_t workspace_bytes,
                         void* stream);
int idn_clahe_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int64_t row_stride,
                 double clip_limit, int tiles_x, int tiles_y, void* workspace,
                 size_t workspace_bytes, void* stream);
int idn_correct_exposure_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w,
                            int64_t row_stride, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---- shader / bloom noise types ---------------------------------------------------------- */

/* add_shader (test.py:1595-1601): np.array(ImageEnhance.Brightness(PIL image).enhance(factor)).
 * src is the BGR image; dst is written in PIL's RGB channel order, as the reference returns it. */
int idn_shader_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c,
                  int64_t row_stride, double factor, void* stream);

/* add_bloom -> Automold add_sun_flare (tools/Automold.py:588-627): per image `ncirc` steps of
 * {filled LINE_8 circle on the overlay, cv2.addWeighted(overlay, a, out, b, 0)}.
 * circles: device int32 [n][ncirc][8] = {cx, cy, radius, c0, c1, c2, reset_overlay, 0};
 * weights: device float [n][ncirc][2] = {a, b}; spans: device int16 half-width table of radius R
 * at row offset t stored at R*(R+1)/2 + t (idn/automold.py).  <= 1 LSB (float blend order). */
int idn_bloom_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, int c, int64_t row_stride,
                 const int32_t* circles, const float* weights, int ncirc, const int16_t* spans,
                 void* stream);

/* ---- blob epilogue (lib/utils/blob.py:17-47) -------------------------------------------- */

/* blob[i, y, x, ch] = float32(float64(img[i,y,x,ch]) - mean[ch]) for y<h, x<w; zero elsewhere
 * in the (n, out_h, out_w, 3) float32 NHWC blob (im_list_to_blob's zero padding).  flip != 0
 * mirrors x (minibatch.py:1676-1677).  c must be 3.  Scale 1.0 only (the 600x1000 case). */
int idn_blob_f32(const uint8_t* src, float* blob, int n, int h, int w, int c,
                 int64_t row_stride, int out_h, int out_w, const double mean[3], int flip,
                 void* stream);

/* blob from a float64 image (dense n*h*w*3): float32(float64(float32(x)) - mean[ch]) -- what
 * prep_im_for_blob does with the float64 output of the "plain" noise branches. */
int idn_blob_from_f64(const double* src, float* blob, int n, int h, int w, int out_h, int out_w,
                      const double mean[3], int flip, void* stream);

/* cv2.resize(im_f32, None, None, fx, fy, INTER_LINEAR) on dense n*h*w*c float32 images
 * (prep_im_for_blob when the image is not already 600 x 1000: lib/utils/blob.py:44-45,
 * lib/model/test.py:75-76).  out_h/out_w = round(h*fy), round(w*fx) as cv2 computes them. */
int idn_resize_linear_f32(const float* src, float* dst, int n, int h, int w, int c, int out_h,
                          int out_w, double fx, double fy, void* stream);

/* ---- decode front-end (cv2.imread: lib/model/test.py:191, minibatch.py:85) --------------- */

/* Header of one JPEG file in host memory (SOI .. EOI): height, width, components (1, 3 or 4).
 * Taken: Huffman-coded baseline, extended sequential and progressive files (SOF0 / SOF1 / SOF2),
 * arithmetic-coded sequential and progressive files (SOF9 / SOF10, DAC conditioning), one or
 * several scans, restart intervals, 4:4:4 / 4:2:2 / 4:2:0 or grayscale; a progressive
 * file whose last scan leaves AC 1..5 imprecise is block-smoothed as libjpeg 9d smooths it
 * (jdcoefct.c smoothing_ok / decompress_smooth_data); three components are YCbCr or RGB as
 * libjpeg decides it (component IDs, JFIF / Adobe markers); four are CMYK or YCCK (Adobe's
 * transform; K sampled as the first component), decoded to libjpeg's CMYK and converted to BGR
 * as OpenCV does (icvCvt_CMYK2BGR_8u_C4C3R).  IDN_EUNSUPPORTED for anything else (lossless,
 * hierarchical, 12-bit, big-gamut colour, DHP / EXP / JPGn / LSE markers, other sampling).
 * height x width is the size cv2.imread returns: after the file's EXIF orientation
 * (idn_jpeg_orientation), so orientations 5..8 report the decoded size transposed. */
int idn_jpeg_info(const uint8_t* file, size_t len, int* height, int* width, int* components);

/* The EXIF orientation (1..8; 1 = none) OpenCV 3.4.2's imread applies to this file after decoding
 * (loadsave.cpp ApplyExifOrientation, unless IMREAD_IGNORE_ORIENTATION): exif.cpp's ExifReader
 * reads Orientation (0x0112) from IFD0 of the FIRST APP1 segment (little- or big-endian TIFF);
 * a marker its walk does not know, or a malformed IFD0 (any offset past the data, a bad tag
 * value among the tags it parses), means 1, as does a value outside 1..8.  The decode applies
 * it: 2 flip(1), 3 flip(-1), 4 flip(0), 5 transpose, 6 transpose + flip(1), 7 transpose +
 * flip(-1), 8 transpose + flip(0) (cv::flip codes).  Restated from OpenCV's published source
 * (parity vs cv2 unpinned: cv2 is not importable where this was built; the decoded pixels are
 * pinned by the real libjpeg 9d, the geometry by Pillow's reading of the tag). */
int idn_jpeg_orientation(const uint8_t* file, size_t len, int* orientation);

/* idn_jpeg_decode_u8 flags.  Default (0): the decode of the reference's pinned libjpeg 9d
 * (requirements.txt:74, linked by its OpenCV 3.4.2): 8x8 ISLOW IDCT for full-size components,
 * libjpeg 9's scaled 16x16 / 16x8 IDCT for 4:2:0 / 4:2:2 chroma (no upsampling pass), libjpeg 9's
 * YCbCr tables.  IDN_JPEG_TURBO: libjpeg-turbo's decode (8x8 IDCT, fancy h2v1 / h2v2
 * upsampling), what a turbo-linked OpenCV or PIL produce (a file libjpeg-turbo would
 * block-smooth is IDN_EUNSUPPORTED in this mode: turbo's smoothing is not restated).  Bits 8..23:
 * entropy chunk size in bits
 * for the self-synchronising decoder (0 = the default: ~100k chunks per batch, 1536..6144 bits;
 * else a multiple of 64, >= 512; does not
 * change the output). */
#define IDN_JPEG_TURBO 1
/* cv2.IMREAD_IGNORE_ORIENTATION: store every image as decoded (h x w is then the decoded size) */
#define IDN_JPEG_IGNORE_ORIENTATION 2
/* device workspace for decoding these files with these flags (0 if any is unsupported) */
size_t idn_jpeg_workspace_size(const uint8_t* const* files, const size_t* lens, int n, int flags);
/* cv2.imread(path) (IMREAD_COLOR) of n JPEG files held in host memory (any mix of the kinds
 * idn_jpeg_info takes: baseline / extended sequential files on the parallel path, progressive and
 * multi-scan files on the scan path), all h x w, into
 * the device u8 BGR NHWC batch dst (row_stride bytes per row), bit-exact with the library the
 * flags name (replaces cv2.imread at lib/model/test.py:191, lib/roi_data_layer/minibatch.py:85).
 * Damaged entropy-coded data decodes as libjpeg decodes it (it only warns): a file cut short (an
 * EOI appended, or none), bit errors, bad Huffman codes, lost / renumbered restart markers and
 * stray markers -- the data runs out, the rest of its restart interval stays gray, restart
 * markers resynchronise as jdmarker.c's jpeg_resync_to_restart does.
 * Each image is turned by its EXIF orientation (idn_jpeg_orientation) unless the flags say
 * IDN_JPEG_IGNORE_ORIENTATION; h x w is the size after that turn.
 * Speed: baseline / extended sequential files (the reference's VOC images) take the parallel
 * self-synchronising entropy decoder (600 x 1000 q90: ~1.3 ms alone, ~28 us each in a batch of
 * 256; one host core with libjpeg 9d: ~14 ms).
 * PROGRESSIVE AND ARITHMETIC-CODED FILES DECODE SLOWER THAN ONE HOST CORE.  They take the scan
 * path, which is serial within a restart interval (one lane per interval).  Measured on MI355X
 * for a 600 x 1000 file without restart markers: progressive 229 ms, arithmetic-coded 796 ms
 * (72.5 ms with a restart marker per MCU row), against ~22 ms for libjpeg 9d on one host core
 * (JPEG section).  The output is still bit-exact; use this path for correctness
 * or for large batches of such files, which run one wave per image side by side.
 * The entropy-coded segments are copied to the workspace in one transfer; synchronous on
 * `stream`. */
int idn_jpeg_decode_u8(const uint8_t* const* files, const size_t* lens, int n, uint8_t* dst,
                       int h, int w, int64_t row_stride, int flags, void* workspace,
                       size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDN_H_ */
