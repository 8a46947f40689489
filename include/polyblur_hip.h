/*
 * polyblur_hip.h -- C ABI of libpolyblur_hip.so, the MI355X (gfx950) Polyblur engine.
 *
 * Drop-in boundary for the hot path of teboli/polyblur (reference @ /root/reference):
 * the reference has no C ABI of its own -- its Python calls ATen ops, and its three
 * side-car pybind11 modules take torch::Tensor (RF.cpp:43-46,97-99,
 * separable_gaussian2d.cpp:186-191,252-255).  Each entry point below names the
 * reference function(s) (file:line) it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no torch / pybind types; every image pointer is a DEVICE pointer to a
 *     contiguous NCHW array (the reference's (B,C,H,W) tensors); `float *host_*`
 *     arguments are HOST pointers and make the call synchronise the stream;
 *   - a device pointer needs the alignment of its element type and no more (4 bytes for
 *     float planes and records, 2 for fp16, 1 for 8-bit planes): a view at any element
 *     offset of a larger buffer is a valid operand.  The 16-byte paths are taken where the
 *     pitches -- and, in the four launchers that look at them, the addresses -- allow,
 *     and give the results of the aligned operand;
 *   - all other calls are asynchronous on the context's stream;
 *   - the caller owns every buffer; inputs are never written; scratch memory lives in
 *     the context; a context runs on one stream at a time and is not thread-safe (one
 *     per host thread / GPU); pb_set_stream orders the new stream behind the work already
 *     queued on the old one, because the scratch buffers are shared;
 *   - return value: PB_OK (0) or a negative pb_status; pb_last_error_string() gives
 *     the text for the most recent failure on that context.
 */
#ifndef POLYBLUR_HIP_H
#define POLYBLUR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PB_VERSION 200           /* major*10000 + minor*100 + patch */
#define PB_KSIZE 25              /* kernel support of the reference (ker_size=25, deblurring.py:23) */
#define PB_KRAD 12
#define PB_MAX_ANGLES 13         /* n_angles + 1 <= 13 */
#define PB_MAX_INTERP 64         /* n_interpolated_angles <= 64 */
#define PB_MAX_PHASES 175        /* 25 kernel rows x 7 window chunks */

typedef struct pb_ctx pb_ctx;

typedef enum pb_status {
    PB_OK = 0,
    PB_ERR_BADARG = -1,
    PB_ERR_UNSUPPORTED = -2,
    PB_ERR_HIP = -3,
    PB_ERR_NOMEM = -4
} pb_status;

/* PB_U8: 8-bit images at the file edge of the reference's CLI flow (main.py:80-82,146): loaded as
 * v * float32(1/255) (skimage 0.19.2 img_as_float32) and stored as clip(rint(v*255), 0, 255)
 * (img_as_ubyte) inside the first / last kernels that touch them; everything in between is fp32.
 * Accepted by pb_polyblur_batch, pb_estimate_blur, pb_u8_interleave / pb_u8_deinterleave.     */
typedef enum pb_dtype { PB_F32 = 0, PB_F16 = 1, PB_U8 = 2 } pb_dtype;

/* Outer boundary of the three reblurring convolutions on the replicate-padded domain:
 * PB_WRAP == reference method='fft'  (circular, deblurring.py:141-169, filters.py:31-35)
 * PB_ZERO == reference method='direct' (zero 'same' padding, filters.py:45-49).        */
typedef enum pb_boundary { PB_WRAP = 0, PB_ZERO = 1 } pb_boundary;

typedef enum pb_prefilter { PB_PREFILTER_NONE = 0, PB_PREFILTER_BILATERAL = 1,
                            PB_PREFILTER_DOMAIN_TRANSFORM = 2,      /* recursive filter, N = 1  */
                            PB_PREFILTER_NORMALIZED_CONVOLUTION = 3 /* NC variant,       N = 1  */ } pb_prefilter;

/* Kernel-support policy: PB_SUPPORT_FULL evaluates every tap of the reference's 25x25 kernel
 * that is not exactly 0.0f (4-tap segments of a kernel row, and outer rows / columns, whose taps
 * all underflowed to zero are skipped, which is bit-identical to evaluating them);
 * PB_SUPPORT_ADAPTIVE also drops the rows / columns whose marginal mass is < 1e-8 and, inside
 * that box, the row segments whose taps are all < 1e-10 (the corners outside the Gaussian's
 * ellipse) -- results agree to fp32 rounding.  The staged halo is rounded up to 4, 6, 8, 10
 * or 12 samples (4, 8 or 12 for rank-1 kernels).                                          */
typedef enum pb_support { PB_SUPPORT_FULL = 0, PB_SUPPORT_ADAPTIVE = 1,
                          /* test/bench flag, OR-ed in: never take the rank-1 (separable) path */
                          PB_SUPPORT_FORCE_GENERAL = 16 } pb_support;

/* Keyword arguments of polyblur_deblurring() (deblurring.py:23-25). */
typedef struct pb_options {
    int32_t n_iter;
    float c, b;                 /* affine blur model (blur_estimation.py:171-185) */
    float alpha, beta;          /* polynomial parameters (deblurring.py:133-135) */
    float sigma_s, sigma_r;     /* domain-transform prefilter (deblurring.py:107) */
    float q;                    /* normalisation quantile in [0, 0.5) (blur_estimation.py:102-105); q > 0 is an exact
                                   torch.quantile by radix select on the device */
    int32_t n_angles;           /* 6 */
    int32_t n_interpolated_angles; /* 30 */
    int32_t remove_halo;
    int32_t edgetaping;
    int32_t prefilter;          /* pb_prefilter; reference prefiltering=True == BILATERAL */
    int32_t discard_saturation;
    int32_t boundary;           /* pb_boundary */
    int32_t support;            /* pb_support */
    float force_theta_deg;      /* < 0: estimate (default); >= 0: bench knob, overrides the
                                   estimated direction so that every kernel is rank-1 */
    int32_t separable_approx;   /* method='direct_separable': every reblurring K is replaced by the x-t separable
                                   APPROXIMATION of the same Gaussian (intent of separable_gaussian2d.cpp:91-183, whose own
                                   formulas do not run).  With q = A X^2 + 2 B X Y + C Y^2 the kernel's quadratic form
                                   (blur_estimation.py:204-207), q = A (X + (B/A) Y)^2 + (C - B^2/A) Y^2: a 1-D Gaussian of
                                   variance 1/A along X, then one of variance A/(AC - B^2) in Y taken along the line
                                   X = -(B/A) Y, each offset split between the two nearest samples by linear
                                   interpolation; X and Y swap roles when C > A (keeps |shear| <= 1).  Both 1-D kernels
                                   are sampled on the ker_size grid and normalised to sum 1.  Opt-in: deviates from the
                                   exact kernel by ~1e-2 (tests state the bound).  Zero boundary; not with edgetaping. */
    int32_t half_temporaries;   /* fp16 images only: store the two Horner temporaries t1, t2 as fp16 (accumulation and the
                                   x operand stay fp32; the images between iterations stay fp32).  Opt-in: the temporaries
                                   reach 9x the image range, where an fp16 ulp is 7.8e-3 -- measured 2e-3 .. 4.4e-3 from
                                   the fp32-temporary result; default 0 = fp32 temporaries             */
    int32_t ker_size;           /* support of the estimated Gaussian and, halved, the replicate pad (deblurring.py:23,
                                   blur_estimation.py:211-232, utils.py:48-53): 2 .. 49 (default 25; 0 means 25); even sizes are
                                   off-centre as in the reference and keep the stencil bodies.  Sizes above 25 do not fit
                                   pb_blur_info: their taps live in the context's scratch and every reblurring step is a plain
                                   LDS-tiled stencil (conv_big.hip: up to 2401 multiply-adds per sample -- 10 to 40 times the
                                   time of the default size); the record's `kernel` then holds the central 25 x 25 taps
                                   renormalised, theta / sigma / rho are exact.  Edgetaping and separable_approx are
                                   built for ODD sizes up to 25 only: with an even size or one above 25 pb_polyblur_batch and
                                   pb_make_separable_kernels return PB_ERR_UNSUPPORTED */
} pb_options;

/* Per-image, per-iteration estimation record (device or host copy). Mirrors the values the
 * reference computes in blur_estimation.py:59-73. */
typedef struct pb_blur_info {
    float gray_min, gray_max;           /* blur_estimation.py:107-108 */
    float mags[PB_MAX_ANGLES];          /* :122-134 */
    float interp[PB_MAX_INTERP];        /* :138-148 */
    int32_t i_min;                      /* :160 */
    float theta;                        /* radians, :167 */
    float sigma, rho;                   /* :171-185 */
    int32_t separable;                  /* 1 if the 25x25 kernel is rank-1 (theta % 90 == 0 or sigma == rho) */
    int32_t radius;                     /* support radius class actually evaluated: 4, 6, 8, 10 or 12 */
    float kernel[PB_KSIZE * PB_KSIZE];  /* :211-232, row-major [y][x] */
    float kx[PB_KSIZE], ky[PB_KSIZE];   /* marginals kx[j] = sum_i k[i][j], ky[i] = sum_j k[i][j];
                                           the exact rank-1 factors when `separable` */
    float acorr_y[PB_KSIZE], acorr_x[PB_KSIZE]; /* autocorrelation of ky / kx at lags 0..24: the closed
                                           form of edgetaper_alpha's 1-D FFTs (edgetaper.py:11-21) */
    float gtaps[(PB_KSIZE + 1) * 32];   /* kernel rows re-laid for the tile stencil: row y = {0,0,0, k[y][0..24], 0,0,0,0};
                                           row 25 is all zeros (the taps of the list's filler phases) */
    float gtaps_odd[(PB_KSIZE + 1) * 32]; /* the same rows shifted by one tap (gtaps_odd[y][n] = gtaps[y][n+1]): the second
                                           alignment of adjacent tap pairs for the packed-FMA stencil */
    /* x-t separable approximation (pb_options.separable_approx; filled in the SECOND record of a pair by
     * pb_make_separable_kernels): xt_first = 1 when the 1-D pass runs along x and the oblique pass walks rows, 0 for the
     * transposed arrangement; xt_g1 = the 1-D pass's taps; per offset i = -12..12 along the oblique pass's axis, the line
     * sits xt_m[i] + f samples across it and the two neighbours get the weights xt_wa[i] = g2 (1-f), xt_wb[i] = g2 f.   */
    int32_t xt_first;
    int32_t xt_exact_rank1;             /* the image's EXACT kernel is rank-1: it takes the exact separable body instead */
    float xt_g1[PB_KSIZE];
    int32_t xt_m[PB_KSIZE];
    float xt_wa[PB_KSIZE], xt_wb[PB_KSIZE];
    int32_t nphase[3];                  /* general (non rank-1) stencil: number of (kernel row, 4-tap segment) phases of
                                           kind 0 (inner chunk of a window row), 1 (first chunk), 2 (last chunk); each
                                           count is even (an all-zero filler phase pads an odd one)                  */
    int32_t phase[PB_MAX_PHASES + 9];   /* their descriptors, grouped by kind, row-major inside a kind: byte offset of the
                                           segment in the (64 + 2*radius)-wide staged tile | index of its first tap in
                                           gtaps << 16; three pad entries (read ahead, never evaluated) */
} pb_blur_info;

/* ---- context ------------------------------------------------------------------------- */
int pb_version(void);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the
 * device's default stream. */
int pb_create(pb_ctx **out, int device, void *stream);
int pb_destroy(pb_ctx *ctx);
int pb_set_stream(pb_ctx *ctx, void *stream);
int pb_synchronize(pb_ctx *ctx);
const char *pb_last_error_string(pb_ctx *ctx);
void pb_default_options(pb_options *opt);        /* the functional API's defaults, deblurring.py:23-25 */
/* How dense (non rank-1) kernels are evaluated by the reblurring pass.  PB_DENSE_STENCIL: always by the 2-D stencil
 * body (up to 625 multiply-adds per sample, fp32-vector-bound).  PB_DENSE_AUTO (default, min_phases = 16): images whose
 * stencil would run at least `min_phases` live (kernel row, 4-tap segment) phases (8 more when the support fits a
 * 4-sample halo; min_phases = 0: every dense point-symmetric kernel) are evaluated per 64 x 64 window in
 * the frequency domain inside LDS (overlap-save; same taps, same boundary models, results agree to fp32 rounding);
 * the others and rank-1 kernels keep the stencil bodies (fp32 planes: one wave per window pair, conv_wfft.hip; fp16 and
 * 8-bit planes, and passes too small to fill the chip: one workgroup per pair, conv_fft.hip).  Replaces nothing in the reference: both are
 * evaluations of filters.convolve2d (filters.py:14-49).  This call is the only way to choose: no environment variable does.
 * (PB_STRIP=1 -- rank-1 kernels of full support through the streaming strip body, conv_strip.hip, an experiment measured
 * slower than the tile body -- exists in `python -m polyblur_amd.build --experimental` builds only; the default library
 * ignores it.  INTEGRATION.md section 5 lists every environment knob.)
 * With the wrap boundary and no edgetaper the three Horner steps of an image's polynomial are ONE filter,
 * a3 K^3 + a2 K^2 + a1 K + b -- the reference's own 'fft' form, deblurring.py:139-169.  The engine measures that filter's
 * halo per axis and takes the polynomial as one window pass with the polynomial's spectrum wherever that costs less than
 * three passes with the kernel's halos (pb_polyblur_batch, pb_inverse_filter, pb_time_inner_loop; per image, decided on
 * the device): same taps, same results to fp32 rounding (fewer roundings), 2 words per sample through HBM instead of 8.
 * PB_POLY1=0 in the environment switches the form off, PB_POLY1=1 restricts it to kernels within the 4-sample halo class
 * (round 3's form); the cost model's constants are in csrc/common.h and csrc/khat.h.  pb_body_selection reports the
 * choice.  Environment variables are read when the context is created. */
typedef enum pb_dense_eval { PB_DENSE_STENCIL = 0, PB_DENSE_AUTO = 1 } pb_dense_eval;
int pb_set_dense_eval(pb_ctx *ctx, int mode, int min_phases);
/* Diagnostics: how the B images of iteration `iteration` of the most recent pb_polyblur_batch call on this context were
 * evaluated (-1: the most recent estimation / reblurring pass of any entry point) --
 * host[6 b + 0..5] = { tile-spectrum body (1) or a stencil body (0), halo class of the workgroup form (-1: a one-pass image
 * whose taps the device did NOT find point-symmetric although the call's class vouched for it -- NaN taps: the output is
 * then whatever the one-pass form makes of them), rank-1 strip flag,
 * whole polynomial in one window pass (1 / 2: on 64 x 64 / 128 x 128 windows) or three Horner steps (0), window halo along x,
 * along y }.  The choice is made
 * on the device from each record (no reference counterpart: filters.convolve2d, filters.py:14-49, has one evaluation);
 * bench.py labels its roofline line with it.  Synchronises the context's stream.                                   */
int pb_body_selection(pb_ctx *ctx, int iteration, int *host, int B);
/* bytes of scratch the context currently holds (for the HBM-footprint report) */
size_t pb_workspace_bytes(pb_ctx *ctx);

/* ---- plain device-memory helpers so a host without torch can drive the engine ------- */
int pb_malloc(pb_ctx *ctx, void **dptr, size_t bytes);
int pb_free(pb_ctx *ctx, void *dptr);
int pb_memcpy_h2d(pb_ctx *ctx, void *dst, const void *src, size_t bytes);   /* synchronous */
int pb_memcpy_d2h(pb_ctx *ctx, void *dst, const void *src, size_t bytes);   /* synchronous */

/* ---- whole pipeline: polyblur_deblurring (deblurring.py:23-96) ------------------------
 * in/out: (B,C,H,W) of `dtype`; out may not alias in.  host_info (optional) receives
 * n_iter*B records, iteration-major.                                                    */
int pb_polyblur_batch(pb_ctx *ctx, const void *in, void *out, int dtype,
                      int B, int C, int H, int W, const pb_options *opt,
                      pb_blur_info *host_info);

/* (H,W,C) interleaved bytes <-> (C,H,W) planar bytes for B images, the layouts either side of
 * utils.to_tensor / utils.to_array (utils.py:8-31) when the pixels stay uint8 on the device.  */
int pb_u8_deinterleave(pb_ctx *ctx, const unsigned char *hwc, unsigned char *chw, int B, int C, int H, int W);
int pb_u8_interleave(pb_ctx *ctx, const unsigned char *chw, unsigned char *hwc, int B, int C, int H, int W);

/* ---- stage entry points (each is also what the pipeline calls) ----------------------- */

/* gaussian_blur_estimation (blur_estimation.py:18-79): gray -> normalise -> spectral
 * gradients -> directional maxima -> direction -> (sigma, rho) -> 25x25 kernel.
 * Writes B records to dev_info (device memory).                                         */
int pb_estimate_blur(pb_ctx *ctx, const void *in, int dtype, int B, int C, int H, int W,
                     const pb_options *opt, pb_blur_info *dev_info);

/* create_gaussian_filter (blur_estimation.py:211-232) + support analysis, for caller-
 * supplied parameters: fills kernel/separable/radius of B device records from host arrays.
 * pb_make_kernels and pb_set_kernels synchronise, and the context remembers which bodies of the reblurring pass
 * these B records need (later passes on them skip the launch no image needs).  Records are to be rewritten through
 * this API only (pb_make_kernels, pb_set_kernels, pb_estimate_blur, pb_make_separable_kernels, pb_memcpy_h2d -- each
 * makes the context forget); after a raw copy into them call pb_set_dense_eval, which forgets everything.         */
int pb_make_kernels(pb_ctx *ctx, int B, const float *host_sigma, const float *host_rho,
                    const float *host_theta_rad, int support, pb_blur_info *dev_info);
/* Same, but the caller supplies arbitrary 25x25 taps (host, B*625 floats), in the orientation of the reference's kernel
 * tensors.  The reference applies such a kernel as a correlation under method='direct' (F.conv2d, filters.py:40-49) and as a
 * true circular convolution under method='fft' (K = p2o(kernel), filters.py:33-36) -- the same thing for point-symmetric
 * taps only.  The stage entry points follow it: with PB_ZERO the taps as given, with PB_WRAP -- where they are not
 * point-symmetric -- their point reflection (a second set of records built on the fly).                                 */
int pb_set_kernels(pb_ctx *ctx, int B, const float *host_taps, int support, pb_blur_info *dev_info);

/* method='direct_separable' (pb_options.separable_approx): from B records that hold (sigma, rho, theta) build the two
 * correlation kernels of the x-t separable approximation -- dev_sep[b] the 1-D pass, dev_sep[B + b] the oblique pass
 * with linear interpolation (intent of separable_gaussian2d.cpp:91-183; definition at pb_options.separable_approx).
 * ker_size: odd, 3 .. 25 (0 means 25); an even size -- the reference's off-centre grid, filters.py:78 -- or a larger one
 * returns PB_ERR_UNSUPPORTED.                                                                                          */
int pb_make_separable_kernels(pb_ctx *ctx, int B, const pb_blur_info *dev_info, pb_blur_info *dev_sep, int support,
                              int ker_size);

/* filters.fourier_gradients (filters.py:159-186) on P = B*C planes of H x W float32.
 * gx or gy may be NULL.  The transform keeps whole image lines in LDS when they fit -- up to 20480
 * samples when every prime factor is <= 7, up to 8192 otherwise: pb_fft_length_supported() == 1 --
 * and runs the same stages on a line buffer in device memory (context scratch, at most 256 MB; several
 * times slower per sample) for longer lines up to 65536 samples: == 2.  Beyond that: 0, and every
 * entry point that estimates blur or removes halos returns PB_ERR_UNSUPPORTED (the reference's
 * torch.fft takes any size). */
int pb_fft_length_supported(int n);                 /* 0, 1 or 2 (see above); needs no context */
int pb_fourier_gradients(pb_ctx *ctx, const float *planes, int P, int H, int W,
                         float *gx, float *gy);

/* inverse_filtering_rank3 (deblurring.py:211-239): replicate pad -> [edgetaper] ->
 * polynomial (three fused separable / general Gaussian stencil passes) -> crop ->
 * [halo masking with grad0 = gradients of the original image] -> clamp.
 * grad0_x/grad0_y: (B,C,H,W) float32, required iff remove_halo.                          */
int pb_inverse_filter(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                      const pb_blur_info *dev_info, float alpha, float beta, int boundary,
                      int edgetaping, int remove_halo, const float *grad0_x, const float *grad0_y);

/* filters.convolve2d on an already padded (B,C,Hp,Wp) float32 image: one reblurring pass
 * out = K * in with the given outer boundary (filters.py:14-37).                          */
int pb_convolve2d(pb_ctx *ctx, const float *in, float *out, int B, int C, int Hp, int Wp,
                  const pb_blur_info *dev_info, int boundary);

/* edgetaper.edgetaper (edgetaper.py:26-33) on a padded float32 image, per-image maximum. */
int pb_edgetaper(pb_ctx *ctx, const float *in, float *out, int B, int C, int Hp, int Wp,
                 const pb_blur_info *dev_info, int boundary);

/* ---- caller-owned kernel sets: the non-blind step with a PSF of the caller's, any kh x kw with 1 <= kh <= 49 and
 * 2 <= kw <= 49 (even, odd, square or rectangular) -- a calibrated lens blur, a motion streak, one kernel per colour plane.
 * The reference's inverse_filtering_rank3, filters.convolve2d and edgetaper.edgetaper take such a (B,C,h,w) kernel tensor
 * directly (deblurring.py:211-239, filters.py:14-37, edgetaper.py:26-33).
 *
 * pb_taps_create: host_taps holds B kernels of kh x kw floats, row-major, in the orientation of the reference's kernel
 * tensors (correlate=True is rot90(kernel, 2) on the host, deblurring.py:225-226); the taps are used as given -- nothing is
 * normalised.  One kernel per image; a caller with one kernel per plane passes its (B,C,H,W) batch as B*C one-channel images.
 * With PB_ZERO the kernel is applied as F.conv2d(padding='same') applies it (filters.py:40-49): tap (i, j) multiplies the
 * sample (i - (kh-1)/2, j - (kw-1)/2) away from the output.  With PB_WRAP as the circular convolution with the PSF rolled by
 * -(kh/2), -(kw/2) (p2o, filters.py:255-273): tap (i, j) multiplies the sample (kh/2 - i, kw/2 - j) away.  The set keeps both
 * forms in device memory of its own -- 25 x 25 records where the kernel fits them, tap tables of the large-kernel pass
 * otherwise --, valid across any other call on the context until pb_taps_free, which must come before pb_destroy.
 * Synchronises.  PB_ERR_BADARG: kw == 1 (the reference's crop [0:-0] is empty, utils.py:63-67); PB_ERR_UNSUPPORTED: a side above 49.
 * `support`: pb_support, as for pb_set_kernels.                                                                            */
typedef struct pb_taps pb_taps;
int pb_taps_create(pb_ctx *ctx, int B, int kh, int kw, const float *host_taps, int support, pb_taps **taps);
int pb_taps_free(pb_taps *taps);

/* filters.convolve2d(img, kernel, method) (filters.py:14-37) on a (B,C,H,W) float32 image that is the whole domain: zero
 * outside it (PB_ZERO) or circular over it (PB_WRAP).  out may not alias in.  PB_ERR_BADARG: kh > H - 1 or kw > W - 1.
 * PB_ERR_UNSUPPORTED: PB_WRAP with a kernel taller than wide (kh/2 > kw/2) -- the reference pads circularly by the half-WIDTH
 * only (filters.py:33, utils.py:48-61), so its result there is no circular convolution over the given domain; also below.   */
int pb_convolve2d_taps(pb_ctx *ctx, const float *in, float *out, int B, int C, int H, int W, const pb_taps *taps,
                       int boundary);

/* edgetaper.edgetaper(img, kernel, n_tapers, method) (edgetaper.py:26-33) on the same kind of image: n_tapers >= 0 blends
 * with the weights of THIS kernel -- autocorrelations of its two projections (edgetaper.py:10-23), up to 49 lags.          */
int pb_edgetaper_taps(pb_ctx *ctx, const float *in, float *out, int B, int C, int H, int W, const pb_taps *taps,
                      int boundary, int n_tapers);

/* inverse_filtering_rank3(img, kernel, alpha, b, ..., method) (deblurring.py:211-239) for fp32 or fp16 images: replicate pad
 * by kw / 2 on all four sides (utils.py:48-61: the kernel's height plays no part) -> [three edgetaper blends] -> polynomial
 * -> crop -> [halo masking] -> clamp to [0, 1].  grad0_x / grad0_y: (B,C,H,W) float32 or both NULL -- the reference's
 * grad_img=None: the gradients of the (tapered) image itself, deblurring.py:200-201.  PB_ERR_BADARG: kh > H + 2 (kw/2) - 1.
 * A kernel taller than wide is taken by the plain polynomial under either boundary (compute_polynomial_fft is circular over
 * the padded domain, deblurring.py:141-169) and refused with PB_WRAP and edgetaping (PB_ERR_UNSUPPORTED, as above).        */
int pb_inverse_filter_taps(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                           const pb_taps *taps, float alpha, float beta, int boundary, int edgetaping,
                           int remove_halo, const float *grad0_x, const float *grad0_y);

/* deblurring.compute_polynomial (deblurring.py:113-169) on a (B,C,H,W) float32 image that is the whole domain; no pad, no
 * crop, no clamp.  not_symmetric != 0: the pure-phase filter of compute_polynomial_fft -- the image spectrum times
 * conj(K) / (|K| + 1e-8) before the Horner steps, K = fft2(p2o(kernel)) --, PB_WRAP only (PB_ZERO -> PB_ERR_BADARG: the
 * reference's direct form accepts the flag and ignores it; a silent no-op is refused here).  It is one transform over the whole
 * domain: both sides need pb_fft_length_supported == 1 (PB_ERR_UNSUPPORTED otherwise).  Where |K| falls to fp32 roundoff
 * (about 1e-7; a wide Gaussian has such bins near Nyquist) the phase of that factor is noise, in the reference as much as here.
 * not_symmetric == 0: the existing reblurring passes over the given domain, either boundary.  A kernel taller than wide is
 * taken (p2o is circular over the domain).  out may not alias in.                                                      */
int pb_compute_polynomial_taps(pb_ctx *ctx, const float *in, float *out, int B, int C, int H, int W,
                               const pb_taps *taps, float alpha, float beta, int boundary, int not_symmetric);

/* inverse_filtering_rank3's chain (deblurring.py:211-239) with compute_polynomial(..., method='fft', not_symmetric=True) in
 * the polynomial's place: replicate pad by kw / 2 -> [three edgetaper blends, PB_WRAP] -> phase-corrected polynomial -> crop
 * -> [halo masking] -> clamp.  fp32 or fp16 images.  The argument rules and refusals of pb_inverse_filter_taps under PB_WRAP,
 * and PB_ERR_UNSUPPORTED where a padded side has pb_fft_length_supported != 1.  out may not alias in.                   */
int pb_inverse_filter_phase_taps(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                                 const pb_taps *taps, float alpha, float beta, int edgetaping, int remove_halo,
                                 const float *grad0_x, const float *grad0_y);

/* ---- gradients of the non-blind step.  The reference's README ("Import into your projects") promises: "The module and the
 * functional version above are fully differentiable.  They thus can be put within neural networks as training losses" -- there
 * ATen's autograd differentiates filters.convolve2d and deblurring.compute_polynomial; here these three calls are their backward
 * passes.  ODD kh and kw only (PB_ERR_UNSUPPORTED otherwise: the adjoint of an even-sized kernel sits one sample off the two forms a
 * set holds).  All planes (B,C,H,W) float32 that are the whole domain; outputs may not alias inputs.
 *
 * pb_tap_gradient: the lag correlation behind every tap gradient -- dev_grad[b][i][j] (= when accumulate == 0, += otherwise)
 * scale * sum over the C planes of image b and over every sample p of u[p] * v[p + off(i, j)], off(i, j) = (i - kh/2, j - kw/2)
 * with v zero outside the domain (PB_ZERO) or (kh/2 - i, kw/2 - j) with indices modulo the domain (PB_WRAP): d loss / d taps of
 * out = pb_convolve2d_taps(v) (filters.py:14-37) for the upstream gradient u.  1 <= kh, kw <= 49; no fit check (lags may exceed
 * the domain).  dev_grad: DEVICE memory, (B,kh,kw).  fp32 sums in a fixed order, no atomics: the same call gives the same bits.  */
int pb_tap_gradient(pb_ctx *ctx, const float *u, const float *v, int B, int C, int H, int W, int kh, int kw,
                    int boundary, float scale, int accumulate, float *dev_grad);

/* Backward of pb_convolve2d_taps (filters.convolve2d, filters.py:14-37): grad_x = K^T grad_out -- the same pass with the set's
 * other orientation --, grad_taps (device, (B,kh,kw)) = the lag correlation of grad_out with x.  grad_x or grad_taps may be NULL,
 * not both; x may be NULL when grad_taps is.  The argument rules and refusals of pb_convolve2d_taps.                          */
int pb_convolve2d_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps,
                                int B, int C, int H, int W, const pb_taps *taps, int boundary);

/* Backward of pb_compute_polynomial_taps with not_symmetric == 0 (deblurring.compute_polynomial, deblurring.py:113-169;
 * the pure-phase variant: pb_compute_polynomial_phase_taps_backward).  With g = grad_out, g2 = K^T g, g1 = K^T g2:
 *   grad_x = b g + a1 g2 + a2 g1 + a3 K^T g1 -- the same polynomial of K^T, in whichever form the forward would take;
 *   grad_taps (device, (B,kh,kw)) = L(g, t2) + L(g2, t1) + L(g1, a3 x) with the forward's temporaries t1, t2 formed again by
 *   explicit Horner steps (context scratch: four plane sets of the domain, "grad.t1" .. "grad.g1", and the partial tables).
 * NULL rules as above.  The argument rules and refusals of pb_compute_polynomial_taps.                                        */
int pb_compute_polynomial_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps,
                                        int B, int C, int H, int W, const pb_taps *taps, float alpha, float beta, int boundary);

/* The polynomial's own parameters: d loss / d alpha = 1/2 <G, K (1 - K)^2 x> and d loss / d beta = <G, (1 - K)^3 x>
 * for out = pb_compute_polynomial_taps(x) with not_symmetric == 0 and G = grad_out.  Evaluated in that factored form -- the detail
 * images u1 = x - K x, u2 = u1 - K u1, u3 = u2 - K u2 by three explicit Horner steps of the forward's pass under the call's boundary,
 * then one reduction  d beta = sum G u3,  d alpha = 1/2 sum G (u2 - u3)  -- because the sums of <G, K^i x> they expand to cancel a
 * hundredfold in fp32 on a blurred image.  grad_params: DEVICE memory, (B,2): (d / d alpha, d / d beta) per image as the engine
 * counts images (B; with one kernel per plane the caller passes B*C one-channel images); written, not accumulated.  alpha and beta
 * are taken for symmetry with the forward: the polynomial is linear in both, neither gradient depends on them.  The argument rules
 * and refusals of pb_compute_polynomial_taps_backward: ODD kh and kw (PB_ERR_UNSUPPORTED), the fit and shape checks; x, grad_out or
 * grad_params NULL, or grad_params aliasing an input: PB_ERR_BADARG; B above 65535: PB_ERR_UNSUPPORTED; every refusal before any
 * launch.  Scratch: two plane sets of the domain, "ppg.u1" (u1, then u3) and "ppg.u2", and the partials "ppg.partial".  Sums in
 * double at every level in an order the shape alone fixes, no float atomics: the same call gives the same bits, and operands at
 * any element offset give the aligned call's bits.  pb_compute_polynomial_taps_backward is untouched by it.                  */
int pb_compute_polynomial_taps_params_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_params,
                                               int B, int C, int H, int W, const pb_taps *taps, float alpha, float beta, int boundary);

/* Backward of pb_edgetaper_taps (edgetaper.edgetaper, edgetaper.py:10-33), with respect to the image and to the taps -- the taper
 * weights A = v1 (x) v2 are functions of the kernel (autocorrelations of its projections, normalised per kernel: the "per-image
 * maximum" above) and are differentiated too.  With x_0 = x, x_{i+1} = A x_i + (1 - A) (K x_i) and g_n = grad_out, for
 * i = n - 1 .. 0:  u_i = (1 - A) g_{i+1};  g_i = A g_{i+1} + K^T u_i (the pass with the set's other orientation);
 * grad_taps += L(u_i, x_i) (pb_tap_gradient's lag correlation);  Abar += sum over the image's planes of g_{i+1} (x_i - K x_i).
 * grad_x = g_0.  Then once per kernel, per axis (n the side, k the projection, ac its autocorrelation, z[p] = ac[p] + ac[n-1-p]):
 *   vbar1[py] = sum_px Abar v2[px], vbar2[px] = sum_py Abar v1[py];  zbar[p] = -vbar[p] / ac[0];
 *   acbar[l] = zbar[l] + zbar[n-1-l], acbar[0] += sum_p vbar[p] z[p] / ac[0]^2;  kbar[m] = sum_l acbar[l] (k[m+l] + k[m-l]);
 * and grad_taps[b][i][j] += kbar_y[i] + kbar_x[j].  grad_taps: device, (B,kh,kw), in the orientation of the caller's taps.
 * The taps' placement per boundary is the forward's (convolution under PB_WRAP, correlation under PB_ZERO), through the passes of
 * pb_convolve2d_taps_backward.  ODD kh and kw, up to 49 (PB_ERR_UNSUPPORTED otherwise); the fit and shape refusals of
 * pb_edgetaper_taps; n_tapers < 0: PB_ERR_BADARG; B above 65535: PB_ERR_UNSUPPORTED; n_tapers == 0: grad_x = grad_out, grad_taps = 0.  grad_x or grad_taps may be
 * NULL (then not computed, and no bit of the other changes), not both; grad_out may not be NULL; x may be NULL when grad_taps is --
 * the image gradient is linear in grad_out and reads only the kernel.  Outputs are written, not accumulated, and alias neither an
 * input nor each other (PB_ERR_BADARG).  Every refusal comes before any launch.
 * Scratch, in plane sets of the domain (B*C*H*W floats): "etg.u", "etg.ag" always, "etg.g" when n_tapers > 1 -- three; with grad_taps
 * also "etg.kx" (K x_i) and "etg.x" (x_1 .. x_{n-1}, formed again by the forward's own blends: n_tapers - 1 sets) -- n_tapers + 3 in
 * all --, "etg.abar" (B planes), "etg.vbar" (B * (H + W) floats) and pb_tap_gradient's partial tables.  fp32 sums in an order the
 * shape alone fixes, no float atomics: the same call gives the same bits.  Timed under PB_PROF_OTHER and the passes' own tags.  */
int pb_edgetaper_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps,
                               int B, int C, int H, int W, const pb_taps *taps, int boundary, int n_tapers);

/* Backward of pb_compute_polynomial_taps with not_symmetric != 0 (deblurring.compute_polynomial_fft with the pure-phase filter,
 * deblurring.py:141-169; p2o: filters.py:255-273).  H x W is the whole circular domain.  With K = fft2(p2o(kernel)), r = |K|,
 * C = conj(K) / (r + 1e-8), P the polynomial of K, P' its derivative, M = C P, N = H W, g = grad_out:
 *   grad_x = Re ifft2(conj(M) fft2(g)) -- the forward's passes with the conjugate multiplier;
 *   grad_taps (device, (B,kh,kw))[i][j] = Re fft2(S) at ((i - kh/2) mod H, (j - kw/2) mod W) -- the adjoint of p2o, a gather --,
 *   S = A (C_K P + C P') + conj(A C_Kbar P), A = (1 / N) sum over the image's planes of fft2(x) conj(fft2(g)),
 *   C_K = -conj(K)^2 / (2 r (r + eps)^2), C_Kbar = 1 / (r + eps) - r / (2 (r + eps)^2): C is a function of K and of conj(K).
 * Kernel sides even or odd, as the forward takes them.  grad_x or grad_taps may be NULL (then not computed, and no bit of the other
 * changes), not both; x may be NULL when grad_taps is.  Outputs are written, not accumulated, and alias neither an input nor each
 * other (PB_ERR_BADARG, before any launch).  PB_ERR_UNSUPPORTED before any launch where a side has pb_fft_length_supported != 1.
 * Scratch: complex H x W planes "phaseg.k", "phaseg.g" (one per plane pair of a group) and, with grad_taps, "phaseg.x" (as many)
 * and "phaseg.a"; groups as pb_set_phase_budget sizes them, two planes a pair with grad_taps.  fp32 sums in an order the shape
 * alone fixes, no float atomics: the same call gives the same bits, whatever the budget.                                     */
int pb_compute_polynomial_phase_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps,
                                              int B, int C, int H, int W, const pb_taps *taps, float alpha, float b);

/* ---- gradient of the blind estimation.  The README's promise covers the headline call too: in the reference the kernel that
 * gaussian_blur_estimation returns (blur_estimation.py:18-79) is a differentiable function of the image -- through the tap formula
 * (:189-232), sigma and rho (:171-185), the cubic interpolation (:138-148), the directional maxima (torch.amax: to the arg-max
 * pixel, :122-134), the spectral derivative (filters.py:159-186) and the min / max normalisation (:96-109).
 *
 * pb_estimate_blur_backward: grad_in (B,C,H,W; written, not accumulated) = d loss / d in for the upstream gradients grad_kernel
 * ((B, ker_size, ker_size), of the central taps of the records' kernels; or NULL) and grad_sigma_rho ((B, 2), of (sigma, rho); or
 * NULL; not both NULL) -- all DEVICE memory.  dev_info: the B records pb_estimate_blur wrote for `in` with the same options; the
 * direction (i_min, theta), the range (gray_min, gray_max) and the state of the clamps of sigma^2 / rho^2 are taken from them;
 * the arg-max pixels are found again, and the magnitudes, sigma and rho are evaluated again at those pixels in double (the
 * records' fp32 values carry the line transforms' rounding, which the chain amplifies).  fp32 images, opt->q == 0, odd
 * ker_size up to 25 (0 means 25), no forced direction: PB_ERR_UNSUPPORTED otherwise, before any launch.  Scratch: three fp32 planes per image ("estg.gray", "estg.gx", "estg.gy") and the partials ("estg.part").  fp32 sums
 * in a fixed order, no float atomics: the same call gives the same bits.  theta carries no gradient (it comes from integers).   */
int pb_estimate_blur_backward(pb_ctx *ctx, const float *in, int B, int C, int H, int W, const pb_options *opt,
                              const pb_blur_info *dev_info, const float *grad_kernel, const float *grad_sigma_rho,
                              int ker_size, float *grad_in);

/* pb_estimate_blur_backward with one more output: grad_cb (device, (B,2); written) = d loss / d (c, b) of the
 * affine model sigma^2 = c^2 / (m^2 + 1e-8) - b^2 per image, from the same scalar chain: with dv_e = d loss / d (sigma^2, rho^2),
 * d c = sum_e dv_e 2 c / (m_e^2 + 1e-8), d b = -2 b sum_e dv_e, in double, rounded once.  A clamped sigma^2 or rho^2 contributes
 * exactly 0 (the clamp's state is the forward's record's).  grad_in or grad_cb may be NULL, not both; with grad_in NULL the scatter
 * is not launched; with both, grad_in has the bits it has alone.  pb_estimate_blur_backward is this call with grad_cb == NULL:
 * the same launches, the same bits.  Every other rule, refusal and scratch name as above.                                      */
int pb_estimate_blur_params_backward(pb_ctx *ctx, const float *in, int B, int C, int H, int W, const pb_options *opt,
                                     const pb_blur_info *dev_info, const float *grad_kernel, const float *grad_sigma_rho,
                                     int ker_size, float *grad_in, float *grad_cb);

/* The pure-phase polynomial takes the plane pairs of an image in groups whose complex scratch (one Hp x Wp float2 plane per
 * pair) stays within `bytes`; one pair is always allowed.  0 = the default, 256 MiB.  Results do not depend on it.       */
int pb_set_phase_budget(pb_ctx *ctx, size_t bytes);

/* halo_masking (deblurring.py:193-208), bug-compatible.  All (B,C,H,W) float32.           */
int pb_halo_mask(pb_ctx *ctx, const float *x, const float *y, const float *grad0_x,
                 const float *grad0_y, float *out, int B, int C, int H, int W);

/* ---- gradient of halo masking (remove_halo=True under autograd).
 * pb_fourier_gradients_backward: the backward of pb_fourier_gradients (filters.fourier_gradients, filters.py:159-186).  The
 * circulant of the spectral derivative is odd, so its transpose is its negative: grad_planes (P planes of H x W; written, not
 * accumulated) = -(Dx grad_gx + Dy grad_gy).  Either upstream gradient may be NULL, not both; grad_planes may alias neither.
 * Scratch: one plane set ("halog.fy") when both are given.                                                                  */
int pb_fourier_gradients_backward(pb_ctx *ctx, const float *grad_gx, const float *grad_gy, int P, int H, int W,
                                  float *grad_planes);

/* pb_halo_mask_backward: the backward of pb_halo_mask (deblurring.halo_masking, deblurring.py:173-208, bug-compatible: M uses
 * grad_y * grad_y, :174; torch.clamp(min=0), :184, passes the gradient where M / (nM + M) >= 0).  grad_out is the upstream
 * gradient of out; grad_x, grad_y, grad_grad0_x, grad_grad0_y are d loss / d x, y, grad0_x, grad0_y.  Any of the four outputs may
 * be NULL (not all), and what a NULL output makes unnecessary is not computed; all (B,C,H,W) float32 DEVICE memory, written, not
 * accumulated; no output may alias an input or another output.  nM and the x-derivative of y are formed again by the forward's
 * launchers and M, z are evaluated as the forward evaluates them: a sample is on the side of the clamp the forward put it on.
 * Scratch: two plane sets ("halog.ox", and "halog.t" with grad_y), P floats of nM ("halog.nM") and, with a grad0 output, P of S
 * and the partial sums ("halog.S", "halog.part").  fp32 sums in a fixed order, no float atomics: the same call gives the same
 * bits.  Widths that pb_fft_length_supported rejects: PB_ERR_UNSUPPORTED before any launch.                                  */
int pb_halo_mask_backward(pb_ctx *ctx, const float *x, const float *y, const float *grad0_x, const float *grad0_y,
                          const float *grad_out, float *grad_x, float *grad_y, float *grad_grad0_x, float *grad_grad0_y,
                          int B, int C, int H, int W);

/* domain_transform.recursive_filter (domain_transform.py:6-63; native twin RF.cpp:43-92).
 * joint may be NULL (filter guided by itself).                                           */
int pb_dt_recursive_filter(pb_ctx *ctx, const void *in, const void *joint, void *out, int dtype,
                           int B, int C, int H, int W, float sigma_s, float sigma_r, int num_iterations);

/* pb_dt_recursive_filter_backward: the backward of pb_dt_recursive_filter (domain_transform.py:6-85 under autograd) with respect to
 * the image and to the guide; no gradient with respect to the two sigma.  in, joint, grad_out (the upstream gradient of out),
 * grad_in and grad_joint are (B,C,H,W) float32 DEVICE memory.  joint == NULL: the filter is guided by `in`; grad_joint must then be
 * NULL and grad_in receives both paths.  Either output may be NULL (not both), and what a NULL output makes unnecessary is not
 * computed: without a guide gradient neither the planes of the weights' adjoint nor the guide kernel.  Outputs are written, not
 * accumulated; they alias no input and do not alias each other.  A NULL context, non-positive sizes, a sigma that is not positive
 * and finite or num_iterations < 1: PB_ERR_BADARG before any launch.  The 2 N passes are run again keeping the input of each
 * (the forward saves nothing; the filter's only kink, |J[i] - J[i-1]|, is decided by the inputs, so nothing depends on the
 * forward's bits), then each pass backward: two sweeps per line that form f with P and g with Q (csrc/stage_math.h).  Scratch:
 * 2 N + 2 plane sets -- "dtg.x" (2 N - 1 of them: the inputs of passes 1 .. 2 N - 1), "dtg.f", "dtg.p", "dtg.g" -- and, with a guide
 * gradient, two (B,H,W) planes ("dtg.dx", "dtg.dy").  fp32 sums in an order the shape alone fixes, no float atomics: the same call
 * gives the same bits.  Timed under PB_PROF_PREFILTER.  Asynchronous on the context's stream.                                  */
int pb_dt_recursive_filter_backward(pb_ctx *ctx, const float *in, const float *joint, const float *grad_out,
                                    float *grad_in, float *grad_joint,
                                    int B, int C, int H, int W, float sigma_s, float sigma_r, int num_iterations);

/* normalized_convolution (NC.cpp:143-204), the domain-transform variant built on box filters in the
 * transformed domain; single-image semantics of the reference applied per image, any C.  H, W <= 8190. */
int pb_dt_normalized_convolution(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                                 float sigma_s, float sigma_r, int num_iterations);

/* filters.bilateral_filter (filters.py:107-148), 5x5, sigma_spatial=5, sigma_color=0.1. */
int pb_bilateral5(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W);

/* filters.bilateral_filter (filters.py:107-148) with its arguments: per plane, replicate pad of ksize / 2, the weight of a tap
 * exp(-(dx^2 + dy^2) / (2 sigma_spatial^2)) exp(-(v - centre)^2 / (2 sigma_color^2)), out = sum w v / (sum w + 1e-5).
 * dtype PB_F32 or PB_F16 (out has the same; fp32 accumulation); in and out (B,C,H,W) DEVICE memory, out may not alias in.
 * ksize odd, 1 .. PB_KSIZE; both sigma positive and finite -- anything else is PB_ERR_BADARG before any launch.  ksize == 5 is
 * pb_bilateral5's kernel with these sigma: at 5.0 / 0.1 the same bits.  Asynchronous on the context's stream; no scratch. */
int pb_bilateral(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                 int ksize, float sigma_spatial, float sigma_color);

/* pb_bilateral_backward: the backward of pb_bilateral with respect to the image (prefiltering=True under autograd; no gradient
 * with respect to the two sigma).  in, grad_out (the upstream gradient of out) and grad_in are (B,C,H,W) float32 DEVICE memory;
 * grad_in is written, not accumulated, and may alias neither input.  Shapes, window sizes and sigma as pb_bilateral's (odd ksize
 * from 1 to PB_KSIZE, 5 included); anything else is PB_ERR_BADARG before any launch.  D and out are formed again by the backward's
 * own arithmetic -- the filter has no kink, so nothing depends on the forward's bits.  Three launches: the centre term with out
 * and G = grad_out / (D + 1e-5), the tap term gathered over the replicate-padded domain, the fold of the pad.  Scratch: two plane
 * sets ("bilg.out", "bilg.G") and one padded plane set of (H + ksize - 1) x (W + ksize - 1) ("bilg.T").  fp32 sums in an order
 * the shape alone fixes, no float atomics: the same call gives the same bits.  Asynchronous on the context's stream.          */
int pb_bilateral_backward(pb_ctx *ctx, const float *in, const float *grad_out, float *grad_in, int B, int C, int H, int W,
                          int ksize, float sigma_spatial, float sigma_color);

/* ---- patch decomposition with windowed overlap-add (PolyblurDeblurring(patch_decomposition=True),
 * deblurring.py:269-340; "next" row 1 of SURVEY 8f).  The image is (virtually) replicate-padded by
 * (pad_top, pad_left) to a grid of n_i x n_j patches of ph x pw with strides (step_h, step_w).
 * pb_extract_patches gathers patches [first, first+count) of every image into
 * patches[(n-first)*B + b, c, y, x]; pb_overlap_add blends ALL n_i*n_j restored patches (laid out
 * [n*B + b, c, y, x]) with the separable window dev_win_y (x) dev_win_x, normalises by the summed
 * window (+1e-8), clamps to [0,1] and writes the H x W result.                               */
int pb_extract_patches(pb_ctx *ctx, const void *img, void *patches, int dtype, int B, int C, int H, int W,
                       int ph, int pw, int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left,
                       int first, int count);
int pb_overlap_add(pb_ctx *ctx, const void *patches, void *out, int dtype, int B, int C, int H, int W,
                   int ph, int pw, int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left,
                   const float *dev_win_y, const float *dev_win_x);

/* pb_extract_patches_backward: the backward of pb_extract_patches with respect to the image, over ALL n_i*n_j patches (no first /
 * count).  grad_patches ([n*B + b, c, y, x], the upstream gradient of the patches) and grad_img (B,C,H,W) are float32 DEVICE
 * memory; grad_img is written, not accumulated, and may not alias grad_patches.  grad_img[b,c,Y,X] is the sum of
 * grad_patches[n*B + b, c, py - i0(n), px - j0(n)] over every padded position (py, px) that clamps to (Y, X) and every patch that
 * holds it: one position inside, a run of pad + 1 on an edge, a rectangle in a corner.  The lattice arguments are the forward's;
 * ph, pw < 2, a step < 1, a lattice without a patch or a null pointer is PB_ERR_BADARG before any launch.  Three launches: the
 * cover gathered into a padded plane set, the fold of the padded rows, the fold of the padded columns -- no thread adds more than
 * a pad's run or a cover's patches.  Scratch: one padded plane set of new_h x new_w ("patchg.P") and one of H x new_w
 * ("patchg.R").  fp32 sums in an order the shape alone fixes, no float atomics: the same call gives the same bits.  Asynchronous
 * on the context's stream.                                                                                                        */
int pb_extract_patches_backward(pb_ctx *ctx, const float *grad_patches, float *grad_img, int B, int C, int H, int W,
                                int ph, int pw, int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left);

/* pb_overlap_add_backward: the backward of pb_overlap_add with respect to the patches (no gradient with respect to the window).
 * patches (the forward's input) and grad_patches are [n*B + b, c, y, x], grad_out (the upstream gradient of out) is (B,C,H,W), all
 * float32 DEVICE memory; grad_patches is written everywhere, zeros included, and may alias no input.  With num, den the forward's
 * cover sums at the image sample (Y, X) of a patch element and v = num / (den + 1e-8),
 *   grad_patches[n*B + b, c, y, x] = win_y[y] win_x[x] m grad_out[b,c,Y,X] / (den + 1e-8),   m = [0 <= v <= 1],
 * and exactly 0 for the elements in the cropped pad.  The mask is inclusive at both ends (torch.clamp's gradient), and v is formed
 * again from `patches` by the forward's own cover function, so m comes from the forward's bits.  Arguments and refusals as
 * pb_extract_patches_backward's.  Two launches: S = m grad_out / (den + 1e-8) per image sample into a scratch plane set
 * ("patchg.S"), then the windowed gather per patch element.  Deterministic, no float atomics.  Asynchronous on the context's
 * stream.                                                                                                                         */
int pb_overlap_add_backward(pb_ctx *ctx, const float *patches, const float *grad_out, float *grad_patches, int B, int C, int H, int W,
                            int ph, int pw, int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left,
                            const float *dev_win_y, const float *dev_win_x);

/* ---- timing hooks used by bench.py ------------------------------------------------------
 * Runs only the polynomial inner loop (three stencil passes, the SURVEY 8d "inner loop")
 * `reps` times on resident data and returns the average milliseconds per repetition
 * measured with hipEvents on the context's stream.                                       */
int pb_time_inner_loop(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                       const pb_blur_info *dev_info, float alpha, float beta, int boundary,
                       int reps, float *host_ms);

/* Per-kernel-class device timing with hipEvents on the context's stream.  Between begin and
 * end every launch is bracketed by two events; end synchronises and returns, per tag, the
 * summed milliseconds and the launch count (arrays of PB_PROF_NTAGS).                        */
#define PB_PROF_NTAGS 10
typedef enum pb_prof_tag {
    PB_PROF_CONV = 0,        /* stencil pass (one Horner step / taper blend) */
    PB_PROF_GRAY = 1,        /* gray + min/max */
    PB_PROF_GRAD_ROWS = 2,   /* row spectral derivative */
    PB_PROF_GRAD_COLS = 3,   /* column spectral derivative (+ directional maxima) */
    PB_PROF_PARAMS = 4,      /* parameter / kernel generation */
    PB_PROF_HALO = 5,        /* halo masking + its reductions */
    PB_PROF_PREFILTER = 6,   /* bilateral / domain transform / recombination */
    PB_PROF_OTHER = 7,
    PB_PROF_CONV_FUSED = 8,  /* reserved (an experiment of round 2 used it) */
    PB_PROF_CONV_FFT = 9     /* the same pass for dense kernels: tile-spectrum body (conv_fft.hip) */
} pb_prof_tag;
int pb_profile_begin(pb_ctx *ctx);
int pb_profile_end(pb_ctx *ctx, float *host_ms, int *host_count);

/* ---- batch scatter / gather over RCCL (one process per GPU) ----------------------------------
 * The reference has no communication (its only batching is the sequential patch-group loop of
 * deblurring.py:310-336).  Images are independent, so the one exchange the engine needs is: the batch
 * lives on a root rank, every rank deblurs a contiguous shard, the results return to the root.  These
 * entry points give that to a host without torch.distributed (the Python layer uses torch's process
 * group, polyblur_amd/distributed.py): grouped ncclSend / ncclRecv on the context's stream, xGMI
 * inside a node.  RCCL (librccl.so) is loaded when the first id / communicator is made.
 *
 *   rank 0:      pb_comm_unique_id(id);  ship the 128 bytes to the other ranks (file, socket, MPI ...)
 *   every rank:  pb_comm_init(&comm, ctx, rank, world, id);        (world == 1: id may be NULL)
 *                pb_comm_shard(B, world, rank, &first, &count);    contiguous shards, the first B % world get one more
 *                pb_comm_scatter(comm, root_batch, shard, dtype, B, C, H, W, root);
 *                pb_polyblur_batch(ctx, shard, shard_out, dtype, count, C, H, W, &opt, NULL);
 *                pb_comm_gather(comm, shard_out, root_batch_out, dtype, B, C, H, W, root);
 * root_batch is read / written on the root only (NULL elsewhere); a rank whose shard is empty may pass
 * NULL for its shard.  Everything is asynchronous on the context's stream.                              */
#define PB_COMM_ID_BYTES 128
typedef struct pb_comm pb_comm;
int pb_comm_shard(int B, int world, int rank, int *first, int *count);
int pb_comm_unique_id(unsigned char *id);
int pb_comm_init(pb_comm **comm, pb_ctx *ctx, int rank, int world, const unsigned char *id);
int pb_comm_destroy(pb_comm *comm);
int pb_comm_scatter(pb_comm *comm, const void *root_batch, void *shard, int dtype, int B, int C, int H, int W, int root);
int pb_comm_gather(pb_comm *comm, const void *shard, void *root_batch, int dtype, int B, int C, int H, int W, int root);
/* The overlapped form of scatter -> deblur -> gather (what polyblur_amd/distributed.py:deblur_from_root does over
 * torch.distributed; the reference's analogue is the sequential patch-group loop of deblurring.py:310-336): the batch
 * lives on `root` and travels in CHUNKS of k consecutive images -- exchange step t is one grouped ncclSend / ncclRecv
 * operation on a stream of its own in which the root sends chunk t of every peer's shard and receives result chunk t - 2
 * from every peer --, every rank deblurs chunk t - 1 meanwhile (ONE pb_polyblur_batch call of k images: a lone 1080p image
 * costs twice what it costs inside a batch), and the results land in root_out on the root.  Called by every rank with the
 * same B, C, H, W, dtype, options, root and chunk; root_batch / root_out are read / written on the root only (NULL
 * elsewhere).  Returns with the context's stream behind every transfer.  k: pb_comm_set_chunk -- 0 (the default) = image by
 * image (k = 1: the chunked exchange stays opt-in until it has run on two GPUs), k >= 1 = that many images per step,
 * PB_COMM_CHUNK_AUTO = pb_comm_default_chunk = about sqrt(largest peer shard / 2): 4 for 32 images per GPU, 1 for one.
 *   On an error between two steps (a failed pb_polyblur_batch, a HIP error) every remaining step is still posted -- moving
 * buffers whose content no longer matters -- so that no peer is left waiting for a matching send / recv; the first error
 * is returned once the exchange stream has been joined.
 *   EXPERIMENTAL for world > 1: the exchange has run over gloo (2 and 3 ranks, bit-exact) and in a world of one on an
 * MI355X; no grouped ncclSend / ncclRecv of it has executed on two GPUs yet (tests/test_gpu_rccl.py runs it on first
 * contact with a node that shows more than one).
 * pb_comm_plan_steps(_chunked) / pb_comm_plan(_chunked) state the order of a step's operations -- chunked: ops[4 i + 0..3] =
 * { 1 send | 0 recv, peer, first image, images }; image by image (k = 1): ops[3 i + 0..2] = { 1 send | 0 recv, peer, image
 * index } -- at most 2 (world - 1) of them, the order both sides enumerate them in; host-only, no GPU needed.   */
int pb_comm_deblur_from_root(pb_comm *comm, const void *root_batch, void *root_out, int dtype, int B, int C, int H, int W,
                             const pb_options *opt, int root);
#define PB_COMM_CHUNK_AUTO (-1)
int pb_comm_set_chunk(pb_comm *comm, int chunk);
int pb_comm_default_chunk(int B, int world, int root);
int pb_comm_plan_steps(int B, int world, int root);
int pb_comm_plan(int B, int world, int root, int rank, int step, int *ops, int *n_ops);
int pb_comm_plan_steps_chunked(int B, int world, int root, int chunk);
int pb_comm_plan_chunked(int B, int world, int root, int rank, int step, int chunk, int *ops, int *n_ops);

#ifdef __cplusplus
}
#endif
#endif /* POLYBLUR_HIP_H */
