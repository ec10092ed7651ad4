/*
 * depthstereo.h -- C ABI of libdepthstereo_hip.so: the MI355X (gfx950) replacement for the per-pixel
 * hot path of thygate/stable-diffusion-webui-depthmap-script v0.4.8.
 *
 * The reference has no FFI layer: the path is plain Python/numba.  Each entry point
 * below names the reference code it replaces (file:line under the reference tree); INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative DS_E* code on failure; nothing throws across
 *     the ABI; ds_last_error() returns a thread-local message for the last failure.
 *   - all image/depth/output pointers are DEVICE pointers (HBM) owned by the caller; the callee
 *     never frees or retains them.  Buffers are batched: n images of h x w pixels, c channels,
 *     pixel-interleaved (HWC), densely packed unless a stride argument says otherwise.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous with respect to the host unless stated otherwise.
 *   - a ds_ctx owns scratch memory (row flags, work lists, min/max slots, LUTs).  One ctx per
 *     host thread/stream; calls on the same ctx must be issued on one stream at a time.
 *   - results are bit-identical to the reference (uint8/uint16 outputs); float64 arithmetic is
 *     done in IEEE-754 binary64 without FMA contraction, in the reference's operation order.
 */
#ifndef DEPTHSTEREO_H
#define DEPTHSTEREO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_VERSION 100

/* error codes */
#define DS_OK            0
#define DS_EINVAL       -1   /* bad argument (null pointer, bad shape, unknown enum) */
#define DS_EUNSUPPORTED -2   /* legal in the reference but outside what the kernels cover */
#define DS_EHIP         -3   /* a HIP runtime call failed (message has the hipError string) */
#define DS_ENOMEM       -4

/* depth element types accepted by the stereo entry points */
#define DS_DEPTH_U16 0       /* what core_generation_funnel passes (core.py:211,253) */
#define DS_DEPTH_F32 1
#define DS_DEPTH_F64 2

/* fill techniques, src/stereoimage_generation.py:85-92 */
#define DS_FILL_NONE                0
#define DS_FILL_NAIVE               1
#define DS_FILL_NAIVE_INTERPOLATING 2
#define DS_FILL_POLYLINES_SOFT      3
#define DS_FILL_POLYLINES_SHARP     4

typedef struct ds_ctx ds_ctx;

/* library / context ----------------------------------------------------------------------------- */
int ds_version(void);
const char *ds_last_error(void);
/* device = HIP device ordinal the context allocates its scratch on */
int ds_ctx_create(ds_ctx **out, int device);
int ds_ctx_destroy(ds_ctx *ctx);

/* One eye of a stereo pair: where it is written and how far pixels move. */
typedef struct ds_eye {
    double divergence_px;    /* (divergence/100)*w, signed; stereoimage_generation.py:82 */
    double separation_px;    /* (separation/100)*w, signed; stereoimage_generation.py:83 */
    uint8_t *out;            /* device pointer of pixel (image 0, row 0, col 0) of this eye */
    int64_t out_row_stride;  /* bytes between rows     (w*c for a lone eye, 2*w*c inside a side-by-side) */
    int64_t out_img_stride;  /* bytes between images */
} ds_eye;

/*
 * ds_stereo_warp -- replaces apply_stereo_divergence (src/stereoimage_generation.py:77-92) and the
 * numba kernels it dispatches to: apply_stereo_divergence_naive (:95-159) and
 * apply_stereo_divergence_polylines (:162-283).  One call renders n_eyes (1 or 2) views of each of
 * the n images; min/max normalisation of the depth (:79-81) is done per image on the device.
 *   image   n*h*w*c uint8, c in 1..4
 *   depth   n*h*w elements of depth_dtype
 *   exponent  stereo_offset_exponent.  1.0 is computed directly; any other value needs a host-built
 *           table (pow must match the host libm): pass pow_lut = device pointer to n*65536 doubles,
 *           pow_lut[i*65536+v] = ((v-min_i)/(max_i-min_i))**exponent, depth_dtype must be U16.
 *           pow_lut == NULL with exponent != 1.0 -> DS_EUNSUPPORTED.
 * Undefined corners of the reference are defined in DESIGN.md ("Defined corners").
 */
int ds_stereo_warp(ds_ctx *ctx, const uint8_t *image, const void *depth, int depth_dtype,
                   int n, int h, int w, int c, double exponent, const double *pow_lut,
                   int fill, const ds_eye *eyes, int n_eyes, void *stream);

/* Per-image depth min/max as doubles {min,max} (device, n*2 doubles) -- the reduction of
 * stereoimage_generation.py:79-80 exposed so the host can build pow_lut.  Asynchronous. */
int ds_depth_minmax(ds_ctx *ctx, const void *depth, int depth_dtype, int n, int h, int w,
                    double *minmax_out, void *stream);

/* Kernel timing for roofline accounting.  When enabled, ds_stereo_warp brackets its dominant kernel (the naive or
 * polylines render kernel) and the exact-fallback kernel with HIP events recorded ON THE CALLER'S STREAM;
 * ds_profile_last_ms synchronises those events and returns the two durations of the most recent call. */
int ds_profile_enable(ds_ctx *ctx, int enable);
int ds_profile_last_ms(ds_ctx *ctx, float *render_ms, float *exact_ms);

/* In-step kernel timers (no counterpart in the reference; bench.py's `roofline` is the average duration of a kernel INSIDE the
 * timed step, measured on the stream it is launched on).  While enabled, the entry points below bracket their kernel launch with
 * a pair of HIP events out of a ring of 1024 pairs per kind (launches beyond the ring, and launches made while the stream is
 * being captured into a graph, are not timed); nothing synchronises until ds_kernel_timer_read, which waits for the last pair of
 * the kind and returns how many launches were timed and the sum of their durations.  Enabling (or disabling) resets every ring.
 * One thread at a time may launch on a context while its timers are on (the slot counters are not atomic).
 * A GEMM kind that hands its last tiles to the ragged round has a second timer, kind + DS_KT_RAGGED, around that launch. */
#define DS_KT_LINEAR_GELU      0   /* ds_linear, act = 1 (fc1 + GELU of an encoder block) */
#define DS_KT_ATTENTION        1   /* ds_attention_fwd */
#define DS_KT_LINEAR_RESIDUAL  2   /* ds_linear_residual (projection / fc2 + LayerScale + residual) */
#define DS_KT_LINEAR           3   /* ds_linear, act = 0 or 2 */
#define DS_KT_LINEAR_VT        4   /* ds_linear_vt */
#define DS_KT_CONV3X3          5   /* ds_conv3x3_nhwc */
#define DS_KT_LINEAR_READOUT   6   /* ds_linear_readout */
#define DS_KT_LINEAR_SHUFFLE   7   /* ds_linear_shuffle */
#define DS_KT_NORMALMAP        8   /* ds_normalmap (uint16, the fused kernel) */
#define DS_KT_DEPTH_REFINE     9   /* ds_joint_bilateral_u16 */
#define DS_KT_SPARSE_BILATERAL 10  /* ds_sparse_bilateral_f32, ds_sparse_bilateral_jump_f32 */
#define DS_KT_AOMAP           11   /* ds_aomap_u16 */
#define DS_KT_RAGGED          12   /* + kind: the ragged round (k_linear_ragged) of that GEMM kind */
int ds_kernel_timer_enable(ds_ctx *ctx, int enable);
int ds_kernel_timer_read(ds_ctx *ctx, int kind, int64_t *launches, double *total_ms);
/* the same, launch by launch in launch order: the first min(*launches, capacity) durations (ms) go to ms_out (bench.py tells the
 * projection launches of ds_linear_residual from the fc2 launches: they alternate) */
int ds_kernel_timer_read_each(ds_ctx *ctx, int kind, float *ms_out, int64_t capacity, int64_t *launches);

/* Number of image rows the last ds_stereo_warp on this ctx re-rendered with the exact sequential
 * sweep (polylines only; see DESIGN.md "exact fallback").  Synchronises the stream. */
int ds_stereo_last_exact_rows(ds_ctx *ctx, int64_t *rows_out, void *stream);
/* Same, plus the number of queue chunks (128 pixels each, partly filled) the polylines kernel handed to its
 * general-pixel kernel: stats_out[0] = exact rows, stats_out[1] = queue chunks.  Synchronises the stream. */
int ds_stereo_last_stats(ds_ctx *ctx, int64_t *stats_out, void *stream);

/*
 * ds_copy_view -- the "eye is the untouched original" branch of create_stereoimages
 * (stereoimage_generation.py:46,49) plus the np.hstack/np.vstack copies (:56-62): strided copy of
 * n images h x (w*c bytes) into a packed output.
 */
int ds_copy_view(ds_ctx *ctx, const uint8_t *src, int64_t src_row_stride, int64_t src_img_stride,
                 uint8_t *dst, int64_t dst_row_stride, int64_t dst_img_stride,
                 int n, int h, int64_t row_bytes, void *stream);

/*
 * ds_overlap_red_cyan -- replaces overlap_red_cyan (src/stereoimage_generation.py:286-307):
 * out[...,0] = im1[...,0]; out[...,1:3] = im2[...,1:3]; out is n*h*w*3 dense.
 * im1/im2 are addressed with (row, image) byte strides so they can live inside a side-by-side.
 */
int ds_overlap_red_cyan(ds_ctx *ctx, const uint8_t *im1, int64_t im1_row_stride, int64_t im1_img_stride,
                        const uint8_t *im2, int64_t im2_row_stride, int64_t im2_img_stride,
                        int n, int h, int w, int c, uint8_t *out, void *stream);

/*
 * ds_normalmap -- replaces create_normalmap (src/normalmap_generation.py:5-56) for uint16 depth.
 *   pre_blur / post_blur: Gaussian kernel size (odd, >0) or 0 to disable (:23-24, :42-48)
 *   sobel_ksize: 3 (default) / 1 / 5 / 7 ... odd, or 0 for np.gradient (:27-31)
 *   out: n*h*w*3 uint8
 */
int ds_normalmap(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int pre_blur,
                 int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream);

/*
 * ds_normalmap_f64 -- the same for float64 depth: create_normalmap accepts any real array
 * (src/normalmap_generation.py:20-21 promote `depthmap * (-1.0) / 256.0` to float64; integer and float32
 * inputs are cast to float64 by the host, which is exact).  Always the separable float64 passes.
 */
int ds_normalmap_f64(ds_ctx *ctx, const double *depth, int n, int h, int w, int pre_blur,
                     int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream);

/*
 * ds_normalmap_gradient_f32 -- create_normalmap(float32 depth, sobel_gradient=None) without blurs: the one combination the
 * reference evaluates in FLOAT32 from end to end (src/normalmap_generation.py:20-21 keep float32, :31 np.gradient, :34-39
 * np.linalg.norm + three divisions, :51-54 quantisation; cv2.Sobel would be fed np.float64(...) at :28-29, np.gradient is
 * not).  One fused pass, every operation the correctly rounded binary32 one in numpy's order: bit-identical.
 * depth n*h*w float32, h, w >= 2; out n*h*w*3 uint8.
 */
int ds_normalmap_gradient_f32(ds_ctx *ctx, const float *depth, int n, int h, int w, int invert, uint8_t *out, void *stream);

/*
 * ds_normalmap_gradient_f16 -- create_normalmap(float16 depth, sobel_gradient=None) without blurs: numpy keeps float16 from end to
 * end (src/normalmap_generation.py:20-21 do not promote, :31 np.gradient returns the input's inexact dtype, :34-39 and :51-54 are
 * float16 ufunc loops: each operation is computed in float32 and rounded to half; np.linalg.norm's add.reduce sums the squares in
 * float32 and rounds once).  One fused pass with exactly those roundings: bit-identical.  depth n*h*w IEEE binary16 (2 bytes each),
 * h, w >= 2; out n*h*w*3 uint8.
 */
int ds_normalmap_gradient_f16(ds_ctx *ctx, const void *depth, int n, int h, int w, int invert, uint8_t *out, void *stream);

/*
 * ds_normalmap_gradient_blur_f32 -- create_normalmap(float32 depth, sobel_gradient=None, pre_blur and / or post_blur): the reference
 * runs cv2.GaussianBlur on float32 data (src/normalmap_generation.py:23-24 the depth plane, :42-48 the three-channel normal followed
 * by the second normalisation) between numpy float32 steps.  CV_32F coefficients (getGaussianKernel's float rounding), float32
 * accumulation, BORDER_REFLECT_101; OpenCV's summation order is unpinned (cv2 is absent), everything else is numpy's float32
 * arithmetic.  Blur sizes odd, <= 63; 0 / negative = off (both off forwards to ds_normalmap_gradient_f32).
 */
int ds_normalmap_gradient_blur_f32(ds_ctx *ctx, const float *depth, int n, int h, int w, int pre_blur, int post_blur, int invert,
                                   uint8_t *out, void *stream);

/*
 * ds_normalmap_wrap, ds_normalmap_f64_wrap, ds_normalmap_gradient_f32_wrap, ds_normalmap_gradient_f16_wrap,
 * ds_normalmap_gradient_blur_f32_wrap -- the five entry points above on a depth map that is ONE PERIOD OF A TILING: the normal map
 * of a tileable depth map tiles.  The reference has no such mode and says so (src/normalmap_generation.py:16, "TODO: Tiling can be
 * improved (gradients could be matched)"): its borders put a frame around the normal map of a seamless texture.  Same parameter
 * lists, shape rules, dtype rules, error codes and kernel timer (DS_KT_NORMALMAP) as the entry point of the same name without
 * `_wrap`; the kernels are the same ones with one more compile-time mode that changes only which sample a tap outside the image
 * reads:
 *   cv2.Sobel / cv2.GaussianBlur taps (BORDER_REFLECT_101 above: index -1 reads 1, index size reads size - 2): here index i reads
 *     i mod size, a true modulo -- -1 reads size - 1, size reads 0, and a kernel wider than the image goes round more than once;
 *   np.gradient (above: f[1] - f[0] at index 0, f[size - 1] - f[size - 2] at index size - 1, (f[i + 1] - f[i - 1]) / 2 between):
 *     here (f[(i + 1) mod size] - f[(i - 1) mod size]) / 2 at every index, the two ends included.
 * Tap order, operation order and every rounding are those of the entry point without `_wrap`.  Hence, with
 *   R = pre_blur / 2 + (max(sobel_ksize, 3) / 2 for Sobel, 1 for np.gradient) + post_blur / 2     (integer divisions, 0 for a blur
 *   that is off),
 *   wrap(d) = plain(np.pad(d, R, mode='wrap'))[R:R+h, R:R+w]     bit for bit,
 * the result commutes with np.roll bit for bit, and every pixel at least R from the border gets the same bytes from both entry
 * points.  Images of a batch stay independent: the neighbour across a border is a sample of the same image.
 */
int ds_normalmap_wrap(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int pre_blur,
                      int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream);
int ds_normalmap_f64_wrap(ds_ctx *ctx, const double *depth, int n, int h, int w, int pre_blur,
                          int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream);
int ds_normalmap_gradient_f32_wrap(ds_ctx *ctx, const float *depth, int n, int h, int w, int invert, uint8_t *out, void *stream);
int ds_normalmap_gradient_f16_wrap(ds_ctx *ctx, const void *depth, int n, int h, int w, int invert, uint8_t *out, void *stream);
int ds_normalmap_gradient_blur_f32_wrap(ds_ctx *ctx, const float *depth, int n, int h, int w, int pre_blur, int post_blur, int invert,
                                        uint8_t *out, void *stream);

/*
 * ds_bilateral_u16 -- edge-preserving pre-filter for uint16 depth maps in front of the normal map ("16 bit deflickering": the
 * reference leaves it as a TODO, src/normalmap_generation.py:17, and has no implementation; this comment is the definition).
 * depth [n,h,w] uint16 -> out [n,h,w] float64 in the units of depth; feed out to ds_normalmap_f64[_wrap].
 *   ws: (2 radius + 1)^2 float64 spatial weights in raster order (dy outer, dx inner, both -radius..radius), made on the host:
 *       exp(-(dx^2 + dy^2) / (2 sigma_space^2)) where dx^2 + dy^2 <= radius^2, exactly 0.0 outside that circle;
 *   wr: 65536 float64 range weights, wr[k] = exp(-k^2 / (2 sigma_color^2)), made on the host.  Its argument is the INTEGER
 *       |D(q) - D(p)|: no exp runs on the device.
 *   For pixel p: num = den = 0; for every tap t in raster order with ws[t] != 0: q = p + (dy, dx) after the border rule, v = D(q);
 *       wgt = ws[t] * wr[|D(q) - D(p)|];  num = num + wgt * v (the product rounded, then the sum: no fused multiply-add);
 *       den = den + wgt;  out(p) = num / den, one IEEE division (the centre tap makes den >= 1).
 *   Borders: wrap == 0 BORDER_REFLECT_101 (radius < min(h, w) required), wrap != 0 tap index modulo the image size (any size).
 * One accumulation chain per pixel: a pixel's result does not depend on the tiling of the launch, the batch size or its position in
 * the batch; a float64 NumPy loop over the taps gives the same bits (tests/normalmap_bilateral_cases.py).
 * DS_EINVAL: a null pointer; n, h or w <= 0; radius outside 1..15; radius >= min(h, w) without wrap; out overlapping depth; out, ws
 * or wr not 8-byte aligned (depth: 2-byte).  DS_EUNSUPPORTED: n > 65535 or h > 32 * 65535.  Asynchronous on `stream`; the kernel
 * timer DS_KT_NORMALMAP brackets the launch.
 */
int ds_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int radius, const double *ws, const double *wr,
                     int wrap, double *out, void *stream);

/*
 * ds_joint_bilateral_u16 -- depth refinement: the joint (cross) bilateral filter of a uint16 depth map guided by the image.  The
 * spatial kernel is a Gaussian; the range weight is taken from the COLOUR difference of the guide, not from the depth, so depth
 * averages only within a colour region and a silhouette's ramp collects at the colour edge.  The reference has no counterpart; this
 * comment is the definition.
 * depth D [n,h,w] uint16, guide G [n,h,w,c] uint8 dense with c = guide_channels in {3, 4} -> out [n,h,w] uint16.  Only the first three
 * bytes of a guide pixel are read; for c == 4 the fourth byte is ignored.
 *   ws: (2 radius + 1)^2 float64 spatial weights in raster order (dy outer, dx inner, both -radius..radius), made on the host exactly
 *       as for ds_bilateral_u16: exp(-(dx^2 + dy^2) / (2 sigma_space^2)) where dx^2 + dy^2 <= radius^2, exactly 0.0 outside that circle;
 *   wc: 766 float64 colour weights, wc[k] = exp(-k^2 / (2 sigma_color^2)), made on the host.  Its argument is the INTEGER
 *       k(q, p) = |R_q - R_p| + |G_q - G_p| + |B_q - B_p|, in 0..765: no exp runs on the device, and sigma_color is in units of summed
 *       8-bit channel difference.
 *   For pixel p: num = den = 0; for every tap t in raster order with ws[t] != 0: q = p + (dy, dx) after the border rule;
 *       wgt = ws[t] * wc[k(q, p)];  num = num + wgt * (double)D(q) (the product rounded, then the sum: no fused multiply-add);
 *       den = den + wgt.  Then F = num / den, one IEEE division, and out(p) = (uint16) rint(F), round-half-to-even.
 *   The centre tap makes den >= 1.  F is a convex combination of uint16 values, so rint(F) lies in 0..65535: no clamp is part of the
 *   definition.
 *   Borders: wrap == 0 BORDER_REFLECT_101 (radius < min(h, w) required), wrap != 0 tap index modulo the image size (any size); the same
 *   rule for D and G.
 * One accumulation chain per pixel: a pixel's bits depend neither on the tiling of the launch, nor on the batch size, nor on its
 * position in the batch; a float64 NumPy loop over the taps gives the same bits (tests/depth_refine_cases.py).  Iterations are a host
 * loop over this entry point between two buffers: pass i + 1 filters the uint16 result of pass i with the same guide.
 * DS_EINVAL: a null pointer; n, h or w <= 0; guide_channels not in {3, 4}; radius outside 1..15; radius >= min(h, w) without wrap; out
 * overlapping depth; ws or wc not 8-byte aligned, depth or out not 2-byte aligned (the guide may have any alignment).
 * DS_EUNSUPPORTED: n > 65535 or h > 32 * 65535.  Asynchronous on `stream`; the kernel timer DS_KT_DEPTH_REFINE brackets the launch.
 */
int ds_joint_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, const uint8_t *guide, int guide_channels, int n, int h, int w, int radius,
                           const double *ws, const double *wc, int wrap, uint16_t *out, void *stream);

/*
 * ds_sparse_bilateral_f32 -- one pass of the 3D-photo pipeline's depth preparation: the discontinuity-masked median that
 * inpaint.bilateral_filtering.sparse_bilateral_filtering runs (five times by default) on the float32 depth map in front of the mesh
 * code.  The reference is a Python loop over every pixel (inpaint/bilateral_filtering.py:105-172, the branch with a discontinuity
 * map and no mask; sigma_s and sigma_r are read there and never used).  A pass computes no depth: every output is ONE OF THE WINDOW'S
 * DEPTHS, so the result equals the reference bit for bit.  This comment is the definition.
 * V [n,h,w] float32: the map of this pass.  V0 [n,h,w] float32: the map the driver was called with (V0 == V as one buffer is legal:
 * the first pass).  window s: odd, 1..15, m = s / 2.  t = threshold.  c(i, size) = min(max(i, 1), size - 2).
 *   disp = 1.0f / V, one correctly rounded binary32 division (1 / 0 = inf).
 *   Jump map J of V: for 1 <= y <= h - 2 and 1 <= x <= w - 2, J(y, x) = 1 if |disp(y, x) - disp(q)| > t in binary32 for any of the
 *       four neighbours q (up, down, left, right), else 0; J = 0 on the outermost ring.  IEEE throughout: inf - finite is a jump,
 *       inf - inf is NaN and NaN is no jump.
 *   Discontinuity map D = J | (V0 == 0): V0, the ORIGINAL map, on every pass.
 *   The tap at window offset (dy, dx), -m <= dy, dx <= m, of pixel (y, x) reads V and D at (c(y + dy, h), c(x + dx, w)): the
 *       outermost ring is replaced by its inner neighbour, and the same clamp pads the image by any width.
 *   out(y, x): if no tap has D set, the centre tap.  Else, with n the number of taps with D == 0: the centre tap if n == 0, else the
 *       tap value of 0-based rank rank[n] in ascending order among those n taps (ties carry equal values: their order is immaterial).
 *   rank: 226 int32 made on the host (src/_native.py: sparse_bilateral_rank_table), rank[n] = np.digitize(0.5, np.cumsum(c / c.sum()))
 *       with c = np.ones(n, np.float32): the reference's float32 running sum of 1 / n.  It is NOT n / 2 (n = 20, 22, 28, 36, 40, 44,
 *       48 ... differ); no kernel holds a closed form of it.
 *   jump [n,h,w] uint8 receives J (not D): the driver blackens its image of the pass with it.
 * Precondition: every V and V0 finite and >= 0 (the order of such binary32 values is the order of their bit patterns, which is what
 * the selection compares).  Other values are memory-safe and give J by the rules above, but out is unspecified.
 * A pixel's bits depend on its window alone: not on the tiling of the launch, the batch size or its position in the batch; the NumPy
 * model is tests/sparse_bilateral_cases.py.
 * DS_EINVAL: a null pointer; n <= 0; h < 3 or w < 3 (the reference fails there); window even or outside 1..15; V, V0, out or rank
 * not 4-byte aligned; out overlapping V or V0; jump overlapping V, V0 or out.  DS_EUNSUPPORTED: n > 65535 or h > 32 * 65535 (the limits of ds_bilateral_u16), or an image of
 * more than 2^31 - 1 tiles of 64 x 8 pixels.  Every
 * refusal returns before any launch.  Asynchronous on `stream`; one kernel, no workspace; the kernel timer DS_KT_SPARSE_BILATERAL
 * brackets the launch.
 *
 * ds_sparse_bilateral_jump_f32 -- J of V alone, by the same rules and with the same checks (those that name its arguments) and
 * timer: the image of the driver's LAST pass needs the jump map of that pass's input, and nothing returns that pass's output.
 */
int ds_sparse_bilateral_f32(ds_ctx *ctx, const float *v, const float *v0, int n, int h, int w, int window, float threshold,
                            const int32_t *rank, float *out, uint8_t *jump, void *stream);
int ds_sparse_bilateral_jump_f32(ds_ctx *ctx, const float *v, int n, int h, int w, float threshold, uint8_t *jump, void *stream);

/*
 * ds_aomap_u16 -- ambient-occlusion map of a uint16 depth map taken as a height field: per pixel, the mean over K directions of the
 * sine of the horizon's elevation above the horizontal, subtracted from 1.  The reference has no counterpart; this comment is the
 * definition, and the only normative text.
 * Inputs.  depth D [n,h,w] uint16, white = near = high.  H = D, or H = 65535 - D with invert != 0.  radius R: an integer in 1..32.
 *   directions K: one of 4, 8, 16.  relief: the height in pixels that the full uint16 range stands for, finite and > 0; intensity:
 *   finite and > 0.  The host computes z = relief / 65535.0 and c = intensity / K in float64 and passes both as doubles.
 * Rays.  The directions are the 16-point rose, indexed o = k * 16 / K for k = 0..K-1; q = o / 4 is the quadrant and r = o % 4 the
 *   position inside it.  For step s = 1..R let m = rint(s * (sqrt(2.0) - 1.0)) in float64 (no s <= 32 comes within 0.0147 of a tie).
 *   The base offset (dx, dy) is (s, 0) for r = 0, (s, m) for r = 1, (s, s) for r = 2, (m, s) for r = 3, rotated q times by
 *   (x, y) -> (-y, x); x runs along a row and y down the rows.  A tap is kept iff d2 = dx^2 + dy^2 <= R^2 (at R = 1 the diagonals are
 *   empty); the taps of a ray are visited in increasing s.
 *   taps: int32 (dx, dy) pairs, ray after ray; dir_start: K + 1 int32, ray k owns taps dir_start[k] .. dir_start[k + 1] - 1.  Both are
 *   made on the host (src/_native.py: aomap_offsets); no kernel holds a closed form.  A table that is not the one above cannot make
 *   the kernel read outside its arguments (offsets are clamped to -R..R, indices to 0..16 R), but the output is then unspecified.
 * Horizon of ray k at pixel p.  Start with bn = 0, bd = 1.  A tap at q = p + (dx, dy) takes part if it lies inside the image: with
 *   wrap == 0 taps outside the image are skipped, with wrap != 0 indices are taken modulo the size, by as many periods as needed.
 *   Let D = H(q) - H(p).  If D > 0 and D^2 * bd > bn^2 * d2, the tap becomes the best: bn = D, bd = d2.  The compare is exact (both
 *   sides are below 2^43: 64-bit integers, or exact float64 products) and strict, so the earlier tap wins a tie.
 * Value.  a = (double)bn * z;  o_k = a / sqrt((double)bd + a * a), each multiply, add, sqrt and division rounded on its own (no
 *   contraction);  S = ((o_0 + o_1) + ...) + o_{K-1}, summed in direction order from 0.0 (a ray with no rising tap gives +0.0);
 *   v = 1.0 - S * c, the product rounded first, then the difference.
 * Outputs.  out_f64 [n,h,w] float64: v, unclamped; the pointer may be NULL.  out_u8 [n,h,w] uint8: rint(255.0 * min(max(v, 0.0), 1.0)),
 *   rounding half to even.
 * A pixel's bits depend on its rays alone: not on its tile, its position in the batch or the launch; the NumPy model is
 * tests/aomap_cases.py.
 * This is the height-field form of horizon-based ambient occlusion; it ignores the surface's own tilt, so a ramp darkens uniformly.
 * DS_EINVAL, before any launch: a null pointer other than out_f64; n, h or w <= 0; radius outside 1..32; directions not in {4, 8, 16};
 * z or c not finite or <= 0; taps or dir_start not 4-byte aligned, out_f64 not 8-byte aligned, depth not 2-byte aligned (out_u8 may
 * have any alignment); an output overlapping depth or the other output.  DS_EUNSUPPORTED: n > 65535 or h > 32 * 65535.  Asynchronous
 * on `stream`; one kernel, no workspace; the kernel timer DS_KT_AOMAP brackets the launch.
 */
int ds_aomap_u16(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int radius, int directions, const int32_t *taps,
                 const int32_t *dir_start, double z, double c, int invert, int wrap, uint8_t *out_u8, double *out_f64, void *stream);

/*
 * ds_lensblur_u8 -- lens blur from depth: a synthetic shallow depth of field, gathered per output pixel over a disc whose radius
 * follows the distance of the depth from a focus depth, with an occlusion rule.  The reference has no counterpart; this comment is the
 * definition, and the only normative text.  Everything is an integer: every sum is order-independent.
 * Inputs, per batch.  image [n,h,w,3] uint8.  depth [n,h,w] uint16.  focus [n] uint16, on the device: one focus depth per image, in the
 *   units of depth as stored.  Integers R in 1..32 (the largest blur radius in pixels), A in 1..65535, band in 0..65535.  Flag invert.
 * Nearness.  z = depth, or 65535 - depth with invert != 0; a larger z is nearer.
 * Circle of confusion, in quarter pixels.  e = max(|depth - focus| - band, 0);  rho = min(4 R, (e * A + 32768) >> 16), where
 *   e * A + 32768 < 2^32.  rho does not depend on invert.
 * Disc and weights.  For rho in 0..4 R:  n(rho) = #{(dx, dy) in Z^2 : 16 (dx^2 + dy^2) <= rho^2}  and  W[rho] = 2^20 // n(rho).
 *   n(0..3) = 1, n(4) = 5, n(128) = 3209, W[128] = 326.  table: the 4 R + 1 uint32 W[0..4 R], made on the host (src/_native.py:
 *   lensblur_table); no kernel holds a closed form.  The kernel uses the low 24 bits of an entry and never uses one as an address: a
 *   table that is not the one above cannot make it read outside its arguments, but the output is then unspecified.
 * Gather.  For an output pixel p consider every pixel q of the same image with d2 = |q - p|^2 <= R^2; taps outside the image are
 *   skipped (there is no wrap mode).  far = z(q) < z(p);  rho_e = far ? min(rho(q), rho(p)) : rho(q).  The tap counts iff
 *   16 d2 <= rho_e^2; a counted tap adds W[rho_e] to den and W[rho_e] * c(q) to num_c for each of the three channels c.
 *   So a nearer blurred pixel spreads over what is behind it, a farther pixel reaches p only as far as p's own blur allows, and an
 *   in-focus foreground keeps a hard edge against a blurred background.  The self tap always counts: den > 0.
 * Outputs.  out_rgb [n,h,w,3] uint8: out_c = (2 num_c + den) // (2 den).  out_coc [n,h,w] uint8: rho; the pointer may be NULL.
 * Accumulators.  A tap at offset (dx, dy) adds at most W[ceil(4 sqrt(d2))]; summed over the disc at R = 32 that is 8,103,748, times 255
 *   it is 2,066,455,740 < 2^31: den, the three num_c and 2 num_c + den fit uint32.
 * Identities.  If every rho < 4 the output equals the image.  A constant-colour image comes back unchanged for any depth.
 * A pixel's bits depend on its disc alone: not on its tile, its position in the batch or the launch; the NumPy model is
 * tests/lensblur_cases.py.
 * DS_EINVAL, before any launch: a null pointer other than out_coc; n, h or w <= 0; R outside 1..32, A outside 1..65535, band outside
 * 0..65535; table not 4-byte aligned, focus or depth not 2-byte aligned (image, out_rgb and out_coc may have any alignment); an output
 * overlapping image, depth, focus, table or the other output.  DS_EUNSUPPORTED: n > 65535 or h > 32 * 65535.  Asynchronous on `stream`;
 * one kernel, no workspace; no kernel-timer kind (the kinds below DS_KT_RAGGED are used up).
 */
int ds_lensblur_u8(ds_ctx *ctx, const uint8_t *image, const uint16_t *depth, const uint16_t *focus, int n, int h, int w, int radius,
                   int aperture, int band, int invert, const uint32_t *table, uint8_t *out_rgb, uint8_t *out_coc, void *stream);

/*
 * ds_parallax_u8 -- parallax frames from depth: F novel views of each of n images by its uint16 depth map, for small camera motions.
 * Every source pixel is pushed to where it lands in the new view (splat), the nearest pixel wins each target pixel, and the
 * disocclusion holes are closed from the background side (resolve).  The reference renders such clips from a layered, inpainted mesh;
 * this comment is the definition, and the only normative text.  Everything is an integer, and the depth test is a maximum, so the
 * result does not depend on the order in which anything runs.  `>>` is an arithmetic shift: a floor.
 * Inputs.  image [n,h,w,3] uint8.  depth [n,h,w] uint16.  focus [n] uint16, on the device, in the units of depth as stored.
 *   poses [F,3] int32 (tx, ty, tz), on the device: tx, ty in sixteenths of a pixel of shift per full uint16 range of depth difference,
 *   tz in 1/4096 of scale per full range; each component is clamped to -1024..1024 in the kernel (a bad device array can then not
 *   address outside the arguments; the host wrapper rejects such poses before that).  fill G in 1..64.  Flag invert.
 *   Workspace keys [n,F,h,w] uint64, any content: the entry point clears it.
 * Nearness.  z = depth, or 65535 - depth with invert != 0; z0 = focus, mapped the same way; e = z - z0, |e| <= 65535.
 * Landing point of source pixel (x, y) under pose k, in sixteenths of a pixel with the pixel centre at 16 x + 8:
 *   sx = (e * tx + 32768) >> 16;  sy = (e * ty + 32768) >> 16;  m = (e * tz + 32768) >> 16;
 *   cx = 16 x + 8 - 8 w;  cy = 16 y + 8 - 8 h;
 *   ux = 16 x + 8 + sx + ((cx * m + 2048) >> 12);  uy = 16 y + 8 + sy + ((cy * m + 2048) >> 12).
 *   |e * t| < 2^26 and |c * m| < 2^28: int32 suffices.
 * Footprint, 1.5 pixels wide, so that a stretch of up to 1.5 leaves no cracks: target columns X0..X1 with X0 = (ux - 5) >> 4 and
 *   X1 = ((ux + 19) >> 4) - 1 -- one column, or two exactly when (ux - 8) mod 16 is in 5..12 -- and rows Y0..Y1 likewise from uy.
 *   Targets outside the image are dropped.  At zero displacement the footprint is the pixel itself.
 * Splat.  key = ((z + 1) << 32) | (y w + x); keys starts at 0 everywhere; every covered target takes the maximum of the keys offered
 *   to it.  So the nearer pixel wins, among equal z the larger source index, and 0 means that nothing landed.
 * Resolve, per target (X, Y) of view k.  key != 0: out = image[key & 0xFFFFFFFF] (a pixel index of the same image), mask = 0.
 *   Otherwise scan left, right, up and down, in that order, each over steps 1..G and not beyond the image border; the first target
 *   with key != 0 is the direction's candidate.  The candidate with the smallest key >> 32 -- the farthest: a disocclusion belongs to
 *   the background -- gives its source pixel, the earlier direction on a tie, and mask = 1.  No candidate: out = image[Y][X] of the
 *   same image, mask = 2.
 * Outputs.  out [n,F,h,w,3] uint8.  out_mask [n,F,h,w] uint8; the pointer may be NULL.
 * Identities.  Pose (0, 0, 0) returns the image with an all-zero mask, for any depth.  A depth equal to the focus everywhere returns
 * the image for any pose.  Views and images are independent of each other.  The NumPy model is tests/parallax_cases.py.
 * DS_EINVAL, before any launch: a null pointer other than out_mask; n, h, w or F <= 0; fill outside 1..64; keys not 8-byte aligned,
 * poses not 4-byte aligned, depth or focus not 2-byte aligned (image, out and out_mask may have any alignment).  Then DS_EUNSUPPORTED:
 * n * F > 65535, or h or w > 16384.  Then DS_EINVAL: out, out_mask or keys overlapping an input or each other.  Asynchronous on
 * `stream`: a memset of keys on that stream and two launches, so the call is safe under graph capture.  No kernel-timer kind; with
 * ds_profile_enable the context's two event pairs bracket the splat and the resolve launch, and ds_profile_last_ms returns them.
 */
int ds_parallax_u8(ds_ctx *ctx, const uint8_t *image, const uint16_t *depth, const uint16_t *focus, int n, int h, int w,
                   const int32_t *poses, int F, int fill, int invert, void *keys, uint8_t *out, uint8_t *out_mask, void *stream);

/*
 * ds_autostereogram_u8 -- autostereograms from depth: the single-image stereogram ("magic eye": random dots, or a texture) of each of
 * n uint16 depth maps.  The depth map alone decides which pixels of a row must share a colour: every column links the two columns in
 * which the two eyes see it, and a pixel takes its colour from the connected component it ends up in.  The reference has no
 * counterpart; this comment is the definition, and the only normative text.  Everything is an integer, every row is independent, and a
 * component's representative is a maximum, so the result does not depend on the order in which anything runs.
 * Inputs.  depth [n,h,w] uint16, white = near.  period P in 16..512: the on-screen separation in pixels of the far plane, the width of
 *   a strip.  m in 1..128: the depth factor mu = m / 256 (mu = 1/3, m = 85: the near plane sits a third of the way from the screen to
 *   the eyes).  mode 0 = coloured dots, 1 = black / white dots, 2 = a pattern tile [ph,pw,3] uint8 on the device, ph and pw in 1..4096
 *   (with mode 0 or 1, tile, ph and pw are not looked at, and tile may be NULL).  seed: any uint32.  Flag invert.
 * Nearness.  z = depth, or 65535 - depth with invert != 0.  A = 256 * 65535.
 * Separation of a column of nearness z, rounded half up, in 64-bit integers:
 *   den = 2 A - m z;  num = 2 P (A - m z);  s(z) = (2 num + den) / (2 den).
 *   s(0) = P and s never increases with z; P = 96, m = 85 gives 96, 92, 87, 82, 77 at z = 0, 16384, 32768, 49152, 65535.
 * Link.  Column x, with s = s(z[x]), l = x - (s >> 1) and r = l + s, offers the undirected link {l, r} when 0 <= l, r < w and x is
 *   visible.
 * Visibility (hidden-surface removal).  k = 2 A - m z[x].  For t = 1, 2, ...: zt = z[x] + (2 t k) / (m 2 P), an integer division; stop
 *   at the first t with zt >= 65535 (after at most m P / 512 + 1 steps: at most 129).  x is hidden when for some t before that
 *   z[x - t] >= zt or z[x + t] >= zt; columns outside the row occlude nothing.
 * Colour.  rep(x) = the largest column index in the connected component of x under all links offered in its row.  Pixel (y, x):
 *   modes 0 and 1: hash = lowbias32(seed ^ (y * 0x9E3779B1) ^ (rep * 0x85EBCA77)) in uint32 wrap-around arithmetic, lowbias32(v) being
 *     v ^= v >> 16; v *= 0x7FEB352D; v ^= v >> 15; v *= 0x846CA68B; v ^= v >> 16.
 *     Mode 0: R, G, B = bits 0-7, 8-15, 16-23 of hash.  Mode 1: 255 * (hash >> 31) on all three channels.
 *   mode 2: tile[y mod ph][rep mod pw].
 * Output.  out [n,h,w,3] uint8, at any byte address.  The image index does not enter: an image's output does not depend on its batch.
 * Identities.  rep(x) >= x.  Both ends of every offered link have one colour.  On a flat map out[y][x] == out[y][x + s] for every x
 * with x + s < w.  The NumPy model is tests/autostereogram_cases.py.
 * DS_EINVAL, before any launch: a null ctx, depth or out, a null tile with mode 2; n, h or w <= 0; period outside 16..512, m outside
 * 1..128, mode outside 0..2, with mode 2 ph or pw outside 1..4096; depth not 2-byte aligned.  Then DS_EUNSUPPORTED: h or w > 16384, or
 * n > 65535.  Then DS_EINVAL: out overlapping depth or (mode 2) tile.  Asynchronous on `stream`: one launch, one workgroup per image
 * row, no workspace and no global atomics, so the call is safe under graph capture.  No kernel-timer kind.
 * ds_autostereogram_rounds_u8 is the same call, and writes into rounds [n,h] uint16 (not NULL, 2-byte aligned, overlapping nothing) how
 * many rounds of label propagation each row's workgroup made, the last, idle one included (tools/autostereogram_ab.py reports them).
 */
int ds_autostereogram_u8(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int period, int m, int mode, uint32_t seed,
                         const uint8_t *tile, int ph, int pw, int invert, uint8_t *out, void *stream);
int ds_autostereogram_rounds_u8(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int period, int m, int mode, uint32_t seed,
                                const uint8_t *tile, int ph, int pw, int invert, uint8_t *out, uint16_t *rounds, void *stream);

/*
 * ds_stereo_match_u8 -- depth from stereo pairs: the disparity map of the LEFT view of each of n row-aligned pairs by four-path
 * semi-global matching (Hirschmueller 2008) on a 5x5 census, and from it a depth map, white = near.  The reference has no counterpart;
 * this comment is the definition, and the only normative text.  Everything is an integer, and every step is min, +, a compare or an
 * integer division, so the result does not depend on the order in which anything runs.  floor() below is the floor of the exact quotient.
 * Inputs.  left, right [n,h,w,c] uint8, c in {1, 3, 4}, at any byte address.  The left image is the reference view.  Disparity delta means:
 *   left column x shows what the right image shows at column x - delta; a larger delta is nearer.  D in {32, 64, 128}: the number of
 *   disparities.  d0 in -128..127: the smallest one (negative: content in front of the screen plane); the candidates are delta = d0 + d,
 *   d = 0..D-1.  P1 in 1..64, P2 in P1..255: the penalties of a disparity step of one and of more than one.  u in 0..50: the uniqueness
 *   margin in percent.  lr in -1..3: the left-right tolerance, -1 = no check.
 * 1. Luma.  Y = (77 R + 150 G + 29 B + 128) >> 8; with c = 1 the byte itself; with c = 4 the fourth channel is ignored.
 * 2. Census, per image: 24 bits from the 5x5 window around a pixel, a bit set where the neighbour's Y is SMALLER than the centre's;
 *    a neighbour outside the image is the nearest edge pixel.  Only Hamming distances are used: the bit order is the implementation's.
 * 3. Cost.  C(y,x,d) = popcount(cl[y,x] ^ cr[y, x - (d0 + d)]) when that column lies in 0..w-1, else 24.
 * 4. Paths, four directions r: left->right, right->left, top->bottom, bottom->top.  At the first pixel of a path L_r(p,.) = C(p,.);
 *    afterwards, with q = p - r and m_r(q) = min_d L_r(q,d),
 *      L_r(p,d) = C(p,d) + min(L_r(q,d), L_r(q,d-1) + P1, L_r(q,d+1) + P1, m_r(q) + P2) - m_r(q),
 *    a d +- 1 outside 0..D-1 being absent.  S = sum_r L_r.  L_r <= 24 + 255 and S <= 1116: uint16 holds everything.
 * 5. Winner.  d* = the SMALLEST d that minimises S(p,.), S1 its value.  The pixel fails uniqueness when some e with |e - d*| > 1 has
 *    S(p,e) (100 - u) < S1 100.
 * 6. Left-right check (lr >= 0).  dR(y,xr) = the smallest d minimising S(y, xr + d0 + d, d) over the d whose column xr + d0 + d lies in
 *    the row; undefined when there is none.  With xr = x - (d0 + d*) the pixel fails when xr is outside the row, or dR(y,xr) is
 *    undefined, or |dR(y,xr) - d*| > lr.
 * 7. Sub-pixel.  For 0 < d* < D-1: a, b, c = S(d*-1), S(d*), S(d*+1), den = a + c - 2 b, frac = floor((16 (a - c) + den) / (2 den))
 *    when den > 0, else 0.  (d* is the smallest minimiser, so a > b and den > 0 always: frac = floor(8 (a - c) / den + 1/2) with
 *    -1 < (a - c) / den <= 1, so frac is in -8..8; c = b gives 8, a = b + 1 under a large c gives -8.)  At d* = 0 and
 *    d* = D-1 frac = 0.  disp16 = 16 (d0 + d*) + frac, in 1/16 pixel.  valid = 1 for a pixel that passed 5 and 6, else 0.
 * 8. Fill.  An invalid pixel takes the SMALLER of the nearest valid disp16 to its left and to its right in its own row (an occlusion
 *    belongs to the background); with one side only, that side's; in a row without a valid pixel 16 d0.
 * 9. Median.  disparity = the 3x3 median of the filled map, nearest-edge borders.
 * 10. Depth.  Per image lo, hi = min, max of disparity; depth = floor(((v - lo) 131070 + (hi - lo)) / (2 (hi - lo))), and all zeros when
 *    hi = lo.
 * Outputs.  disparity [n,h,w] int16 (step 9).  valid [n,h,w] uint8, the mask of step 7, before the fill; may be NULL, at any byte
 * address.  depth [n,h,w] uint16; may be NULL.  An image's result does not depend on its batch, on `group` or on the launch.
 * Workspace.  ds_stereo_match_workspace_bytes(h, w, D) is one image's share -- the S volume (2 h w D bytes), two census planes, the filled
 *   map, the lo / hi words, each rounded to 256 bytes -- and 0 for a size or a D the entry point refuses.  `workspace` holds `group`
 *   shares (group in 1..n), 256-byte aligned, any content: images are processed `group` at a time, the workspace reused in stream order.
 * DS_EINVAL, before any launch: a null pointer other than valid / depth; n, h or w <= 0; c, D, d0, P1, P2, u or lr out of range; group
 * outside 1..n; workspace not 256-byte aligned, disparity or depth not 2-byte aligned.  Then DS_EUNSUPPORTED: h or w > 16384, n > 65535,
 * or one image's workspace above 2 GiB (element offsets then stay inside 31 bits; byte offsets are size_t all the same).  Then DS_EINVAL:
 * an output or the workspace overlapping an input or each other.  Asynchronous on `stream`, no allocation; per group five launches, six
 * with depth (census, horizontal paths, vertical paths, winner + fill, median + min / max, depth).  No kernel-timer kind.
 * The NumPy model is tests/stereo_match_cases.py.
 * ds_stereo_match_stages_u8 is the same call restricted to the launches named by `stages`, a sum of 1 = census, 2 = horizontal paths,
 * 4 = vertical paths, 8 = winner + fill, 16 = median, 32 = depth (1..63; 63 is ds_stereo_match_u8): tools/stereo_match_ab.py times each
 * launch with it.  A partial run leaves partial results.
 */
size_t ds_stereo_match_workspace_bytes(int h, int w, int D);
int ds_stereo_match_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1, int P2, int u,
                       int lr, void *workspace, int group, int16_t *disparity, uint8_t *valid, uint16_t *depth, void *stream);
int ds_stereo_match_stages_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1, int P2,
                              int u, int lr, void *workspace, int group, int16_t *disparity, uint8_t *valid, uint16_t *depth, int stages,
                              void *stream);

/*
 * ds_stereo_match_ex_u8 -- ds_stereo_match_u8 with eight paths and a speckle filter.  The definition is that of ds_stereo_match_u8,
 * steps 1-10 of the comment above, with three more parameters and two extended steps; this comment and that one are the normative text.
 * paths in {4, 8}.  With 8, step 4 has four more directions r = (dy, dx): (+1,+1), (-1,-1), (+1,-1), (-1,+1).  The recurrence, P1, P2,
 *   the absent d +- 1 and "at the first pixel of a path L_r = C" are unchanged; the first pixel of a path is the one whose predecessor
 *   p - r lies outside the image, so in an image of one row or one column every diagonal path has length 1 and L_r = C there.  S is the
 *   sum over all eight directions: L_r <= 24 + 255 = 279, S <= 8 * 279 = 2232, uint16 holds it, and S (100 - u) <= 223200 fits an int32.
 *   Steps 5-7 read the new S unchanged: den = a + c - 2 b <= 2 * 2232, and frac stays in -8..8 by the argument of step 7, which uses
 *   a > b, c >= b and nothing else.
 * speckle_size in 0..65535, 0 = off; speckle_range in 0..16 pixels.  With speckle_size > 0 a step 7b runs between steps 7 and 8: the
 *   speckle filter below on (disp16, valid) of step 7 with size = speckle_size and t = 16 speckle_range.  The `valid` output and the
 *   fill of step 8 use the mask AFTER 7b (with speckle_size = 0: the mask of step 7, as before).
 * With paths = 4 and speckle_size = 0 every output equals ds_stereo_match_u8's bit for bit.
 * ds_stereo_match_ex_workspace_bytes(h, w, D, paths, speckle_size) is one image's share: ds_stereo_match_workspace_bytes(h, w, D) and,
 *   with speckle_size > 0, behind it disp16 (2 h w bytes), the masks of steps 7 and 7b (h w each), the links and the counters of the
 *   filter (4 h w each), each rounded to 256 bytes; 0 for whatever the entry point refuses.  `workspace` holds `group` shares, 256-byte
 *   aligned, any content.
 * Refusals, before any launch, as ds_stereo_match_u8's and in its order, the entry point naming itself in ds_last_error(): DS_EINVAL for
 *   a null pointer other than valid / depth, n, h or w <= 0, c, D, d0, P1, P2, u, lr, paths, speckle_size or speckle_range out of range,
 *   group outside 1..n, misalignment; then DS_EUNSUPPORTED for h or w > 16384, n > 65535 or a share above 2 GiB; then DS_EINVAL for an
 *   output or the workspace overlapping an input or each other.  Asynchronous on `stream`, no allocation.  Launches per group: those of
 *   ds_stereo_match_u8; with paths = 8 two more behind the vertical paths, one per diagonal orientation (each S element lies on exactly
 *   one line of an orientation, so a launch never shares an element between lines; stream order hands S from launch to launch); with
 *   speckle_size > 0 the winner launch stops before its fill and leaves disp16 and valid in the workspace, the filter's four launches
 *   follow, then one row-fill launch: 5 (6 with depth) + 2 + 5.  No kernel-timer kind.
 * ds_stereo_match_ex_stages_u8 is the same call restricted to the launches named by `stages` (1..255): the bits of
 *   ds_stereo_match_stages_u8, 64 = the two diagonal launches, 128 = the speckle filter and the fill behind it; a bit whose launches the
 *   parameters switch off does nothing.  tools/stereo_match_ex_ab.py times with it.  A partial run leaves partial results.
 * The NumPy model is tests/stereo_match_ex_cases.py.
 *
 * ds_speckle_filter_i16 -- step 7b as an entry point of its own: rejects small connected regions of similar disparity.
 * disp [n,h,w] int16, valid [n,h,w] uint8 (any byte address), size in 1..65535, t in 0..65535.  Per image: the nodes are the pixels with
 *   valid != 0.  Two 4-neighbours are linked exactly when both are nodes and |disp(p) - disp(q)| <= t, the difference taken in int32
 *   (-32768 beside 32767 differ by 65535).  No link crosses an image border or joins two images.  A component is a connected component
 *   of that graph; links are not transitive in value: a ramp in steps of t is one component.
 * size_out [n,h,w] uint32 (may be NULL; 4-byte aligned): the pixel count of the pixel's component, 0 for a non-node.
 * valid_out [n,h,w] uint8 (any byte address; may not alias valid): 1 for a node whose component has MORE than `size` pixels, else 0.
 *   Membership and counts are properties of the graph: no schedule can change a bit.
 * ds_speckle_filter_workspace_bytes(h, w) is one image's share: links and counters, 4 h w bytes each, each rounded to 256; 0 for a
 *   refused shape.  `workspace` holds `group` shares (group in 1..n), 256-byte aligned, any content: the first launch writes every link
 *   and counter before any launch reads one.
 * DS_EINVAL, before any launch: a null pointer other than size_out; n, h or w <= 0; size or t out of range; group outside 1..n; workspace
 *   not 256-byte aligned, disp not 2-byte or size_out not 4-byte aligned.  Then DS_EUNSUPPORTED: h or w > 16384, n > 65535, or a share
 *   above 2 GiB (h w <= 2^28: pixel indices are int32).  Then DS_EINVAL: valid_out, size_out or the workspace overlapping an input or each
 *   other.  Asynchronous on `stream`, no allocation; four launches per group (links, merge, roots + counts, outputs); no kernel waits
 *   for another workgroup.  The model is the flood fill of tests/stereo_match_ex_cases.py.
 */
size_t ds_stereo_match_ex_workspace_bytes(int h, int w, int D, int paths, int speckle_size);
int ds_stereo_match_ex_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1, int P2,
                          int u, int lr, int paths, int speckle_size, int speckle_range, void *workspace, int group, int16_t *disparity,
                          uint8_t *valid, uint16_t *depth, void *stream);
int ds_stereo_match_ex_stages_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1,
                                 int P2, int u, int lr, int paths, int speckle_size, int speckle_range, void *workspace, int group,
                                 int16_t *disparity, uint8_t *valid, uint16_t *depth, int stages, void *stream);
size_t ds_speckle_filter_workspace_bytes(int h, int w);
int ds_speckle_filter_i16(ds_ctx *ctx, const int16_t *disp, const uint8_t *valid, int n, int h, int w, int size, int t, void *workspace,
                          int group, uint8_t *valid_out, uint32_t *size_out, void *stream);

/*
 * ds_mesh_render_u8 -- mesh videos: F views of one coloured triangle mesh through F pinhole cameras, by a triangle rasteriser with a
 * visibility buffer.  The reference renders its "generate video from mesh" clips through OpenGL; this comment is the definition, and the
 * only normative text.  It renders the SIMPLE mesh (occluded or stretched) or any other triangle mesh; the inpainted mesh is not built
 * here.  After the vertex stage everything is an integer, and the depth test is a maximum over 64-bit keys, so the result does not
 * depend on the order in which anything runs.  `//` is the floor of the exact quotient (all its operands are >= 0 here).
 * Inputs, all four arrays on the device.  verts [N,3] float64.  colors [N,3] uint8, at any byte address.  faces [M,3] int32.
 *   cameras [F,6] float64 (tx, ty, tz, f, cx, cy): a translation in the mesh's units, the focal length and the principal point in
 *   output pixels.  Output size H, W.  Supersampling s in 1..4: the raster has Hs = s H rows of Ws = s W samples.  near: finite, > 0.
 *   background: three integers 0..255, by value.  M = 0 is legal (faces may then be NULL): every pixel is `background`.
 *   small_cap in 0..64 and group in 1..F change the launches, never a bit (below).
 * Vertex (x, y, z) under camera k.  Every float64 operation is rounded on its own (no contraction):
 *   xc = x - tx;  yc = y - ty;  zc = z - tz.  The vertex is dead unless zc >= near (a NaN fails this).
 *   sx = cx - (f xc) / zc;  sy = cy - (f yc) / zc: the simple mesh's x = -(u - cx) d / f lands on column u, and an output pixel IS the
 *   sample at integer coordinates.  Then sx = sx s + (s - 1) 0.5, and sy likewise: pixel u owns the samples s u .. s u + s - 1.
 *   The vertex is dead unless sx and sy are finite and |sx|, |sy| <= 16384.
 *   X = rint(16 sx), Y = rint(16 sy): int32 with 4 fraction bits, half to even.
 *   iz = max(1, floor((near / zc) 2^31)): uint32, 1..2^31; inverse depth, which is linear in screen space.
 *   A camera row with a NaN or an infinity in any of its six numbers kills every vertex of its frame (tested explicitly: tz = -inf
 *   would otherwise leave finite coordinates).  The host wrapper refuses such a row beforehand.
 * Face t with vertices a, b, c is skipped when an index lies outside 0..N-1 (a bad device array cannot address outside the arguments),
 *   when a vertex is dead (there is no near-plane clipping), when A = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) is 0, or when
 *   max X - min X or max Y - min Y of its vertices exceeds 2048 * 16.
 *   Coverage of sample (px, py), 0 <= px < Ws, 0 <= py < Hs, with PX = 16 px, PY = 16 py:
 *     w0 = (Xb - PX)(Yc - PY) - (Yb - PY)(Xc - PX);  w1 = (Xc - PX)(Ya - PY) - (Yc - PY)(Xa - PX);
 *     with A < 0 (both orientations are drawn): w0 = -w0, w1 = -w1, A = -A;  then w2 = A - w0 - w1.
 *   The sample is covered when w0, w1, w2 >= 0: edges are inclusive on all sides, overlaps are settled by the key and not by a fill
 *   rule, so the last row and column of a grid mesh are covered.
 *   izp = (w0 iz_a + w1 iz_b + w2 iz_c) // A, in 1..2^31.  Inside the bounding box of a kept face every coordinate difference is
 *   <= 2^15, so |w| <= 2^31 and A <= 2^30; the weights of a covered sample sum to A: the numerator is <= 2^61.  int64 holds everything.
 * Visibility.  key = (izp << 32) | (0xFFFFFFFF - t).  Keys start at 0 (nothing landed; a hit has izp >= 1); every covered sample takes
 *   the maximum of the keys offered to it: the nearest face wins, among equal izp the LOWER face index.
 * Resolve, per output pixel (u, v) of frame k, over its s^2 samples (s u + i, s v + j).  key = 0: the sample is `background`.  Else
 *   t = 0xFFFFFFFF - (key & 0xFFFFFFFF), w0, w1, w2, A as above, and per channel (w0 c_a + w1 c_b + w2 c_c + A // 2) // A: affine,
 *   screen-space Gouraud shading -- NOT perspective-correct, which shows on stretched faces.  The pixel is (sum + s^2 // 2) // s^2 per
 *   channel.
 * Outputs.  out [F,H,W,3] uint8, at any byte address.  out_hits [F,H,W] uint8: how many of the pixel's samples something landed on,
 *   0..16; the pointer may be NULL.
 * Identities.  Let the mesh be the simple mesh of an h x w image with every quad kept (keep_edges), the camera (0, 0, 0, f, cx, cy)
 *   with the mesh's own intrinsics, and H = h, W = w.  Every vertex lands on X = 16 s u + 8 (s - 1), Y = 16 s v + 8 (s - 1).  With
 *   s = 1 the output is the image and out_hits = 1 everywhere.  With s > 1 a pixel's samples lie around its vertex, so on the first
 *   and last row and column some fall outside the mesh, and Gouraud shading mixes the neighbours in: out_hits = n(u, w) n(v, h) with
 *   n = s inside and (s + 1) // 2 (s odd) or s / 2 (s even) on a first or last index; every channel lies between the minimum and the
 *   maximum of `background` and the image's 3 x 3 neighbourhood; an image of one colour on a background of that colour comes back.
 *   Frames are independent of each other and of `group`.  Renumbering the vertices, with the faces remapped, changes nothing.
 *   The NumPy model is tests/mesh_render_cases.py.
 * Workspace.  ds_mesh_render_workspace_bytes(N, M, H, W, s) is one frame's share: its keys (8 Hs Ws bytes), a 256-byte counter block,
 *   its vertex records (16 N bytes: X, Y, iz, live) and its list of large faces (4 M bytes), each rounded to 256 bytes; 0 for sizes the
 *   entry point refuses.  `workspace` holds `group` shares, 256-byte aligned, any content: frames are rendered `group` at a time, the
 *   workspace reused in stream order; the memset and the vertex launch write everything a later launch reads.
 * DS_EINVAL, before any launch: a null pointer other than out_hits (and faces with M = 0); N, F, H or W <= 0, M < 0; s outside 1..4; near not
 *   finite or <= 0; a background component outside 0..255; small_cap outside 0..64; group outside 1..F; workspace not 256-byte aligned, verts or cameras not 8-byte, faces not 4-byte aligned.
 *   Then DS_EUNSUPPORTED: Hs or Ws > 16384, N or M >= 2^31, F > 65535, or a share above 2 GiB.  Then DS_EINVAL: an output or the
 *   workspace overlapping an input or each other.  Asynchronous on `stream`, no allocation, safe under graph capture.  Per group one
 *   memset (keys and counters) and four launches: vertices; faces (a thread per face walks a bounding box of at most small_cap samples
 *   itself and appends the others to the frame's list); the listed faces (a fixed grid, one wave per face, the count read from device
 *   memory; small_cap = 0 sends every face with a non-empty box here); resolve.  Every loop is bounded (small_cap samples per thread,
 *   2048^2 per wave, s^2 per pixel); no kernel waits for another workgroup.  No kernel-timer kind.
 * ds_mesh_render_stages_u8 is the same call restricted to the launches named by `stages`, a sum of 1 = memset, 2 = vertices, 4 = faces,
 *   8 = listed faces, 16 = resolve (1..31; 31 is ds_mesh_render_u8): tools/mesh_render_ab.py times each with it.  A partial run leaves
 *   partial results.
 */
size_t ds_mesh_render_workspace_bytes(int64_t N, int64_t M, int H, int W, int s);
int ds_mesh_render_u8(ds_ctx *ctx, const double *verts, const uint8_t *colors, const int32_t *faces, int64_t N, int64_t M,
                      const double *cameras, int F, int H, int W, int s, double near, int bg_r, int bg_g, int bg_b, int small_cap,
                      void *workspace, int group, uint8_t *out, uint8_t *out_hits, void *stream);
int ds_mesh_render_stages_u8(ds_ctx *ctx, const double *verts, const uint8_t *colors, const int32_t *faces, int64_t N, int64_t M,
                             const double *cameras, int F, int H, int W, int s, double near, int bg_r, int bg_g, int bg_b, int small_cap,
                             void *workspace, int group, uint8_t *out, uint8_t *out_hits, int stages, void *stream);

/*
 * ds_frame_luma_hist -- per-frame luma histograms of a uint8 clip: the input of video mode's scene-cut detector (the reference
 * leaves cut detection as a TODO, src/video_mode.py:114, and has no implementation; this comment is the definition).
 * frames [n,h,w,c] uint8, dense, ANY byte alignment -> hist [n,256] uint32: hist[f][v] = the number of pixels of frame f with Y == v.
 *   c == 1: Y = the sample.  c == 3 or 4: Y = (77 R + 150 G + 29 B + 128) >> 8 in integer arithmetic on channels 0, 1, 2 (the
 *   weights sum to 256: Y lies in 0..255, white gives 255); channel 3 is ignored.
 * The entry point OVERWRITES hist (it does not accumulate; the caller need not clear it).  Counts are integers: every summation
 * order gives the same bits, a frame's row does not depend on the batch, and np.bincount on the same Y is the model
 * (tests/video_cuts_cases.py).
 * DS_EINVAL: a null pointer; n, h or w <= 0; c outside {1, 3, 4}; hist not 4-byte aligned.  DS_EUNSUPPORTED: h * w >= 2^32, or
 * n > 65535.  Asynchronous on `stream` (a clear of hist and one kernel); no allocation, no workspace.
 */
int ds_frame_luma_hist(ds_ctx *ctx, const uint8_t *frames, int n, int h, int w, int c, uint32_t *hist, void *stream);

/*
 * ds_temporal_smooth5_f32 -- the 5-tap temporal filter of video mode's 'experimental' smoothening (src/video_mode.py:119-124) on a
 * run of frames whose taps are clamped to [lo, hi]: with lo and hi the first and last frame of a scene nothing is smoothed across
 * a cut; with lo = 0 and hi = m - 1 it is the reference's clip().
 * src [m, plane] float32 -> out [count, plane] float32; out must not overlap src.  For j < count, i = first + j,
 * W = float32 {0.10, 0.20, 0.40, 0.20, 0.10} and k_u = min(max(i + u - 2, lo), hi):
 *   out[j][p] = ((((+0.0f + W0 * src[k_0][p]) + W1 * src[k_1][p]) + W2 * src[k_2][p]) + W3 * src[k_3][p]) + W4 * src[k_4][p]
 * every product rounded to binary32, then every sum rounded to binary32: no fused multiply-add, subnormals kept.  That is the
 * reference's `f += mul * predictions[clip(...)]` on float32 frames, operation for operation: a NumPy loop with these roundings
 * gives the same bits (tests/video_cuts_cases.py).  Which NaN comes out of inf - inf is not specified.
 * A caller whose frames are sharded passes src = its halo plus its frames and first / lo / hi as indices into that.
 * DS_EINVAL: a null pointer; m, plane or count <= 0; 0 <= lo <= first, first + count - 1 <= hi or hi < m broken; src or out not
 * 4-byte aligned (any other alignment and any plane are legal); out overlapping src.  DS_EUNSUPPORTED: plane > 2^32.
 * Asynchronous on `stream`; one kernel, no workspace.
 */
int ds_temporal_smooth5_f32(ds_ctx *ctx, const float *src, int m, int64_t plane, int first, int count, int lo, int hi, float *out,
                            void *stream);

/*
 * ds_temporal_joint_bilateral_u16 -- video mode's temporal depth filter: the joint (cross) bilateral filter ALONG TIME of the uint16
 * depth frames of a clip guided by its uint8 frames.  The depth at a pixel is averaged over the neighbouring frames of the same
 * scene; the temporal kernel is a Gaussian, the range weight is taken from how much the PIXEL'S COLOUR changed between the two
 * frames, so a static region loses the frame-to-frame noise of the network while a pixel that something moved over keeps its own
 * depth (no ghosting).  The reference has no counterpart; this comment is the definition.
 * depth D [m,h,w] uint16, guide G [m,h,w,c] uint8 dense with c = guide_channels in {3, 4} -> out [count,h,w] uint16.  Only the first
 * three bytes of a guide pixel are read; for c == 4 the fourth byte is ignored.  The guide may have any byte alignment.
 *   wt: radius + 1 float64 temporal weights made on the host, wt[a] = exp(-a^2 / (2 sigma_time^2)), wt[0] == 1.0;
 *   wc: the 766 float64 colour weights of ds_joint_bilateral_u16, made by the same host code: wc[k] = exp(-k^2 / (2 sigma_color^2)).
 *       No exp runs on the device; sigma_color is in units of summed 8-bit channel difference, sigma_time in frames.
 *   For j < count, i = first + j and pixel p: num = den = 0.0; for u = -radius .. radius in increasing order, s = i + u:
 *       a tap with s < lo or s > hi is OMITTED (not clamped: a weighted mean needs no replicated frame);
 *       k = |R_s(p) - R_i(p)| + |G_s(p) - G_i(p)| + |B_s(p) - B_i(p)|, in 0..765;
 *       wgt = wt[|u|] * wc[k];  num = num + wgt * (double)D_s(p) (the product rounded, then the sum: no fused multiply-add);
 *       den = den + wgt.
 *   Then F = num / den, one IEEE division, and out[j](p) = (uint16) rint(F), round-half-to-even.
 *   The centre tap has weight exactly 1, so den >= 1.  F is a convex combination of uint16 values, so rint(F) lies in 0..65535: no
 *   clamp is part of the definition.
 * One accumulation chain per pixel and output frame: a pixel's bits depend only on the frames max(lo, i - radius) ..
 * min(hi, i + radius) at that pixel -- not on first, not on count, not on how the launch tiles space or time, not on frames outside
 * [lo, hi] (they are never read); a float64 NumPy loop over the taps gives the same bits (tests/video_stabilize_cases.py).  With lo
 * and hi the first and last frame of a scene nothing is averaged across a cut.  A caller whose frames are sharded passes its halo
 * plus its frames and first / lo / hi as indices into that, as for ds_temporal_smooth5_f32.
 * DS_EINVAL: a null pointer; m, h, w or count <= 0; guide_channels not in {3, 4}; radius outside 1..4; 0 <= lo <= first,
 * first + count - 1 <= hi or hi < m broken; wt or wc not 8-byte aligned; depth or out not 2-byte aligned; out overlapping depth
 * (neighbouring frames are read: nothing is in place).  DS_EUNSUPPORTED: h * w >= 2^32.  Asynchronous on `stream`; one kernel, no
 * workspace, no allocation.
 */
int ds_temporal_joint_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, const uint8_t *guide, int guide_channels, int m, int h, int w,
                                    int radius, const double *wt, const double *wc, int first, int count, int lo, int hi, uint16_t *out,
                                    void *stream);

/*
 * ds_normalmap_selfcheck -- device self-test of the fused normal-map kernels' arithmetic (tests): their square root and reciprocal
 * are the generic float64 expansions WITHOUT range scaling and special-case fix-ups (dead for n^2 = zx^2 + zy^2 + 1 in [1, 2^22],
 * src/normalmap_generation.py:34-39); the kernel compares them with sqrt() and 1.0 / n on n^2 = K / 2^18, K = k0 + stride * i,
 * i < count, K in [2^18, 2^40), and returns the number of operands on which they differ (must be 0).  Synchronises the stream.
 */
int ds_normalmap_selfcheck(ds_ctx *ctx, unsigned long long k0, unsigned long long stride, unsigned long long count,
                           unsigned long long *mismatches, void *stream);

/*
 * ds_depth_to_u16 -- replaces the depth post-processing of core_generation_funnel
 * (src/core.py:189-206, no-clip branch) followed by convert_to_i16 (src/core.py:44-50) for a batch
 * of float32 predictions: per image min/max, optional negate (models whose raw output is
 * near-is-dark), normalise to [0,1] in float32, then clip(x*65536+1e-4, 0, 65535.9) -> uint16.
 * A flat prediction (max-min <= float64 eps) gives zeros (:204-206).
 *   pred n*h*w float32; out n*h*w uint16; norm_out (optional, may be NULL) n*h*w float32 = the
 *   normalised map before quantisation.
 */
int ds_depth_to_u16(ds_ctx *ctx, const float *pred, int n, int h, int w, int invert,
                    uint16_t *out, float *norm_out, void *stream);

/*
 * ds_colorize_u16 -- the heat map output of core_generation_funnel (src/core.py:271-274), i.e.
 * dzoedepth/utils/misc.py:97-150 colorize(depth, cmap=...) with its default arguments: per image
 *     value = (depth - vmin) / (vmax - vmin)   in float64 (zeros when vmin == vmax, :124-127)
 *     index = trunc(value * lut_n), below 0 -> entry 0, >= lut_n -> the last entry (matplotlib Colormap.__call__)
 *     out   = lut_rgba[index]
 *   depth      n*h*w uint16;  vmin_vmax  n*2 doubles (device): the reference's np.percentile(depth, 2 / 85);
 *   lut_rgba   lut_n*4 bytes (device), the colormap's bytes=True table;  out  n*h*w*4 bytes (RGBA).
 */
int ds_colorize_u16(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, const double *vmin_vmax,
                    const uint8_t *lut_rgba, int lut_n, uint8_t *out, void *stream);

/* convert_to_i16 alone (src/core.py:44-50): float32 or float64 input already in [0,1]. */
int ds_convert_to_i16(ds_ctx *ctx, const void *arr, int is_f64, int64_t count, uint16_t *out, void *stream);

/* pixel types of the custom-depth entry points: Pillow modes L (and a band of RGB / RGBX), I;16, I, F */
#define DS_PIX_U8  0
#define DS_PIX_U16 1
#define DS_PIX_I32 2
#define DS_PIX_F32 3

/*
 * ds_resize_lanczos -- Image.resize(size, Image.Resampling.LANCZOS) of the custom-depth ingest (src/core.py:147-153) as Pillow's
 * Resample.c computes it: a horizontal pass when the width changes, then a vertical pass when the height changes, each rounded
 * into the pixel type (8-bit: 22-bit fixed point from 2^21, clipped; 16-bit: float64 sum, round half away, below 0 -> 0, above
 * 65535 -> 0xFF00 | low byte; int32: float64 sum, round half away; float32: float64 sum, one cast).  Taps in ascending order.
 *   src        n images of in_h * in_w pixels of type `pix`; strides in ELEMENTS (a pixel stride of 3 or 4 reads band 0 of
 *              interleaved RGB / RGBX in place)
 *   dst        n * out_h * out_w pixels of the same type, dense
 *   h_bounds   out_w * {first tap, tap count} int32;  h_coeffs  [h_taps][out_w] weights (TAP-MAJOR): float64, for DS_PIX_U8 the
 *              int32 fixed-point weights.  v_* likewise for out_h.  Built on the host (the libm sin Pillow calls); the arrays of a
 *              pass that does not run may be NULL.  A window that leaves the source or the table contributes nothing.
 *   tmp        n * in_h * out_w pixels, needed when both passes run (the rounded intermediate)
 * Equal sizes -> DS_EINVAL (nothing to resize); more than 1024 taps per output pixel -> DS_EUNSUPPORTED.  Asynchronous.
 */
int ds_resize_lanczos(ds_ctx *ctx, const void *src, int pix, int n, int in_h, int in_w, int64_t src_px_stride, int64_t src_row_stride,
                      int64_t src_img_stride, void *dst, int out_h, int out_w, const int32_t *h_bounds, const void *h_coeffs, int h_taps,
                      const int32_t *v_bounds, const void *v_coeffs, int v_taps, void *tmp, void *stream);

/*
 * ds_custom_depth_to_f64 -- the rest of the custom-depth ingest (src/core.py:155-174): np.asarray(dp, dtype="float") and the divide.
 *   DS_CD_WIDEN        out = (double)pixel                                   (an ndarray depth map, :172)
 *   DS_CD_SINGLE_BAND  out = pixel / 2^bits, bits = 8 if max < 256, 16 if max < 65536, else 32, max = the image's maximum
 *                      as np.max takes it (a NaN wins, and then fails both tests)   (:156-165)
 *   DS_CD_MULTI_BAND   out = pixel / 256 (the caller's pixel stride selects channel 0)   (:169-170)
 *   src as above; out n*h*w doubles; workspace (SINGLE_BAND only) n * (2 + DS_CD_WORKSPACE_BLOCKS) doubles, of which the first
 *   n * 2 hold {maximum, divisor} per image afterwards.  Asynchronous.
 */
#define DS_CD_WIDEN       0
#define DS_CD_SINGLE_BAND 1
#define DS_CD_MULTI_BAND  2
#define DS_CD_WORKSPACE_BLOCKS 256
int ds_custom_depth_to_f64(ds_ctx *ctx, const void *src, int pix, int n, int h, int w, int64_t src_px_stride, int64_t src_row_stride,
                           int64_t src_img_stride, int rule, double *out, double *workspace, void *stream);

/* element types of the tensor-core entry points */
#define DS_DTYPE_F16  1
#define DS_DTYPE_BF16 2
#define DS_DTYPE_F32  3       /* ds_preprocess_bicubic and ds_dwconv_nhwc only */

/*
 * ds_attention_fwd -- fused attention forward of one transformer block; replaces the q@k^T -> (+bias) -> softmax -> @v
 * sequence of ddepth_anything_v2/depth_anything_v2/dinov2_layers/attention.py:49-62 (MemEffAttention falls back to it,
 * :65-82) and of dmidas/backbones/beit.py:65-91 (attention_forward with relative position bias); head_dim = 64.
 *   qk      [B, Np, 2, H, 64]  Q (index 0) and K (index 1), token major, as the projection GEMM writes them
 *   vt      [B, H*64, Np]      V transposed (key index contiguous)
 *   bias_packed  NULL, or the operand made by ds_attention_bias_pack for this H and Np ROUNDED UP to a multiple of 64, same dtype
 *   out     [B, Np, H*64]
 * Np is the token stride of the operands, a multiple of 8 (the padded token count: a tight pad keeps the token GEMMs around
 * the kernel close to whole rounds of tiles -- 32 x 1032 rows are 129 row panels, 32 x 1088 are 136); the kernel walks whole
 * 64-key tiles, rows in [Np, roundup(Np, 64)) read as pad keys and are not stored.  Keys >= n_valid are masked; query rows >=
 * n_valid are computed like any other row (they stay finite) and are never read as keys.  scale multiplies q.k before the bias
 * is added.
 */
int ds_attention_fwd(ds_ctx *ctx, const void *qk, const void *vt, const void *bias_packed, void *out,
                     int B, int Np, int H, int n_valid, float scale, int dtype, void *stream);

/*
 * ds_attention_bias_pack -- prepares the additive logits bias of ds_attention_fwd (the relative position bias of
 * dmidas/backbones/beit.py:29-62,84-88: bias[h][query][key], one table per block, constant per input resolution).
 *   bias    [H, n, n] float32, natural units (what the reference adds to q.k*scale)
 *   packed  H*Np*Np elements of dtype, OPAQUE to the caller -- only ds_attention_fwd of the same library build reads it.
 *           Layout (informative): the bias enters the logits through the matrix pipe (S^T = K.Q^T + Bias^T.I), so the operand
 *           is stored as the MFMA A fragments of that product, in units of 1/scale (head_dim 64: the values times 8, exact in
 *           f16/bf16 up to the rounding of the value itself), zero padded to Np x Np:
 *           [H][Np/32 query blocks][Np/64 key tiles][4 chunks c = 2*kb + s][64 lanes][8 values t], where lane (hi = lane >> 5,
 *           l = lane & 31) of chunk c holds bias[query 32*qblock + 16*s + 8*hi + t][key 64*ktile + 32*kb + l] / scale.
 *           A wave reads its 32 x 64 bias tile with four coalesced 16-byte loads.  ds_attention_fwd therefore requires
 *           scale == 0.125 when a packed bias is given (DS_EUNSUPPORTED otherwise).
 * Run once per (block, resolution); the packed operand is reused by every forward.
 */
int ds_attention_bias_pack(ds_ctx *ctx, const float *bias, int H, int n, int Np, int dtype, void *packed, void *stream);

/*
 * ds_attention_reload_env -- ds_attention_fwd reads its A/B switches (DS_ATT_GEN = 2 / 4: kernel generation -- generation 4 runs
 * one wave per SIMD with two query sub-blocks skewed inside the wave, generation 2, the default, two to four waves per SIMD;
 * DS_ATT_TAIL = 0 / 1: query blocks with at most four live rows as GEMVs instead of tiles; DS_ATT_NQB, DS_ATT_LATE, DS_ATT_ORDER)
 * once per process; this call reads them again.  These five are all the switches there are: generations 1 and 3, the ablation
 * masks and the phase clock were removed from the library.  Every setting computes the same function (dmidas/backbones/beit.py:65-91);
 * generations 2 and 4 are bit-identical with DS_ATT_TAIL = 0.  Tests and A/B runs only.
 */
int ds_attention_reload_env(void);

/*
 * ds_preprocess_bicubic -- image -> network input in one pass: the chain `cv2.cvtColor(.., COLOR_BGR2RGB) / 255.0`
 * (src/depthmap_generation.py:381) -> Resize(.., INTER_CUBIC) -> NormalizeImage -> PrepareForNet (:457-476, dmidas/transforms.py;
 * ddepth_anything_v2/depth_anything_v2/dpt.py:196-221) that estimatemidas / estimatedepthanything_v2 run on the host.
 *   images  uint8 [batch, in_h, in_w, 3]
 *   out     [batch, 3, out_h, out_w] in channels_last memory (physically [batch, out_h, out_w, 3]) of `dtype` (f16 / bf16 / f32):
 *           out[b][c][y][x] = (bicubic(images[b][:, :, flip_channels ? 2 - c : c] / 255)(y, x) - mean[c]) / std[c]
 * Resampling: the cubic convolution kernel (A = -0.75) on half-pixel centres, replicated border, no antialiasing -- cv2's
 * INTER_CUBIC definition as torch's upsample_bicubic2d evaluates it (float32).  mean / std: 3 host floats each.
 */
int ds_preprocess_bicubic(ds_ctx *ctx, const void *images, void *out, int batch, int in_h, int in_w, int out_h, int out_w,
                          int flip_channels, const float *mean, const float *std, int dtype, void *stream);

/*
 * ds_residual_layernorm -- the element-wise part of a transformer block between two GEMMs, fused:
 *     x_out = x + gamma * branch           (LayerScale + residual; dinov2_layers/block.py:100-107, beit.py:101-106)
 *     h_out = LayerNorm(x_out) * ln_weight + ln_bias
 * x, branch, x_out, h_out: [rows, channels]; gamma, ln_weight, ln_bias: [channels]; all of `dtype` (f16/bf16).
 * branch == NULL: plain LayerNorm of x (x_out unused).  gamma == NULL: gamma = 1.  x_out may alias x.
 * channels in {384, 768, 1024, 1536}.
 */
int ds_residual_layernorm(ds_ctx *ctx, const void *x, const void *branch, const void *gamma, const void *ln_weight,
                          const void *ln_bias, void *x_out, void *h_out, int64_t rows, int channels, float eps, int dtype,
                          void *stream);

/*
 * ds_reassemble_readout -- epilogue of the DPT reassemble read-out (ProjectReadout, dmidas/backbones/utils.py:28-39;
 * forward_adapted_unflatten :83-124): the reference concatenates every token with the cls token, applies Linear(2C -> C)
 * and GELU.  The host splits the linear map (W.[tok ; cls] + b = W_tok.tok + (W_cls.cls + b)) into the token GEMM and one
 * vector per image; this entry point does the rest in one pass:
 *     out[b, n-1, :] = gelu_erf(proj[b, n, :] + clsvec[b, :]),  n = 1 .. tokens-1
 * proj [batch, tokens, channels] (the token GEMM's output, cls row included), clsvec [batch, channels],
 * out [batch, tokens-1, channels] = the NHWC operand of the 1x1 convolution that follows.  f16/bf16, channels % 8 == 0.
 */
int ds_reassemble_readout(ds_ctx *ctx, const void *proj, const void *clsvec, void *out, int batch, int tokens, int channels,
                          int dtype, void *stream);

/*
 * ds_bias_act_nhwc -- element-wise tail of a decoder convolution on a channels-last activation, one pass:
 *     out = [relu]( x + bias[channel] [+ res1] [+ res2] )
 * (ResidualConvUnit_custom, dmidas/blocks.py:352-377; ResidualConvUnit, ddepth_anything_v2/.../util/blocks.py:56-85; the
 * skip add of the fusion blocks).  x, res1, res2, out: `elements` values, channel fastest; res1 / res2 may be NULL; out may
 * alias x.  f16/bf16, channels % 8 == 0.  The sum is taken in float32 (x + bias, + res1, + res2, in that order) and rounded once.
 * NaN rule (this entry point and ds_dwconv_nhwc): an activation function never hides a NaN.  relu(NaN) = NaN and relu6(NaN) = NaN,
 * as torch's ReLU and ReLU6 (hardtanh) give; relu(-0.0) may be either zero.
 */
int ds_bias_act_nhwc(ds_ctx *ctx, const void *x, const void *bias, const void *res1, const void *res2, void *out,
                     int64_t elements, int channels, int relu, int dtype, void *stream);

/*
 * ds_group_norm_nchw -- GroupNorm [+ residual] [+ ReLU] of an NCHW activation in two launches (no counterpart function in the
 * reference: it is timm's GroupNormAct inside the ResNetV2-50 stem of dpt_hybrid_384, which the reference obtains through
 * timm.create_model in dmidas/backbones/vit.py:_make_pretrained_vitb_rn50_384; torch spends three launches + a ReLU + an add on it):
 *     out = [relu]( (x - mean_g) * rstd_g * gamma[c] + beta[c] [+ res] ),   mean / biased variance over the group's channels x pixels
 * x, res, out [n, channels, hw] contiguous (res may be NULL, out may alias x), gamma / beta [channels] in the activation's type;
 * f16 / bf16, hw % 8 == 0, n * groups <= 4096.  Moments in float32 per slice, combined in float64; the affine map in float32.
 */
int ds_group_norm_nchw(ds_ctx *ctx, const void *x, const void *gamma, const void *beta, const void *res, void *out, int n, int channels,
                       int hw, int groups, float eps, int relu, int dtype, void *stream);

/*
 * ds_linear -- y = act(x . W^T + bias), the token GEMMs of the ViT encoders with the epilogue fused (csrc/ds_linear.hip):
 * `fc1 -> nn.GELU` of the encoder MLP (timm Mlp as run by dmidas/backbones/beit.py:93-107; ddepth_anything_v2/
 * depth_anything_v2/dinov2_layers/mlp.py:33-39) is ONE kernel (act = 1: erf-GELU evaluated on the fp32 accumulator, see
 * ln_gelu for the error bound), act = 0 is a plain Linear (fc2, proj, qkv), act = 2 applies ReLU.
 * x [rows, in_features], W [out_features, in_features] (torch.nn.Linear layout), bias [out_features] or NULL,
 * y [rows, ldy] (ldy >= out_features, in elements).  f16/bf16, fp32 accumulation.  out_features % 256 == 0,
 * in_features % 128 == 0, rows >= 256 (the last 256-row panel is shifted up to end at the last row).  y must not alias x.
 * 256 x 256 tiles on the MFMA units, walked by one persistent workgroup per CU; when the last round of that walk would be
 * at most a quarter full, its tiles are rendered as 128 x 64 pieces by a second kernel on the same stream (the "ragged
 * round": 544 tiles on 256 CUs cost 2 rounds + the pieces instead of 3 rounds).  Long contractions (>= 2048) of a small ragged
 * round are shared by up to 8 workgroups per piece through a per-context workspace (8 MB, allocated at the first such launch:
 * one more reason why calls on one ctx go to one stream at a time); results stay bit-reproducible run to run.
 */
int ds_linear(ds_ctx *ctx, const void *x, const void *w, const void *bias, void *y, int64_t rows, int64_t out_features,
              int64_t in_features, int64_t ldy, int act, int dtype, void *stream);

/*
 * ds_linear_residual -- y = res + [gamma *] (x . W^T + bias): ds_linear with the residual add (and, when gamma is not NULL,
 * the LayerScale factor per output feature) in the epilogue: `x + gamma_1 * attn.proj(...)` of the encoder blocks
 * (dmidas/backbones/beit.py:99-103; dinov2_layers/block.py:88-96).  res and y [rows, out_features]; y must not alias res.
 * Shapes as ds_linear.  Used for the attention output projection and for fc2 of every encoder block: the LayerNorm pass that
 * follows then reads one operand instead of two.
 */
int ds_linear_residual(ds_ctx *ctx, const void *x, const void *w, const void *bias, const void *gamma, const void *res, void *y,
                       int64_t rows, int64_t out_features, int64_t in_features, int dtype, void *stream);

/*
 * ds_linear_vt -- V TRANSPOSED straight out of the projection GEMM: vt[b][c][n] = sum_k w_v[c][k] * h[b][n][k].
 * The reference computes qkv = Linear(h), reshapes and permutes (dmidas/backbones/beit.py:71-74; dinov2_layers/
 * attention.py:52-55); ds_attention_fwd wants V with the key index contiguous ([B, H*64, Np]), so the GEMM runs with W_v as
 * its row operand and all B * Np tokens as columns, and the epilogue scatters every group of 8 columns to its batch element.
 *   w_v [channels, in_features]   h [batch * tokens, in_features]   vt [batch, channels, tokens]
 * tokens % 64 == 0, (batch * tokens) % 256 == 0, channels >= 256, in_features % 128 == 0.  No bias: the V bias commutes with
 * the attention (softmax rows sum to one) and is folded into the output projection's bias by the host.
 */
int ds_linear_vt(ds_ctx *ctx, const void *w_v, const void *h, void *vt, int64_t channels, int64_t batch, int64_t tokens,
                 int64_t in_features, int dtype, void *stream);

/*
 * ds_linear_qkv -- the Q/K projection and V^T of one encoder block in ONE persistent GEMM launch:
 *     qk = h . w_qk^T + b_qk   exactly as ds_linear(h, w_qk, b_qk, qk, batch * tokens, qk_features, in_features, qk_features, 0, ..)
 *     vt                       exactly as ds_linear_vt(w_v, h, vt, v_channels, batch, tokens, in_features, ..)
 * Both GEMMs read the same LayerNorm output and neither depends on the other: the persistent kernel walks the tile list of the first
 * followed by the tile list of the second (operand bases, bias and store map switch per tile), so the two launches share their
 * rounds -- at the benchmark 1032 + 516 tiles are six exact rounds of 256 plus 12 V^T tiles for one ragged launch, instead of
 * 4 + 2 rounds and two ragged launches.  Every output element keeps its accumulation chain: both results are BIT-IDENTICAL to the
 * two calls above (any DS_LIN_* setting but the K split, which does not apply here: every round of this route is one chain).
 *   h [batch * tokens, in_features]   w_qk [qk_features, in_features]   b_qk [qk_features] or NULL   w_v [v_channels, in_features]
 *   qk [batch * tokens, qk_features]  vt [batch, v_channels, tokens]
 * The union of the two entry points' rules: tokens % 8 == 0, (batch * tokens) % 256 == 0, batch * tokens^2 < 2^32 (else
 * DS_EUNSUPPORTED), qk_features % 256 == 0, v_channels >= 256, in_features % 128 == 0 (128 .. 16384), every pointer 16-byte aligned,
 * dtype f16 or bf16; anything else DS_EINVAL.  Timers: the main launch runs under DS_KT_LINEAR, its ragged round under
 * DS_KT_LINEAR + DS_KT_RAGGED (nothing is recorded under DS_KT_LINEAR_VT).  No counterpart in the reference (it runs one qkv Linear
 * and permutes: dmidas/backbones/beit.py:71-74).
 */
int ds_linear_qkv(ds_ctx *ctx, const void *h, const void *w_qk, const void *b_qk, const void *w_v, void *qk, void *vt,
                  int64_t batch, int64_t tokens, int64_t qk_features, int64_t v_channels, int64_t in_features, int dtype, void *stream);

/*
 * ds_linear_shuffle -- ConvTranspose2d with kernel_size == stride as ONE GEMM with the pixel shuffle in the store address: the
 * 4x4-stride-4 and 2x2-stride-2 transposed convolutions of the reassemble stage (dmidas/backbones/utils.py:196-205 and :215-224,
 * `nn.ConvTranspose2d(features[i], features[i], kernel_size=4 / 2, stride=4 / 2, padding=0)`; ddepth_anything_v2/
 * depth_anything_v2/dpt.py:57-71).  With kernel == stride no two input pixels write the same output pixel:
 *     y[b, yy*s + ky, xx*s + kx, co] = bias[(ky*s + kx)*C + co] + sum_ci x[b, yy, xx, ci] * w[(ky*s + kx)*C + co, ci]
 *   x     [pixels, in_features]   the NHWC input, pixels = batch * h * width (image-major rows)
 *   w     [stride*stride*out_channels, in_features]: torch's [in, out, kH, kW] weight permuted to (kH, kW, out, in) by the host
 *   bias  [stride*stride*out_channels] (the module's bias repeated per tap) or NULL
 *   y     [batch, h*stride, width*stride, out_channels] NHWC
 * stride*stride*out_channels % 256 == 0, out_channels % 8 == 0, in_features % 128 == 0, pixels >= 256.  f16 / bf16, fp32 accumulation.
 */
int ds_linear_shuffle(ds_ctx *ctx, const void *x, const void *w, const void *bias, void *y, int64_t pixels, int64_t in_features,
                      int width, int stride, int out_channels, int dtype, void *stream);

/*
 * ds_linear_readout -- the read-out of the reassemble stage as one GEMM on the padded token sequence: ProjectReadout
 * (dmidas/backbones/utils.py:28-39: `features = cat(x[:, start_index:], readout.expand_as(...)); project(features)` with project =
 * Linear(2C -> C) + GELU) followed by the Transpose(1, 2) / Unflatten of :165-169.  The linear map of a concatenation splits,
 * W.[tok ; cls] + b = W_tok.tok + (W_cls.cls + b), and the second term is one vector per image:
 *     y[b*(tokens-1) + t - 1, :] = GELU( x[b*tokens_padded + t, :] . w_tok^T + cls_vec[b, :] ),   t = 1 .. tokens - 1
 *   x        [images * tokens_padded, in_features]   block output as the encoder leaves it (row 0 of an image = cls token, rows >=
 *            tokens = padding)
 *   w_tok    [out_features, in_features]   the token half of the projection weight;  cls_vec [images, out_features]
 *   y        [images * (tokens - 1) + 1, out_features]: token-major = NHWC of the [h, w] patch grid; the LAST row is a dummy that
 *            receives the cls / pad rows of every image (a constant store count per tile)
 * out_features % 256 == 0, in_features % 128 == 0, images * tokens_padded >= 256.  erf-GELU on the fp32 accumulator as ds_linear.
 */
int ds_linear_readout(ds_ctx *ctx, const void *x, const void *w_tok, const void *cls_vec, void *y, int64_t images,
                      int64_t tokens_padded, int64_t tokens, int64_t out_features, int64_t in_features, int dtype, void *stream);

/*
 * ds_conv3x3_nhwc_pair -- two independent convolutions y0 = conv3x3(x0, w0), y1 = conv3x3(x1, w1) (stride 1, zero padding 1, no bias,
 * no activation, no residual operands) with common in_channels and out_channels in ONE persistent launch: scratch.layer3_rn and
 * layer4_rn of the DPT decoders (dmidas/blocks.py:64-80, both 1024 -> 256 at the large backbones).  A launch below one round of
 * tiles costs one tile's K loop whatever its size; the walk covers the tile list of the first followed by the tile list of the
 * second (image geometry, operand bases and output base switch per tile), so two launches that fit one round together cost one.
 * Every output element keeps its accumulation chain: both results are BIT-IDENTICAL to two ds_conv3x3_nhwc calls.
 *   x_i [batch_i, height_i, width_i, in_channels] NHWC   w_i [out_channels, 3, 3, in_channels]
 *   y_i [batch_i * height_i * width_i + 1, out_channels]: the NHWC result followed by ONE dummy row, which receives the rows of a
 *       partial tile beyond the image (a constant store count per tile); an image may have fewer than 256 pixels
 * in_channels % 128 == 0 (<= 4096), out_channels % 256 == 0, every pointer 16-byte aligned, dtype f16 or bf16; else DS_EINVAL.
 * Timer: DS_KT_CONV3X3 (one launch).
 */
int ds_conv3x3_nhwc_pair(ds_ctx *ctx, const void *x0, const void *w0, void *y0, int batch0, int height0, int width0,
                         const void *x1, const void *w1, void *y1, int batch1, int height1, int width1,
                         int in_channels, int out_channels, int dtype, void *stream);

/*
 * ds_linear_rows4 --up to four small GEMMs with common shape in ONE launch:
 *     y_p[r, :] = x_p[r, :] . w_p^T + bias_p,   r < rows,  p < count <= 4
 * The cls halves of the four read-out projections above (cls_vec of ds_linear_readout): x_p is row 0 of every image of a padded tap,
 * read in place -- row r of problem p starts x_row_pitch ELEMENTS behind row r - 1 (tokens_padded * in_features there), so no
 * gather, no zero padding to a 256-row tile and no concatenation precede the launch.  The pointer sets travel by value in the kernel
 * arguments: no device-side table, no allocation, no synchronisation; the launch can be captured into a hipGraph.
 *   x_p [rows rows of in_features, x_row_pitch apart]   w_p [out_features, in_features]   bias_p [out_features] or NULL
 *   y_p [rows, out_features] contiguous
 * Every output element runs the accumulation chain of ds_linear: the result is BIT-IDENTICAL to ds_linear on the same rows gathered
 * and zero-padded to 256.  Rows beyond `rows` inside the last 32-row block are neither read outside x nor stored.
 * out_features % 64 == 0, in_features % 128 == 0 (128 .. 16384), rows 1 .. 65536, x_row_pitch >= in_features, % 8 == 0 and < 2^25,
 * every pointer 16-byte aligned, dtype f16 or bf16; anything else DS_EINVAL.  Timer: DS_KT_LINEAR.  No counterpart in the reference
 * (it concatenates the cls token to every token and runs one Linear(2C -> C): dmidas/backbones/utils.py:28-39).
 */
typedef struct ds_rows_problem {
    const void *x;
    int64_t x_row_pitch;
    const void *w;
    const void *bias;
    void *y;
} ds_rows_problem;
int ds_linear_rows4(ds_ctx *ctx, const ds_rows_problem *problems, int count, int64_t rows, int64_t out_features,
                    int64_t in_features, int dtype, void *stream);

/*
 * LayerNorm folded into the Linear behind it -- the norm1 -> qkv and norm2 -> fc1 pairs of every encoder block (timm's Block as run
 * by dmidas/backbones/beit.py:94-107: `x + gamma_1 * attn(norm1(x))`, `x + gamma_2 * mlp(norm2(x))`; ddepth_anything_v2/
 * depth_anything_v2/dinov2_layers/block.py:82-107).  With W' = W . diag(ln_weight), colsum[n] = sum_k W'[n][k] (of the rounded
 * weights) and b' = b + W . ln_bias, all prepared once per module by the host,
 *     LN(x) . W^T + b  =  rstd[m] * (x . W'^T)[m][n]  -  mean[m] * rstd[m] * colsum[n]  +  b'[n],
 * so the GEMM reads the residual stream itself and the LayerNorm pass (read x, write the normalised copy: 2 x 67 MB per call at
 * the benchmark's shape) becomes a statistics pass (read x, write 8 bytes per token).
 *   ds_row_stats     stats[m] = {rstd, -mean * rstd} (float32 pairs) of the rows of x [rows, channels]; channels in 384 / 768 /
 *                    1024 / 1536; mean and the centred sum of squares in float32 like ds_residual_layernorm
 *   ds_linear_ln     y = act(rstd (x . w_scaled^T) + (-mean rstd) colsum + bias); shapes and act (0 none, 1 erf-GELU) as ds_linear
 *   ds_linear_vt_ln  ds_linear_vt on the un-normalised x: vt[b][c][n] = rstd[b,n] (w_v_scaled . x[b,n]) + (-mean rstd)[b,n] colsum[c]
 *                    (the constant W_v . ln_bias commutes with the attention like the V bias: the host folds it into the projection bias)
 */
int ds_row_stats(ds_ctx *ctx, const void *x, void *stats, int64_t rows, int channels, float eps, int dtype, void *stream);
int ds_linear_ln(ds_ctx *ctx, const void *x, const void *w_scaled, const float *colsum, const void *bias, const void *stats, void *y,
                 int64_t rows, int64_t out_features, int64_t in_features, int64_t ldy, int act, int dtype, void *stream);
int ds_linear_vt_ln(ds_ctx *ctx, const void *w_v_scaled, const float *colsum, const void *x, const void *stats, void *vt,
                    int64_t channels, int64_t batch, int64_t tokens, int64_t in_features, int dtype, void *stream);

/*
 * ds_linear_reload_env -- the GEMM path (ds_linear, ds_linear_residual, ds_linear_vt, ds_conv3x3_nhwc) reads its A/B switches
 * (DS_LIN_EARLY, DS_LIN_GRID, DS_LIN_RAGGED, DS_LIN_RAGGED_DEN, DS_LIN_RAGGED_RING, DS_LIN_RAGGED_PIPE: none of these changes a
 * result; DS_LIN_RAGGED_KSPLIT, DS_LIN_RAGGED_KSPLIT_MIN, DS_LIN_RAGGED_KSPLIT_KEEP: the K split of the ragged round changes the
 * fp32 SUMMATION ORDER of the rows it touches -- results are equal within fp32 rounding, and bit-reproducible for a fixed
 * setting, but NOT bitwise equal between two settings) from
 * the environment ONCE per process, not per launch; this re-reads them (tests and A/B runs that flip a switch in-process).
 * No counterpart in the reference.
 */
int ds_linear_reload_env(void);

/*
 * ds_conv3x3_nhwc -- y = act(conv3x3(x, W) + bias [+ res1] [+ res2]), stride 1, zero padding 1, as the implicit GEMM of
 * csrc/ds_linear.hip (same 256 x 256 MFMA tiles; a K-tile is 64 channels of one tap, fetched by LDS-DMA from the shifted
 * pixel or from a zero line for the padding ring): the 3x3 convolutions of the DPT decoders with their element-wise tails
 * -- ResidualConvUnit_custom (dmidas/blocks.py:352-377: conv -> +bias -> ReLU, conv -> +bias -> +x [-> +skip]) and
 * scratch.layerN_rn (dmidas/blocks.py:64-80, no bias); ddepth_anything_v2/depth_anything_v2/util/blocks.py:56-85.
 * x [batch, height, width, in_channels] (channels_last), W [out_channels, 3, 3, in_channels] (the channels_last memory of
 * torch's [out, in, 3, 3] weight), bias [out_channels] or NULL, res1 / res2 / y [batch, height, width, out_channels].
 * act: 0 none, 2 ReLU (applied after the adds), 6 = 2 | 4: ReLU on the output AND on x itself -- conv(relu(x)), the first
 * convolution of a residual unit (dmidas/blocks.py:361-363: `out = self.activation(x); out = self.conv1(out)`), the maximum
 * taken on the MFMA fragments inside the K loop instead of in a pass over x (no residual operands, out_channels % 256 == 0;
 * a NaN in x becomes 0 there, as it does in the ReLU of the epilogue).  f16/bf16, fp32 accumulation.  in_channels % 128 == 0,
 * out_channels % 128 == 0 (a multiple of 256 runs 256 x 256 tiles; otherwise 256 x 128 tiles, without residual operands:
 * the head's 256 -> 128 convolution, dmidas/dpt_depth.py:150), batch * height * width >= 256.  y must not alias x, res1 or res2.
 */
int ds_conv3x3_nhwc(ds_ctx *ctx, const void *x, const void *w, const void *bias, const void *res1, const void *res2, void *y,
                    int batch, int height, int width, int in_channels, int out_channels, int act, int dtype, void *stream);

/*
 * ds_conv3x3_nhwc_circular -- ds_conv3x3_nhwc on the CIRCULARLY padded image:
 *     y = act(conv3x3(x circularly padded by 1 in H and W, W) + bias [+ res1] [+ res2])
 * i.e. nn.Conv2d(padding_mode='circular'), which the reference's TILING_MODE sets on every module whose type is exactly
 * nn.Conv2d (src/depthmap_generation.py:251-260) so that the depth map of a tileable texture tiles.  Same parameter list, shape
 * rules, epilogues (act 0, 2 and 6) and dtype rules as ds_conv3x3_nhwc.  The kernel is the same implicit GEMM with one more
 * compile-time mode: where the zero-padding form fetches a neighbour outside the image from the zero line, this one fetches the
 * pixel on the opposite side (row -1 = row height - 1, row height = row 0, likewise the columns; height == 1 or width == 1 wraps
 * a pixel onto itself, as F.pad(mode='circular') does).  Tap order, channel order and the fp32 chain per output element are the
 * zero-padding kernel's: every pixel at least one step from the border gets bit-identical output from the two entry points.
 */
int ds_conv3x3_nhwc_circular(ds_ctx *ctx, const void *x, const void *w, const void *bias, const void *res1, const void *res2, void *y,
                             int batch, int height, int width, int in_channels, int out_channels, int act, int dtype, void *stream);

/*
 * ds_upsample_bilinear_nhwc -- torch.nn.functional.interpolate(x, size, mode="bilinear", align_corners) for channels_last
 * activations: the x2 upsamples of the DPT decoders (dmidas/blocks.py:429-431; ddepth_anything_v2/.../util/blocks.py:141-145;
 * the heads' Interpolate, dmidas/dpt_depth.py:151, dpt.py:146).  in [batch, in_h, in_w, channels], out [batch, out_h, out_w,
 * channels]; channels % 8 == 0; f16/bf16; float32 interpolation arithmetic like torch's.
 */
int ds_upsample_bilinear_nhwc(ds_ctx *ctx, const void *in, void *out, int batch, int channels, int in_h, int in_w,
                              int out_h, int out_w, int align_corners, int dtype, void *stream);

/*
 * ds_dpt_head_front -- the front of the DPT depth heads in one kernel: refinenet1's final bilinear upsample (align_corners=True)
 * and the head's first convolution (dmidas/dpt_depth.py:150 output_conv[0] behind dmidas/blocks.py:429-431;
 * ddepth_anything_v2/depth_anything_v2/dpt.py:146 output_conv1 behind util/blocks.py:141-145):
 *     out = conv3x3(upsample_bilinear(x, (out_h, out_w), align_corners=True), w, zero padding 1) + bias
 *   x     [batch, in_h, in_w, in_channels] f16/bf16, channels_last
 *   w     [out_channels][tap = ky * 3 + kx][in_channels], same dtype: what ds_conv3x3_nhwc takes;  bias [out_channels], same dtype, or NULL
 *   out   [batch, out_h, out_w, out_channels], same dtype; nothing outside it is written
 * The upsampled map exists only tile by tile in LDS.  The result is BIT-IDENTICAL to ds_upsample_bilinear_nhwc followed by
 * ds_conv3x3_nhwc (act 0, no residual operands): an upsampled value is that kernel's expression (four rounded float32 products added
 * left to right, one rounding), the halo outside the upsampled image is literal zeros, and an output element's float32 chain is the
 * convolution's term for term (64-channel chunks ascending, taps 0..8 inside a chunk, four 32x32x16 MFMAs per tap, then + bias and
 * one rounding).  Built for out_channels == 128 and in_channels % 64 == 0 (<= 4096), and for upsample factors whose source pixels
 * under a 10 x 34 patch fit 6 x 18 (a factor of exactly 2 always does); everything else returns DS_EUNSUPPORTED and the caller runs the two
 * launches.  Allocates nothing and synchronises nothing: capturable in a hipGraph.  out must not alias x.
 */
int ds_dpt_head_front(ds_ctx *ctx, const void *x, const void *w, const void *bias, void *out, int batch, int in_h, int in_w,
                      int out_h, int out_w, int in_channels, int out_channels, int dtype, void *stream);

/*
 * ds_dpt_head_tail -- the tail of the DPT depth heads in one kernel: bilinear upsample (align_corners=True) ->
 * conv3x3 128->32 (padding 1) -> ReLU -> conv1x1 32->1 -> optional ReLU (dmidas/dpt_depth.py:150-158 output_conv[1:6];
 * ddepth_anything_v2/depth_anything_v2/dpt.py:146-147 with output_conv2 :105-111).
 *   x            [batch, in_h, in_w, 128] f16/bf16, channels_last: the output of the head's first convolution
 *   conv3_wfrag  the 3x3 weights [32, 128, 3, 3] rearranged as MFMA fragments [tap 9][k-slice 8][half 2][co 32][8 ci]
 *                (ci = 16*slice + 8*half + j), same dtype as x
 *   conv3_bias, conv1_weight  float32 [32];  conv1_bias scalar
 *   out          [batch, out_h, out_w] same dtype as x
 */
int ds_dpt_head_tail(ds_ctx *ctx, const void *x, int batch, int in_h, int in_w, int out_h, int out_w,
                     const void *conv3_wfrag, const float *conv3_bias, const float *conv1_weight, float conv1_bias,
                     int relu_out, void *out, int dtype, void *stream);

/*
 * ds_dpt_head_tail_circular -- ds_dpt_head_tail for a head whose 3x3 convolution has padding_mode='circular' (the reference's
 * TILING_MODE, src/depthmap_generation.py:251-260, applied to dmidas/dpt_depth.py:150-158 and ddepth_anything_v2/.../dpt.py:105-111).
 * Same parameter list.  The bilinear upsample is unchanged -- it is not a convolution; the 3x3 128->32 convolution reads the
 * UPSAMPLED map circularly: the halo row -1 is upsampled row out_h - 1, row out_h is row 0, likewise the columns.
 * This entry point ALWAYS launches the tile kernel (k_dpt_head_tail), whatever DS_HEAD_MODE / DS_HEAD_PERSIST say: the
 * persistent and the streaming kernel pad with zeros only.
 */
int ds_dpt_head_tail_circular(ds_ctx *ctx, const void *x, int batch, int in_h, int in_w, int out_h, int out_w,
                              const void *conv3_wfrag, const float *conv3_bias, const float *conv1_weight, float conv1_bias,
                              int relu_out, void *out, int dtype, void *stream);

/*
 * ds_gconv3x3_nhwc_f32 -- the grouped 3x3 convolution of the ResNeXt-101 32x8d bottlenecks of LeReS, Boost's base estimator, in
 * float32 with the folded BatchNorm's bias and the ReLU in the epilogue: `conv2` -> `bn2` -> `relu` of lib/Resnext_torch.py:104-110
 * (groups = 32, stride 1, padding 1; the strided first block of a stage stays a library call).  Direct convolution on the float32
 * vector pipe, input tile staged once in LDS, weights through the scalar path (csrc/ds_gconv.hip).
 *   x, y    [batch, height, width, channels] float32, channels_last;  channels % 32 == 0
 *   w_gtio  [channels / cpg groups][9 taps (ky * 3 + kx)][cpg in][cpg out] float32: torch's [out, in / groups, 3, 3] weight
 *           (BatchNorm folded in) regrouped by the host;  bias [channels] or NULL
 *   channels_per_group  8, 16 or 32
 * ds_add_relu_f32 -- y = relu(a + b) over `count` float32 values (count % 4 == 0): `self.relu(out + identity)`, the tail of every
 * bottleneck (lib/Resnext_torch.py:115-118), one pass instead of torch's add + clamp.
 */
int ds_gconv3x3_nhwc_f32(ds_ctx *ctx, const float *x, const float *w_gtio, const float *bias, float *y, int batch, int height, int width,
                         int channels, int channels_per_group, int relu, void *stream);
int ds_add_relu_f32(ds_ctx *ctx, const float *a, const float *b, float *y, int64_t count, void *stream);

/*
 * ds_bias_act_f32 -- y = [relu]((x + bias[c]) [+ res]) on float32 rows of `channels` values (channels_last activations; y may be x):
 * the element-wise tail of a LIBRARY convolution of LeReS in the reference's own order -- the BatchNorm that follows the
 * convolution (folded into weight and bias here; torch adds a convolution's bias in a separate pass on ROCm), the ReLU
 * (lib/Resnext_torch.py:100-102,104-110), for conv3 the shortcut add and its ReLU (:112-118), and the decoder's conv -> bias ->
 * ReLU / conv -> bias -> + x -> ReLU pairs (lib/network_auxi.py:116-121).  channels % 4 == 0; res NULL or laid out like x.
 * ds_relu_cat_f32 -- y[p] = relu(cat(a[p], b[p])) on float32 rows: the skip concatenation of the pix2pix U-Net's up path together
 * with the ReLU the parent level applies to it (pix2pix/models/networks.py:545-550 and :519); the concatenated tensor has no other
 * reader.  layout 0: a, b, y channels_last ([batch, plane, channels] rows; channel counts % 4 == 0).  layout 1: a channels_last, b and y
 * NCHW -- what the up path runs in (MIOpen computes the float32 transposed convolutions on NCHW tensors, the down path's skips are
 * channels_last; torch.cat of the two is NCHW); layout 2: all NCHW.  Layouts 1 / 2: channel counts % 32 == 0.  y must not alias an input.
 */
int ds_bias_act_f32(ds_ctx *ctx, const float *x, const float *bias, const float *res, float *y, int64_t pixels, int channels, int relu,
                    void *stream);

/*
 * ds_dwconv_nhwc -- the depthwise convolution of an EfficientNet-Lite block with the element-wise tails on both sides, one pass: the
 * 24 depthwise convolutions of MiDaS v2.1 small (model id 6; dmidas/midas_net_custom.py:12-67 on gen-efficientnet's
 * tf_efficientnet_lite3, dmidas/blocks.py:169-189) -- InvertedResidual `conv_pw -> bn1 -> act1 -> conv_dw -> bn2 -> act2` from the
 * second step on, and DepthwiseSeparableConv `conv_dw -> bn1 -> act1` with the stem's `bn1 -> act1` in front (BatchNorm folded):
 *     a(n, iy, ix, c) = min(max(x[n, iy, ix, c] + bias_in[c], 0), 6) inside the image, 0 outside (zero padding of the ACTIVATED x)
 *     y[n, oy, ox, c] = min(max(bias[c] + sum_{ky,kx} w[ky * kernel + kx][c] * a(n, oy * stride - pad_top + ky,
 *                                                                               ox * stride - pad_left + kx, c), 0), 6)
 * x [batch, in_h, in_w, channels], y [batch, out_h, out_w, channels]: channels_last, f16 or f32; w [kernel * kernel][channels] float32
 * (the folded weight, tap-major), bias_in / bias [channels] float32.  kernel 3 or 5, stride 1 or 2, 0 <= pad_top, pad_left < kernel;
 * the bottom / right padding follows from out_h / out_w and lies in (-stride, kernel).  channels % 8 == 0, operands 16-byte aligned,
 * y must not alias x (DS_EINVAL otherwise; bf16: DS_EUNSUPPORTED).  fp32 accumulation in ky-major tap order, + bias, one rounding to
 * the output type: an image's output does not depend on the batch size or on its position in the batch.  No workspace.
 * min / max above follow the NaN rule stated at ds_bias_act_nhwc: a NaN in x (or in a sum) stays NaN, so it reaches exactly the
 * outputs of its channel whose window holds it.
 */
int ds_dwconv_nhwc(ds_ctx *ctx, const void *x, const float *w, const float *bias_in, const float *bias, void *y, int batch, int in_h,
                   int in_w, int channels, int out_h, int out_w, int kernel, int stride, int pad_top, int pad_left, int dtype, void *stream);
int ds_relu_cat_f32(ds_ctx *ctx, const float *a, const float *b, float *y, int batch, int64_t plane, int channels_a, int channels_b, int layout,
                    void *stream);

/*
 * ds_boost_blend -- the patch-merge step of Boost, all patches in one launch; replaces, per patch, np.polyval (:916),
 * cv2.resize INTER_CUBIC of the merged patch (:918), cv2.resize INTER_LINEAR of the Gaussian mask (:930) and the blend
 * `dst[rect] = dst[rect]*(1-mask) + merged*mask` (:936) of src/depthmap_generation.py:estimateboost.
 *   dst            float32 [height, width] running estimate, updated in place (row stride in ELEMENTS)
 *   patches        n_patches records {int32 x0, y0, w, h; float64 p0, p1} (32 bytes each, device memory), in BLEND ORDER
 *   preds          float32 [n_patches, pred_size, pred_size]: (fake_B + 1)/2 of the merge network per patch
 *   mask_template  float32 [mask_size, mask_size]: generatemask((3000, 3000)) (:944-953)
 */
int ds_boost_blend(ds_ctx *ctx, float *dst, int64_t dst_row_stride, int height, int width, const void *patches,
                   int n_patches, const float *preds, int pred_size, const float *mask_template, int mask_size,
                   void *stream);

/*
 * The two ends of a DPT forward (csrc/ds_forward_ends.hip).  Each entry point below replaces a chain of copy / conversion passes
 * and leaves the same bits; none allocates or synchronises; all are asynchronous on `stream`.
 *
 * ds_preprocess_bicubic_rows -- ds_preprocess_bicubic, storing the operand of the patch-embedding GEMM instead of the NHWC network
 * input.  With gh = out_h / patch, gw = out_w / patch:
 *   rows [batch, n_pad, kpad] (f16 / bf16, 16-byte aligned):
 *     rows[b][1 + gy * gw + gx][(py * patch + px) * 3 + c] = ds_preprocess_bicubic's out[b][c][gy * patch + py][gx * patch + px]
 *     row 0, rows 1 + gh * gw .. n_pad - 1 and columns 3 * patch^2 .. kpad - 1 are zero (written here: no fill needed);
 *     output pixels beyond gh * patch x gw * patch are not computed.
 *   patch 1..32, kpad % 8 == 0, kpad >= 3 * patch^2, n_pad >= 1 + gh * gw.  Any input / output size and row pitch; source bytes
 *   come in through LDS in aligned 16-byte pieces, horizontal sums are shared by the output rows that tap the same source row.
 *   Per output element the operation order, and so the value, is ds_preprocess_bicubic's.
 */
int ds_preprocess_bicubic_rows(ds_ctx *ctx, const void *images, void *rows, int batch, int in_h, int in_w, int out_h, int out_w,
                               int flip_channels, const float *mean, const float *std, int patch, int n_pad, int kpad, int dtype,
                               void *stream);

/*
 * ds_tokens_fixup -- tokens [batch, n_pad, channels] (f16 / bf16): row 0 of every image <- cls [channels], rows n_valid .. n_pad - 1
 * <- 0.  After ds_linear on the rows above this is pad_tokens(cat(cls, patch_embed(x))).  channels % 8 == 0, 16-byte alignment.
 */
int ds_tokens_fixup(ds_ctx *ctx, void *tokens, const void *cls, int batch, int n_pad, int n_valid, int channels, int dtype, void *stream);

/*
 * ds_upsample_bicubic_to_f32 -- in [batch, in_h, in_w] (f16 / bf16) -> out float32 [batch, out_h, out_w]:
 * F.interpolate(in[:, None], (out_h, out_w), mode="bicubic", align_corners=False)[:, 0].float() in one pass, bit for bit: cubic
 * convolution (A = -0.75) on half-pixel centres, replicated border, float32 accumulation in torch's operation order, one rounding
 * to the input type, widened (src/depthmap_generation.py:484-489 + the .float() of the callers).
 */
int ds_upsample_bicubic_to_f32(ds_ctx *ctx, const void *in, void *out, int batch, int in_h, int in_w, int out_h, int out_w, int dtype,
                               void *stream);

/*
 * ds_im2col3x3_s2_nhwc -- x [batch, height, width, channels] (f16 / bf16) -> rows [batch * ho * wo, 9 * channels], ho = (height - 1) / 2 + 1,
 * wo likewise: rows[(b, oy, ox)][(ky, kx, c)] = x[b][2 * oy + ky - 1][2 * ox + kx - 1][c], outside the map 0 (circular: the pixel
 * on the opposite side, F.pad(mode="circular")) -- the GEMM operand of a 3x3 / stride 2 / padding 1 convolution.  channels % 8 == 0.
 */
int ds_im2col3x3_s2_nhwc(ds_ctx *ctx, const void *x, void *rows, int batch, int height, int width, int channels, int circular, int dtype,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEPTHSTEREO_H */
