// ds_resize_lanczos, ds_custom_depth_to_f64: the custom-depth branch of the funnel (reference: src/core.py:145-174) on the device.
//
// The reference takes a caller's depth map, resizes it to the image with Pillow's LANCZOS filter when the sizes differ (:147-153),
// widens it to float64 (:156 / :169), takes the maximum to guess the bit depth (:157-164) and divides by 2^bits (:165) -- channel 0
// divided by 256 for a multi-band map (:169-170).  Both halves are restated here.
//
// The resize is Pillow's Resample.c: separable, a horizontal pass (when the width changes) then a vertical one (when the height
// changes), EACH rounded into the image's own pixel type.  The tap windows and weights of an axis come from the host
// (src/resample_model.lanczos_coeffs: the libm sin Pillow calls); a lane makes one output pixel and adds its taps in ascending
// order, the multiply and the add as separate float64 operations (the library is built with -ffp-contract=off):
//   8-bit         int32 accumulator from 2^21, weights in 22-bit fixed point, (acc >> 22) clipped to 0..255
//   16-bit        float64 sum, ROUND_UP, then Pillow's byte-wise store: below 0 -> 0, above 65535 -> 0xFF00 | low byte
//   int32         float64 sum, ROUND_UP (add half away from zero, truncate)
//   float32       float64 sum, one cast
// The weights are stored tap-major ([tap][output index]) so that the lanes of the horizontal pass read consecutive words; in the
// vertical pass a row of lanes shares one output row and its weights.  Source reads go through L2: neighbouring lanes read
// neighbouring (enlarging: the same) source pixels, a few bytes per output pixel in and out.
#include "ds_common.h"

#include <algorithm>

#define DS_RESAMPLE_MAX_TAPS 1024

template <int PIX> struct rs_pix;
template <> struct rs_pix<DS_PIX_U8>  { typedef uint8_t T;  typedef int32_t K; };
template <> struct rs_pix<DS_PIX_U16> { typedef uint16_t T; typedef double K; };
template <> struct rs_pix<DS_PIX_I32> { typedef int32_t T;  typedef double K; };
template <> struct rs_pix<DS_PIX_F32> { typedef float T;    typedef double K; };

__device__ __forceinline__ int rs_round_up(double ss)
{
    const double r = ss >= 0.0 ? ss + 0.5 : ss - 0.5;
    return (int)r;                                            // (saturating on the device; Pillow's inputs never get there)
}

template <int PIX> struct rs_acc;
template <> struct rs_acc<DS_PIX_U8> {
    int32_t ss = 1 << 21;
    __device__ __forceinline__ void tap(uint8_t p, int32_t k) { ss += (int32_t)p * k; }
    __device__ __forceinline__ uint8_t result() const { const int32_t v = ss >> 22; return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
};
template <> struct rs_acc<DS_PIX_U16> {
    double ss = 0.0;
    __device__ __forceinline__ void tap(uint16_t p, double k) { const double m = (double)(int)p * k; ss = ss + m; }
    __device__ __forceinline__ uint16_t result() const
    {
        const int r = rs_round_up(ss);
        return (uint16_t)(r < 0 ? 0 : (r > 65535 ? (0xFF00 | (r & 255)) : r));
    }
};
template <> struct rs_acc<DS_PIX_I32> {
    double ss = 0.0;
    __device__ __forceinline__ void tap(int32_t p, double k) { const double m = (double)p * k; ss = ss + m; }
    __device__ __forceinline__ int32_t result() const { return rs_round_up(ss); }
};
template <> struct rs_acc<DS_PIX_F32> {
    double ss = 0.0;
    __device__ __forceinline__ void tap(float p, double k) { const double m = (double)p * k; ss = ss + m; }
    __device__ __forceinline__ float result() const { return (float)ss; }
};

// One pass: dense output [n][out_h][out_w], one lane per output pixel.  HORIZONTAL: the window of a lane is chosen by its column and
// runs along the source row (step s_px); otherwise it is chosen by its row and runs down the source column (step s_row).
// All strides in ELEMENTS of T.  bounds: out * {first tap, tap count}; kk: [taps][out]; in_len: length of the resampled axis.
template <int PIX, bool HORIZONTAL>
__global__ __launch_bounds__(256) void k_resample_pass(const typename rs_pix<PIX>::T *__restrict__ src, long long s_img, long long s_row,
                                                       long long s_px, typename rs_pix<PIX>::T *__restrict__ dst, int out_h, int out_w,
                                                       const int *__restrict__ bounds, const typename rs_pix<PIX>::K *__restrict__ kk,
                                                       int in_len, int taps)
{
    const long long per_image = (long long)out_h * out_w;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_image) return;
    const int y = (int)(i / out_w), x = (int)(i - (long long)y * out_w);
    const int o = HORIZONTAL ? x : y, outs = HORIZONTAL ? out_w : out_h;
    const int first = bounds[2 * o];
    int count = bounds[2 * o + 1];
    if (first < 0 || count > taps || count > in_len - first) count = 0;      // a window outside the source or the table: nothing is read
    const typename rs_pix<PIX>::T *s = src + (long long)blockIdx.y * s_img
                                       + (HORIZONTAL ? (long long)y * s_row + (long long)first * s_px
                                                     : (long long)first * s_row + (long long)x * s_px);
    const long long step = HORIZONTAL ? s_px : s_row;
    rs_acc<PIX> acc;
    for (int t = 0; t < count; ++t) acc.tap(s[(long long)t * step], kk[(long long)t * outs + o]);
    dst[(long long)blockIdx.y * per_image + i] = acc.result();
}

template <int PIX>
static int rs_launch(ds_ctx *ctx, const void *src, int n, int in_h, int in_w, int64_t px, int64_t row, int64_t img, void *dst, int out_h,
                     int out_w, const int *hb, const void *hk, int ht, const int *vb, const void *vk, int vt, void *tmp, hipStream_t st)
{
    typedef typename rs_pix<PIX>::T T;
    typedef typename rs_pix<PIX>::K K;
    const bool horiz = out_w != in_w, vert = out_h != in_h;
    const T *s = (const T *)src;
    if (horiz) {
        T *d = (T *)dst;
        if (vert) d = (T *)tmp;                               // the rounded intermediate: [n][in_h][out_w]
        const long long per_image = (long long)in_h * out_w;
        hipLaunchKernelGGL((k_resample_pass<PIX, true>), dim3((unsigned)((per_image + 255) / 256), n), dim3(256), 0, st, s, (long long)img,
                           (long long)row, (long long)px, d, in_h, out_w, hb, (const K *)hk, in_w, ht);
        DS_HIP_CHECK(hipGetLastError());
        s = d; px = 1; row = out_w; img = per_image;
    }
    if (vert) {
        const long long per_image = (long long)out_h * out_w;
        hipLaunchKernelGGL((k_resample_pass<PIX, false>), dim3((unsigned)((per_image + 255) / 256), n), dim3(256), 0, st, s, (long long)img,
                           (long long)row, (long long)px, (T *)dst, out_h, out_w, vb, (const K *)vk, in_h, vt);
        DS_HIP_CHECK(hipGetLastError());
    }
    return DS_OK;
}

DS_API int ds_resize_lanczos(ds_ctx *ctx, const void *src, int pix, int n, int in_h, int in_w, int64_t src_px_stride,
                             int64_t src_row_stride, int64_t src_img_stride, void *dst, int out_h, int out_w, const int32_t *h_bounds,
                             const void *h_coeffs, int h_taps, const int32_t *v_bounds, const void *v_coeffs, int v_taps, void *tmp, void *stream)
{
    DS_REQUIRE(ctx && src && dst, DS_EINVAL, "ds_resize_lanczos: null argument");
    DS_REQUIRE(n > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, DS_EINVAL, "ds_resize_lanczos: bad shape n=%d %dx%d -> %dx%d", n,
               in_h, in_w, out_h, out_w);
    DS_REQUIRE(pix >= DS_PIX_U8 && pix <= DS_PIX_F32, DS_EUNSUPPORTED, "ds_resize_lanczos: unknown pixel type %d", pix);
    DS_REQUIRE(src_px_stride >= 1 && src_row_stride >= src_px_stride * (int64_t)(in_w - 1) + 1
               && src_img_stride >= src_row_stride * (int64_t)(in_h - 1) + src_px_stride * (int64_t)(in_w - 1) + 1,
               DS_EINVAL, "ds_resize_lanczos: source strides overlap");
    const bool horiz = out_w != in_w, vert = out_h != in_h;
    DS_REQUIRE(horiz || vert, DS_EINVAL, "ds_resize_lanczos: source and destination have one size, nothing to resize");
    DS_REQUIRE((!horiz || (h_bounds && h_coeffs && h_taps > 0)) && (!vert || (v_bounds && v_coeffs && v_taps > 0)), DS_EINVAL,
               "ds_resize_lanczos: the coefficients of a pass that runs are missing");
    DS_REQUIRE(!(horiz && vert) || (tmp && tmp != dst && tmp != src), DS_EINVAL, "ds_resize_lanczos: two passes need an intermediate buffer of their own");
    DS_REQUIRE((!horiz || h_taps <= DS_RESAMPLE_MAX_TAPS) && (!vert || v_taps <= DS_RESAMPLE_MAX_TAPS), DS_EUNSUPPORTED,
               "ds_resize_lanczos: more than %d taps per output pixel", DS_RESAMPLE_MAX_TAPS);
    DS_REQUIRE(n <= 65535, DS_EUNSUPPORTED, "ds_resize_lanczos: batch too large for the grid");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    switch (pix) {
    case DS_PIX_U8:  return rs_launch<DS_PIX_U8>(ctx, src, n, in_h, in_w, src_px_stride, src_row_stride, src_img_stride, dst, out_h, out_w, h_bounds, h_coeffs, h_taps, v_bounds, v_coeffs, v_taps, tmp, st);
    case DS_PIX_U16: return rs_launch<DS_PIX_U16>(ctx, src, n, in_h, in_w, src_px_stride, src_row_stride, src_img_stride, dst, out_h, out_w, h_bounds, h_coeffs, h_taps, v_bounds, v_coeffs, v_taps, tmp, st);
    case DS_PIX_I32: return rs_launch<DS_PIX_I32>(ctx, src, n, in_h, in_w, src_px_stride, src_row_stride, src_img_stride, dst, out_h, out_w, h_bounds, h_coeffs, h_taps, v_bounds, v_coeffs, v_taps, tmp, st);
    default:         return rs_launch<DS_PIX_F32>(ctx, src, n, in_h, in_w, src_px_stride, src_row_stride, src_img_stride, dst, out_h, out_w, h_bounds, h_coeffs, h_taps, v_bounds, v_coeffs, v_taps, tmp, st);
    }
}

// ------------------------------------------------------------------------------------------------
// The rest of the branch: np.asarray(dp, dtype="float"), .max(), / 2^bits.
#define CD_BLOCK 256
#define CD_MAX_BLOCKS DS_CD_WORKSPACE_BLOCKS

// np.max: a NaN wins, whatever came before it and whatever follows
__device__ __forceinline__ double cd_max(double m, double v) { return (v > m || v != v) ? v : m; }

template <typename T>
__global__ __launch_bounds__(CD_BLOCK) void k_cd_max_stage1(const T *__restrict__ src, long long s_img, long long s_row, long long s_px,
                                                            int h, int w, double *__restrict__ partials)
{
    __shared__ double s_m[CD_BLOCK / 64];
    const long long per_image = (long long)h * w;
    const T *s = src + (long long)blockIdx.y * s_img;
    double m = -__builtin_inf();
    for (long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x; i < per_image; i += (long long)gridDim.x * CD_BLOCK) {
        const long long y = i / w, x = i - y * w;
        m = cd_max(m, (double)s[y * s_row + x * s_px]);
    }
    for (int o = 32; o > 0; o >>= 1) m = cd_max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < CD_BLOCK / 64; ++k) m = cd_max(m, s_m[k]);
        partials[(long long)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

// one wave per image: the maximum of the block partials, then the reference's bit-depth rule (:158-165)
__global__ __launch_bounds__(64) void k_cd_max_stage2(const double *__restrict__ partials, int nb, double *__restrict__ max_div)
{
    double m = -__builtin_inf();
    for (int k = threadIdx.x; k < nb; k += 64) m = cd_max(m, partials[(long long)blockIdx.x * nb + k]);
    for (int o = 32; o > 0; o >>= 1) m = cd_max(m, __shfl_xor(m, o, 64));
    if (threadIdx.x == 0) {
        max_div[2 * blockIdx.x] = m;
        max_div[2 * blockIdx.x + 1] = m < 256.0 ? 256.0 : (m < 65536.0 ? 65536.0 : 4294967296.0);      // a NaN fails both: 2^32
    }
}

template <typename T>
__global__ __launch_bounds__(CD_BLOCK) void k_cd_widen(const T *__restrict__ src, long long s_img, long long s_row, long long s_px, int h,
                                                       int w, const double *__restrict__ max_div, double fixed_div, double *__restrict__ out)
{
    const long long per_image = (long long)h * w;
    const T *s = src + (long long)blockIdx.y * s_img;
    const double div = max_div ? max_div[2 * blockIdx.y + 1] : fixed_div;
    double *o = out + (long long)blockIdx.y * per_image;
    for (long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x; i < per_image; i += (long long)gridDim.x * CD_BLOCK) {
        const long long y = i / w, x = i - y * w;
        o[i] = (double)s[y * s_row + x * s_px] / div;
    }
}

template <typename T>
static int cd_launch(ds_ctx *ctx, const void *src, int n, int h, int w, int64_t px, int64_t row, int64_t img, int rule, double *out,
                     double *workspace, hipStream_t st)
{
    const long long per_image = (long long)h * w;
    const int nb = (int)std::min<long long>((per_image + CD_BLOCK * 4 - 1) / (CD_BLOCK * 4), CD_MAX_BLOCKS);
    const double *max_div = nullptr;
    if (rule == DS_CD_SINGLE_BAND) {
        double *md = workspace, *parts = workspace + (size_t)n * 2;       // n * {maximum, divisor}, then n * nb block partials
        hipLaunchKernelGGL(k_cd_max_stage1<T>, dim3(nb, n), dim3(CD_BLOCK), 0, st, (const T *)src, (long long)img, (long long)row,
                           (long long)px, h, w, parts);
        hipLaunchKernelGGL(k_cd_max_stage2, dim3(n), dim3(64), 0, st, (const double *)parts, nb, md);
        DS_HIP_CHECK(hipGetLastError());
        max_div = md;
    }
    hipLaunchKernelGGL(k_cd_widen<T>, dim3(nb, n), dim3(CD_BLOCK), 0, st, (const T *)src, (long long)img, (long long)row, (long long)px, h, w,
                       max_div, rule == DS_CD_MULTI_BAND ? 256.0 : 1.0, out);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_custom_depth_to_f64(ds_ctx *ctx, const void *src, int pix, int n, int h, int w, int64_t src_px_stride, int64_t src_row_stride,
                                  int64_t src_img_stride, int rule, double *out, double *workspace, void *stream)
{
    DS_REQUIRE(ctx && src && out, DS_EINVAL, "ds_custom_depth_to_f64: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "ds_custom_depth_to_f64: bad shape n=%d h=%d w=%d", n, h, w);
    DS_REQUIRE(pix >= DS_PIX_U8 && pix <= DS_PIX_F32, DS_EUNSUPPORTED, "ds_custom_depth_to_f64: unknown pixel type %d", pix);
    DS_REQUIRE(rule >= DS_CD_WIDEN && rule <= DS_CD_MULTI_BAND, DS_EINVAL, "ds_custom_depth_to_f64: unknown rule %d", rule);
    DS_REQUIRE(workspace || rule != DS_CD_SINGLE_BAND, DS_EINVAL, "ds_custom_depth_to_f64: the single-band rule needs its workspace");
    DS_REQUIRE(src_px_stride >= 1 && src_row_stride >= src_px_stride * (int64_t)(w - 1) + 1
               && src_img_stride >= src_row_stride * (int64_t)(h - 1) + src_px_stride * (int64_t)(w - 1) + 1,
               DS_EINVAL, "ds_custom_depth_to_f64: source strides overlap");
    DS_REQUIRE(n <= 65535, DS_EUNSUPPORTED, "ds_custom_depth_to_f64: batch too large for the grid");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    switch (pix) {
    case DS_PIX_U8:  return cd_launch<uint8_t>(ctx, src, n, h, w, src_px_stride, src_row_stride, src_img_stride, rule, out, workspace, st);
    case DS_PIX_U16: return cd_launch<uint16_t>(ctx, src, n, h, w, src_px_stride, src_row_stride, src_img_stride, rule, out, workspace, st);
    case DS_PIX_I32: return cd_launch<int32_t>(ctx, src, n, h, w, src_px_stride, src_row_stride, src_img_stride, rule, out, workspace, st);
    default:         return cd_launch<float>(ctx, src, n, h, w, src_px_stride, src_row_stride, src_img_stride, rule, out, workspace, st);
    }
}
