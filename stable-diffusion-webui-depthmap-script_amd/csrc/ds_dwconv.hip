// ds_dwconv_nhwc: the depthwise convolutions of the EfficientNet-Lite3 encoder of MiDaS v2.1 small (model id 6; the reference builds
// it in dmidas/midas_net_custom.py:12-67 on gen-efficientnet's tf_efficientnet_lite3, dmidas/blocks.py:169-189).  Each of its 24
// blocks is built around one k x k depthwise convolution (k = 3 / 5, stride 1 / 2) between the tail of the convolution in front --
// the stem or the expand 1x1 of an inverted residual: bias (the folded BatchNorm) + ReLU6 -- and its own folded BatchNorm + ReLU6.
// Run stock, that is a bias pass, a clamp pass, the convolution, a bias pass and a clamp pass over tensors 6x wider than the block's
// input; here it is one pass: read x once, write y once.
//
// A workgroup owns a th x tw tile of output pixels and a block of cv 16-byte channel vectors (8 channels each, cv <= 8 divides C / 8).
// The input tile with its halo, ((th - 1) s + k) x ((tw - 1) s + k) pixels of those channels, is read ONCE from HBM (16-byte loads
// along C), activated (bias_in + ReLU6, zero outside the image: the padding is applied to the ACTIVATED tensor) and staged in LDS as
// float32, the two 4-channel halves of a vector in separate planes so that lanes of consecutive pixels read consecutive 16-byte
// slots; the folded weights of the block's channels ([tap][half][cv] float4) are staged beside it.  One thread = one (pixel, vector)
// output item: k^2 fp32 FMAs per channel in ky-major tap order, + bias, ReLU6, one rounding to the output type, one 16-byte store.
// The value of an output depends on nothing but its own window: not on the tile size the host picks, the batch size or the batch
// position.  Bound: HBM (read x + halo, write y); the host shrinks the tile until the launch has two workgroups per CU where the map
// allows (the 8 x 8 maps at /32 of a 256^2 input).
#include "ds_common.h"

#define DW_NT 256                       // threads per workgroup at most
#define DW_LDS_MAX (48 * 1024)          // bytes of LDS per workgroup at most: three workgroups per CU

typedef float dw_f4 __attribute__((ext_vector_type(4)));

// ReLU6 as torch's hardtanh computes it: a NaN stays NaN (fminf(fmaxf(v, 0), 6) would turn it into 0)
__device__ __forceinline__ float dw_relu6(float v) { return v < 0.f ? 0.f : (v > 6.f ? 6.f : v); }

template <typename T> struct dw_io;
template <> struct dw_io<_Float16> {
    static __device__ __forceinline__ void load8(const _Float16 *p, float *v)
    {
        _Float16 h[8];
        __builtin_memcpy(h, p, 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
    }
    static __device__ __forceinline__ void store8(_Float16 *p, const float *v)
    {
        _Float16 h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (_Float16)v[j];
        __builtin_memcpy(p, h, 16);
    }
};
template <> struct dw_io<float> {
    static __device__ __forceinline__ void load8(const float *p, float *v)
    {
        const dw_f4 a = *(const dw_f4 *)p, b = *(const dw_f4 *)(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void store8(float *p, const float *v)
    {
        *(dw_f4 *)p = dw_f4{v[0], v[1], v[2], v[3]};
        *(dw_f4 *)(p + 4) = dw_f4{v[4], v[5], v[6], v[7]};
    }
};

// x [batch, in_h, in_w, C], y [batch, out_h, out_w, C]; w [K * K][C], bias_in [C], bias [C] float32.
// Grid: (tiles_x * tiles_y * batch, C / (8 cv)).  Dynamic LDS: (2 tin_h tin_w cv + 2 K^2 cv) float4.
template <typename T, int K, int S>
__global__ __launch_bounds__(DW_NT) void k_dwconv_nhwc(const T *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias_in,
                                                       const float *__restrict__ bias, T *__restrict__ y, int in_h, int in_w, int out_h, int out_w,
                                                       int C, int pad_top, int pad_left, int th, int tw, int tiles_x, int tiles_y, int cv)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dw_lds[];
    const int tin_h = (th - 1) * S + K, tin_w = (tw - 1) * S + K;
    const int npix = tin_h * tin_w;
    dw_f4 *tile = (dw_f4 *)dw_lds;                 // [2 halves][npix][cv]: channels 0-3 / 4-7 of each vector
    dw_f4 *wl = tile + 2 * npix * cv;              // [K * K taps][2 halves][cv]
    int t = blockIdx.x;
    const int bx = t % tiles_x;
    t /= tiles_x;
    const int by = t % tiles_y;
    const int n = t / tiles_y;
    const int c0 = blockIdx.y * cv * 8;
    const int oy0 = by * th, ox0 = bx * tw;
    const int iy0 = oy0 * S - pad_top, ix0 = ox0 * S - pad_left;

    for (int i = threadIdx.x; i < K * K * 2 * cv; i += blockDim.x) {
        const int v = i % cv, hv = i / cv;          // hv = tap * 2 + half
        wl[i] = *(const dw_f4 *)(w + (size_t)(hv >> 1) * C + c0 + v * 8 + (hv & 1) * 4);
    }
    const T *xb = x + (size_t)n * in_h * in_w * C + c0;
    for (int i = threadIdx.x; i < npix * cv; i += blockDim.x) {
        const int v = i % cv, p = i / cv;
        const int py = p / tin_w, px = p - py * tin_w;
        const int gy = iy0 + py, gx = ix0 + px;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < in_h && gx >= 0 && gx < in_w) {
            float xv[8];
            dw_io<T>::load8(xb + ((size_t)gy * in_w + gx) * C + v * 8, xv);
            const dw_f4 b0 = *(const dw_f4 *)(bias_in + c0 + v * 8), b1 = *(const dw_f4 *)(bias_in + c0 + v * 8 + 4);
            const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = dw_relu6(xv[j] + bv[j]);
        }
        tile[p * cv + v] = dw_f4{a[0], a[1], a[2], a[3]};
        tile[(npix + p) * cv + v] = dw_f4{a[4], a[5], a[6], a[7]};
    }
    __syncthreads();

    T *yb = y + (size_t)n * out_h * out_w * C + c0;
    for (int i = threadIdx.x; i < th * tw * cv; i += blockDim.x) {
        const int v = i % cv, p = i / cv;
        const int ty = p / tw, tx = p - ty * tw;
        const int oy = oy0 + ty, ox = ox0 + tx;
        if (oy >= out_h || ox >= out_w) continue;
        dw_f4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int pix = (ty * S + ky) * tin_w + tx * S + kx;
                const dw_f4 a0 = tile[pix * cv + v], a1 = tile[(npix + pix) * cv + v];
                const dw_f4 w0 = wl[(ky * K + kx) * 2 * cv + v], w1 = wl[((ky * K + kx) * 2 + 1) * cv + v];
                lo.x = __builtin_fmaf(w0.x, a0.x, lo.x); lo.y = __builtin_fmaf(w0.y, a0.y, lo.y);
                lo.z = __builtin_fmaf(w0.z, a0.z, lo.z); lo.w = __builtin_fmaf(w0.w, a0.w, lo.w);
                hi.x = __builtin_fmaf(w1.x, a1.x, hi.x); hi.y = __builtin_fmaf(w1.y, a1.y, hi.y);
                hi.z = __builtin_fmaf(w1.z, a1.z, hi.z); hi.w = __builtin_fmaf(w1.w, a1.w, hi.w);
            }
        }
        const dw_f4 b0 = *(const dw_f4 *)(bias + c0 + v * 8), b1 = *(const dw_f4 *)(bias + c0 + v * 8 + 4);
        const float o[8] = {dw_relu6(lo.x + b0.x), dw_relu6(lo.y + b0.y), dw_relu6(lo.z + b0.z), dw_relu6(lo.w + b0.w),
                            dw_relu6(hi.x + b1.x), dw_relu6(hi.y + b1.y), dw_relu6(hi.z + b1.z), dw_relu6(hi.w + b1.w)};
        dw_io<T>::store8(yb + ((size_t)oy * out_w + ox) * C + v * 8, o);
    }
}

static size_t dw_lds_bytes(int th, int tw, int k, int s, int cv)
{
    const size_t tin = (size_t)((th - 1) * s + k) * ((tw - 1) * s + k);
    return (2 * tin * cv + 2 * (size_t)k * k * cv) * 16;
}

template <typename T, int K, int S>
static int dw_launch(dim3 grid, int nt, size_t lds, hipStream_t st, const void *x, const float *w, const float *bias_in, const float *bias, void *y,
                     int in_h, int in_w, int out_h, int out_w, int C, int pad_top, int pad_left, int th, int tw, int tiles_x, int tiles_y, int cv)
{
    hipLaunchKernelGGL((k_dwconv_nhwc<T, K, S>), grid, dim3(nt), lds, st, (const T *)x, w, bias_in, bias, (T *)y, in_h, in_w, out_h, out_w, C,
                       pad_top, pad_left, th, tw, tiles_x, tiles_y, cv);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_dwconv_nhwc(ds_ctx *ctx, const void *x, const float *w, const float *bias_in, const float *bias, void *y, int batch, int in_h,
                          int in_w, int channels, int out_h, int out_w, int kernel, int stride, int pad_top, int pad_left, int dtype, void *stream)
{
    DS_REQUIRE(ctx && x && w && bias_in && bias && y, DS_EINVAL, "ds_dwconv_nhwc: null argument");
    DS_REQUIRE(dtype != DS_DTYPE_BF16, DS_EUNSUPPORTED, "ds_dwconv_nhwc: bf16 is not built (f16 or f32)");
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_F32, DS_EINVAL, "ds_dwconv_nhwc: dtype must be f16 or f32 (got %d)", dtype);
    DS_REQUIRE((kernel == 3 || kernel == 5) && (stride == 1 || stride == 2), DS_EINVAL,
               "ds_dwconv_nhwc: kernel must be 3 or 5, stride 1 or 2 (got %d, %d)", kernel, stride);
    DS_REQUIRE(pad_top >= 0 && pad_top < kernel && pad_left >= 0 && pad_left < kernel, DS_EINVAL,
               "ds_dwconv_nhwc: pads must lie in [0, kernel) (got %d, %d)", pad_top, pad_left);
    DS_REQUIRE(batch > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && channels > 0 && channels % 8 == 0, DS_EINVAL,
               "ds_dwconv_nhwc: bad shape (batch %d, in %d x %d, out %d x %d, channels %d: a multiple of 8)", batch, in_h, in_w, out_h, out_w, channels);
    // bottom / right padding implied by the output size: 0 <= pad < kernel, or a negative one above -stride (the last rows
    // are not reached, as a floor division of the output size leaves them)
    const long long pad_bottom = (long long)(out_h - 1) * stride + kernel - pad_top - in_h;
    const long long pad_right = (long long)(out_w - 1) * stride + kernel - pad_left - in_w;
    DS_REQUIRE(pad_bottom > -stride && pad_bottom < kernel && pad_right > -stride && pad_right < kernel, DS_EINVAL,
               "ds_dwconv_nhwc: output %d x %d does not follow from input %d x %d, kernel %d, stride %d, pads %d / %d", out_h, out_w, in_h,
               in_w, kernel, stride, pad_top, pad_left);
    DS_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias_in | (uintptr_t)bias | (uintptr_t)y) & 15) == 0, DS_EINVAL,
               "ds_dwconv_nhwc: operands must be 16-byte aligned");
    const size_t es = dtype == DS_DTYPE_F16 ? 2 : 4;
    const uintptr_t xs = (uintptr_t)x, xe = xs + (size_t)batch * in_h * in_w * channels * es;
    const uintptr_t ys = (uintptr_t)y, ye = ys + (size_t)batch * out_h * out_w * channels * es;
    DS_REQUIRE(ye <= xs || xe <= ys, DS_EINVAL, "ds_dwconv_nhwc: y must not alias x");

    // channel block: the largest count of 8-channel vectors <= 8 that divides channels / 8 (32 -> 4, 144 -> 6, 192 -> 8, 1392 -> 6)
    const int c8 = channels / 8;
    int cv = 8;
    while (c8 % cv) --cv;
    const int nblk = c8 / cv;
    DS_REQUIRE(nblk <= 65535, DS_EUNSUPPORTED, "ds_dwconv_nhwc: too many channels (%d)", channels);
    if (!ctx->ncu) {
        int ncu = 0;
        DS_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->ncu = ncu >= 8 ? ncu / 8 * 8 : 8;
    }
    // tile: the largest candidate within the LDS budget whose launch has two workgroups per CU, else the smallest
    static const int cand[][2] = {{8, 16}, {8, 8}, {4, 8}, {4, 4}, {2, 4}, {2, 2}};
    int th = 0, tw = 0;
    for (const auto &c : cand) {
        if (dw_lds_bytes(c[0], c[1], kernel, stride, cv) > DW_LDS_MAX) continue;
        th = c[0];
        tw = c[1];
        const long long wgs = (long long)((out_h + th - 1) / th) * ((out_w + tw - 1) / tw) * batch * nblk;
        if (wgs >= 2ll * ctx->ncu) break;
    }
    DS_REQUIRE(th > 0, DS_EUNSUPPORTED, "ds_dwconv_nhwc: no tile fits the LDS budget");
    const int tiles_x = (out_w + tw - 1) / tw, tiles_y = (out_h + th - 1) / th;
    DS_REQUIRE((long long)tiles_x * tiles_y * batch < (1ll << 31), DS_EUNSUPPORTED, "ds_dwconv_nhwc: grid too large");
    const size_t lds = dw_lds_bytes(th, tw, kernel, stride, cv);
    int nt = (th * tw * cv + 63) / 64 * 64;
    if (nt > DW_NT) nt = DW_NT;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)(tiles_x * tiles_y * batch), (unsigned)nblk);
    hipStream_t st = (hipStream_t)stream;
#define DW_CASE(TT, KK, SS)                                                                                                                \
    if (kernel == KK && stride == SS)                                                                                                       \
        return dw_launch<TT, KK, SS>(grid, nt, lds, st, x, w, bias_in, bias, y, in_h, in_w, out_h, out_w, channels, pad_top, pad_left, th, tw, \
                                     tiles_x, tiles_y, cv);
    if (dtype == DS_DTYPE_F16) {
        DW_CASE(_Float16, 3, 1) DW_CASE(_Float16, 3, 2) DW_CASE(_Float16, 5, 1) DW_CASE(_Float16, 5, 2)
    } else {
        DW_CASE(float, 3, 1) DW_CASE(float, 3, 2) DW_CASE(float, 5, 1) DW_CASE(float, 5, 2)
    }
#undef DW_CASE
    return DS_EINVAL;
}
