// The two ends of a DPT forward as streaming passes (include/depthstereo.h):
//   ds_preprocess_bicubic_rows   uint8 image -> the zero padded patch rows the patch-embedding GEMM reads (ds_preprocess_bicubic's
//                                arithmetic; no NHWC network input, no gather, no cat, no pad copy)
//   ds_tokens_fixup              cls token into row 0, zeros into the pad rows of the GEMM's output
//   ds_upsample_bicubic_to_f32   the half-precision prediction -> float32 [B, H, W] in one pass (torch's upsample_bicubic2d + .float())
//   ds_im2col3x3_s2_nhwc         the 3x3 / stride 2 / padding 1 windows of an NHWC map as GEMM rows
// All of them move bytes; none changes a bit of what the passes they replace produced.
#include <algorithm>

#include "ds_common.h"

template <int BF16> struct fe_traits;
template <> struct fe_traits<0> { typedef _Float16 T; };
template <> struct fe_traits<1> { typedef __bf16 T; };

// ------------------------------------------------------------------------------------------------------------------------
// ds_preprocess_bicubic_rows.  A workgroup renders one strip of `twp` patches (p output rows x twp * p <= 64 output columns):
//   1. the coefficient sets and clamped source columns / rows of the strip, once per output column and once per output row;
//   2. the source bytes the strip touches, global -> LDS in aligned 16-byte pieces (a row's first piece starts at the 16-byte
//      boundary below its first byte, so any row pitch works; pieces that leave the image tensor are read byte by byte);
//   3. the horizontal sums h[source row][output column][c] -- ONE per source row, shared by every output row that taps it;
//   4. the vertical sums, flip, normalisation and the one rounding, written into an LDS image of the strip's patch rows
//      ([patch][(py * p + px) * 3 + c], zero padded to kpad);
//   5. that image -> global memory, 16 bytes per lane (the strip's patch rows are adjacent rows of the operand).
// Operation order per output element is k_preprocess_bicubic's: h += cx[kx] * (px / 255) over kx, acc += cy[ky] * h over ky.
// px / 255 is the correctly rounded quotient without a division: q = px * r, q + (px - q * 255) * r with r = RN(1 / 255) and
// fused multiply-adds gives RN(px / 255) for every px in 0..255 (checked exhaustively in exact arithmetic; the tests compare
// every byte value against the dividing kernel).
// A strip whose source region does not fit the LDS budget (strong downsampling) takes the generic path: steps 3-4 read their
// taps straight from global memory like k_preprocess_bicubic -- same sums, same bits.
#define FE_ROWS_MAX 160          // staged source rows of one strip
#define FE_P_MAX 32              // patch size
struct RowsParams {
    const uint8_t *in, *in_end;  // the image tensor's first byte and one past its last
    const uint8_t *safe;         // a 16-byte aligned address with 16 bytes of the tensor behind it (what a masked lane loads)
    void *rows;
    int ih, iw, flip;
    float sy, sx, mean[3], istd[3];
    int p, gh, gw, n_pad, kpad, twp;
    int src_rows, src_pitch;     // LDS room: staged rows and bytes per staged row (a multiple of 16); src_rows == 0: generic path
    int region;                  // bytes of the LDS region shared by the staged source and the strip's patch rows
};

__device__ __forceinline__ float fe_u8_unit(uint8_t v)      // RN(v / 255.0f)
{
    const float r = 1.0f / 255.0f, x = (float)v, q = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), r, q);
}

template <int BF16>
__global__ __launch_bounds__(256) void k_preprocess_rows(RowsParams P)
{
    typedef typename fe_traits<BF16>::T T;
    extern __shared__ uint4 fe_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.z, gy = blockIdx.y, C8 = P.kpad >> 3;
    uint4 *rows = (uint4 *)P.rows + (size_t)b * P.n_pad * C8;
    const uint4 z4 = make_uint4(0, 0, 0, 0);
    if (gy == P.gh) {                                          // the zero rows of this image: row 0 and rows 1 + gh * gw .. n_pad - 1
        const int nz = P.n_pad - P.gh * P.gw;
        for (int z = blockIdx.x; z < nz; z += gridDim.x) {
            uint4 *dst = rows + (size_t)(z == 0 ? 0 : P.gh * P.gw + z) * C8;
            for (int i = tid; i < C8; i += 256) dst[i] = z4;
        }
        return;
    }
    const int gx0 = blockIdx.x * P.twp, np = min(P.twp, P.gw - gx0), npx = np * P.p, K = 3 * P.p * P.p;
    // LDS: the tables, then ONE region that holds the staged source bytes and, once the horizontal sums are taken, the strip's
    // patch rows, then the horizontal sums
    unsigned char *sm = (unsigned char *)fe_smem;
    int *xs = (int *)sm;                       sm += 64 * 4 * sizeof(int);
    float *cxs = (float *)sm;                  sm += 64 * 4 * sizeof(float);
    int *ys = (int *)sm;                       sm += FE_P_MAX * 4 * sizeof(int);
    float *cys = (float *)sm;                  sm += FE_P_MAX * 4 * sizeof(float);
    int *colmeta = (int *)sm;                  sm += 64 * sizeof(int);
    unsigned char *src = sm;
    T *otile = (T *)sm;                        sm += P.region;
    float *hbuf = (float *)sm;

    if (tid < npx) {                                                           // wave 0: one output column each
        const float fx = P.sx * ((float)(gx0 * P.p + tid) + 0.5f) - 0.5f, fx0 = floorf(fx);
        float c[4];
        pre_cubic(fx - fx0, c);
        const int ix = (int)fx0;
#pragma unroll
        for (int k = 0; k < 4; k++) { xs[tid * 4 + k] = min(max(ix - 1 + k, 0), P.iw - 1); cxs[tid * 4 + k] = c[k]; }
        const int pj = tid / P.p;
        colmeta[tid] = pj * P.kpad + (tid - pj * P.p) * 3;
    } else if (tid >= 64 && tid < 64 + P.p) {                                  // wave 1: one output row each
        const int py = tid - 64;
        const float fy = P.sy * ((float)(gy * P.p + py) + 0.5f) - 0.5f, fy0 = floorf(fy);
        float c[4];
        pre_cubic(fy - fy0, c);
        const int iy = (int)fy0;
#pragma unroll
        for (int k = 0; k < 4; k++) { ys[py * 4 + k] = min(max(iy - 1 + k, 0), P.ih - 1); cys[py * 4 + k] = c[k]; }
    }
    __syncthreads();
    // (the clamped taps are monotone in the output index: the strip's source region is first tap of the first .. last tap of the last)
    const int x_lo = xs[0], x_hi = xs[(npx - 1) * 4 + 3], y_lo = ys[0], y_hi = ys[(P.p - 1) * 4 + 3];
    const int nrows = y_hi - y_lo + 1, nbytes = (x_hi - x_lo + 1) * 3;
    const uint8_t *img = P.in + (size_t)b * P.ih * P.iw * 3;
    const bool staged = nrows <= P.src_rows && nbytes + 30 <= P.src_pitch;     // uniform
    int xo[4];
    float cx[4];
    if (lane < npx) {
#pragma unroll
        for (int k = 0; k < 4; k++) { xo[k] = xs[lane * 4 + k]; cx[k] = cxs[lane * 4 + k]; }
    }
    if (staged) {
        // piece i of the region = piece i % nch of staged row i / nch; four loads in flight per lane before the first LDS write
        const int nch = P.src_pitch >> 4, total = nrows * nch;
        for (int base = tid; base < total; base += 1024) {
            uint4 v[4];
            const uint8_t *s[4];
            bool whole[4], part[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = min(base + u * 256, total - 1);
                const int r = (int)((unsigned)i / (unsigned)nch), c = i - r * nch;
                const uint8_t *a = img + ((size_t)(y_lo + r) * P.iw + x_lo) * 3;
                const int sh = (int)((uintptr_t)a & 15);
                s[u] = a - sh + 16 * c;
                const bool need = 16 * c < sh + nbytes;                        // (sh + nbytes <= 15 + nbytes <= src_pitch - 15)
                whole[u] = need && s[u] >= P.in && s[u] + 16 <= P.in_end;
                part[u] = need && !whole[u];
                v[u] = *(const uint4 *)(whole[u] ? s[u] : P.safe);            // unconditional: the four loads fly together
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (part[u]) {                                                 // a piece that leaves the tensor: its inside bytes only
                    unsigned char t[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) t[k] = (s[u] + k >= P.in && s[u] + k < P.in_end) ? s[u][k] : (unsigned char)0;
                    __builtin_memcpy(&v[u], t, 16);
                }
                if (base + u * 256 < total) ((uint4 *)src)[base + u * 256] = v[u];
            }
        }
        __syncthreads();
        if (lane < npx) {
            for (int r = wv; r < nrows; r += 4) {
                const int sh = (int)((uintptr_t)(img + ((size_t)(y_lo + r) * P.iw + x_lo) * 3) & 15);
                const unsigned char *row = src + (size_t)r * P.src_pitch + sh;
                float h[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int kx = 0; kx < 4; kx++) {
                    const unsigned char *px = row + (xo[kx] - x_lo) * 3;
#pragma unroll
                    for (int c = 0; c < 3; c++) h[c] += cx[kx] * fe_u8_unit(px[c]);
                }
                float *hh = hbuf + (r * 64 + lane) * 3;
                hh[0] = h[0]; hh[1] = h[1]; hh[2] = h[2];
            }
        }
        __syncthreads();                                                       // the source bytes are dead: the region is the patch rows now
    }
    for (int i = tid; i < np * (P.kpad - K); i += 256) {                       // the zero columns K .. kpad - 1 of every patch row
        const int pj = i / (P.kpad - K);
        otile[pj * P.kpad + K + (i - pj * (P.kpad - K))] = (T)0.f;
    }
    if (lane < npx) {
        const int cm = colmeta[lane];
        for (int py = wv; py < P.p; py += 4) {
            float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 4; ky++) {
                const int y = ys[py * 4 + ky];
                const float cy = cys[py * 4 + ky];
                float h[3];
                if (staged) {
                    const float *hh = hbuf + ((y - y_lo) * 64 + lane) * 3;
                    h[0] = hh[0]; h[1] = hh[1]; h[2] = hh[2];
                } else {
                    const uint8_t *row = img + (size_t)y * P.iw * 3;
                    h[0] = h[1] = h[2] = 0.f;
#pragma unroll
                    for (int kx = 0; kx < 4; kx++) {
                        const uint8_t *px = row + (size_t)xo[kx] * 3;
#pragma unroll
                        for (int c = 0; c < 3; c++) h[c] += cx[kx] * fe_u8_unit(px[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] += cy * h[c];
            }
            T *q = otile + cm + py * P.p * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) q[c] = (T)((acc[P.flip ? 2 - c : c] - P.mean[c]) * P.istd[c]);
        }
    }
    __syncthreads();
    uint4 *dst = rows + (size_t)(1 + gy * P.gw + gx0) * C8;
    for (int i = tid; i < np * C8; i += 256) dst[i] = ((const uint4 *)otile)[i];
}

DS_API int ds_preprocess_bicubic_rows(ds_ctx *ctx, const void *images, void *rows, int batch, int in_h, int in_w, int out_h, int out_w,
                                      int flip_channels, const float *mean, const float *std, int patch, int n_pad, int kpad,
                                      int dtype, void *stream)
{
    DS_REQUIRE(ctx && images && rows && mean && std, DS_EINVAL, "ds_preprocess_bicubic_rows: null argument");
    DS_REQUIRE(batch > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, DS_EINVAL, "ds_preprocess_bicubic_rows: bad shape");
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_preprocess_bicubic_rows: dtype must be f16 or bf16");
    DS_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, DS_EINVAL, "ds_preprocess_bicubic_rows: std must be non-zero");
    DS_REQUIRE(patch >= 1 && patch <= FE_P_MAX && out_h >= patch && out_w >= patch, DS_EINVAL, "ds_preprocess_bicubic_rows: patch size 1..32, at most the output size");
    const int gh = out_h / patch, gw = out_w / patch;
    DS_REQUIRE(kpad >= 3 * patch * patch && (kpad % 8) == 0 && (long long)n_pad >= 1 + (long long)gh * gw, DS_EINVAL,
               "ds_preprocess_bicubic_rows: kpad must be a multiple of 8 that holds 3 * patch^2 values, n_pad at least 1 + the patch count");
    DS_REQUIRE(((uintptr_t)rows & 15) == 0, DS_EINVAL, "ds_preprocess_bicubic_rows: rows must be 16-byte aligned");
    DS_REQUIRE(gh + 1 <= 65535 && batch <= 65535 && (long long)batch * in_h * in_w * 3 < (1ll << 46) && (long long)in_h * in_w < (1ll << 29),
               DS_EUNSUPPORTED, "ds_preprocess_bicubic_rows: tensor too large");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    RowsParams P;
    P.in = (const uint8_t *)images; P.in_end = P.in + (size_t)batch * in_h * in_w * 3; P.rows = rows;
    P.ih = in_h; P.iw = in_w; P.flip = flip_channels ? 1 : 0;
    P.sy = (float)in_h / (float)out_h; P.sx = (float)in_w / (float)out_w;
    for (int c = 0; c < 3; c++) { P.mean[c] = mean[c]; P.istd[c] = 1.0f / std[c]; }
    P.p = patch; P.gh = gh; P.gw = gw; P.n_pad = n_pad; P.kpad = kpad;
    P.twp = 64 / patch;
    const size_t tables = 64 * 4 * 8 + FE_P_MAX * 4 * 8 + 64 * 4, otile = (size_t)P.twp * kpad * 2;
    DS_REQUIRE(tables + otile <= 48 * 1024, DS_EUNSUPPORTED, "ds_preprocess_bicubic_rows: kpad too large");
    // what the strip's source region can need (the kernel checks the region it actually finds against this room)
    const double need_rows = (double)patch * P.sy + 5.0, need_cols = (double)(P.twp * patch) * P.sx + 5.0;
    size_t lds = tables + otile;
    P.src_rows = 0; P.src_pitch = 0; P.region = (int)otile;
    P.safe = (const uint8_t *)(((uintptr_t)P.in + 15) & ~(uintptr_t)15);
    if (need_rows <= FE_ROWS_MAX && need_cols <= 4096 && P.safe + 16 <= P.in_end) {
        const int nr = (int)need_rows + 1, pitch = (((int)need_cols + 1) * 3 + 30 + 15) & ~15;
        const size_t region = std::max(otile, (size_t)nr * pitch);
        const size_t want = tables + region + (size_t)nr * 64 * 3 * sizeof(float);
        if (want <= 64 * 1024) { P.src_rows = nr; P.src_pitch = pitch; P.region = (int)region; lds = want; }
    }
    dim3 grid((unsigned)((gw + P.twp - 1) / P.twp), (unsigned)(gh + 1), (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DS_DTYPE_F16) hipLaunchKernelGGL((k_preprocess_rows<0>), grid, dim3(256), lds, st, P);
    else hipLaunchKernelGGL((k_preprocess_rows<1>), grid, dim3(256), lds, st, P);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// ds_tokens_fixup: the rows of the patch-embedding GEMM's output that are not patches.  One workgroup per row.
template <int BF16>
__global__ __launch_bounds__(256) void k_tokens_fixup(void *tokens_, const void *cls_, int n_pad, int n_valid, int C8)
{
    const int per = 1 + n_pad - n_valid, b = blockIdx.x / per, k = blockIdx.x - b * per;
    uint4 *dst = (uint4 *)tokens_ + ((size_t)b * n_pad + (k == 0 ? 0 : n_valid + k - 1)) * C8;
    const uint4 *cls = (const uint4 *)cls_;
    for (int i = threadIdx.x; i < C8; i += 256) dst[i] = k == 0 ? cls[i] : make_uint4(0, 0, 0, 0);
}

DS_API int ds_tokens_fixup(ds_ctx *ctx, void *tokens, const void *cls, int batch, int n_pad, int n_valid, int channels, int dtype,
                           void *stream)
{
    DS_REQUIRE(ctx && tokens && cls, DS_EINVAL, "ds_tokens_fixup: null argument");
    DS_REQUIRE(batch > 0 && n_valid >= 1 && n_pad >= n_valid && channels > 0 && (channels % 8) == 0, DS_EINVAL,
               "ds_tokens_fixup: bad shape (channels must be a multiple of 8)");
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_tokens_fixup: dtype must be f16 or bf16");
    DS_REQUIRE(((uintptr_t)tokens & 15) == 0 && ((uintptr_t)cls & 15) == 0, DS_EINVAL, "ds_tokens_fixup: 16-byte alignment");
    DS_REQUIRE((long long)batch * (1 + n_pad - n_valid) < (1ll << 31), DS_EUNSUPPORTED, "ds_tokens_fixup: tensor too large");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    dim3 grid((unsigned)(batch * (1 + n_pad - n_valid)));
    if (dtype == DS_DTYPE_F16) hipLaunchKernelGGL((k_tokens_fixup<0>), grid, dim3(256), 0, (hipStream_t)stream, tokens, cls, n_pad, n_valid, channels / 8);
    else hipLaunchKernelGGL((k_tokens_fixup<1>), grid, dim3(256), 0, (hipStream_t)stream, tokens, cls, n_pad, n_valid, channels / 8);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// ds_upsample_bicubic_to_f32: F.interpolate(pred[:, None], size, mode="bicubic", align_corners=False)[:, 0].float() of a
// half-precision prediction in one pass.  torch's upsample_bicubic2d in its own operation order: per output pixel the four source
// rows are interpolated horizontally (cubic_interp1d with the coefficients of t_x), those four values vertically, float32
// throughout, one rounding to the input type at the end; here the result is widened to float32 in the same store.
//
// Bit identity needs more than the order of the source: torch's kernel is compiled with floating-point contraction on, and WHICH
// multiply-adds were fused decides the last bit.  The forms below are those of upsample_bicubic2d_out_frame<Half / BFloat16, float>
// in torch 2.10 for ROCm 7.0 (gfx950 code object), read off its instructions -- tests/test_gpu_forward_ends.py holds them to it:
//   source index  fma(scale, dst + 0.5, -0.5);   coefficients: every a * x + b of cubic_convolution1 / 2 is one fma
//   x0 c0 + x1 c1 + x2 c2 + x3 c3, "form A":  fma(x3, c3, fma(x2, c2, fma(x0, c0, x1 * c1)))
//                                  "form B":  fma(x3, c3, fma(x2, c2, fma(x1, c1, x0 * c0)))
//   float16:   the four horizontal sums form A, the vertical sum form B;
//   bfloat16:  (the loop over the four rows is vectorised in pairs) the horizontal sums of rows k = 0, 2 form A, of rows
//              k = 1, 3 form B, the vertical sum unfused: ((h0 c0 + h1 c1) + h2 c2) + h3 c3 with four separate products.
// The horizontal sum of (source row, output column) does not depend on the output row -- for bfloat16: only on the parity of the
// tap index k it is used as -- so a workgroup (32 x 64 output pixels) computes it once per source row of its tile in LDS (both
// forms for bfloat16).  Tiles whose source region exceeds the LDS room (downsampling) take their taps from global memory.
#define BT_TH 32
#define BT_TW 64
#define BT_SRC_ROWS 40
#define BT_SRC_COLS 72
struct TailParams {
    const void *in;
    float *out;
    int ih, iw, oh, ow;
    float sy, sx;
};

__device__ __forceinline__ void bt_coeffs(float t, float *c)
{
    const float A = -0.75f;
    const float x1 = t, x0 = x1 + 1.0f, x2 = 1.0f - t, x3 = x2 + 1.0f;
    c[0] = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(A, x0, -5.0f * A), x0, 8.0f * A), x0, -4.0f * A);
    c[1] = __builtin_fmaf(__builtin_fmaf(A + 2.0f, x1, -(A + 3.0f)) * x1, x1, 1.0f);
    c[2] = __builtin_fmaf(__builtin_fmaf(A + 2.0f, x2, -(A + 3.0f)) * x2, x2, 1.0f);
    c[3] = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(A, x3, -5.0f * A), x3, 8.0f * A), x3, -4.0f * A);
}

template <int FORM>      // 0 unfused, 1 form A, 2 form B
__device__ __forceinline__ float bt_interp(float v0, float v1, float v2, float v3, const float *c)
{
    if (FORM == 1) return __builtin_fmaf(v3, c[3], __builtin_fmaf(v2, c[2], __builtin_fmaf(v0, c[0], v1 * c[1])));
    if (FORM == 2) return __builtin_fmaf(v3, c[3], __builtin_fmaf(v2, c[2], __builtin_fmaf(v1, c[1], v0 * c[0])));
    return v0 * c[0] + v1 * c[1] + v2 * c[2] + v3 * c[3];
}

template <int BF16>
__global__ __launch_bounds__(256) void k_upsample_bicubic_f32(TailParams P)
{
    typedef typename fe_traits<BF16>::T T;
    constexpr int NF = BF16 ? 2 : 1;                                           // horizontal forms kept per (source row, column)
    __shared__ int xs[BT_TW * 4], ys[BT_TH * 4];
    __shared__ float cxs[BT_TW * 4], cys[BT_TH * 4];
    __shared__ T src[BT_SRC_ROWS * BT_SRC_COLS];
    __shared__ float hbuf[BT_SRC_ROWS * BT_TW * NF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.z;
    const int ox0 = blockIdx.x * BT_TW, oy0 = blockIdx.y * BT_TH;
    const T *in = (const T *)P.in + (size_t)b * P.ih * P.iw;
    float *out = P.out + (size_t)b * P.oh * P.ow;
    const int ox = ox0 + lane;
    if (P.ih == P.oh && P.iw == P.ow) {                                        // torch copies when the sizes agree
        if (ox < P.ow)
            for (int oy = oy0 + wv; oy < min(oy0 + BT_TH, P.oh); oy += 4) out[(size_t)oy * P.ow + ox] = (float)in[(size_t)oy * P.iw + ox];
        return;
    }
    if (tid < BT_TW) {                                                         // columns past the edge repeat the last one: never stored
        const float f = __builtin_fmaf(P.sx, (float)min(ox0 + tid, P.ow - 1) + 0.5f, -0.5f);
        const int i0 = (int)floorf(f);
        float c[4];
        bt_coeffs(f - (float)i0, c);
#pragma unroll
        for (int k = 0; k < 4; k++) { xs[tid * 4 + k] = max(min(i0 - 1 + k, P.iw - 1), 0); cxs[tid * 4 + k] = c[k]; }
    } else if (tid < BT_TW + BT_TH) {
        const int j = tid - BT_TW;
        const float f = __builtin_fmaf(P.sy, (float)min(oy0 + j, P.oh - 1) + 0.5f, -0.5f);
        const int i0 = (int)floorf(f);
        float c[4];
        bt_coeffs(f - (float)i0, c);
#pragma unroll
        for (int k = 0; k < 4; k++) { ys[j * 4 + k] = max(min(i0 - 1 + k, P.ih - 1), 0); cys[j * 4 + k] = c[k]; }
    }
    __syncthreads();
    const int x_lo = xs[0], x_hi = xs[BT_TW * 4 - 1], y_lo = ys[0], y_hi = ys[BT_TH * 4 - 1];
    const int nrows = y_hi - y_lo + 1, ncols = x_hi - x_lo + 1;
    const bool staged = nrows <= BT_SRC_ROWS && ncols <= BT_SRC_COLS;          // uniform
    int xo[4];
    float cx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { xo[k] = xs[lane * 4 + k]; cx[k] = cxs[lane * 4 + k]; }
    if (staged) {
        for (int r = wv; r < nrows; r += 4)
            for (int c = lane; c < ncols; c += 64) src[r * BT_SRC_COLS + c] = in[(size_t)(y_lo + r) * P.iw + x_lo + c];
        __syncthreads();
        for (int r = wv; r < nrows; r += 4) {
            const T *row = src + r * BT_SRC_COLS;
            const float v0 = (float)row[xo[0] - x_lo], v1 = (float)row[xo[1] - x_lo], v2 = (float)row[xo[2] - x_lo], v3 = (float)row[xo[3] - x_lo];
            hbuf[(r * BT_TW + lane) * NF] = bt_interp<1>(v0, v1, v2, v3, cx);
            if (BF16) hbuf[(r * BT_TW + lane) * NF + NF - 1] = bt_interp<2>(v0, v1, v2, v3, cx);
        }
        __syncthreads();
    }
    if (ox >= P.ow) return;
    for (int j = wv; j < BT_TH; j += 4) {
        const int oy = oy0 + j;
        if (oy >= P.oh) break;
        float h[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int y = ys[j * 4 + k];
            const bool form_b = BF16 && (k & 1);
            if (staged) {
                h[k] = hbuf[((y - y_lo) * BT_TW + lane) * NF + (form_b ? 1 : 0)];
            } else {
                const T *row = in + (size_t)y * P.iw;
                const float v0 = (float)row[xo[0]], v1 = (float)row[xo[1]], v2 = (float)row[xo[2]], v3 = (float)row[xo[3]];
                h[k] = form_b ? bt_interp<2>(v0, v1, v2, v3, cx) : bt_interp<1>(v0, v1, v2, v3, cx);
            }
        }
        const float v = BF16 ? bt_interp<0>(h[0], h[1], h[2], h[3], cys + j * 4) : bt_interp<2>(h[0], h[1], h[2], h[3], cys + j * 4);
        out[(size_t)oy * P.ow + ox] = (float)(T)v;
    }
}

DS_API int ds_upsample_bicubic_to_f32(ds_ctx *ctx, const void *in, void *out, int batch, int in_h, int in_w, int out_h, int out_w,
                                      int dtype, void *stream)
{
    DS_REQUIRE(ctx && in && out, DS_EINVAL, "ds_upsample_bicubic_to_f32: null argument");
    DS_REQUIRE(batch > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, DS_EINVAL, "ds_upsample_bicubic_to_f32: bad shape");
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_upsample_bicubic_to_f32: dtype must be f16 or bf16");
    DS_REQUIRE((out_h + BT_TH - 1) / BT_TH <= 65535 && batch <= 65535, DS_EUNSUPPORTED, "ds_upsample_bicubic_to_f32: tensor too large");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    TailParams P;
    P.in = in; P.out = (float *)out; P.ih = in_h; P.iw = in_w; P.oh = out_h; P.ow = out_w;
    P.sy = (float)in_h / (float)out_h; P.sx = (float)in_w / (float)out_w;
    dim3 grid((unsigned)((out_w + BT_TW - 1) / BT_TW), (unsigned)((out_h + BT_TH - 1) / BT_TH), (unsigned)batch);
    if (dtype == DS_DTYPE_F16) hipLaunchKernelGGL((k_upsample_bicubic_f32<0>), grid, dim3(256), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL((k_upsample_bicubic_f32<1>), grid, dim3(256), 0, (hipStream_t)stream, P);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// ds_im2col3x3_s2_nhwc: rows[(b, oy, ox)][(ky, kx, c)] = x[b][2 * oy + ky - 1][2 * ox + kx - 1][c], outside the map zero (or,
// circular, the pixel on the opposite side) -- the operand of the strided 3x3 convolution as a GEMM.  One workgroup per output
// pixel, 16 bytes per lane; the source map is small (it stays in cache), the 9x larger operand is written once.
__global__ __launch_bounds__(256) void k_im2col3x3_s2(const uint4 *in, uint4 *rows, int h, int w, int C8, int circular)
{
    const int ox = blockIdx.x, oy = blockIdx.y, b = blockIdx.z, ho = gridDim.y, wo = gridDim.x;
    uint4 *dst = rows + (((size_t)b * ho + oy) * wo + ox) * 9 * C8;
    const uint4 *img = in + (size_t)b * h * w * C8;
    for (int i = threadIdx.x; i < 9 * C8; i += 256) {
        const int tap = (int)((unsigned)i / (unsigned)C8), c8 = i - tap * C8, ky = tap / 3, kx = tap - ky * 3;
        int y = 2 * oy + ky - 1, x = 2 * ox + kx - 1;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (circular) {
            y = y < 0 ? h - 1 : (y >= h ? 0 : y);
            x = x < 0 ? w - 1 : (x >= w ? 0 : x);
        }
        if (y >= 0 && y < h && x >= 0 && x < w) v = img[((size_t)y * w + x) * C8 + c8];
        dst[i] = v;
    }
}

DS_API int ds_im2col3x3_s2_nhwc(ds_ctx *ctx, const void *x, void *rows, int batch, int height, int width, int channels, int circular,
                                int dtype, void *stream)
{
    DS_REQUIRE(ctx && x && rows, DS_EINVAL, "ds_im2col3x3_s2_nhwc: null argument");
    DS_REQUIRE(batch > 0 && height > 0 && width > 0 && channels > 0 && (channels % 8) == 0, DS_EINVAL,
               "ds_im2col3x3_s2_nhwc: bad shape (channels must be a multiple of 8)");
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_im2col3x3_s2_nhwc: dtype must be f16 or bf16");
    DS_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)rows & 15) == 0, DS_EINVAL, "ds_im2col3x3_s2_nhwc: 16-byte alignment");
    const int ho = (height - 1) / 2 + 1, wo = (width - 1) / 2 + 1;
    DS_REQUIRE(ho <= 65535 && batch <= 65535 && 9ll * (channels / 8) < (1ll << 30), DS_EUNSUPPORTED, "ds_im2col3x3_s2_nhwc: tensor too large");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_im2col3x3_s2, dim3((unsigned)wo, (unsigned)ho, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                       (const uint4 *)x, (uint4 *)rows, height, width, channels / 8, circular ? 1 : 0);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
