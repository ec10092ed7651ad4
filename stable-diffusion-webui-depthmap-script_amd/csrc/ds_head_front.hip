// ds_dpt_head_front: the front of the DPT depth heads in ONE kernel --
//     out = conv3x3(upsample_bilinear(x, (out_h, out_w), align_corners=True), w) + bias          (256 -> 128 channels in the heads)
// refinenet1's final x2 upsample and the head's first convolution (dmidas/dpt_depth.py:150, ddepth_anything_v2/.../dpt.py:89-90).
// As two launches (k_upsample_bilinear_nhwc, then k_linear256<CONV 1, NH 1>) the upsampled map -- 1.07 GB at the benchmark's
// shapes -- is written once and gathered nine times; here a tile of it exists only in LDS.
//
// The result is bit-identical to ds_upsample_bilinear_nhwc followed by ds_conv3x3_nhwc:
//   * an upsampled value is hf_lerp4 below: the expression of k_upsample_bilinear_nhwc, copied (four float32 products, each rounded,
//     added left to right, one rounding to the activation type; the library is built with -ffp-contract=off, so nothing is fused).
//     NOT hts_lerp4 of ds_encoder_ops.hip: that one is a chain of three fused multiply-adds and gives other bits, so the two cannot
//     share a helper without changing one of them.  Weights and source indices are formed as that kernel forms them.
//   * positions of the halo outside the upsampled image are literal zeros in LDS (the convolution's zero padding), never products
//     with zero weights: a NaN or Inf source pixel stays where the upsample kernel would have put it.
//   * the accumulation chain of an output element is k_linear256<CONV 1>'s, term for term: zero float32 accumulator, 64-channel chunks
//     ascending, inside a chunk taps 0 .. 8, inside a tap four v_mfma_f32_32x32x16 over 16-channel slices ascending with the weights as
//     the first operand and a lane's eight channels at 16 ks + 8 (lane >> 5); then + bias in float32 and one rounding.
//
// Structure.  A workgroup of 8 waves owns a tile of 8 x 32 output pixels and all 128 output channels; wave (pg, wch) = 2 rows x 32
// pixels and 64 channels: four 32 x 32 accumulators.  The workgroup is persistent and walks (tile, chunk) steps; per step the
// upsampled patch of the tile (10 x 34 pixels x 64 channels, pixel pitch 144 bytes: the fragment reads of 32 consecutive pixels are
// conflict-free without a swizzle) is read from LDS while the patch of the NEXT step is interpolated into the other buffer, one
// 16-byte item per thread in six of the step's nine taps, out of a staging tile of the source pixels (6 x 18 pixels x 128 bytes)
// that was fetched two steps ahead through registers.  The 16 KB weight tile of a (chunk, tap) is staged two taps ahead into a ring
// of three with the swizzle of k_linear256.  One barrier per tap; the fragments of a tap's first two k steps are read during the
// tap before it, so the MFMAs start right behind the barrier.  LDS: 2 x 48 960 + 3 x 16 384 + 13 824 = 160 896 bytes.
//   read-after-write: what tap g reads was written before the barrier that ends tap g - 2 (weights: written in tap g - 2, first read
//     in tap g - 1), the barrier that ends tap 6 of the previous step (patch) or tap 0 of this step (staging tile);
//   write-after-read: the weight slot written in tap g was last read in tap g - 1, the patch buffer written in step q in step q - 1,
//     the staging tile written in tap 0 of step q in taps 1 .. 6 of step q - 1 -- each with a barrier in between.
// Workgroup -> tile order is XCD-aware as in k_linear256: the workgroups of one XCD walk a contiguous range of the tile list, 32
// neighbouring tiles at a time, so the halos they share and the weights stay in one L2.
#include "ds_common.h"

#include <algorithm>

typedef _Float16 hf_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 hf_bf16x8 __attribute__((ext_vector_type(8)));
typedef float hf_f32x16 __attribute__((ext_vector_type(16)));

template <int BF16> struct hf_traits;
template <> struct hf_traits<0> {
    typedef _Float16 T; typedef hf_f16x8 V8;
    static __device__ __forceinline__ hf_f32x16 mfma(V8 a, V8 b, hf_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct hf_traits<1> {
    typedef __bf16 T; typedef hf_bf16x8 V8;
    static __device__ __forceinline__ hf_f32x16 mfma(V8 a, V8 b, hf_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

#define HF_TH 8
#define HF_TW 32
#define HF_PH (HF_TH + 2)
#define HF_PW (HF_TW + 2)
#define HF_PIXB 144                                   // 128 bytes of a chunk's 64 channels + 16: consecutive pixels start 36 banks apart
#define HF_PATCH_BYTES (HF_PH * HF_PW * HF_PIXB)
#define HF_W_BYTES 16384                              // 128 output channels x 64 input channels of one (chunk, tap)
#define HF_SRC_ROWS 6                                 // source pixels under 10 x 34 upsampled ones at a scale factor of 2 and above:
#define HF_SRC_COLS 18                                // s (t0 - 1) = t0 / 2 - 1/2 - d, + 9 s < 9/2: 4 + 2 rows; + 33 s < 33/2: 16 + 2 columns
#define HF_SRC_PIECES (HF_SRC_ROWS * HF_SRC_COLS * 8)
#define HF_SRC_LOADS ((HF_SRC_PIECES + 511) / 512)
#define HF_OFF_W (2 * HF_PATCH_BYTES)
#define HF_W_RING 3
#define HF_OFF_SRC (HF_OFF_W + HF_W_RING * HF_W_BYTES)
#define HF_LDS_BYTES (HF_OFF_SRC + HF_SRC_PIECES * 16)
#define HF_ITEMS (HF_PH * HF_PW * 8)                  // 16-byte items of a patch
#define HF_NIT ((HF_ITEMS + 511) / 512)               // per thread: 6, one in each of taps 1 .. 6
static_assert(HF_OFF_W % 128 == 0 && HF_OFF_SRC % 16 == 0 && HF_LDS_BYTES <= 160 * 1024, "LDS map");
static_assert(HF_NIT == 6 && HF_SRC_LOADS == 2 && HF_SRC_PIECES > 512, "the tap schedule below places six items and two loads");

struct HeadFrontParams {
    const void *x, *w, *bias;
    void *out;
    int ih, iw, oh, ow;
    int C, nc;                                         // input channels, 64-channel chunks
    float sy, sx;
    int tiles_x, tiles_per_img, ntiles;
};

__device__ __forceinline__ void hf_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// The upsampled value of eight channels: k_upsample_bilinear_nhwc's statement (a, b = row y0 at x0, x1; c, d = row y1).
template <int BF16>
__device__ __forceinline__ uint4 hf_lerp4(const uint4 &a, const uint4 &b, const uint4 &c, const uint4 &d, float w00, float w01, float w10, float w11)
{
    typedef typename hf_traits<BF16>::T T;
    union { uint4 q; T h[8]; } A, B, C, D, O;
    A.q = a; B.q = b; C.q = c; D.q = d;
#pragma unroll
    for (int k = 0; k < 8; k++)
        O.h[k] = (T)(w00 * (float)A.h[k] + w01 * (float)B.h[k] + w10 * (float)C.h[k] + w11 * (float)D.h[k]);
    return O.q;
}

// where a step of the walk works: image, tile origin, chunk, and the first source row / column of its staging tile
struct HfStep {
    int valid, b, ty0, tx0, c, ylo, xlo;
};
// the staging tile's pieces of one thread (named registers, not an array: carried across the step loop an array stays in scratch memory)
struct HfSrc { uint4 r0, r1; };

template <int BF16>
__global__ __launch_bounds__(512) void k_dpt_head_front(HeadFrontParams P)
{
    typedef hf_traits<BF16> TR;
    typedef typename TR::T T;
    typedef typename TR::V8 V8;
    extern __shared__ __attribute__((aligned(128))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = wave >> 1, wch = wave & 1;                            // rows 2 pg, 2 pg + 1 of the tile; output channels 64 wch ..

    const int grid = (int)gridDim.x;
    const int mine = (P.ntiles - (int)blockIdx.x + grid - 1) / grid;     // tiles of this workgroup
    const int nsteps = mine * P.nc;
    const int pixb = P.C * 2;                                            // bytes of a source pixel

    // step q of this workgroup = chunk q % nc of its tile q / nc; position orig of the XCD-aware tile list (k_linear256's set_tile)
    auto step_of = [&](const int q) -> HfStep {
        HfStep S;
        S.valid = q < nsteps;
        const int qq = S.valid ? q : 0;
        const int k = qq / P.nc;
        S.c = qq - k * P.nc;
        const int orig = (int)blockIdx.x + k * grid;
        const int xcd = orig & 7, q8 = P.ntiles >> 3, r8 = P.ntiles & 7;
        const int tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
        S.b = tile / P.tiles_per_img;
        const int rem = tile - S.b * P.tiles_per_img, tyi = rem / P.tiles_x;
        S.ty0 = tyi * HF_TH;
        S.tx0 = (rem - tyi * P.tiles_x) * HF_TW;
        S.ylo = min((int)(P.sy * max(S.ty0 - 1, 0)), P.ih - 1);
        S.xlo = min((int)(P.sx * max(S.tx0 - 1, 0)), P.iw - 1);
        return S;
    };

    // ---- producers ------------------------------------------------------------------------------------------------------------
    // the staging tile of step S: piece id = pixel (r, cx) of the tile x 16-byte slot, addresses clamped into the image
    auto src_load1 = [&](const unsigned char *xb, const HfStep &S, const int m) -> uint4 {
        const int id = min(tid + 512 * m, HF_SRC_PIECES - 1);            // (the last load of most threads is a duplicate, dropped by src_write)
        const int slot = id & 7, pix = id >> 3, r = pix / HF_SRC_COLS, cx = pix - r * HF_SRC_COLS;
        const int y = min(S.ylo + r, P.ih - 1), x = min(S.xlo + cx, P.iw - 1);
        return *reinterpret_cast<const uint4 *>(xb + ((size_t)y * P.iw + x) * pixb + slot * 16);
    };
    auto src_load = [&](const HfStep &S, HfSrc &R) {
        const unsigned char *xb = (const unsigned char *)P.x + (size_t)S.b * P.ih * P.iw * pixb + S.c * 128;
        R.r0 = src_load1(xb, S, 0); R.r1 = src_load1(xb, S, 1);
    };
    auto src_write = [&](const HfSrc &R) {
        uint4 *d = reinterpret_cast<uint4 *>(lds + HF_OFF_SRC) + tid;
        d[0] = R.r0;
        if (tid + 512 < HF_SRC_PIECES) d[512] = R.r1;
    };
    // item j of this thread: 16 bytes (8 channels) of patch pixel (prow, pcol) of step S, out of the staging tile
    auto lerp_item = [&](const HfStep &S, const int j, unsigned char *patch) {
        const int i = tid + 512 * j;
        if (i >= HF_ITEMS) return;
        const int slot = i & 7, p = i >> 3, prow = p / HF_PW, pcol = p - prow * HF_PW;
        const int oy = S.ty0 - 1 + prow, ox = S.tx0 - 1 + pcol;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);                            // outside the upsampled image: the zero padding itself
        if (oy >= 0 && oy < P.oh && ox >= 0 && ox < P.ow) {
            const float fy = P.sy * oy, fx = P.sx * ox;
            const int y0 = min((int)fy, P.ih - 1), y1 = min(y0 + 1, P.ih - 1);
            const int x0 = min((int)fx, P.iw - 1), x1 = min(x0 + 1, P.iw - 1);
            const float ty = fy - y0, tx = fx - x0;
            const float w00 = (1.f - ty) * (1.f - tx), w01 = (1.f - ty) * tx, w10 = ty * (1.f - tx), w11 = ty * tx;
            const unsigned char *s = lds + HF_OFF_SRC + slot * 16;
            const int r0 = (y0 - S.ylo) * HF_SRC_COLS, r1 = (y1 - S.ylo) * HF_SRC_COLS, c0 = x0 - S.xlo, c1 = x1 - S.xlo;
            const uint4 a = *reinterpret_cast<const uint4 *>(s + (r0 + c0) * 128), b = *reinterpret_cast<const uint4 *>(s + (r0 + c1) * 128);
            const uint4 c = *reinterpret_cast<const uint4 *>(s + (r1 + c0) * 128), d = *reinterpret_cast<const uint4 *>(s + (r1 + c1) * 128);
            o = hf_lerp4<BF16>(a, b, c, d, w00, w01, w10, w11);
        }
        *reinterpret_cast<uint4 *>(patch + p * HF_PIXB + slot * 16) = o;
    };
    // the weight tile of (chunk, tap): this thread's two 16-byte pieces, rows n = tid / 8 and + 64; LDS slot ^= (n >> 1) & 7
    const int wn = tid >> 3, wslot = tid & 7;
    const unsigned wdst = (unsigned)(wn * 128 + ((wslot ^ ((wn >> 1) & 7)) << 4));       // (row + 64: the same swizzle)
    auto w_load = [&](const int c, const int tap, uint4 (&WR)[2]) {
        const unsigned char *wb = (const unsigned char *)P.w + ((size_t)tap * P.C + c * 64) * 2 + wslot * 16;
#pragma unroll
        for (int i = 0; i < 2; i++) WR[i] = *reinterpret_cast<const uint4 *>(wb + (size_t)(wn + 64 * i) * 9 * pixb);
    };
    auto w_write = [&](const uint4 (&WR)[2], const int ring) {
#pragma unroll
        for (int i = 0; i < 2; i++) *reinterpret_cast<uint4 *>(lds + HF_OFF_W + ring * HF_W_BYTES + wdst + i * 8192) = WR[i];
    };

    // ---- consumers: fragment addresses ----------------------------------------------------------------------------------------
    const unsigned a_lane = (unsigned)((2 * pg * HF_PW + l31) * HF_PIXB + hi * 16);       // + ((r + dy + 1) * 34 + dx + 1) * 144 + ks * 32
    const unsigned w_lane = HF_OFF_W + (unsigned)((wch * 64 + l31) * 128);                // + nb * 4096 + woff[ks]
    unsigned woff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) woff[ks] = (unsigned)(((2 * ks + hi) ^ ((l31 >> 1) & 7)) << 4);

    if (nsteps <= 0) return;
    HfSrc R;
    uint4 WR[2];
    hf_f32x16 acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][nb][e] = 0.f;

    // one tap's fragments of k steps ks0, ks0 + 1: weights of ring slot `slot`, activations of the patch at pap for tap t
    auto read_frags = [&](V8 (&fw)[2][2], V8 (&fa)[2][2], const int slot, const unsigned char *pap, const int t, const int ks0) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        const unsigned char *pw = lds + w_lane + slot * HF_W_BYTES;
#pragma unroll
        for (int k = 0; k < 2; k++) {
#pragma unroll
            for (int nb = 0; nb < 2; nb++) fw[nb][k] = *reinterpret_cast<const V8 *>(pw + nb * 4096 + woff[ks0 + k]);
#pragma unroll
            for (int r = 0; r < 2; r++) fa[r][k] = *reinterpret_cast<const V8 *>(pap + ((r + dy + 1) * HF_PW + dx + 1) * HF_PIXB + (ks0 + k) * 32);
        }
    };

    // ---- prologue: patch of step 0, weights of (chunk 0, taps 0 and 1), the first fragments, source pixels of step 1 in flight ------
    HfStep cur = step_of(0);
    src_load(cur, R);
    w_load(0, 0, WR);
    src_write(R);
    w_write(WR, 0);
    w_load(0, 1, WR);
    w_write(WR, 1);
    hf_barrier();
#pragma unroll
    for (int j = 0; j < HF_NIT; j++) lerp_item(cur, j, lds);
    hf_barrier();
    HfStep nxt = step_of(1);
    if (nxt.valid) src_load(nxt, R);
    V8 fw01[2][2], fa01[2][2];                                           // k steps 0, 1 of the tap to come: read one tap ahead, across its barrier
    read_frags(fw01, fa01, 0, lds + a_lane, 0, 0);

    for (int q = 0; q < nsteps; q++) {
        const unsigned char *pa = lds + (q & 1) * HF_PATCH_BYTES + a_lane;
        const unsigned char *pa1 = lds + ((q + 1) & 1) * HF_PATCH_BYTES + a_lane;
        unsigned char *pnext = lds + ((q + 1) & 1) * HF_PATCH_BYTES;
        const int cnext = cur.c + 1 < P.nc ? cur.c + 1 : 0;              // the chunk of the next step (the weights do not depend on the tile)
#pragma unroll
        for (int t = 0; t < 9; t++) {
            // Tap g = 9 q + t reads weight slot g % 3 = t % 3.  The weights of tap g + 2 are loaded now and written at the end of this tap
            // into slot (t + 2) % 3, whose last reader was tap g - 1; taps 7 and 8 fetch taps 0 and 1 of the next step's chunk (loaded even
            // where no step follows).
            if (t < 7) w_load(cur.c, t + 2, WR);
            else w_load(cnext, t - 7, WR);
            if (t == 0 && nxt.valid) src_write(R);                       // the staging tile of step q + 1 (loaded in tap 1 of step q - 1)
            if (t == 1) {                                                // right behind that write: eight taps for the loads to land (HBM latency)
                const HfStep nn = step_of(q + 2);
                if (nn.valid) src_load(nn, R);
            }
            // k steps 2, 3 of this tap are read under the MFMAs of k steps 0, 1, whose fragments came across the barrier; k steps 0, 1 of
            // the NEXT tap (its weights were written in tap g - 1, its patch is complete since tap 6 of the previous step) under the rest
            V8 fw23[2][2], fa23[2][2], fwn[2][2], fan[2][2];
            read_frags(fw23, fa23, t % 3, pa, t, 2);
#pragma unroll
            for (int k = 0; k < 2; k++)
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int nb = 0; nb < 2; nb++) acc[r][nb] = TR::mfma(fw01[nb][k], fa01[r][k], acc[r][nb]);
            if (t >= 1 && t <= HF_NIT && nxt.valid) lerp_item(nxt, t - 1, pnext);
            read_frags(fwn, fan, (t + 1) % 3, t < 8 ? pa : pa1, (t + 1) % 9, 0);
#pragma unroll
            for (int k = 0; k < 2; k++)
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int nb = 0; nb < 2; nb++) acc[r][nb] = TR::mfma(fw23[nb][k], fa23[r][k], acc[r][nb]);
            w_write(WR, (t + 2) % 3);
#pragma unroll
            for (int k = 0; k < 2; k++)
#pragma unroll
                for (int i = 0; i < 2; i++) { fw01[i][k] = fwn[i][k]; fa01[i][k] = fan[i][k]; }
            hf_barrier();
        }
        if (cur.c == P.nc - 1) {
            // ---- epilogue: k_linear256's -- one v_permlane32_swap per register pair gives a lane 8 consecutive channels of its pixel
            const int ox = cur.tx0 + l31;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int oy = cur.ty0 + 2 * pg + r;
                T *orow = (T *)P.out + (((size_t)cur.b * P.oh + oy) * P.ow + ox) * 128;
#pragma unroll
                for (int nb = 0; nb < 2; nb++)
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const int n0 = wch * 64 + nb * 32 + 16 * k + 8 * hi;
                        V8 bv;
                        if (P.bias) bv = *reinterpret_cast<const V8 *>((const T *)P.bias + n0);
                        else {
#pragma unroll
                            for (int e = 0; e < 8; e++) bv[e] = (T)0.f;
                        }
                        float v[8];
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float f0 = acc[r][nb][8 * k + e], f1 = acc[r][nb][8 * k + 4 + e];
                            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(f0), __float_as_uint(f1), false, false);
                            v[e] = __uint_as_float(sw[0]);
                            v[4 + e] = __uint_as_float(sw[1]);
                        }
                        V8 o;
#pragma unroll
                        for (int e = 0; e < 8; e++) o[e] = (T)(v[e] + (float)bv[e]);
                        if (oy < P.oh && ox < P.ow) *reinterpret_cast<V8 *>(orow + n0) = o;
                    }
            }
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int nb = 0; nb < 2; nb++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[r][nb][e] = 0.f;
        }
        cur = nxt;
        nxt = step_of(q + 2);
    }
}

// 1 where every tile's source pixels fit the staging tile (the device's arithmetic, the extremes of each tile row / column)
static int hf_fits(int in_n, int out_n, float s, int tile, int rows)
{
    for (int t0 = 0; t0 < out_n; t0 += tile) {
        const int lo = std::min((int)(s * std::max(t0 - 1, 0)), in_n - 1);
        const int last = std::min(t0 + tile, out_n - 1);
        const int hi1 = std::min(std::min((int)(s * last), in_n - 1) + 1, in_n - 1);
        if (hi1 - lo > rows - 1) return 0;
    }
    return 1;
}

DS_API int ds_dpt_head_front(ds_ctx *ctx, const void *x, const void *w, const void *bias, void *out, int batch, int in_h, int in_w,
                             int out_h, int out_w, int in_channels, int out_channels, int dtype, void *stream)
{
    DS_REQUIRE(ctx && x && w && out, DS_EINVAL, "ds_dpt_head_front: null argument");
    DS_REQUIRE(batch > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && in_channels > 0 && out_channels > 0, DS_EINVAL,
               "ds_dpt_head_front: bad shape");
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_dpt_head_front: dtype must be f16 or bf16");
    DS_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)bias & 15) == 0, DS_EINVAL,
               "ds_dpt_head_front: x, w, bias and out must be 16-byte aligned");
    DS_REQUIRE(out_channels == 128 && in_channels % 64 == 0 && in_channels <= 4096, DS_EUNSUPPORTED,
               "ds_dpt_head_front: built for out_channels == 128 and in_channels %% 64 == 0 (<= 4096), got %d -> %d", in_channels, out_channels);
    DS_REQUIRE(in_h < 32768 && in_w < 32768 && out_h < 32768 && out_w < 32768, DS_EUNSUPPORTED, "ds_dpt_head_front: image too large");
    HeadFrontParams P;
    P.x = x; P.w = w; P.bias = bias; P.out = out;
    P.ih = in_h; P.iw = in_w; P.oh = out_h; P.ow = out_w; P.C = in_channels; P.nc = in_channels / 64;
    P.sy = out_h > 1 ? (float)(in_h - 1) / (float)(out_h - 1) : 0.f;          // as ds_upsample_bilinear_nhwc forms them
    P.sx = out_w > 1 ? (float)(in_w - 1) / (float)(out_w - 1) : 0.f;
    DS_REQUIRE(hf_fits(in_h, out_h, P.sy, HF_TH, HF_SRC_ROWS) && hf_fits(in_w, out_w, P.sx, HF_TW, HF_SRC_COLS), DS_EUNSUPPORTED,
               "ds_dpt_head_front: the upsample factor is below what the staging tile holds (%d x %d -> %d x %d)", in_h, in_w, out_h, out_w);
    P.tiles_x = (out_w + HF_TW - 1) / HF_TW;
    P.tiles_per_img = P.tiles_x * ((out_h + HF_TH - 1) / HF_TH);
    const long long nt = (long long)P.tiles_per_img * batch;
    DS_REQUIRE(nt * P.nc < (1ll << 30), DS_EUNSUPPORTED, "ds_dpt_head_front: too many tiles");
    P.ntiles = (int)nt;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->ncu) {
        int ncu = 0;
        DS_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->ncu = ncu >= 8 ? ncu / 8 * 8 : 8;
    }
    const int grid = (int)std::min<long long>(ctx->ncu, nt);                 // one workgroup per CU; fewer tiles: one tile each
    if (dtype == DS_DTYPE_F16) {
        DS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dpt_head_front<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)HF_LDS_BYTES));
        hipLaunchKernelGGL((k_dpt_head_front<0>), dim3(grid), dim3(512), HF_LDS_BYTES, (hipStream_t)stream, P);
    } else {
        DS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_dpt_head_front<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)HF_LDS_BYTES));
        hipLaunchKernelGGL((k_dpt_head_front<1>), dim3(grid), dim3(512), HF_LDS_BYTES, (hipStream_t)stream, P);
    }
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
