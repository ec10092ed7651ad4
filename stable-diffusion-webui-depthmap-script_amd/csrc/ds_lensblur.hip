// Lens blur from depth on gfx950: the depth-of-field gather of ds_lensblur_u8.  The reference has no counterpart; the definition is the
// comment of ds_lensblur_u8 in include/depthstereo.h, tests/lensblur_cases.py is its NumPy model, and the kernel gives the model's bits.
// Every sum of the definition is an integer sum, so the kernel may visit the taps in any order and leave out taps that cannot count.
//
// k_lensblur_u8<RCAP>: a 256-thread workgroup owns a 64 x 32 tile of output pixels, eight per thread (rows ty, ty + 4, ... of the tile,
// the layout of bl_tile in ds_bilateral.hip and of k_aomap_u16: one LDS address per tap for all eight, the row distance in the read's
// immediate offset).  The tile and its R-wide halo are staged in LDS once, 6 bytes per position: a uint32 rgb | rho << 24 and a uint16
// z; rho is computed while staging, invert applied to z there.  A position outside the image is staged as rho = 0: a tap counts iff
// 16 d2 <= rho_e^2 with rho_e <= rho(q), so such a position can count only as its own self tap, and a pixel outside the image is
// never written.  The tap loop therefore has no bounds test.
// The tap test is  rho_e >= t(dx, dy),  t = the least integer with t^2 >= 16 d2: a byte table over (|dx|, |dy|), computed while staging
// and read at one address by the whole workgroup.  W[rho_e] is a gather from the 4 R + 1 weights staged next to it (masked to 24 bits,
// so the three products are v_mul_u32_u24 whatever the table holds; rho_e is computed here and is never above 4 R, so no value of the
// uploaded table is used as an address).
// Taps that cannot count are left out: the workgroup takes the largest rho it staged, rho_max, and visits only the taps with
// 16 d2 <= rho_max^2 -- row by row, the span of dx from an integer square root.  A tile whose pixels and halo are all in focus
// (rho_max < 4) visits the self tap alone.
//
// RCAP is the largest radius an instantiation serves (8, 16, 32): the static LDS arrays are sized by it -- 23, 37 and 74 KiB -- so a
// small radius is not held to the two workgroups per CU that R = 32 allows (profiles/lensblur_resources.txt).
// Accumulators: den and three numerators per pixel, uint32; the header derives num < 2,066,455,740 < 2^31, so 2 num + den < 2^32 too.
#include "ds_common.h"

#define LB_TW 64                    // tile width = one wave per tile row
#ifndef LB_TH
#define LB_TH 32                    // tile height: 8 pixels per thread (-DLB_TH=16: the other shape DESIGN.md 3.24 measures; same bits)
#endif
#define LB_PPT (LB_TH / 4)
#define LB_RMAX 32

__device__ __forceinline__ int lb_floor_sqrt(int v)                  // the largest t with t^2 <= v, 0 <= v < 2^24
{
    int t = (int)sqrtf((float)v);
    while (t * t > v) t--;
    while ((t + 1) * (t + 1) <= v) t++;
    return t;
}

template <int RCAP>
__global__ __launch_bounds__(256) void k_lensblur_u8(const uint8_t *__restrict__ image, const uint16_t *__restrict__ depth,
                                                     const uint16_t *__restrict__ focus, int h, int w, int radius, uint32_t aperture,
                                                     uint32_t band, int invert, const uint32_t *__restrict__ table,
                                                     uint8_t *__restrict__ out_rgb, uint8_t *__restrict__ out_coc)
{
    constexpr int PITCH = LB_TW + 2 * RCAP;
    constexpr int ROWS = LB_TH + 2 * RCAP;
    constexpr int TSIDE = RCAP + 1;
    __shared__ uint32_t px[ROWS * PITCH];                                // rgb | rho << 24
    __shared__ uint16_t zz[ROWS * PITCH];                                // nearness
    __shared__ uint32_t wt[4 * RCAP + 1];                                // W[rho], 24 bits
    __shared__ uint8_t thr[TSIDE * TSIDE];                               // the least t with t^2 >= 16 (dx^2 + dy^2), at [|dy|][|dx|]
    __shared__ int rho_max_lds;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * LB_TW, y0 = blockIdx.y * LB_TH;
    const size_t first = (size_t)blockIdx.z * h * w;
    if (tid == 0) rho_max_lds = 0;
    __syncthreads();
    {
        const uint32_t f = focus[blockIdx.z];
        const uint32_t rho_cap = 4u * (uint32_t)radius;
        const int pw = LB_TW + 2 * radius, ph = LB_TH + 2 * radius;     // the staged rectangle, pitch PITCH
        uint32_t seen = 0;
        for (int i = tid; i < ph * PITCH; i += 256) {
            const int ly = i / PITCH, lx = i - ly * PITCH;
            if (lx >= pw) continue;
            const int gx = x0 + lx - radius, gy = y0 + ly - radius;
            uint32_t a = 0;
            uint16_t z = 0;
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const size_t at = first + (size_t)gy * w + gx;
                const uint32_t d = depth[at];
                const uint32_t diff = d > f ? d - f : f - d;
                const uint32_t e = diff > band ? diff - band : 0u;
                uint32_t rho = (e * aperture + 32768u) >> 16;            // e * aperture + 32768 < 2^32
                rho = rho < rho_cap ? rho : rho_cap;
                const uint8_t *c = image + 3 * at;
                a = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | rho << 24;
                z = (uint16_t)(invert ? 65535u - d : d);
                seen = rho > seen ? rho : seen;
            }
            px[i] = a;
            zz[i] = z;
        }
        atomicMax(&rho_max_lds, (int)seen);
        for (int i = tid; i <= 4 * RCAP; i += 256) wt[i] = i <= 4 * radius ? table[i] & 0xffffffu : 0u;
        for (int i = tid; i < TSIDE * TSIDE; i += 256) {
            const int ay = i / TSIDE, ax = i - ay * TSIDE;
            const int v = 16 * (ax * ax + ay * ay);
            thr[i] = (uint8_t)(v ? lb_floor_sqrt(v - 1) + 1 : 0);       // at most ceil(4 sqrt(2) 32) = 182
        }
    }
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6;
    const int centre = (ty + radius) * PITCH + tx + radius;
    uint32_t zp[LB_PPT], rp[LB_PPT], den[LB_PPT], nr[LB_PPT], ng[LB_PPT], nb[LB_PPT];
#pragma unroll
    for (int k = 0; k < LB_PPT; k++) {
        rp[k] = px[centre + 4 * k * PITCH] >> 24;
        zp[k] = zz[centre + 4 * k * PITCH];
        den[k] = nr[k] = ng[k] = nb[k] = 0;
    }
    const int rho_max = __builtin_amdgcn_readfirstlane(rho_max_lds);     // <= 4 radius: computed above, not read from the table
    const int reach = rho_max >> 2;                                      // the window: |dy| <= reach <= radius
    const int lim = (rho_max * rho_max) >> 4;                            // and dx^2 + dy^2 <= lim
    for (int dy = -reach; dy <= reach; dy++) {
        const int span = lb_floor_sqrt(lim - dy * dy);
        const uint8_t *trow = thr + (dy < 0 ? -dy : dy) * TSIDE;
        for (int dx = -span; dx <= span; dx++) {
            const uint32_t t = trow[dx < 0 ? -dx : dx];
            const int q = centre + dy * PITCH + dx;
            uint32_t a[LB_PPT], z[LB_PPT], re[LB_PPT], wv[LB_PPT];
#pragma unroll
            for (int k = 0; k < LB_PPT; k++) {                           // the reads in flight first, then the arithmetic
                a[k] = px[q + 4 * k * PITCH];
                z[k] = zz[q + 4 * k * PITCH];
            }
#pragma unroll
            for (int k = 0; k < LB_PPT; k++) {
                const uint32_t rq = a[k] >> 24;
                const uint32_t rmin = rq < rp[k] ? rq : rp[k];
                re[k] = z[k] < zp[k] ? rmin : rq;                        // a farther pixel reaches p only as far as p's own blur
                wv[k] = wt[re[k]];
            }
#pragma unroll
            for (int k = 0; k < LB_PPT; k++) {
                const uint32_t wk = re[k] >= t ? wv[k] : 0u;             // 16 d2 <= rho_e^2
                den[k] += wk;
                nr[k] += __umul24(wk, a[k] & 255u);
                ng[k] += __umul24(wk, (a[k] >> 8) & 255u);
                nb[k] += __umul24(wk, (a[k] >> 16) & 255u);
            }
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
#pragma unroll
    for (int k = 0; k < LB_PPT; k++) {
        const int y = y0 + ty + 4 * k;
        if (y >= h) continue;
        const size_t at = first + (size_t)y * w + x;
        const uint32_t d = den[k] ? den[k] : 1u;                         // the self tap always counts; 0 only with a table of zeros
        uint8_t *o = out_rgb + 3 * at;
        o[0] = (uint8_t)((2u * nr[k] + d) / (2u * d));
        o[1] = (uint8_t)((2u * ng[k] + d) / (2u * d));
        o[2] = (uint8_t)((2u * nb[k] + d) / (2u * d));
        if (out_coc) out_coc[at] = (uint8_t)rp[k];
    }
}

static bool lb_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

DS_API int ds_lensblur_u8(ds_ctx *ctx, const uint8_t *image, const uint16_t *depth, const uint16_t *focus, int n, int h, int w,
                          int radius, int aperture, int band, int invert, const uint32_t *table, uint8_t *out_rgb, uint8_t *out_coc,
                          void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && image && depth && focus && table && out_rgb, DS_EINVAL, "ds_lensblur_u8: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "ds_lensblur_u8: bad shape n=%d h=%d w=%d", n, h, w);
    DS_REQUIRE(radius >= 1 && radius <= LB_RMAX, DS_EINVAL, "ds_lensblur_u8: radius %d outside 1..%d", radius, LB_RMAX);
    DS_REQUIRE(aperture >= 1 && aperture <= 65535, DS_EINVAL, "ds_lensblur_u8: aperture %d outside 1..65535", aperture);
    DS_REQUIRE(band >= 0 && band <= 65535, DS_EINVAL, "ds_lensblur_u8: band %d outside 0..65535", band);
    DS_REQUIRE(((uintptr_t)table & 3) == 0 && (((uintptr_t)focus | (uintptr_t)depth) & 1) == 0, DS_EINVAL,
               "ds_lensblur_u8: table must be 4-byte aligned, focus and depth 2-byte aligned");
    const size_t count = (size_t)n * h * w;
    const void *in[4] = {image, depth, focus, table};
    const size_t in_bytes[4] = {3 * count, 2 * count, 2 * (size_t)n, (4 * (size_t)radius + 1) * sizeof(uint32_t)};
    for (int i = 0; i < 4; i++)
        DS_REQUIRE(!lb_overlap(out_rgb, 3 * count, in[i], in_bytes[i]) && !(out_coc && lb_overlap(out_coc, count, in[i], in_bytes[i])),
                   DS_EINVAL, "ds_lensblur_u8: an output overlaps an input");
    DS_REQUIRE(!(out_coc && lb_overlap(out_coc, count, out_rgb, 3 * count)), DS_EINVAL, "ds_lensblur_u8: the outputs overlap");
    const dim3 grid((w + LB_TW - 1) / LB_TW, (h + LB_TH - 1) / LB_TH, n);
    DS_REQUIRE(n <= 65535 && grid.y <= 65535, DS_EUNSUPPORTED, "ds_lensblur_u8: n and h / %d must be <= 65535", LB_TH);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    auto kernel = radius <= 8 ? k_lensblur_u8<8> : radius <= 16 ? k_lensblur_u8<16> : k_lensblur_u8<LB_RMAX>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, image, depth, focus, h, w, radius, (uint32_t)aperture, (uint32_t)band, invert,
                       table, out_rgb, out_coc);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
