// Ambient-occlusion maps from uint16 depth maps on gfx950: the horizon scan of ds_aomap_u16.  The reference has no counterpart; the
// definition is the comment of ds_aomap_u16 in include/depthstereo.h, tests/aomap_cases.py is its NumPy model, and the kernel gives the
// model's bits.
//
// Per pixel and ray the kernel keeps the best tap so far as (bn^2, bd) and, per tap, decides  D^2 * bd > bn^2 * d2  with D = max(H(q) -
// H(p), 0): a tap that does not rise has D = 0 and 0 > x never holds for x >= 0, so "rises" needs no test of its own, and with the
// start (bn, bd) = (0, 1) the first rising tap wins by the same compare.  Both products are below 2^43 and are formed in float64, where
// every factor and every product is an exact integer (D^2 < 2^32, bd and d2 <= 1024): three v_mul_f64, one conversion and one compare
// per tap and pixel, and no 64-bit integer multiply.  bn is recovered at the end of the ray as sqrt(bn^2), exact for a perfect square
// below 2^32.  Then the handful of float64 operations of the definition, each rounded on its own (-ffp-contract=off; division and sqrt
// are the correctly rounded expansions).
//
// k_aomap_u16: a 256-thread workgroup owns a 64 x 32 tile of output pixels, eight per thread (rows ty, ty + 4, ... of the tile, the
// layout of bl_tile in ds_bilateral.hip: eight independent compare chains per lane, one LDS address computation per tap for all
// eight, the row distance folded into the read's immediate offset).  The tile of H and its R-wide halo are staged in LDS once, invert
// applied while staging.  Without wrap a position outside the image is staged as height 0: then D = 0 there and the tap never takes
// part, so the tap loop has no bounds test.  With wrap the staged index is taken modulo the size.  The pitch is fixed (64 + 2 * 32
// uint16 = 256 B): a wave reads 64 consecutive uint16 of one row per tap and pixel (two lanes per dword: broadcast, no bank conflict
// at any offset).
// The ray table is staged in LDS too, as the tap's LDS offset dy * pitch + dx and its d2 as a float64; both are one address for the
// whole workgroup (broadcast reads; the source reads one tap ahead, the compiler issues them at the head of the tap).  While staging, dx and dy are clamped to -R..R and the start
// indices to 0..AO_MAX_TAPS: whatever the table holds, every LDS read stays inside the staged rectangle.
//
// Tile shape and its cost.  64 x 32, eight pixels per lane: the once-per-tap work is shared by eight pixel-taps.  At R = 32 it stages
// 128 x 96 uint16 = 24 KiB (+ 6 KiB of ray table) and reads every pixel of the map 6 times from L2 (12 B per pixel of a pass that computes
// up to 448 taps per pixel: nothing; a 64 x 8 tile would read it 18 times, nothing either).  The cost is parallelism: LDS admits 5
// workgroups per CU, one fewer than the registers (profiles/aomap_resources.txt), and ONE 1024 x 1024 map is only 512 workgroups, two per
// CU: measured, a map costs 1.36-1.46 times as much alone as in a batch of eight.
// Bound: vector issue.  Per tap and pixel one ds_read_u16 and ten VALU instructions, five of them float64 (DESIGN.md 3.23 has the
// measured time per pixel and tap).
#include "ds_common.h"

#define AO_TW 64                    // tile width = one wave per tile row
#define AO_TH 32                    // tile height: 8 pixels per thread
#define AO_PPT 8
#define AO_RMAX 32
#define AO_PITCH (AO_TW + 2 * AO_RMAX)
#define AO_ROWS (AO_TH + 2 * AO_RMAX)
#define AO_MAX_TAPS (16 * AO_RMAX)  // directions * radius bounds the table

template <int WRAP>
__global__ __launch_bounds__(256) void k_aomap_u16(const uint16_t *__restrict__ depth, int h, int w, int radius, int directions,
                                                   const int32_t *__restrict__ taps, const int32_t *__restrict__ dir_start, double z,
                                                   double c, int invert, uint8_t *__restrict__ out_u8, double *__restrict__ out_f64)
{
    __shared__ uint16_t tile[AO_ROWS * AO_PITCH];
    __shared__ double d2_lds[AO_MAX_TAPS + 1];                           // + 1: the tap loop reads one entry ahead
    __shared__ int off_lds[AO_MAX_TAPS + 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * AO_TW, y0 = blockIdx.y * AO_TH;
    const uint16_t *d = depth + (size_t)blockIdx.z * h * w;
    const int pw = AO_TW + 2 * radius, ph = AO_TH + 2 * radius;          // the staged rectangle, pitch AO_PITCH
    {
        const int lx = tid & (AO_PITCH - 1);                             // a thread stages one column, every second row
        int gx = x0 + lx - radius;
        const bool in_x = WRAP || (gx >= 0 && gx < w);
        if (WRAP) gx = ds_mod(gx, w);
        if (lx < pw) {
            for (int ly = tid / AO_PITCH; ly < ph; ly += 256 / AO_PITCH) {
                int gy = y0 + ly - radius;
                uint16_t v = 0;
                if (WRAP) gy = ds_mod(gy, h);
                if (in_x && gy >= 0 && gy < h) {
                    v = d[(size_t)gy * w + gx];
                    if (invert) v = (uint16_t)(65535 - v);
                }
                tile[ly * AO_PITCH + lx] = v;
            }
        }
    }
    const int last = dir_start[directions];
    const int ntaps = last < 0 ? 0 : last > AO_MAX_TAPS ? AO_MAX_TAPS : last;
    for (int i = tid; i <= AO_MAX_TAPS; i += 256) {
        int dx = 0, dy = 0;
        if (i < ntaps) {
            dx = taps[2 * i];
            dy = taps[2 * i + 1];
            dx = dx < -radius ? -radius : dx > radius ? radius : dx;
            dy = dy < -radius ? -radius : dy > radius ? radius : dy;
        }
        off_lds[i] = dy * AO_PITCH + dx;
        d2_lds[i] = (double)(dx * dx + dy * dy);
    }
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6;
    const uint16_t *centre = tile + (ty + radius) * AO_PITCH + tx + radius;
    uint16_t hc[AO_PPT];
    double sum[AO_PPT];
#pragma unroll
    for (int k = 0; k < AO_PPT; k++) {
        hc[k] = centre[4 * k * AO_PITCH];
        sum[k] = 0.0;
    }
    for (int ray = 0; ray < directions; ray++) {
        int t = dir_start[ray], t_end = dir_start[ray + 1];
        t = t < 0 ? 0 : t > ntaps ? ntaps : t;
        t_end = t_end < t ? t : t_end > ntaps ? ntaps : t_end;
        double bn2[AO_PPT], bd[AO_PPT];
#pragma unroll
        for (int k = 0; k < AO_PPT; k++) {
            bn2[k] = 0.0;
            bd[k] = 1.0;
        }
        int off_next = off_lds[t];
        double d2_next = d2_lds[t];
        while (t < t_end) {
            const uint16_t *q = centre + off_next;
            const double d2 = d2_next;
            t++;
            off_next = off_lds[t];
            d2_next = d2_lds[t];
            uint16_t hq[AO_PPT];
#pragma unroll
            for (int k = 0; k < AO_PPT; k++) hq[k] = q[4 * k * AO_PITCH];                // eight reads in flight, then the arithmetic
#pragma unroll
            for (int k = 0; k < AO_PPT; k++) {
                const double rise = (double)__builtin_elementwise_sub_sat(hq[k], hc[k]);  // max(H(q) - H(p), 0)
                const double rise2 = rise * rise;                                        // exact: below 2^32
                const bool better = rise2 * bd[k] > bn2[k] * d2;                         // exact: below 2^43; strict, so the earlier tap keeps a tie
                bn2[k] = better ? rise2 : bn2[k];
                bd[k] = better ? d2 : bd[k];
            }
        }
#pragma unroll
        for (int k = 0; k < AO_PPT; k++) {
            const double a = sqrt(bn2[k]) * z;                                           // sqrt of a perfect square: bn itself
            sum[k] = sum[k] + a / sqrt(bd[k] + a * a);
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
    const size_t image = (size_t)blockIdx.z * h * w;
#pragma unroll
    for (int k = 0; k < AO_PPT; k++) {
        const int y = y0 + ty + 4 * k;
        if (y >= h) continue;
        const double v = 1.0 - sum[k] * c;
        const size_t at = image + (size_t)y * w + x;
        if (out_f64) out_f64[at] = v;
        out_u8[at] = (uint8_t)(int)__builtin_rint(255.0 * fmin(fmax(v, 0.0), 1.0));
    }
}

static bool ao_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

DS_API int ds_aomap_u16(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int radius, int directions, const int32_t *taps,
                        const int32_t *dir_start, double z, double c, int invert, int wrap, uint8_t *out_u8, double *out_f64,
                        void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && depth && taps && dir_start && out_u8, DS_EINVAL, "ds_aomap_u16: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "ds_aomap_u16: bad shape n=%d h=%d w=%d", n, h, w);
    DS_REQUIRE(radius >= 1 && radius <= AO_RMAX, DS_EINVAL, "ds_aomap_u16: radius %d outside 1..%d", radius, AO_RMAX);
    DS_REQUIRE(directions == 4 || directions == 8 || directions == 16, DS_EINVAL, "ds_aomap_u16: directions %d not 4, 8 or 16", directions);
    DS_REQUIRE(z > 0.0 && z <= 1.7976931348623157e308 && c > 0.0 && c <= 1.7976931348623157e308, DS_EINVAL,
               "ds_aomap_u16: z and c must be finite and > 0, got %g and %g", z, c);
    DS_REQUIRE((((uintptr_t)taps | (uintptr_t)dir_start) & 3) == 0 && ((uintptr_t)depth & 1) == 0 && ((uintptr_t)out_f64 & 7) == 0, DS_EINVAL,
               "ds_aomap_u16: taps and dir_start must be 4-byte aligned, depth 2-byte aligned, out_f64 8-byte aligned");
    const size_t count = (size_t)n * h * w;
    DS_REQUIRE(!ao_overlap(out_u8, count, depth, count * sizeof(uint16_t))
                   && !(out_f64 && (ao_overlap(out_f64, count * sizeof(double), depth, count * sizeof(uint16_t))
                                    || ao_overlap(out_f64, count * sizeof(double), out_u8, count))),
               DS_EINVAL, "ds_aomap_u16: an output overlaps depth or the other output");
    const dim3 grid((w + AO_TW - 1) / AO_TW, (h + AO_TH - 1) / AO_TH, n);
    DS_REQUIRE(n <= 65535 && grid.y <= 65535, DS_EUNSUPPORTED, "ds_aomap_u16: n and h / %d must be <= 65535", AO_TH);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_AOMAP, stream);
    if (wrap) hipLaunchKernelGGL(k_aomap_u16<1>, grid, dim3(256), 0, stream, depth, h, w, radius, directions, taps, dir_start, z, c, invert, out_u8, out_f64);
    else hipLaunchKernelGGL(k_aomap_u16<0>, grid, dim3(256), 0, stream, depth, h, w, radius, directions, taps, dir_start, z, c, invert, out_u8, out_f64);
    ds_kt_end(ctx, DS_KT_AOMAP, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
