// ds_joint_bilateral_u16: depth refinement -- the joint (cross) bilateral filter of a uint16 depth map GUIDED BY THE RGB IMAGE, on
// gfx950.  The reference has no counterpart (its only remedy for the halo at silhouettes is Boost); the sibling in front of the normal
// map, ds_bilateral_u16 (ds_bilateral.hip), takes its range weight from the depth itself.
//
// Definition (include/depthstereo.h; tests/depth_refine_cases.py is its float64 NumPy model):
//     F(p) = sum_t ws[t] wc[k(q_t, p)] D(q_t)  /  sum_t ws[t] wc[k(q_t, p)],      k(q, p) = |Rq - Rp| + |Gq - Gp| + |Bq - Bp|
//     out(p) = (uint16) rint(F(p))                                                (round half to even; no clamp: F is a convex combination)
// over the (2R+1)^2 taps t in raster order, those with ws[t] == 0 skipped, every product and every sum rounded on its own (no fused
// multiply-add), one IEEE division at the end.  Both tables are made on the host: the argument of the colour weight is an INTEGER in
// 0..765, so no exp runs here and host and device cannot disagree in its last bit.
//
// Kernel: the shape of k_bilateral_u16 -- a 256-thread workgroup owns a 64 x 32 tile of output pixels, eight per thread (rows ty,
// ty + 4, ... of the tile: eight independent accumulation chains per lane hide the latency of the table reads; each chain is ONE
// pixel's, in raster tap order, so a pixel's result depends neither on its tile nor on the batch).  The uint16 depth tile and its
// R-wide halo are staged in LDS once, border rule applied while staging, for every position of the tile whether inside the image or
// not: the tap loop has no bounds test, only the final store is guarded.  New here: the guide is staged NEXT to the depth, same
// positions, as one packed 32-bit word (R, G, B, 0) per position, read from memory byte by byte (with c == 3 a row is not 4-byte
// aligned, and the guide may sit at any address); k(q, p) is then ONE v_sad_u8 of two words.  All 766 entries of wc live in LDS: there
// is no memory path in the tap loop.
//
// LDS, at R = 15: depth 62 x 94 x 2 B = 11.4 KiB, guide 62 x 94 x 4 B = 22.8 KiB, wc 766 x 8 B = 6.0 KiB, ws 962 x 8 B = 7.5 KiB:
// 47.7 KiB per workgroup, so THREE workgroups fit the 160 KiB of a CU (12 waves, 3 per SIMD) -- LDS is what limits occupancy; the
// register budget that goes with 3 waves per SIMD (170 VGPRs) is far above what eight chains need.  At smaller radii the static
// allocation is the same (the arrays are sized for R = 15), so the occupancy is three workgroups at every radius.
// Banks: a wave reads 64 CONSECUTIVE guide words of one tile row per tap and pixel (ds_read_b32: lanes l and l + 32 share a bank but
// sit in different 32-lane groups -- conflict-free at any pitch, so the pitch is simply 64 + 2 RMAX) and 64 consecutive uint16 (two
// lanes per dword: broadcast).  ws[t] is one address for the whole workgroup.  The DATA-DEPENDENT reads are wc[k]: ds_read_b64, bank
// pair (k mod 32), conflicts counted per 32-lane half.  On a photograph neighbouring pixels ask for the same few small k (mostly
// broadcast); on white noise k spreads over ~400 values and a half-wave's 32 reads collide like 32 balls in 32 bins (about 3.5-way on
// average): that, not arithmetic, is the new cost compared with the sibling (DESIGN.md has the measured ratio on both inputs).
#include "ds_common.h"

#pragma clang fp contract(off)      // the definition: product rounded, then sum rounded (the library's build sets it too)

#define JB_TW 64                    // tile width = one wave per tile row
#define JB_TH 32                    // tile height: 8 pixels per thread
#define JB_PPT 8
#define JB_RMAX 15
#define JB_PITCH (JB_TW + 2 * JB_RMAX)
#define JB_ROWS (JB_TH + 2 * JB_RMAX)
#define JB_WC 766                   // 3 * 255 + 1 colour differences

template <int WRAP>
__global__ __launch_bounds__(256) void k_joint_bilateral_u16(const uint16_t *__restrict__ depth, const uint8_t *__restrict__ guide,
                                                             int gc, int h, int w, int radius, const double *__restrict__ ws,
                                                             const double *__restrict__ wc, uint16_t *__restrict__ out)
{
    __shared__ uint32_t gtile[JB_ROWS * JB_PITCH];
    __shared__ uint16_t tile[JB_ROWS * JB_PITCH];
    __shared__ double wc_lds[JB_WC];
    __shared__ double ws_lds[(2 * JB_RMAX + 1) * (2 * JB_RMAX + 1) + 1];        // + 1: the tap loop reads one entry ahead
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * JB_TW, y0 = blockIdx.y * JB_TH;
    const uint16_t *d = depth + (size_t)blockIdx.z * h * w;
    const uint8_t *g = guide + (size_t)blockIdx.z * h * w * gc;
    const int pw = JB_TW + 2 * radius, ph = JB_TH + 2 * radius;          // the staged rectangle, pitch JB_PITCH
    for (int i = tid; i < pw * ph; i += 256) {
        const int ly = i / pw, lx = i - ly * pw;
        const int gy = WRAP ? ds_mod(y0 + ly - radius, h) : ds_reflect101(y0 + ly - radius, h);
        const int gx = WRAP ? ds_mod(x0 + lx - radius, w) : ds_reflect101(x0 + lx - radius, w);
        const size_t at = (size_t)gy * w + gx;
        tile[ly * JB_PITCH + lx] = d[at];
        const uint8_t *px = g + at * gc;                                 // three byte loads: any alignment, the fourth byte never read
        gtile[ly * JB_PITCH + lx] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    }
    for (int i = tid; i < JB_WC; i += 256) wc_lds[i] = wc[i];
    const int side = 2 * radius + 1;
    for (int i = tid; i <= side * side; i += 256) ws_lds[i] = i < side * side ? ws[i] : 0.0;
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6;
    uint32_t c[JB_PPT];
    double num[JB_PPT], den[JB_PPT];
#pragma unroll
    for (int k = 0; k < JB_PPT; k++) {
        c[k] = gtile[(ty + 4 * k + radius) * JB_PITCH + tx + radius];
        num[k] = 0.0;
        den[k] = 0.0;
    }
    double s_next = ws_lds[0];
    for (int dy = 0, t = 0; dy < side; dy++) {
        const uint16_t *row = tile + (ty + dy) * JB_PITCH + tx;
        const uint32_t *grow = gtile + (ty + dy) * JB_PITCH + tx;
        for (int dx = 0; dx < side; dx++) {
            const double s = s_next;                                     // one address for the whole workgroup: a broadcast read,
            s_next = ws_lds[++t];                                        // issued one tap ahead of its use
            if (s == 0.0) continue;
            int q[JB_PPT];
            double r[JB_PPT];
#pragma unroll
            for (int k = 0; k < JB_PPT; k++) {
                q[k] = row[4 * k * JB_PITCH + dx];
                // |Rq - Rp| + |Gq - Gp| + |Bq - Bp| (+ |0 - 0|): one v_sad_u8; 0..765, inside the table by construction
                r[k] = wc_lds[__builtin_amdgcn_sad_u8(grow[4 * k * JB_PITCH + dx], c[k], 0u)];
            }
#pragma unroll
            for (int k = 0; k < JB_PPT; k++) {
                const double wgt = s * r[k];
                const double p = wgt * (double)q[k];
                num[k] = num[k] + p;
                den[k] = den[k] + wgt;
            }
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
    uint16_t *o = out + (size_t)blockIdx.z * h * w;
#pragma unroll
    for (int k = 0; k < JB_PPT; k++) {
        const int y = y0 + ty + 4 * k;
        if (y < h) o[(size_t)y * w + x] = (uint16_t)(unsigned)__builtin_rint(num[k] / den[k]);       // v_rndne_f64: half to even
    }
}

DS_API int ds_joint_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, const uint8_t *guide, int guide_channels, int n, int h, int w,
                                  int radius, const double *ws, const double *wc, int wrap, uint16_t *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && depth && guide && ws && wc && out, DS_EINVAL, "ds_joint_bilateral_u16: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "ds_joint_bilateral_u16: bad shape n=%d h=%d w=%d", n, h, w);
    DS_REQUIRE(guide_channels == 3 || guide_channels == 4, DS_EINVAL, "ds_joint_bilateral_u16: guide_channels %d not 3 or 4", guide_channels);
    DS_REQUIRE(radius >= 1 && radius <= JB_RMAX, DS_EINVAL, "ds_joint_bilateral_u16: radius %d outside 1..%d", radius, JB_RMAX);
    DS_REQUIRE(wrap || radius < (h < w ? h : w), DS_EINVAL,
               "ds_joint_bilateral_u16: BORDER_REFLECT_101 needs radius < min(h, w) (radius=%d h=%d w=%d); wrap takes any size", radius, h, w);
    DS_REQUIRE((((uintptr_t)ws | (uintptr_t)wc) & 7) == 0 && ((((uintptr_t)depth) | (uintptr_t)out) & 1) == 0, DS_EINVAL,
               "ds_joint_bilateral_u16: ws and wc must be 8-byte aligned, depth and out 2-byte aligned");
    const size_t bytes = (size_t)n * h * w * sizeof(uint16_t);
    DS_REQUIRE((uintptr_t)out + bytes <= (uintptr_t)depth || (uintptr_t)depth + bytes <= (uintptr_t)out, DS_EINVAL,
               "ds_joint_bilateral_u16: out overlaps depth");
    dim3 grid((w + JB_TW - 1) / JB_TW, (h + JB_TH - 1) / JB_TH, n);
    DS_REQUIRE(n <= 65535 && grid.y <= 65535, DS_EUNSUPPORTED, "ds_joint_bilateral_u16: n and h / %d must be <= 65535", JB_TH);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_DEPTH_REFINE, stream);
    if (wrap) hipLaunchKernelGGL(k_joint_bilateral_u16<1>, grid, dim3(256), 0, stream, depth, guide, guide_channels, h, w, radius, ws, wc, out);
    else hipLaunchKernelGGL(k_joint_bilateral_u16<0>, grid, dim3(256), 0, stream, depth, guide, guide_channels, h, w, radius, ws, wc, out);
    ds_kt_end(ctx, DS_KT_DEPTH_REFINE, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
