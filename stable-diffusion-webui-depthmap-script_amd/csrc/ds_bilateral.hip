// The two spatial bilateral filters of uint16 depth maps on gfx950, ONE tile routine (bl_tile) instantiated twice:
//   ds_bilateral_u16        the edge-preserving pre-filter of the normal-map chain (16-bit deflickering; the reference leaves it as a
//                           TODO, src/normalmap_generation.py:17).  The range weight comes from the depth itself; float64 out.
//   ds_joint_bilateral_u16  depth refinement: the joint (cross) filter GUIDED BY THE RGB IMAGE.  The reference has no counterpart (its
//                           only remedy for the halo at silhouettes is Boost); uint16 out.
//
// Definition (include/depthstereo.h; tests/normalmap_bilateral_cases.py and tests/depth_refine_cases.py are its float64 NumPy models):
//     F(p) = sum_t ws[t] W(q_t, p) D(q_t)  /  sum_t ws[t] W(q_t, p)
//     unguided: W(q, p) = wr[|D(q) - D(p)|],  out(p) = F(p)
//     guided:   W(q, p) = wc[|Rq - Rp| + |Gq - Gp| + |Bq - Bp|],  out(p) = (uint16) rint(F(p))
// over the (2R+1)^2 taps t in raster order; the skipped taps, the unfused rounding, the division and the final rounding are the
// family's rules (ds_bilateral.h).  All tables are made on the host: the argument of W is an INTEGER, so no exp runs here and host and
// device cannot disagree in its last bit.
//
// bl_tile: a 256-thread workgroup owns a 64 x 32 tile of output pixels, eight per thread (rows ty, ty + 4, ... of the tile: eight
// independent accumulation chains per lane hide the latency of the table reads; each chain is ONE pixel's, in raster tap order, so a
// pixel's result depends neither on its tile nor on the batch).  The uint16 tile and its R-wide halo are staged in LDS once, border
// rule applied while staging (BORDER_REFLECT_101, or index modulo size), for every position of the tile whether inside the image or
// not: the tap loop has no bounds test, only the final store is guarded.  ws is staged in LDS too: ws[t] is one address for the whole
// workgroup (a broadcast read, issued one tap ahead).  What differs between the two, at compile time (GUIDED):
//   * the key of a tap.  Unguided: the depth itself, |q - c| is one v_sad_u16.  Guided: the guide is staged NEXT to the depth, same
//     positions, as one packed word per position (ds_bl_rgb: with c == 3 a row is not 4-byte aligned, and the guide may sit at any
//     address); the key difference is one v_sad_u8 of two words.
//   * where the weight is read.  Unguided: the range table's first BL_WR_LDS entries are copied to LDS, the rest is read from memory,
//     by the lanes that need it: neighbouring pixels of a depth map ask for neighbouring (small) entries, so on a depth map nearly
//     every read is an LDS read, and only lanes at a silhouette go to memory; same bits either way.  Guided: all DS_BL_WC entries of wc
//     live in LDS, there is no memory path in the tap loop.
//   * what is stored: the float64 quotient, or ds_bl_finish_u16 of it.
//
// Unguided, bound: float64 vector issue.  Per tap and pixel the definition needs 3 float64 operations (wgt, wgt * v, the sum) -- the
// kernel issues 5 (+ den, + the uint16 -> float64 conversion of v), about as many integer ones and two LDS reads (DESIGN.md 3.16 has
// the measured multiple of the bound, on a depth-map-like input and on white noise, whose every range read goes to memory).
//
// Guided, LDS at R = 15: depth 62 x 94 x 2 B = 11.4 KiB, guide 62 x 94 x 4 B = 22.8 KiB, wc DS_BL_WC x 8 B = 6.0 KiB, ws 962 x 8 B = 7.5 KiB:
// 47.7 KiB per workgroup, so THREE workgroups fit the 160 KiB of a CU (12 waves, 3 per SIMD) -- LDS is what limits occupancy; the
// register budget that goes with 3 waves per SIMD (170 VGPRs) is far above what eight chains need.  At smaller radii the static
// allocation is the same (the arrays are sized for R = 15), so the occupancy is three workgroups at every radius.
// Banks: a wave reads 64 CONSECUTIVE guide words of one tile row per tap and pixel (ds_read_b32: lanes l and l + 32 share a bank but
// sit in different 32-lane groups -- conflict-free at any pitch, so the pitch is simply 64 + 2 RMAX) and 64 consecutive uint16 (two
// lanes per dword: broadcast).  ws[t] is one address for the whole workgroup.  The DATA-DEPENDENT reads are wc[k]: ds_read_b64, bank
// pair (k mod 32), conflicts counted per 32-lane half.  On a photograph neighbouring pixels ask for the same few small k (mostly
// broadcast); on white noise k spreads over ~400 values and a half-wave's 32 reads collide like 32 balls in 32 bins (about 3.5-way on
// average): that, not arithmetic, is the cost the guide adds (DESIGN.md 3.19 has the measured ratio on both inputs).
#include "ds_bilateral.h"

#define BL_TW 64                    // tile width = one wave per tile row
#define BL_TH 32                    // tile height: 8 pixels per thread
#define BL_PPT 8
#define BL_RMAX 15
#define BL_PITCH (BL_TW + 2 * BL_RMAX)
#define BL_ROWS (BL_TH + 2 * BL_RMAX)
#define BL_WR_LDS 2048              // unguided: leading entries of wr kept in LDS (16 KiB)

// gtile: BL_ROWS * BL_PITCH words of LDS for the staged guide (GUIDED), else unused.  wtab: wc (GUIDED) or wr.
template <int WRAP, bool GUIDED, typename OUT>
__device__ __forceinline__ void bl_tile(const uint16_t *__restrict__ depth, const uint8_t *__restrict__ guide, int gc, uint32_t *gtile,
                                        int h, int w, int radius, const double *__restrict__ ws, const double *__restrict__ wtab,
                                        OUT *__restrict__ out)
{
    __shared__ uint16_t tile[BL_ROWS * BL_PITCH];
    __shared__ double wtab_lds[GUIDED ? DS_BL_WC : BL_WR_LDS];
    __shared__ double ws_lds[(2 * BL_RMAX + 1) * (2 * BL_RMAX + 1) + 1];        // + 1: the tap loop reads one entry ahead
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * BL_TW, y0 = blockIdx.y * BL_TH;
    const uint16_t *d = depth + (size_t)blockIdx.z * h * w;
    const uint8_t *g = GUIDED ? guide + (size_t)blockIdx.z * h * w * gc : nullptr;
    const int pw = BL_TW + 2 * radius, ph = BL_TH + 2 * radius;          // the staged rectangle, pitch BL_PITCH
    for (int i = tid; i < pw * ph; i += 256) {
        const int ly = i / pw, lx = i - ly * pw;
        const int gy = WRAP ? ds_mod(y0 + ly - radius, h) : ds_reflect101(y0 + ly - radius, h);
        const int gx = WRAP ? ds_mod(x0 + lx - radius, w) : ds_reflect101(x0 + lx - radius, w);
        const size_t at = (size_t)gy * w + gx;
        tile[ly * BL_PITCH + lx] = d[at];
        if constexpr (GUIDED) gtile[ly * BL_PITCH + lx] = ds_bl_rgb(g + at * gc);
    }
    if constexpr (GUIDED) ds_bl_stage_wc(wtab_lds, wtab, tid, 256);
    else for (int i = tid; i < BL_WR_LDS; i += 256) wtab_lds[i] = wtab[i];
    const int side = 2 * radius + 1;
    for (int i = tid; i <= side * side; i += 256) ws_lds[i] = i < side * side ? ws[i] : 0.0;
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6;
    uint32_t c[BL_PPT];                                                  // the centre's key: its depth, or its guide word
    double num[BL_PPT], den[BL_PPT];
#pragma unroll
    for (int k = 0; k < BL_PPT; k++) {
        const int at = (ty + 4 * k + radius) * BL_PITCH + tx + radius;
        if constexpr (GUIDED) c[k] = gtile[at];
        else c[k] = tile[at];
        num[k] = 0.0;
        den[k] = 0.0;
    }
    double s_next = ws_lds[0];
    for (int dy = 0, t = 0; dy < side; dy++) {
        const uint16_t *row = tile + (ty + dy) * BL_PITCH + tx;
        const uint32_t *grow = GUIDED ? gtile + (ty + dy) * BL_PITCH + tx : nullptr;
        for (int dx = 0; dx < side; dx++) {
            const double s = s_next;                                     // one address for the whole workgroup: a broadcast read,
            s_next = ws_lds[++t];                                        // issued one tap ahead of its use
            if (s == 0.0) continue;
            int q[BL_PPT];
            double r[BL_PPT];
            if constexpr (GUIDED) {
#pragma unroll
                for (int k = 0; k < BL_PPT; k++) {
                    q[k] = row[4 * k * BL_PITCH + dx];
                    r[k] = wtab_lds[__builtin_amdgcn_sad_u8(grow[4 * k * BL_PITCH + dx], c[k], 0u)];
                }
            } else {
                int a[BL_PPT], far = 0;
#pragma unroll
                for (int k = 0; k < BL_PPT; k++) {
                    q[k] = row[4 * k * BL_PITCH + dx];
                    a[k] = (int)__builtin_amdgcn_sad_u16((unsigned)q[k], c[k], 0u);
                    far |= a[k];
                }
                // The range weights: from the LDS slice, unconditionally (index masked into it), and -- only in a lane one of whose
                // eight differences lies beyond the slice -- from memory, all eight.  Two plain loads in two address spaces: a
                // `cond ? wtab_lds[a] : wtab[a]` becomes ONE flat load of a selected pointer, which is slower than either.
#pragma unroll
                for (int k = 0; k < BL_PPT; k++) r[k] = wtab_lds[a[k] & (BL_WR_LDS - 1)];
                if (far >= BL_WR_LDS) {                                  // BL_WR_LDS is a power of two: the OR reaches it iff one does
#pragma unroll
                    for (int k = 0; k < BL_PPT; k++) r[k] = wtab[a[k]];
                }
            }
#pragma unroll
            for (int k = 0; k < BL_PPT; k++) ds_bl_tap(s, r[k], q[k], num[k], den[k]);
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
    OUT *o = out + (size_t)blockIdx.z * h * w;
#pragma unroll
    for (int k = 0; k < BL_PPT; k++) {
        const int y = y0 + ty + 4 * k;
        if (y >= h) continue;
        if constexpr (GUIDED) o[(size_t)y * w + x] = ds_bl_finish_u16(num[k], den[k]);
        else o[(size_t)y * w + x] = num[k] / den[k];
    }
}

template <int WRAP>
__global__ __launch_bounds__(256) void k_bilateral_u16(const uint16_t *__restrict__ depth, int h, int w, int radius,
                                                       const double *__restrict__ ws, const double *__restrict__ wr,
                                                       double *__restrict__ out)
{
    bl_tile<WRAP, false>(depth, nullptr, 0, nullptr, h, w, radius, ws, wr, out);
}

template <int WRAP>
__global__ __launch_bounds__(256) void k_joint_bilateral_u16(const uint16_t *__restrict__ depth, const uint8_t *__restrict__ guide,
                                                             int gc, int h, int w, int radius, const double *__restrict__ ws,
                                                             const double *__restrict__ wc, uint16_t *__restrict__ out)
{
    __shared__ uint32_t gtile[BL_ROWS * BL_PITCH];
    bl_tile<WRAP, true>(depth, guide, gc, gtile, h, w, radius, ws, wc, out);
}

// The launch-argument check of both entry points (`name` opens every message; wtab_name: "wr" or "wc"; out_size: bytes per output
// element, which is also the alignment out needs) and the launch grid.
static int bl_check_launch(const char *name, const char *wtab_name, const ds_ctx *ctx, const void *depth, const void *ws, const void *wtab,
                           const void *out, size_t out_size, int n, int h, int w, int radius, int wrap, dim3 *grid)
{
    DS_REQUIRE(ctx && depth && ws && wtab && out, DS_EINVAL, "%s: null argument", name);
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "%s: bad shape n=%d h=%d w=%d", name, n, h, w);
    DS_REQUIRE(radius >= 1 && radius <= BL_RMAX, DS_EINVAL, "%s: radius %d outside 1..%d", name, radius, BL_RMAX);
    DS_REQUIRE(wrap || radius < (h < w ? h : w), DS_EINVAL,
               "%s: BORDER_REFLECT_101 needs radius < min(h, w) (radius=%d h=%d w=%d); wrap takes any size", name, radius, h, w);
    DS_REQUIRE((((uintptr_t)ws | (uintptr_t)wtab) & 7) == 0 && ((uintptr_t)depth & 1) == 0 && ((uintptr_t)out & (out_size - 1)) == 0, DS_EINVAL,
               "%s: ws and %s must be 8-byte aligned, depth 2-byte aligned, out %d-byte aligned", name, wtab_name, (int)out_size);
    const size_t count = (size_t)n * h * w;
    DS_REQUIRE((uintptr_t)out + count * out_size <= (uintptr_t)depth || (uintptr_t)depth + count * sizeof(uint16_t) <= (uintptr_t)out,
               DS_EINVAL, "%s: out overlaps depth", name);
    *grid = dim3((w + BL_TW - 1) / BL_TW, (h + BL_TH - 1) / BL_TH, n);
    DS_REQUIRE(n <= 65535 && grid->y <= 65535, DS_EUNSUPPORTED, "%s: n and h / %d must be <= 65535", name, BL_TH);
    return DS_OK;
}

DS_API int ds_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int radius, const double *ws, const double *wr,
                            int wrap, double *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    dim3 grid;
    const int rc = bl_check_launch("ds_bilateral_u16", "wr", ctx, depth, ws, wr, out, sizeof(double), n, h, w, radius, wrap, &grid);
    if (rc != DS_OK) return rc;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_NORMALMAP, stream);
    if (wrap) hipLaunchKernelGGL(k_bilateral_u16<1>, grid, dim3(256), 0, stream, depth, h, w, radius, ws, wr, out);
    else hipLaunchKernelGGL(k_bilateral_u16<0>, grid, dim3(256), 0, stream, depth, h, w, radius, ws, wr, out);
    ds_kt_end(ctx, DS_KT_NORMALMAP, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_joint_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, const uint8_t *guide, int guide_channels, int n, int h, int w,
                                  int radius, const double *ws, const double *wc, int wrap, uint16_t *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(guide, DS_EINVAL, "ds_joint_bilateral_u16: null argument");
    DS_REQUIRE(guide_channels == 3 || guide_channels == 4, DS_EINVAL, "ds_joint_bilateral_u16: guide_channels %d not 3 or 4", guide_channels);
    dim3 grid;
    const int rc = bl_check_launch("ds_joint_bilateral_u16", "wc", ctx, depth, ws, wc, out, sizeof(uint16_t), n, h, w, radius, wrap, &grid);
    if (rc != DS_OK) return rc;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_DEPTH_REFINE, stream);
    if (wrap) hipLaunchKernelGGL(k_joint_bilateral_u16<1>, grid, dim3(256), 0, stream, depth, guide, guide_channels, h, w, radius, ws, wc, out);
    else hipLaunchKernelGGL(k_joint_bilateral_u16<0>, grid, dim3(256), 0, stream, depth, guide, guide_channels, h, w, radius, ws, wc, out);
    ds_kt_end(ctx, DS_KT_DEPTH_REFINE, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
