// ds_bilateral_u16: the edge-preserving pre-filter of the normal-map chain (16-bit deflickering; the reference leaves it as a TODO,
// src/normalmap_generation.py:17) on gfx950.
//
// Definition (include/depthstereo.h; tests/normalmap_bilateral_cases.py is its float64 NumPy model):
//     F(p) = sum_t ws[t] wr[|D(q_t) - D(p)|] D(q_t)  /  sum_t ws[t] wr[|D(q_t) - D(p)|]
// over the (2R+1)^2 taps t in raster order, those with ws[t] == 0 skipped, every product and every sum rounded on its own (no fused
// multiply-add), one IEEE division at the end.  Both tables are made on the host: the argument of the range weight is an INTEGER, so
// no exp runs here and host and device cannot disagree in its last bit.
//
// Kernel: a 256-thread workgroup owns a 64 x 32 tile of output pixels, eight per thread (rows ty, ty + 4, ... of the tile: eight
// independent accumulation chains per lane hide the latency of the table reads; each chain is ONE pixel's, in raster tap order, so a
// pixel's result depends neither on its tile nor on the batch).  The uint16 tile and its R-wide halo are staged in LDS once, border
// rule applied while staging (BORDER_REFLECT_101, or index modulo size), for every position of the tile whether inside the image or
// not: the tap loop has no bounds test, only the final store is guarded.  ws is staged in LDS too: ws[t] is one address for the whole
// workgroup (a broadcast read, issued one tap ahead).  The range table's first BL_WR_LDS entries are copied to LDS, the rest is read
// from memory, by the lanes that need it: neighbouring pixels of a depth map ask for neighbouring (small) entries, so on a depth map
// nearly every read is an LDS read, and only lanes at a silhouette go to memory; same bits either way.
//
// Bound: float64 vector issue.  Per tap and pixel the definition needs 3 float64 operations (wgt, wgt * v, the sum) -- the kernel
// issues 5 (+ den, + the uint16 -> float64 conversion of v), about as many integer ones and two LDS reads (DESIGN.md 3.16 has the
// measured multiple of the bound, on a depth-map-like input and on white noise, whose every range read goes to memory).
#include "ds_common.h"

#pragma clang fp contract(off)      // the definition: product rounded, then sum rounded (the library's build sets it too)

#define BL_TW 64                    // tile width = one wave per tile row
#define BL_TH 32                    // tile height: 8 pixels per thread
#define BL_PPT 8
#define BL_RMAX 15
#define BL_PITCH (BL_TW + 2 * BL_RMAX)
#define BL_ROWS (BL_TH + 2 * BL_RMAX)
#define BL_WR_LDS 2048              // leading entries of wr kept in LDS (16 KiB)

template <int WRAP>
__global__ __launch_bounds__(256) void k_bilateral_u16(const uint16_t *__restrict__ depth, int h, int w, int radius,
                                                       const double *__restrict__ ws, const double *__restrict__ wr,
                                                       double *__restrict__ out)
{
    __shared__ uint16_t tile[BL_ROWS * BL_PITCH];
    __shared__ double wr_lds[BL_WR_LDS];
    __shared__ double ws_lds[(2 * BL_RMAX + 1) * (2 * BL_RMAX + 1) + 1];        // + 1: the tap loop reads one entry ahead
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * BL_TW, y0 = blockIdx.y * BL_TH;
    const uint16_t *d = depth + (size_t)blockIdx.z * h * w;
    const int pw = BL_TW + 2 * radius, ph = BL_TH + 2 * radius;          // the staged rectangle, pitch BL_PITCH
    for (int i = tid; i < pw * ph; i += 256) {
        const int ly = i / pw, lx = i - ly * pw;
        const int gy = WRAP ? ds_mod(y0 + ly - radius, h) : ds_reflect101(y0 + ly - radius, h);
        const int gx = WRAP ? ds_mod(x0 + lx - radius, w) : ds_reflect101(x0 + lx - radius, w);
        tile[ly * BL_PITCH + lx] = d[(size_t)gy * w + gx];
    }
    for (int i = tid; i < BL_WR_LDS; i += 256) wr_lds[i] = wr[i];
    const int side = 2 * radius + 1;
    for (int i = tid; i <= side * side; i += 256) ws_lds[i] = i < side * side ? ws[i] : 0.0;
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6;
    int c[BL_PPT];
    double num[BL_PPT], den[BL_PPT];
#pragma unroll
    for (int k = 0; k < BL_PPT; k++) {
        c[k] = tile[(ty + 4 * k + radius) * BL_PITCH + tx + radius];
        num[k] = 0.0;
        den[k] = 0.0;
    }
    double s_next = ws_lds[0];
    for (int dy = 0, t = 0; dy < side; dy++) {
        const uint16_t *row = tile + (ty + dy) * BL_PITCH + tx;
        for (int dx = 0; dx < side; dx++) {
            const double s = s_next;                                     // one address for the whole workgroup: a broadcast read,
            s_next = ws_lds[++t];                                        // issued one tap ahead of its use
            if (s == 0.0) continue;
            int q[BL_PPT], a[BL_PPT], far = 0;
#pragma unroll
            for (int k = 0; k < BL_PPT; k++) {
                q[k] = row[4 * k * BL_PITCH + dx];
                a[k] = (int)__builtin_amdgcn_sad_u16((unsigned)q[k], (unsigned)c[k], 0u);        // |q - c|: one v_sad_u16
                far |= a[k];
            }
            // The range weights: from the LDS slice, unconditionally (index masked into it), and -- only in a lane one of whose
            // eight differences lies beyond the slice -- from memory, all eight.  Two plain loads in two address spaces: a
            // `cond ? wr_lds[a] : wr[a]` becomes ONE flat load of a selected pointer, which is slower than either.
            double r[BL_PPT];
#pragma unroll
            for (int k = 0; k < BL_PPT; k++) r[k] = wr_lds[a[k] & (BL_WR_LDS - 1)];
            if (far >= BL_WR_LDS) {                                      // BL_WR_LDS is a power of two: the OR reaches it iff one does
#pragma unroll
                for (int k = 0; k < BL_PPT; k++) r[k] = wr[a[k]];
            }
#pragma unroll
            for (int k = 0; k < BL_PPT; k++) {
                const double wgt = s * r[k];
                const double p = wgt * (double)q[k];
                num[k] = num[k] + p;
                den[k] = den[k] + wgt;
            }
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
    double *o = out + (size_t)blockIdx.z * h * w;
#pragma unroll
    for (int k = 0; k < BL_PPT; k++) {
        const int y = y0 + ty + 4 * k;
        if (y < h) o[(size_t)y * w + x] = num[k] / den[k];
    }
}

DS_API int ds_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int radius, const double *ws, const double *wr,
                            int wrap, double *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && depth && ws && wr && out, DS_EINVAL, "ds_bilateral_u16: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "ds_bilateral_u16: bad shape n=%d h=%d w=%d", n, h, w);
    DS_REQUIRE(radius >= 1 && radius <= BL_RMAX, DS_EINVAL, "ds_bilateral_u16: radius %d outside 1..%d", radius, BL_RMAX);
    DS_REQUIRE(wrap || radius < (h < w ? h : w), DS_EINVAL,
               "ds_bilateral_u16: BORDER_REFLECT_101 needs radius < min(h, w) (radius=%d h=%d w=%d); wrap takes any size", radius, h, w);
    DS_REQUIRE((((uintptr_t)out | (uintptr_t)ws | (uintptr_t)wr) & 7) == 0 && (((uintptr_t)depth) & 1) == 0, DS_EINVAL,
               "ds_bilateral_u16: out, ws and wr must be 8-byte aligned, depth 2-byte aligned");
    const size_t count = (size_t)n * h * w;
    DS_REQUIRE((uintptr_t)out + count * sizeof(double) <= (uintptr_t)depth || (uintptr_t)depth + count * sizeof(uint16_t) <= (uintptr_t)out,
               DS_EINVAL, "ds_bilateral_u16: out overlaps depth");
    dim3 grid((w + BL_TW - 1) / BL_TW, (h + BL_TH - 1) / BL_TH, n);
    DS_REQUIRE(n <= 65535 && grid.y <= 65535, DS_EUNSUPPORTED, "ds_bilateral_u16: n and h / %d must be <= 65535", BL_TH);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_NORMALMAP, stream);
    if (wrap) hipLaunchKernelGGL(k_bilateral_u16<1>, grid, dim3(256), 0, stream, depth, h, w, radius, ws, wr, out);
    else hipLaunchKernelGGL(k_bilateral_u16<0>, grid, dim3(256), 0, stream, depth, h, w, radius, ws, wr, out);
    ds_kt_end(ctx, DS_KT_NORMALMAP, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
