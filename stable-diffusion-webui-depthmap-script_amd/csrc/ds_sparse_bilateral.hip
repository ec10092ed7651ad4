// The depth preparation of the 3D-photo pipeline on gfx950: one pass of inpaint.bilateral_filtering.sparse_bilateral_filtering, the
// discontinuity-masked median of a float32 depth map (the reference runs it as a Python loop over every pixel in front of its mesh
// code, src/core.py:468-475 and inpaint/main.py:76).
//   ds_sparse_bilateral_f32        one pass: the filtered map AND the jump map of its input;
//   ds_sparse_bilateral_jump_f32   the jump map alone (the driver never returns the output of its last pass: that filter is not run).
//
// Definition: include/depthstereo.h (ds_sparse_bilateral_f32); tests/sparse_bilateral_cases.py is its NumPy model.  Nothing here
// computes a depth: a pass SELECTS one of the window's depths, so the only float arithmetic is sb_disp (one IEEE division) and
// sb_jump (four differences, four compares), each written once below.  Which tap is selected is the host-made rank table's business.
//
// k_sparse_bilateral<S>: a 256-thread workgroup owns a 64 x 8 tile of output pixels, two per thread (rows ty and ty + 4 of the tile,
// one wave per tile row: a wave's 64 lanes read 64 consecutive LDS words, conflict-free).  The tile is this flat because a selecting
// wave works ~1500 S^2 / 49 instructions per row while a copying wave works none: at 64 x 32 the workgroups on a silhouette ran as long
// on a depth map as every workgroup does on white noise, and a 1024^2 map had only 512 of them (DESIGN.md 3.22 has both
// measurements).  With m = S / 2 and H = max(m, 1):
//   1. disp: 1 / V of the tile and a halo of H + 1, at the image's own coordinates (clamped to the image only to stay inside it).
//   2. key:  the tile and a halo of H UNDER THE CLAMP RULE: position (y, x) holds pixel (c(y), c(x)) -- its depth's bit pattern where
//            D == 0, SB_MASKED where D != 0 (D from disp and from V0 == 0).  c(y) and its four neighbours always lie inside disp's
//            rectangle (H >= 1: c moves an index by at most the halo it is in).  The tap loops have no bounds test and no clamp.
//   3. hor:  per key row and tile column the number of masked keys among the S of that row's window: a window's masked count is
//            then S reads, not S * S, and n = S * S - that.
//   4. per tile row of a wave: lanes whose window has no masked tap, or only masked taps, keep the centre; if NO lane of the wave
//            selects (the usual case on a depth map: jumps are sparse), the wave goes on to its next row at once.
//   5. selection: finite non-negative float32 order like their uint32 bit patterns, so the value of rank r among the window's valid
//            keys is found bit by bit from bit 30 down: with the bits found so far as prefix, count the keys below prefix | bit; at
//            most r of them: the value is not below it either, the bit is 1.  31 sweeps of the window out of LDS, a compare and an
//            add per tap, no sort and no per-lane array.  SB_MASKED is above every pivot: a masked tap never counts.
// A pixel's bits depend on its window alone: not on the tile, the batch size or its position in the batch.
//
// LDS per workgroup at every S (the arrays are sized for S = 15): disp 24 x 80 x 4 B = 7.5 KiB, key 22 x 78 x 4 B = 6.7 KiB,
// hor 22 x 64 B = 1.4 KiB, rank 226 x 4 B = 0.9 KiB: 16.5 KiB; the 32 waves of a CU (eight workgroups), not LDS, limit occupancy.
#include "ds_common.h"

#pragma clang fp contract(off)

#define SB_TW 64
#define SB_TH 8
#define SB_PPT 2
#define SB_HMAX 7                            // window <= 15
#define SB_KP (SB_TW + 2 * SB_HMAX)          // key pitch
#define SB_KR (SB_TH + 2 * SB_HMAX)          // key rows
#define SB_DP (SB_KP + 2)                    // disp pitch
#define SB_DR (SB_KR + 2)                    // disp rows
#define SB_NRANK 226                         // rank[n], n = 0 .. 15 * 15
#define SB_MASKED 0xffffffffu

__device__ __forceinline__ float sb_disp(float v) { return 1.0f / v; }

// J of the definition at an interior pixel: c its disparity, u d l r those of its four neighbours.  NaN compares false: no jump.
__device__ __forceinline__ bool sb_jump(float c, float u, float d, float l, float r, float t)
{
    return __builtin_fabsf(c - u) > t || __builtin_fabsf(c - d) > t || __builtin_fabsf(c - l) > t || __builtin_fabsf(c - r) > t;
}

__device__ __forceinline__ int sb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int S>
__global__ __launch_bounds__(256) void k_sparse_bilateral(const float *__restrict__ v, const float *__restrict__ v0, int h, int w, float t,
                                                          const int32_t *__restrict__ rank, float *__restrict__ out,
                                                          uint8_t *__restrict__ jump)
{
    constexpr int M = S / 2, H = M > 1 ? M : 1, OFF = H - M;             // OFF: where a window starts inside the halo (1 for S == 1)
    __shared__ float disp[SB_DR * SB_DP];
    __shared__ uint32_t key[SB_KR * SB_KP];
    __shared__ uint8_t hor[SB_KR * SB_TW];
    __shared__ int32_t rank_lds[SB_NRANK];
    const int tid = threadIdx.x;
    const int tiles_x = (w + SB_TW - 1) / SB_TW;                         // the grid's x counts tiles in raster order
    const int x0 = (blockIdx.x % tiles_x) * SB_TW, y0 = (blockIdx.x / tiles_x) * SB_TH;
    const size_t plane = (size_t)blockIdx.z * h * w;
    const float *vi = v + plane, *v0i = v0 + plane;
    constexpr int DW = SB_TW + 2 * (H + 1), DH = SB_TH + 2 * (H + 1);    // disp's rectangle: origin (y0 - H - 1, x0 - H - 1)
    constexpr int KW = SB_TW + 2 * H, KH = SB_TH + 2 * H;                // key's rectangle: origin (y0 - H, x0 - H)
    for (int i = tid; i < DW * DH; i += 256) {
        const int ly = i / DW, lx = i - ly * DW;
        const int gy = sb_clamp(y0 - (H + 1) + ly, 0, h - 1), gx = sb_clamp(x0 - (H + 1) + lx, 0, w - 1);
        disp[ly * SB_DP + lx] = sb_disp(vi[(size_t)gy * w + gx]);
    }
    for (int i = tid; i < SB_NRANK; i += 256) rank_lds[i] = rank[i];
    __syncthreads();
    for (int i = tid; i < KW * KH; i += 256) {
        const int ly = i / KW, lx = i - ly * KW;
        const int cy = sb_clamp(y0 - H + ly, 1, h - 2), cx = sb_clamp(x0 - H + lx, 1, w - 2);       // c() of the definition
        const float *d = disp + (cy - (y0 - H - 1)) * SB_DP + (cx - (x0 - H - 1));
        const size_t at = (size_t)cy * w + cx;
        const bool masked = sb_jump(d[0], d[-SB_DP], d[SB_DP], d[-1], d[1], t) || v0i[at] == 0.0f;
        key[ly * SB_KP + lx] = masked ? SB_MASKED : __float_as_uint(vi[at]);
    }
    __syncthreads();
    for (int i = tid; i < KH * SB_TW; i += 256) {
        const int ly = i / SB_TW, lx = i - ly * SB_TW;
        const uint32_t *row = key + ly * SB_KP + lx + OFF;
        int c = 0;
#pragma unroll
        for (int dx = 0; dx < S; dx++) c += row[dx] == SB_MASKED;
        hor[i] = (uint8_t)c;
    }
    __syncthreads();

    const int tx = tid & 63, ty = tid >> 6;
    const int x = x0 + tx;
    float *o = out + plane;
    uint8_t *jo = jump + plane;
#pragma unroll 1
    for (int k = 0; k < SB_PPT; k++) {
        const int ly = ty + 4 * k, y = y0 + ly;                          // wave-uniform
        if (y >= h) break;
        int masked = 0;
        for (int dy = 0; dy < S; dy++) masked += hor[(ly + OFF + dy) * SB_TW + tx];
        const int n = S * S - masked;
        const bool selects = masked > 0 && n > 0;
        uint32_t prefix = 0;
        if (__any(selects)) {
            const int r = rank_lds[n];
            const uint32_t *win = key + (ly + OFF) * SB_KP + tx + OFF;
#pragma unroll 1
            for (int bit = 30; bit >= 0; bit--) {
                const uint32_t pivot = prefix | (1u << bit);
                int below = 0;
#pragma unroll 1
                for (int dy = 0; dy < S; dy++) {
                    const uint32_t *row = win + dy * SB_KP;
#pragma unroll
                    for (int dx = 0; dx < S; dx++) below += row[dx] < pivot;
                }
                if (below <= r) prefix = pivot;
            }
        }
        if (x >= w) continue;
        const size_t at = (size_t)y * w + x;
        const bool inner = y >= 1 && y <= h - 2 && x >= 1 && x <= w - 2;
        const float *d = disp + (ly + H + 1) * SB_DP + tx + H + 1;
        jo[at] = inner && sb_jump(d[0], d[-SB_DP], d[SB_DP], d[-1], d[1], t);
        // the centre tap is pixel (c(y), c(x)) whether it is masked or not: its key may be SB_MASKED, so it is read from the map
        o[at] = selects ? __uint_as_float(prefix) : vi[(size_t)sb_clamp(y, 1, h - 2) * w + sb_clamp(x, 1, w - 2)];
    }
}

// The jump map alone, on the same grid: no tile (per pixel five reads of a map the caches hold, five divisions).
__global__ __launch_bounds__(256) void k_sparse_bilateral_jump(const float *__restrict__ v, int h, int w, float t, uint8_t *__restrict__ jump)
{
    const int tiles_x = (w + SB_TW - 1) / SB_TW;
    const int x = (blockIdx.x % tiles_x) * SB_TW + (threadIdx.x & 63);
    if (x >= w) return;
    const size_t plane = (size_t)blockIdx.z * h * w;
    for (int k = 0; k < SB_PPT; k++) {
        const int y = (blockIdx.x / tiles_x) * SB_TH + (threadIdx.x >> 6) + 4 * k;
        if (y >= h) return;
        const float *p = v + plane + (size_t)y * w + x;
        bool j = false;
        if (y >= 1 && y <= h - 2 && x >= 1 && x <= w - 2)
            j = sb_jump(sb_disp(p[0]), sb_disp(p[-w]), sb_disp(p[w]), sb_disp(p[-1]), sb_disp(p[1]), t);
        jump[plane + (size_t)y * w + x] = j;
    }
}

static bool sb_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

// What both entry points require of the map, the shape and the jump map, and their grid.
static int sb_check_map(const char *name, const ds_ctx *ctx, const float *v, const uint8_t *jump, int n, int h, int w, dim3 *grid)
{
    DS_REQUIRE(ctx && v && jump, DS_EINVAL, "%s: null argument", name);
    DS_REQUIRE(n > 0 && h >= 3 && w >= 3, DS_EINVAL, "%s: bad shape n=%d h=%d w=%d (n > 0, h and w >= 3)", name, n, h, w);
    DS_REQUIRE(((uintptr_t)v & 3) == 0, DS_EINVAL, "%s: the maps must be 4-byte aligned", name);
    const size_t count = (size_t)n * h * w;
    DS_REQUIRE(!sb_overlap(jump, count, v, count * sizeof(float)), DS_EINVAL, "%s: jump overlaps a map", name);
    const int64_t tiles = (int64_t)((w + SB_TW - 1) / SB_TW) * ((h + SB_TH - 1) / SB_TH);
    DS_REQUIRE(n <= 65535 && (h + 31) / 32 <= 65535 && tiles <= 0x7fffffff, DS_EUNSUPPORTED,
               "%s: n and h / 32 must be <= 65535 and an image at most 2^31 - 1 tiles of %d x %d", name, SB_TW, SB_TH);
    *grid = dim3((unsigned)tiles, 1, n);
    return DS_OK;
}

DS_API int ds_sparse_bilateral_f32(ds_ctx *ctx, const float *v, const float *v0, int n, int h, int w, int window, float threshold,
                                   const int32_t *rank, float *out, uint8_t *jump, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const char *name = "ds_sparse_bilateral_f32";
    DS_REQUIRE(v0 && rank && out, DS_EINVAL, "%s: null argument", name);
    dim3 grid;
    const int rc = sb_check_map(name, ctx, v, jump, n, h, w, &grid);
    if (rc != DS_OK) return rc;
    DS_REQUIRE(window >= 1 && window <= 2 * SB_HMAX + 1 && (window & 1), DS_EINVAL, "%s: window %d not odd in 1..%d", name, window,
               2 * SB_HMAX + 1);
    DS_REQUIRE((((uintptr_t)v0 | (uintptr_t)rank | (uintptr_t)out) & 3) == 0, DS_EINVAL, "%s: the maps and rank must be 4-byte aligned", name);
    const size_t count = (size_t)n * h * w, bytes = count * sizeof(float);
    DS_REQUIRE(!sb_overlap(out, bytes, v, bytes) && !sb_overlap(out, bytes, v0, bytes), DS_EINVAL, "%s: out overlaps v or v0", name);
    DS_REQUIRE(!sb_overlap(jump, count, v0, bytes) && !sb_overlap(jump, count, out, bytes), DS_EINVAL, "%s: jump overlaps a map", name);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_SPARSE_BILATERAL, stream);
    switch (window) {
#define SB_LAUNCH(S) case S: hipLaunchKernelGGL(k_sparse_bilateral<S>, grid, dim3(256), 0, stream, v, v0, h, w, threshold, rank, out, jump); break
    SB_LAUNCH(1); SB_LAUNCH(3); SB_LAUNCH(5); SB_LAUNCH(7); SB_LAUNCH(9); SB_LAUNCH(11); SB_LAUNCH(13); SB_LAUNCH(15);
#undef SB_LAUNCH
    }
    ds_kt_end(ctx, DS_KT_SPARSE_BILATERAL, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_sparse_bilateral_jump_f32(ds_ctx *ctx, const float *v, int n, int h, int w, float threshold, uint8_t *jump, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    dim3 grid;
    const int rc = sb_check_map("ds_sparse_bilateral_jump_f32", ctx, v, jump, n, h, w, &grid);
    if (rc != DS_OK) return rc;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const int kt = ds_kt_begin(ctx, DS_KT_SPARSE_BILATERAL, stream);
    hipLaunchKernelGGL(k_sparse_bilateral_jump, grid, dim3(256), 0, stream, v, h, w, threshold, jump);
    ds_kt_end(ctx, DS_KT_SPARSE_BILATERAL, kt, stream);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
