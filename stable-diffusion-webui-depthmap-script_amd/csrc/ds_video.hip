// Video mode's three kernels on gfx950 (include/depthstereo.h holds the definitions; the reference has none of them: src/video_mode.py:114,
// "TODO: Detect cuts and process segments separately", and nothing that smooths the OUTPUT depth along time).
//
// ds_frame_luma_hist: a 256-bin histogram of the integer luma of every frame of a uint8 clip (what the cut detector compares between
//   neighbouring frames).  Memory bound: every byte of the clip is read once, 1 KiB per frame is written.
//     * A frame is a byte stream.  A thread takes HC_BYTES consecutive bytes (4 RGB / RGBA pixels, 16 grey ones) as aligned dwords
//       and shifts them into place with v_alignbyte_b32 by the frame's byte offset (one value per frame: HC_BYTES is a multiple of
//       4), so any base alignment and any h * w * c run the same dword loads.  A dword is read only when it starts before the end of
//       the clip (it then holds at least one byte of it), pixels past the end of the frame are masked out of the counts.
//     * Counts go to LDS histograms private to a wave (cdna_hip_programming, "reduce atomic contention"), HC_REP copies per wave
//       interleaved bin-major so that the copies of one bin lie in HC_REP different banks; a lane adds to copy lane % HC_REP.
//     * A frame of one colour would send all 64 lanes of every add to one address.  When the valid lanes of a wave hold ONE luma
//       (two ballots), one lane adds their number instead: flat content costs one LDS add per 64 pixels, not 64 serialised ones.
//     * At the end of a workgroup thread b sums bin b over the 4 * HC_REP copies and adds it to hist[frame][b] with one global
//       integer atomic (skipped when zero).  The entry point clears hist first (hipMemsetAsync on the same stream): integer adds, so
//       the order in which workgroups arrive cannot change a bit.
//
// ds_temporal_smooth5_f32: the reference's 5-tap temporal filter (src/video_mode.py:119-124) on a run of frames, clamped to [lo, hi].
//   Memory bound.  A thread OWNS a pixel and slides a five-register window along the frames: after the first output every further
//   one costs one load (the frame two ahead, none once the window has reached hi: the register is kept) and one store, so each
//   source value comes from HBM once per launch whatever the caches hold; the clamped duplicates of the first window are the only
//   repeated addresses.  (The alternative, one thread per output element with five loads, leans on the last-level cache holding
//   four whole planes between uses; at 1080p that is 33 MB against other traffic, and nothing here depends on it.)  The next frame's
//   load is issued before the current output is computed, and a thread carries TS_PPT pixels, TS_THREADS apart, to keep enough bytes
//   in flight.  Loads and stores are single floats: plane and the base are only 4-byte aligned (an odd plane misaligns every second
//   frame for anything wider), and a wave still moves 256 contiguous bytes per instruction.
//   Rounding: every product and every sum is a separate binary32 operation.  This relies on contraction being OFF -- the pragma
//   below and the library's -ffp-contract=off -- not on __fmul_rn / __fadd_rn, which are plain `*` and `+` to this compiler and
//   would be contracted like them.  Subnormals are kept (the target's default float32 mode).
//
// ds_temporal_joint_bilateral_u16: the joint bilateral filter ALONG TIME of uint16 depth frames guided by the uint8 frames (the depth
//   of a pixel averaged over the neighbouring frames of its scene, weighted by how little the pixel's colour changed).  The shape of
//   the 5-tap filter above: a thread OWNS its pixels (TJ_PPT of them, TJ_THREADS apart) and walks the frames with a window of
//   2 R + 1 packed guide words (R, G, B, 0) and as many depths in registers, shifted by one frame per output; R is a template
//   parameter (1..4), every window index is a compile-time constant after unrolling, so the window is never an indexed array in
//   scratch (the ISA of all four instantiations has no scratch).  Each depth value and each guide byte is loaded
//   ONCE per launch (per time chunk, below); the frame that enters the window for the next output is requested before the current
//   output is computed.  Taps outside [lo, hi] are OMITTED without a branch: the test is on the frame index alone, such a tap gets the
//   weight +0.0, which leaves both sums as they are bit for bit, and its window slot is filled from the nearest frame inside [lo, hi]
//   (at a scene's ends a frame is therefore requested again, from the cache; a frame outside the scene is never read -- it may lie
//   outside the tensor).  With the loads unconditional the compiler waits for them where they are used, one output later, not where
//   they are issued.
//     * The guide is read byte by byte, three loads per pixel and frame: with c == 3 and an odd plane every frame sits at another
//       byte alignment, and the base may be any address.  A wave's three loads cover the same 192 (256) contiguous bytes, so the
//       second and third hit the lines the first brought in; k is then ONE v_sad_u8 of two packed words (ds_bilateral.h).
//     * wc (DS_BL_WC float64) is indexed PER LANE by k.  It is staged in LDS (6 KiB) once per workgroup, as the guided spatial kernel does: a
//       per-lane gather from memory would cost one address per lane in the vector memory path for every tap, next to the frame
//       loads the kernel lives on; in LDS it is one ds_read_b64 whose lanes mostly ask for the same few small k on static content
//       (broadcast) and spread over the 32 bank pairs on moving content.  wt (R + 1 values, the same for every lane) is read once
//       into registers.
//     * Arithmetic per tap and the finish of an output: the family's (ds_bl_tap, ds_bl_finish_u16 of ds_bilateral.h).
//     * Short clips of small frames: when the pixels alone give fewer than TJ_MIN_BLOCKS workgroups, the outputs are split into
//       chunks of at least TJ_MIN_CHUNK frames over grid.y and every chunk primes its own window (2 R more frame reads per chunk).
//       A pixel's chain of operations is the same in every chunking, so the bits do not depend on it.
#include "ds_bilateral.h"

#pragma clang fp contract(off)

#define HC_THREADS 256
#define HC_WAVES (HC_THREADS / 64)
#define HC_REP 4                    // copies of the histogram per wave (16 KiB of LDS per workgroup)
#define HC_CHUNKS_PER_WG 2048       // chunks a workgroup should at least have before a frame gets another one (8 per thread)

template <int C> struct hc_traits;
template <> struct hc_traits<1> { enum { PPT = 16, BYTES = 16 }; };
template <> struct hc_traits<3> { enum { PPT = 4, BYTES = 12 }; };
template <> struct hc_traits<4> { enum { PPT = 4, BYTES = 16 }; };

template <int C>
__global__ __launch_bounds__(HC_THREADS) void k_frame_luma_hist(const uint8_t *__restrict__ frames, uint32_t npix, uint32_t nchunks,
                                                                const uint8_t *clip_end, uint32_t *__restrict__ hist)
{
    enum { PPT = hc_traits<C>::PPT, NDW = hc_traits<C>::BYTES / 4 };
    __shared__ uint32_t lh[HC_WAVES * 256 * HC_REP];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < HC_WAVES * 256 * HC_REP; i += HC_THREADS) lh[i] = 0;
    __syncthreads();
    uint32_t *wh = lh + (tid >> 6) * (256 * HC_REP);

    const uint8_t *frame = frames + (size_t)blockIdx.y * npix * C;
    const unsigned sh = (unsigned)((uintptr_t)frame & 3);
    const uint32_t *aligned = (const uint32_t *)(frame - sh);
    const uint32_t stride = gridDim.x * HC_THREADS;
    const uint32_t rounds = (nchunks + stride - 1) / stride;            // the same for every thread: the ballots below see whole waves
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t q = (uint64_t)r * stride + (uint64_t)blockIdx.x * HC_THREADS + tid;
        uint32_t d[NDW + 1], v[NDW];
#pragma unroll
        for (int j = 0; j <= NDW; j++) {
            const uint32_t *a = aligned + q * NDW + j;
            d[j] = (q < nchunks && (const uint8_t *)a < clip_end) ? *a : 0u;
        }
#pragma unroll
        for (int j = 0; j < NDW; j++) v[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            unsigned y;
            if (C == 1) {
                y = (v[k >> 2] >> (8 * (k & 3))) & 255u;
            } else {
                const int b = k * C;
                const unsigned cr = (v[b >> 2] >> (8 * (b & 3))) & 255u;
                const unsigned cg = (v[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 255u;
                const unsigned cb = (v[(b + 2) >> 2] >> (8 * ((b + 2) & 3))) & 255u;
                y = (77u * cr + 150u * cg + 29u * cb + 128u) >> 8;
            }
            const bool valid = q * PPT + k < npix;
            // validity falls with the lane (q rises with it): when any lane is valid, lane 0 is, and its luma is a valid one
            const unsigned long long mv = __ballot(valid);
            const unsigned y0 = (unsigned)__builtin_amdgcn_readfirstlane((int)y);
            const unsigned long long me = __ballot(valid && y == y0);
            if (me == mv) {
                if (lane == 0 && mv) atomicAdd(&wh[y0 * HC_REP], (uint32_t)__popcll(mv));
            } else if (valid) {
                atomicAdd(&wh[y * HC_REP + (lane & (HC_REP - 1))], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int wv = 0; wv < HC_WAVES; wv++)
#pragma unroll
        for (int c = 0; c < HC_REP; c++) s += lh[wv * (256 * HC_REP) + tid * HC_REP + c];
    if (s) atomicAdd(&hist[(size_t)blockIdx.y * 256 + tid], s);
}

DS_API int ds_frame_luma_hist(ds_ctx *ctx, const uint8_t *frames, int n, int h, int w, int c, uint32_t *hist, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && frames && hist, DS_EINVAL, "ds_frame_luma_hist: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "ds_frame_luma_hist: bad shape n=%d h=%d w=%d", n, h, w);
    DS_REQUIRE(c == 1 || c == 3 || c == 4, DS_EINVAL, "ds_frame_luma_hist: c=%d is not 1, 3 or 4", c);
    DS_REQUIRE(((uintptr_t)hist & 3) == 0, DS_EINVAL, "ds_frame_luma_hist: hist must be 4-byte aligned");
    const uint64_t npix = (uint64_t)h * (uint64_t)w;
    DS_REQUIRE(npix < (1ull << 32), DS_EUNSUPPORTED, "ds_frame_luma_hist: h * w = %llu must be below 2^32", (unsigned long long)npix);
    DS_REQUIRE(n <= 65535, DS_EUNSUPPORTED, "ds_frame_luma_hist: n=%d must be <= 65535 (one grid row per frame)", n);
    const int ppt = c == 1 ? 16 : 4;
    const uint32_t nchunks = (uint32_t)((npix + ppt - 1) / ppt);
    uint32_t per_frame = (nchunks + HC_CHUNKS_PER_WG - 1) / HC_CHUNKS_PER_WG;
    const uint32_t cap = n >= 64 ? 32u : (uint32_t)((2048 + n - 1) / n);       // about 2048 workgroups for a whole clip
    if (per_frame > cap) per_frame = cap;
    const uint8_t *clip_end = frames + (size_t)n * npix * c;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    DS_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(uint32_t), stream));
    const dim3 grid(per_frame, n);
    if (c == 1) hipLaunchKernelGGL(k_frame_luma_hist<1>, grid, dim3(HC_THREADS), 0, stream, frames, (uint32_t)npix, nchunks, clip_end, hist);
    else if (c == 3) hipLaunchKernelGGL(k_frame_luma_hist<3>, grid, dim3(HC_THREADS), 0, stream, frames, (uint32_t)npix, nchunks, clip_end, hist);
    else hipLaunchKernelGGL(k_frame_luma_hist<4>, grid, dim3(HC_THREADS), 0, stream, frames, (uint32_t)npix, nchunks, clip_end, hist);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// ---- temporal filter --------------------------------------------------------------------------------------------------------------
#define TS_THREADS 256
#define TS_PPT 2

__device__ __forceinline__ int ts_clamp(int k, int lo, int hi) { return k < lo ? lo : (k > hi ? hi : k); }

__global__ __launch_bounds__(TS_THREADS) void k_temporal_smooth5_f32(const float *__restrict__ src, int64_t plane, int first, int count,
                                                                     int lo, int hi, float *__restrict__ out)
{
    const float W0 = 0.10f, W1 = 0.20f, W2 = 0.40f;                   // the taps are {W0, W1, W2, W1, W0}
    const int64_t p0 = (int64_t)blockIdx.x * (TS_THREADS * TS_PPT) + threadIdx.x;
    bool ok[TS_PPT];
    const float *s[TS_PPT];
    float r[TS_PPT][5], nxt[TS_PPT];
#pragma unroll
    for (int e = 0; e < TS_PPT; e++) {
        const int64_t p = p0 + (int64_t)e * TS_THREADS;
        ok[e] = p < plane;
        s[e] = src + (ok[e] ? p : 0);                                    // a pixel past the plane reads pixel 0 and stores nothing
#pragma unroll
        for (int u = 0; u < 5; u++) r[e][u] = s[e][(int64_t)ts_clamp(first + u - 2, lo, hi) * plane];
    }
    for (int j = 0; j < count; j++) {
        const int ahead = first + j + 3;                                 // tap 4 of the NEXT output; past hi it is the frame r[4] holds
        const bool fetch = j + 1 < count && ahead <= hi;
#pragma unroll
        for (int e = 0; e < TS_PPT; e++) nxt[e] = fetch ? s[e][(int64_t)ahead * plane] : r[e][4];
#pragma unroll
        for (int e = 0; e < TS_PPT; e++) {
            float f = 0.0f + W0 * r[e][0];
            f = f + W1 * r[e][1];
            f = f + W2 * r[e][2];
            f = f + W1 * r[e][3];
            f = f + W0 * r[e][4];
            if (ok[e]) out[(int64_t)j * plane + p0 + (int64_t)e * TS_THREADS] = f;
            r[e][0] = r[e][1];
            r[e][1] = r[e][2];
            r[e][2] = r[e][3];
            r[e][3] = r[e][4];
            r[e][4] = nxt[e];
        }
    }
}

DS_API int ds_temporal_smooth5_f32(ds_ctx *ctx, const float *src, int m, int64_t plane, int first, int count, int lo, int hi,
                                   float *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && src && out, DS_EINVAL, "ds_temporal_smooth5_f32: null argument");
    DS_REQUIRE(m > 0 && plane > 0 && count > 0, DS_EINVAL, "ds_temporal_smooth5_f32: bad size m=%d plane=%lld count=%d", m, (long long)plane, count);
    DS_REQUIRE(0 <= lo && lo <= first && (int64_t)first + count - 1 <= hi && hi < m, DS_EINVAL,
               "ds_temporal_smooth5_f32: need 0 <= lo <= first, first + count - 1 <= hi < m (lo=%d first=%d count=%d hi=%d m=%d)", lo, first, count, hi, m);
    DS_REQUIRE((((uintptr_t)src | (uintptr_t)out) & 3) == 0, DS_EINVAL, "ds_temporal_smooth5_f32: src and out must be 4-byte aligned");
    DS_REQUIRE(plane <= (int64_t)1 << 32, DS_EUNSUPPORTED, "ds_temporal_smooth5_f32: plane=%lld is above 2^32", (long long)plane);
    const uintptr_t sb = (uintptr_t)src, se = sb + (size_t)m * plane * sizeof(float);
    const uintptr_t ob = (uintptr_t)out, oe = ob + (size_t)count * plane * sizeof(float);
    DS_REQUIRE(oe <= sb || se <= ob, DS_EINVAL, "ds_temporal_smooth5_f32: out overlaps src");
    const int64_t blocks = (plane + TS_THREADS * TS_PPT - 1) / (TS_THREADS * TS_PPT);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_temporal_smooth5_f32, dim3((unsigned)blocks), dim3(TS_THREADS), 0, stream, src, plane, first, count, lo, hi, out);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// ---- temporal joint bilateral filter ------------------------------------------------------------------------------------------------
#define TJ_THREADS 256
#define TJ_PPT 2
#define TJ_MIN_BLOCKS 1024          // below this many workgroups from the pixels alone, the time axis is split over grid.y
#define TJ_MIN_CHUNK 8              // ... into chunks of at least this many output frames

template <int R>
__global__ __launch_bounds__(TJ_THREADS) void k_temporal_joint_bilateral_u16(const uint16_t *__restrict__ depth, const uint8_t *__restrict__ guide,
                                                                             int gc, int64_t plane, int first, int count, int chunk, int lo,
                                                                             int hi, const double *__restrict__ wt, const double *__restrict__ wc,
                                                                             uint16_t *__restrict__ out)
{
    enum { W = 2 * R + 1 };
    __shared__ double wc_lds[DS_BL_WC];
    ds_bl_stage_wc(wc_lds, wc, threadIdx.x, TJ_THREADS);
    double t[R + 1];
#pragma unroll
    for (int a = 0; a <= R; a++) t[a] = wt[a];
    __syncthreads();

    const int j0 = (int)blockIdx.y * chunk;                              // this workgroup renders outputs j0 .. j1 - 1
    const int j1 = j0 + chunk < count ? j0 + chunk : count;
    const int64_t p0 = (int64_t)blockIdx.x * (TJ_THREADS * TJ_PPT) + threadIdx.x;
    bool ok[TJ_PPT];
    const uint16_t *dp[TJ_PPT];                                          // the pixel in frame 0; a frame is one uniform offset further
    const uint8_t *gp[TJ_PPT];
    uint16_t *op[TJ_PPT];
    uint32_t g[TJ_PPT][W], d[TJ_PPT][W], gn[TJ_PPT], dn[TJ_PPT];
#pragma unroll
    for (int e = 0; e < TJ_PPT; e++) {
        const int64_t p = p0 + (int64_t)e * TJ_THREADS;
        ok[e] = p < plane;
        dp[e] = depth + (ok[e] ? p : 0);                                 // a pixel past the plane reads pixel 0 and stores nothing
        gp[e] = guide + (ok[e] ? p : 0) * gc;
        op[e] = out + (ok[e] ? p : 0);
    }
    // The window of the first output.  A slot whose frame lies outside [lo, hi] gets the nearest frame inside instead (never an address
    // outside the scene): its tap has weight +0.0 below, so what it holds does not matter, and no load hangs on a branch.
#pragma unroll
    for (int u = 0; u < W; u++) {
        const int64_t fo = (int64_t)ts_clamp(first + j0 + u - R, lo, hi) * plane;
#pragma unroll
        for (int e = 0; e < TJ_PPT; e++) {
            d[e][u] = dp[e][fo];
            g[e][u] = ds_bl_rgb(gp[e] + fo * gc);
        }
    }
    for (int j = j0; j < j1; j++) {
        const int i = first + j;
        {                                                                // the last tap of the NEXT output, requested before this one is computed
            const int64_t fo = (int64_t)ts_clamp(i + R + 1, lo, hi) * plane;
#pragma unroll
            for (int e = 0; e < TJ_PPT; e++) {
                dn[e] = dp[e][fo];
                gn[e] = ds_bl_rgb(gp[e] + fo * gc);
            }
        }
        double num[TJ_PPT], den[TJ_PPT];
#pragma unroll
        for (int e = 0; e < TJ_PPT; e++) num[e] = den[e] = 0.0;
#pragma unroll
        for (int u = 0; u < W; u++) {
            const int s = i + u - R;
            // A tap outside [lo, hi] is OMITTED.  Here: its weight is +0.0, and num + 0.0 * D == num, den + 0.0 == den bit for bit (every
            // term is >= +0.0 and finite), so the chain has the bits it has without the tap -- and no branch splits the tap loop.
            const double tw = (s >= lo && s <= hi) ? t[u < R ? R - u : u - R] : 0.0;
#pragma unroll
            for (int e = 0; e < TJ_PPT; e++)
                ds_bl_tap(tw, wc_lds[__builtin_amdgcn_sad_u8(g[e][u], g[e][R], 0u)], d[e][u], num[e], den[e]);
        }
#pragma unroll
        for (int e = 0; e < TJ_PPT; e++) {
            if (ok[e]) op[e][(int64_t)j * plane] = ds_bl_finish_u16(num[e], den[e]);
#pragma unroll
            for (int u = 0; u + 1 < W; u++) {
                d[e][u] = d[e][u + 1];
                g[e][u] = g[e][u + 1];
            }
            d[e][W - 1] = dn[e];
            g[e][W - 1] = gn[e];
        }
    }
}

DS_API int ds_temporal_joint_bilateral_u16(ds_ctx *ctx, const uint16_t *depth, const uint8_t *guide, int guide_channels, int m, int h, int w,
                                           int radius, const double *wt, const double *wc, int first, int count, int lo, int hi,
                                           uint16_t *out, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && depth && guide && wt && wc && out, DS_EINVAL, "ds_temporal_joint_bilateral_u16: null argument");
    DS_REQUIRE(m > 0 && h > 0 && w > 0 && count > 0, DS_EINVAL, "ds_temporal_joint_bilateral_u16: bad size m=%d h=%d w=%d count=%d", m, h, w, count);
    DS_REQUIRE(guide_channels == 3 || guide_channels == 4, DS_EINVAL, "ds_temporal_joint_bilateral_u16: guide_channels %d not 3 or 4", guide_channels);
    DS_REQUIRE(radius >= 1 && radius <= 4, DS_EINVAL, "ds_temporal_joint_bilateral_u16: radius %d outside 1..4", radius);
    DS_REQUIRE(0 <= lo && lo <= first && (int64_t)first + count - 1 <= hi && hi < m, DS_EINVAL,
               "ds_temporal_joint_bilateral_u16: need 0 <= lo <= first, first + count - 1 <= hi < m (lo=%d first=%d count=%d hi=%d m=%d)",
               lo, first, count, hi, m);
    DS_REQUIRE((((uintptr_t)wt | (uintptr_t)wc) & 7) == 0 && (((uintptr_t)depth | (uintptr_t)out) & 1) == 0, DS_EINVAL,
               "ds_temporal_joint_bilateral_u16: wt and wc must be 8-byte aligned, depth and out 2-byte aligned");
    const uint64_t npix = (uint64_t)h * (uint64_t)w;
    DS_REQUIRE(npix < (1ull << 32), DS_EUNSUPPORTED, "ds_temporal_joint_bilateral_u16: h * w = %llu must be below 2^32", (unsigned long long)npix);
    const uintptr_t sb = (uintptr_t)depth, se = sb + (size_t)m * npix * sizeof(uint16_t);
    const uintptr_t ob = (uintptr_t)out, oe = ob + (size_t)count * npix * sizeof(uint16_t);
    DS_REQUIRE(oe <= sb || se <= ob, DS_EINVAL, "ds_temporal_joint_bilateral_u16: out overlaps depth");
    const uint64_t blocks = (npix + TJ_THREADS * TJ_PPT - 1) / (TJ_THREADS * TJ_PPT);
    int chunk = count;
    if (blocks < TJ_MIN_BLOCKS) {
        const uint64_t want = (TJ_MIN_BLOCKS + blocks - 1) / blocks;                 // chunks that would fill the device
        chunk = (int)(((uint64_t)count + want - 1) / want);
        if (chunk < TJ_MIN_CHUNK) chunk = TJ_MIN_CHUNK;
        if (chunk > count) chunk = count;
    }
    const dim3 grid((unsigned)blocks, (unsigned)((count + chunk - 1) / chunk));      // grid.y <= TJ_MIN_BLOCKS
    DS_HIP_CHECK(hipSetDevice(ctx->device));
#define TJ_LAUNCH(R_)                                                                                                                  \
    hipLaunchKernelGGL(k_temporal_joint_bilateral_u16<R_>, grid, dim3(TJ_THREADS), 0, stream, depth, guide, guide_channels, (int64_t)npix, \
                       first, count, chunk, lo, hi, wt, wc, out)
    if (radius == 1) TJ_LAUNCH(1);
    else if (radius == 2) TJ_LAUNCH(2);
    else if (radius == 3) TJ_LAUNCH(3);
    else TJ_LAUNCH(4);
#undef TJ_LAUNCH
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
