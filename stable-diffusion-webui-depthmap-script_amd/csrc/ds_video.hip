// Video mode's two kernels on gfx950 (include/depthstereo.h holds the definitions; the reference has neither: src/video_mode.py:114,
// "TODO: Detect cuts and process segments separately").
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
#include "ds_common.h"

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
