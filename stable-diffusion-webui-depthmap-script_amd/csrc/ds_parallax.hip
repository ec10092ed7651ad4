// Parallax frames from depth on gfx950: the z-buffered forward splat of ds_parallax_u8 and the pass that resolves it.  The reference
// renders its camera-motion clips from a layered, inpainted mesh (three networks and an OpenGL renderer); this is the image-space
// renderer for small camera motions.  The definition is the comment of ds_parallax_u8 in include/depthstereo.h, tests/parallax_cases.py
// is its NumPy model, and the kernels give the model's bits: everything is an integer, and the depth test is a maximum over 64-bit
// keys, which does not depend on the order in which the keys arrive.
//
// k_parallax_splat: one thread per source pixel, the F views in a loop.  The depth and e = z - z0 are read and formed once; per view the
// landing point (ux, uy) in sixteenths of a pixel, the 1 or 2 target columns and rows of the 1.5-pixel footprint, and per target inside
// the image one no-return 64-bit atomicMax in global memory (global_atomic_umax_x2) -- at most 4 per pixel and view.  A read in front
// of it (a relaxed load served by L2, never by a stale L1 line) that already finds a key >= mine skips the atomic: keys only grow
// during the launch, so a key read early can only be smaller than the current one and the skipped atomic would have changed nothing
// (PX_PRECHECK; DESIGN.md 3.25 has the measurement of both forms).  The colour is not read here.  The pose components are clamped
// to +-1024, which bounds every product below 2^28; a target is addressed only after its bounds test, so no value of `poses` can
// address outside `keys`.
//
// k_parallax_resolve: one thread per target pixel of a view, consecutive lanes on consecutive pixels of a row (coalesced key reads
// and byte stores).  A target that holds a key takes its source pixel's colour; an empty one scans left, right, up and down over
// steps 1..G for the first key in each direction -- keys only, no colour; the four scans step together, so that up to four reads
// are in flight per step -- and takes the candidate with the smallest z + 1 (the farthest: a disocclusion belongs to the
// background), the earlier direction on a tie; without a candidate it keeps the image's own pixel.  One gathered 3-byte colour read
// per target, three byte stores (any byte address, as in ds_lensblur.hip).
//
// The entry point clears `keys` with a memset on the caller's stream, then makes the two launches: safe under graph capture.
#include "ds_common.h"

#define PX_THREADS 256
#define PX_POSE_MAX 1024
#define PX_FILL_MAX 64
#define PX_SIDE_MAX 16384
#ifndef PX_PRECHECK
#define PX_PRECHECK 1               // the read in front of the atomic (-DPX_PRECHECK=0: every offer is an atomic; same bits;
#endif                              // tools/parallax_ab.py times the two)

typedef unsigned long long px_key;

__device__ __forceinline__ int px_clamp_pose(int v) { return v < -PX_POSE_MAX ? -PX_POSE_MAX : v > PX_POSE_MAX ? PX_POSE_MAX : v; }

__global__ __launch_bounds__(PX_THREADS) void k_parallax_splat(const uint16_t *__restrict__ depth, const uint16_t *__restrict__ focus,
                                                               const int32_t *__restrict__ poses, int F, int h, int w, int invert,
                                                               px_key *keys)
{
    const int plane = h * w;                                             // <= 2^28
    const int p = blockIdx.x * PX_THREADS + threadIdx.x;
    if (p >= plane) return;
    const int img = blockIdx.y;
    const int y = p / w, x = p - y * w;
    const int d = depth[(size_t)img * plane + p], f = focus[img];
    const int z = invert ? 65535 - d : d;
    const int e = invert ? f - d : d - f;                                // z - z0, |e| <= 65535
    const px_key key = (px_key)(z + 1) << 32 | (px_key)(uint32_t)p;
    const int cx = 16 * x + 8 - 8 * w, cy = 16 * y + 8 - 8 * h;
    px_key *view = keys + (size_t)img * F * plane;
    for (int k = 0; k < F; k++, view += plane) {
        const int tx = px_clamp_pose(poses[3 * k]), ty = px_clamp_pose(poses[3 * k + 1]), tz = px_clamp_pose(poses[3 * k + 2]);
        const int m = (e * tz + 32768) >> 16;                            // |e * t| < 2^26; >> of a negative int is a floor here
        const int ux = 16 * x + 8 + ((e * tx + 32768) >> 16) + ((cx * m + 2048) >> 12);       // |cx * m| <= 2^17 * 2^10
        const int uy = 16 * y + 8 + ((e * ty + 32768) >> 16) + ((cy * m + 2048) >> 12);
        const int X0 = (ux - 5) >> 4, X1 = ((ux + 19) >> 4) - 1;         // X1 - X0 is 0 or 1
        const int Y0 = (uy - 5) >> 4, Y1 = ((uy + 19) >> 4) - 1;
        for (int Y = Y0; Y <= Y1; Y++) {
            if (Y < 0 || Y >= h) continue;
            for (int X = X0; X <= X1; X++) {
                if (X < 0 || X >= w) continue;
                px_key *at = view + (Y * w + X);
#if PX_PRECHECK
                if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) continue;
#endif
                atomicMax(at, key);                                      // (the result is unused: the no-return form)
            }
        }
    }
}

__global__ __launch_bounds__(PX_THREADS) void k_parallax_resolve(const uint8_t *__restrict__ image, const px_key *__restrict__ keys,
                                                                 int F, int h, int w, int fill, uint8_t *__restrict__ out,
                                                                 uint8_t *__restrict__ out_mask)
{
    const int plane = h * w;
    const int p = blockIdx.x * PX_THREADS + threadIdx.x;
    if (p >= plane) return;
    const int iv = blockIdx.y;                                           // image * F + view
    const int img = iv / F;
    const int Y = p / w, X = p - Y * w;
    const px_key *view = keys + (size_t)iv * plane;
    px_key best = view[p];
    uint32_t src = (uint32_t)p;
    uint8_t mask = 0;
    if (best == 0) {
        mask = 2;
        const int nl = X < fill ? X : fill, nr = w - 1 - X < fill ? w - 1 - X : fill;
        const int nu = Y < fill ? Y : fill, nd = h - 1 - Y < fill ? h - 1 - Y : fill;
        // the four scans step together: up to four independent reads in flight per step instead of one; each direction keeps the
        // first key it meets and stops reading
        px_key cl = 0, cr = 0, cu = 0, cd = 0;
        for (int s = 1; s <= fill; s++) {
            const bool wl = cl == 0 && s <= nl, wr = cr == 0 && s <= nr, wu = cu == 0 && s <= nu, wd = cd == 0 && s <= nd;
            if (!(wl || wr || wu || wd)) break;
            const px_key a = wl ? view[p - s] : 0, b = wr ? view[p + s] : 0, c = wu ? view[p - s * w] : 0, d = wd ? view[p + s * w] : 0;
            if (wl) cl = a;
            if (wr) cr = b;
            if (wu) cu = c;
            if (wd) cd = d;
        }
        // the smallest z + 1 wins, the earlier direction (left, right, up, down) on a tie: strict <
        best = cl;
        if (cr && (best == 0 || (cr >> 32) < (best >> 32))) best = cr;
        if (cu && (best == 0 || (cu >> 32) < (best >> 32))) best = cu;
        if (cd && (best == 0 || (cd >> 32) < (best >> 32))) best = cd;
        if (best) mask = 1;
    }
    if (best) {
        src = (uint32_t)best;
        if (src >= (uint32_t)plane) src = (uint32_t)p;                   // cannot happen with keys this call made: never read outside image
    }
    const uint8_t *c3 = image + 3 * ((size_t)img * plane + src);
    uint8_t *o = out + 3 * ((size_t)iv * plane + p);
    o[0] = c3[0];
    o[1] = c3[1];
    o[2] = c3[2];
    if (out_mask) out_mask[(size_t)iv * plane + p] = mask;
}

static bool px_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

DS_API int ds_parallax_u8(ds_ctx *ctx, const uint8_t *image, const uint16_t *depth, const uint16_t *focus, int n, int h, int w,
                          const int32_t *poses, int F, int fill, int invert, void *keys, uint8_t *out, uint8_t *out_mask, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    DS_REQUIRE(ctx && image && depth && focus && poses && keys && out, DS_EINVAL, "ds_parallax_u8: null argument");
    DS_REQUIRE(n > 0 && h > 0 && w > 0 && F > 0, DS_EINVAL, "ds_parallax_u8: bad shape n=%d h=%d w=%d F=%d", n, h, w, F);
    DS_REQUIRE(fill >= 1 && fill <= PX_FILL_MAX, DS_EINVAL, "ds_parallax_u8: fill %d outside 1..%d", fill, PX_FILL_MAX);
    DS_REQUIRE(((uintptr_t)keys & 7) == 0 && ((uintptr_t)poses & 3) == 0 && (((uintptr_t)focus | (uintptr_t)depth) & 1) == 0, DS_EINVAL,
               "ds_parallax_u8: keys must be 8-byte aligned, poses 4-byte aligned, focus and depth 2-byte aligned");
    // the size limits come before the overlap test: below them every byte count fits 64 bits
    DS_REQUIRE((int64_t)n * F <= 65535 && h <= PX_SIDE_MAX && w <= PX_SIDE_MAX, DS_EUNSUPPORTED,
               "ds_parallax_u8: n * F must be <= 65535, h and w <= %d, got n=%d F=%d h=%d w=%d", PX_SIDE_MAX, n, F, h, w);
    const size_t plane = (size_t)h * w, count = (size_t)n * plane, targets = count * F;
    const void *in[4] = {image, depth, focus, poses};
    const size_t in_bytes[4] = {3 * count, 2 * count, 2 * (size_t)n, 3 * sizeof(int32_t) * (size_t)F};
    void *outs[3] = {out, keys, out_mask};
    const size_t out_bytes[3] = {3 * targets, 8 * targets, targets};
    for (int o = 0; o < 3; o++) {
        if (!outs[o]) continue;
        for (int i = 0; i < 4; i++)
            DS_REQUIRE(!px_overlap(outs[o], out_bytes[o], in[i], in_bytes[i]), DS_EINVAL, "ds_parallax_u8: an output or keys overlaps an input");
        for (int q = 0; q < o; q++)
            DS_REQUIRE(!(outs[q] && px_overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])), DS_EINVAL,
                       "ds_parallax_u8: out, keys and out_mask overlap");
    }
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    DS_HIP_CHECK(hipMemsetAsync(keys, 0, 8 * targets, stream));
    const unsigned blocks = (unsigned)((plane + PX_THREADS - 1) / PX_THREADS);       // <= 2^20
    // ds_profile_enable: the two launches bracketed by the context's two event pairs (tools/parallax_ab.py reads them)
    if (ctx->profile) (void)hipEventRecord(ctx->ev[0], stream);
    hipLaunchKernelGGL(k_parallax_splat, dim3(blocks, n), dim3(PX_THREADS), 0, stream, depth, focus, poses, F, h, w, invert, (px_key *)keys);
    if (ctx->profile) { (void)hipEventRecord(ctx->ev[1], stream); (void)hipEventRecord(ctx->ev[2], stream); }
    hipLaunchKernelGGL(k_parallax_resolve, dim3(blocks, n * F), dim3(PX_THREADS), 0, stream, image, (const px_key *)keys, F, h, w, fill, out,
                       out_mask);
    if (ctx->profile) { (void)hipEventRecord(ctx->ev[3], stream); ctx->ev_recorded = 1; }
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
