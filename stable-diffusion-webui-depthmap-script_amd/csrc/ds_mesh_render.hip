// Mesh videos on gfx950: the triangle rasteriser of ds_mesh_render_u8 -- a coloured triangle mesh seen through F pinhole cameras.  The
// reference renders its "generate video from mesh" clips through OpenGL; this renders the SIMPLE mesh (or any triangle mesh), not the
// inpainted one.  The definition is the comment of ds_mesh_render_u8 in include/depthstereo.h, tests/mesh_render_cases.py is its NumPy
// model, and the kernels give the model's bits: behind the vertex stage everything is an integer, and the depth test is a maximum over
// 64-bit keys, which does not depend on the order in which the keys arrive -- so it does not matter which of the two raster kernels
// takes a face, in which order the faces run, or how the frames are grouped.
//
// k_mr_project: one thread per vertex and frame (blockIdx.y).  The handful of float64 operations of the definition, each rounded on its
// own (-ffp-contract=off; division is the correctly rounded expansion), then one 16-byte record (X, Y, iz, live) -- written for EVERY
// vertex, dead ones with live = 0, so that no later launch reads a record this call did not write.
//
// k_mr_raster: one thread per face and frame.  Three index loads, three record loads (neighbouring faces of a grid mesh share them in
// cache), the skips, the bounding box clipped to the viewport.  A box of at most small_cap samples is walked by the thread itself:
// per covered sample one no-return 64-bit atomicMax (global_atomic_umax_x2), k_parallax_splat's form.  Any other face goes on the
// frame's list: the wave counts its large faces with a ballot and ONE lane adds the count to the frame's counter (one atomic per wave,
// not one per face), every lane then stores its face index at its rank behind the returned base.
//
// k_mr_raster_large: a fixed grid per frame; its waves stride over the frame's list, whose length they read from device memory (no
// host round trip).  One wave takes one face, the lanes stride over its box (at most 2048^2 samples: the extent rule).  The face is
// set up again from the same records by the same routine, so its keys are the ones k_mr_raster would have offered.
//
// k_mr_resolve: one thread per output pixel and frame, consecutive lanes on consecutive pixels of a row.  Per sample (s^2 <= 16) the
// key, and for a hit the winning face's records and colours again: the weights, the three channels, the sum.  Byte stores at any address.
//
// No kernel waits for another workgroup: no flag, no grid barrier, no cooperative launch; the hand-over between launches is stream order.
#include "ds_common.h"

#include <math.h>

#define MR_THREADS 256
#define MR_SIDE_MAX 16384
#define MR_EXTENT_MAX (2048 * 16)
#define MR_CAP_MAX 64
#define MR_LARGE_BLOCKS 64          // per frame: 256 waves stride over the list
#define MR_STAGE_ALL 31

typedef unsigned long long mr_key;

struct mr_ws {                      // byte offsets into the workspace of `group` shares; the *_stride are per frame
    size_t keys_stride, rec_stride, list_stride, counters, records, lists, share;
};

static size_t mr_r256(size_t v) { return (v + 255) & ~(size_t)255; }

static mr_ws mr_layout(int64_t N, int64_t M, int H, int W, int s, int group)
{
    mr_ws l;
    l.keys_stride = mr_r256(8 * (size_t)(s * H) * (size_t)(s * W));
    l.rec_stride = mr_r256(16 * (size_t)N);
    l.list_stride = mr_r256(4 * (size_t)M);
    l.share = l.keys_stride + 256 + l.rec_stride + l.list_stride;
    l.counters = (size_t)group * l.keys_stride;              // the keys of the group, then its counter blocks: one memset clears both
    l.records = l.counters + (size_t)group * 256;
    l.lists = l.records + (size_t)group * l.rec_stride;
    return l;
}

struct mr_face {                    // a kept face, set up for coverage tests
    int Xa, Ya, Xb, Yb, Xc, Yc;
    uint32_t iza, izb, izc;
    int64_t A;                      // > 0 (the sign has been flipped into `flip`)
    int flip;
    int x0, x1, y0, y1;             // the bounding box in samples, clipped to the viewport; empty when x1 < x0 or y1 < y0
};

__device__ __forceinline__ int mr_floor16(int v) { return v >> 4; }                  // >> of a negative int is a floor here
__device__ __forceinline__ int mr_ceil16(int v) { return (v + 15) >> 4; }

// false: the face is skipped.  rec: the frame's records [N].
__device__ __forceinline__ bool mr_setup(const int32_t *__restrict__ faces, const int4 *__restrict__ rec, int64_t t, int64_t N, int Hs,
                                         int Ws, mr_face &f)
{
    const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (a < 0 || b < 0 || c < 0 || a >= N || b >= N || c >= N) return false;
    const int4 ra = rec[a], rb = rec[b], rc = rec[c];
    if (!(ra.w && rb.w && rc.w)) return false;
    f.Xa = ra.x; f.Ya = ra.y; f.Xb = rb.x; f.Yb = rb.y; f.Xc = rc.x; f.Yc = rc.y;
    f.iza = (uint32_t)ra.z; f.izb = (uint32_t)rb.z; f.izc = (uint32_t)rc.z;
    const int minx = min(ra.x, min(rb.x, rc.x)), maxx = max(ra.x, max(rb.x, rc.x));
    const int miny = min(ra.y, min(rb.y, rc.y)), maxy = max(ra.y, max(rb.y, rc.y));
    if (maxx - minx > MR_EXTENT_MAX || maxy - miny > MR_EXTENT_MAX) return false;    // |X| <= 2^18 + 1: no overflow
    const int64_t A = (int64_t)(rb.x - ra.x) * (rc.y - ra.y) - (int64_t)(rb.y - ra.y) * (rc.x - ra.x);
    if (A == 0) return false;
    f.flip = A < 0;
    f.A = A < 0 ? -A : A;
    f.x0 = max(mr_ceil16(minx), 0);
    f.x1 = min(mr_floor16(maxx), Ws - 1);
    f.y0 = max(mr_ceil16(miny), 0);
    f.y1 = min(mr_floor16(maxy), Hs - 1);
    return true;
}

// the weights of sample (px, py), which lies inside the face's clipped bounding box (or is a sample the face won): |differences| <= 2^15
__device__ __forceinline__ void mr_weights(const mr_face &f, int px, int py, int64_t &w0, int64_t &w1, int64_t &w2)
{
    const int PX = 16 * px, PY = 16 * py;
    w0 = (int64_t)(f.Xb - PX) * (f.Yc - PY) - (int64_t)(f.Yb - PY) * (f.Xc - PX);
    w1 = (int64_t)(f.Xc - PX) * (f.Ya - PY) - (int64_t)(f.Yc - PY) * (f.Xa - PX);
    if (f.flip) { w0 = -w0; w1 = -w1; }
    w2 = f.A - w0 - w1;
}

__device__ __forceinline__ void mr_offer(const mr_face &f, int px, int py, uint32_t t, mr_key *__restrict__ plane, int Ws)
{
    int64_t w0, w1, w2;
    mr_weights(f, px, py, w0, w1, w2);
    if ((w0 | w1 | w2) < 0) return;
    const uint64_t num = (uint64_t)w0 * f.iza + (uint64_t)w1 * f.izb + (uint64_t)w2 * f.izc;      // <= 2^61
    const uint64_t izp = num / (uint64_t)f.A;
    atomicMax(plane + ((size_t)py * Ws + px), (mr_key)(izp << 32 | (uint64_t)(0xFFFFFFFFu - t)));   // (result unused: the no-return form)
}

__global__ __launch_bounds__(MR_THREADS) void k_mr_project(const double *__restrict__ verts, const double *__restrict__ cameras, int64_t N,
                                                           int s, double near, int4 *__restrict__ records, size_t rec_stride)
{
    const int64_t i = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
    if (i >= N) return;
    const int k = blockIdx.y;
    const double *cam = cameras + 6 * (size_t)k;
    const double tx = cam[0], ty = cam[1], tz = cam[2], fl = cam[3], cx = cam[4], cy = cam[5];
    int4 r = make_int4(0, 0, 0, 0);
    const bool cam_ok = isfinite(tx) && isfinite(ty) && isfinite(tz) && isfinite(fl) && isfinite(cx) && isfinite(cy);
    const double xc = verts[3 * i] - tx, yc = verts[3 * i + 1] - ty, zc = verts[3 * i + 2] - tz;
    if (cam_ok && zc >= near) {
        double sx = cx - (fl * xc) / zc, sy = cy - (fl * yc) / zc;
        const double sd = (double)s, off = (double)(s - 1) * 0.5;
        sx = sx * sd + off;
        sy = sy * sd + off;
        if (isfinite(sx) && isfinite(sy) && fabs(sx) <= 16384.0 && fabs(sy) <= 16384.0) {
            const double q = floor((near / zc) * 2147483648.0);                       // 0 .. 2^31
            const uint32_t iz = q < 1.0 ? 1u : (uint32_t)q;
            r = make_int4((int)rint(16.0 * sx), (int)rint(16.0 * sy), (int)iz, 1);
        }
    }
    ((int4 *)((char *)records + (size_t)k * rec_stride))[i] = r;
}

__global__ __launch_bounds__(MR_THREADS) void k_mr_raster(const int32_t *__restrict__ faces, int64_t N, int64_t M, int Hs, int Ws, int small_cap,
                                                          const int4 *__restrict__ records, size_t rec_stride, mr_key *keys, size_t keys_stride,
                                                          uint32_t *counters, uint32_t *__restrict__ lists, size_t list_stride)
{
    const int64_t t = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    const int4 *rec = (const int4 *)((const char *)records + (size_t)k * rec_stride);
    mr_key *plane = (mr_key *)((char *)keys + (size_t)k * keys_stride);
    mr_face f;
    bool large = false;
    if (t < M && mr_setup(faces, rec, t, N, Hs, Ws, f) && f.x1 >= f.x0 && f.y1 >= f.y0) {
        const int nx = f.x1 - f.x0 + 1, ny = f.y1 - f.y0 + 1;                     // <= 2049 each
        if (nx * ny <= small_cap) {
            for (int py = f.y0; py <= f.y1; py++)                                 // at most small_cap samples
                for (int px = f.x0; px <= f.x1; px++) mr_offer(f, px, py, (uint32_t)t, plane, Ws);
        } else {
            large = true;
        }
    }
    // the list: one counter add per wave (every lane of the wave reaches this point)
    const unsigned long long mask = __ballot(large);
    if (mask) {
        const int lane = threadIdx.x & 63, leader = __ffsll(mask) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(counters + (size_t)k * 64, (uint32_t)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (large) {
            const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
            if (at < M) ((uint32_t *)((char *)lists + (size_t)k * list_stride))[at] = (uint32_t)t;   // (always: a frame lists a face once)
        }
    }
}

__global__ __launch_bounds__(MR_THREADS) void k_mr_raster_large(const int32_t *__restrict__ faces, int64_t N, int64_t M, int Hs, int Ws,
                                                                const int4 *__restrict__ records, size_t rec_stride, mr_key *keys,
                                                                size_t keys_stride, const uint32_t *__restrict__ counters,
                                                                const uint32_t *__restrict__ lists, size_t list_stride)
{
    const int k = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int4 *rec = (const int4 *)((const char *)records + (size_t)k * rec_stride);
    mr_key *plane = (mr_key *)((char *)keys + (size_t)k * keys_stride);
    const uint32_t *list = (const uint32_t *)((const char *)lists + (size_t)k * list_stride);
    uint32_t count = counters[(size_t)k * 64];
    if (count > M) count = (uint32_t)M;                                           // cannot happen with a counter this call made
    const uint32_t wave = blockIdx.x * (MR_THREADS / 64) + (threadIdx.x >> 6), waves = gridDim.x * (MR_THREADS / 64);
    for (uint32_t i = wave; i < count; i += waves) {
        const uint32_t t = list[i];
        mr_face f;
        if (t >= M || !mr_setup(faces, rec, t, N, Hs, Ws, f) || f.x1 < f.x0 || f.y1 < f.y0) continue;     // (wave-uniform)
        const int nx = f.x1 - f.x0 + 1, ny = f.y1 - f.y0 + 1;
        const int total = nx * ny;                                                // <= 2049^2 < 2^23
        for (int j = lane; j < total; j += 64) {
            const int dy = j / nx, dx = j - dy * nx;
            mr_offer(f, f.x0 + dx, f.y0 + dy, t, plane, Ws);
        }
    }
}

__global__ __launch_bounds__(MR_THREADS) void k_mr_resolve(const uint8_t *__restrict__ colors, const int32_t *__restrict__ faces, int64_t N,
                                                           int64_t M, int H, int W, int s, uint32_t bg, const int4 *__restrict__ records,
                                                           size_t rec_stride, const mr_key *__restrict__ keys, size_t keys_stride,
                                                           uint8_t *__restrict__ out, uint8_t *__restrict__ out_hits)
{
    const int plane_px = H * W;                                                   // <= 2^28
    const int p = blockIdx.x * MR_THREADS + threadIdx.x;
    if (p >= plane_px) return;
    const int k = blockIdx.y;
    const int v = p / W, u = p - v * W;
    const int Hs = s * H, Ws = s * W;
    const int4 *rec = (const int4 *)((const char *)records + (size_t)k * rec_stride);
    const mr_key *plane = (const mr_key *)((const char *)keys + (size_t)k * keys_stride);
    const int bg0 = bg & 255, bg1 = (bg >> 8) & 255, bg2 = (bg >> 16) & 255;
    int sum0 = 0, sum1 = 0, sum2 = 0, hits = 0;
    for (int j = 0; j < s; j++) {
        for (int i = 0; i < s; i++) {
            const int px = s * u + i, py = s * v + j;
            const mr_key key = plane[(size_t)py * Ws + px];
            int c0 = bg0, c1 = bg1, c2 = bg2;
            mr_face f;
            const uint32_t t = 0xFFFFFFFFu - (uint32_t)key;
            if (key != 0 && t < M && mr_setup(faces, rec, t, N, Hs, Ws, f)) {     // (a key this call made names a kept face)
                hits++;
                int64_t w0, w1, w2;
                mr_weights(f, px, py, w0, w1, w2);
                const uint8_t *ca = colors + 3 * (size_t)faces[3 * (size_t)t], *cb = colors + 3 * (size_t)faces[3 * (size_t)t + 1],
                              *cc = colors + 3 * (size_t)faces[3 * (size_t)t + 2];
                const uint64_t A = (uint64_t)f.A, half = A >> 1;
                c0 = (int)(((uint64_t)w0 * ca[0] + (uint64_t)w1 * cb[0] + (uint64_t)w2 * cc[0] + half) / A);
                c1 = (int)(((uint64_t)w0 * ca[1] + (uint64_t)w1 * cb[1] + (uint64_t)w2 * cc[1] + half) / A);
                c2 = (int)(((uint64_t)w0 * ca[2] + (uint64_t)w1 * cb[2] + (uint64_t)w2 * cc[2] + half) / A);
            }
            sum0 += c0; sum1 += c1; sum2 += c2;
        }
    }
    const int ss = s * s, h2 = ss >> 1;
    uint8_t *o = out + 3 * ((size_t)k * plane_px + p);
    o[0] = (uint8_t)((sum0 + h2) / ss);
    o[1] = (uint8_t)((sum1 + h2) / ss);
    o[2] = (uint8_t)((sum2 + h2) / ss);
    if (out_hits) out_hits[(size_t)k * plane_px + p] = (uint8_t)hits;
}

static bool mr_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

static bool mr_sizes_ok(int64_t N, int64_t M, int H, int W, int s)
{
    return N > 0 && M >= 0 && H > 0 && W > 0 && s >= 1 && s <= 4 && N < ((int64_t)1 << 31) && M < ((int64_t)1 << 31) &&
           (int64_t)s * H <= MR_SIDE_MAX && (int64_t)s * W <= MR_SIDE_MAX;
}

DS_API size_t ds_mesh_render_workspace_bytes(int64_t N, int64_t M, int H, int W, int s)
{
    if (!mr_sizes_ok(N, M, H, W, s)) return 0;
    const size_t share = mr_layout(N, M, H, W, s, 1).share;
    return share <= ((size_t)1 << 31) ? share : 0;
}

static int mr_run(const char *who, int stages, ds_ctx *ctx, const double *verts, const uint8_t *colors, const int32_t *faces, int64_t N, int64_t M,
                  const double *cameras, int F, int H, int W, int s, double near, int bg_r, int bg_g, int bg_b, int small_cap, void *workspace,
                  int group, uint8_t *out, uint8_t *out_hits, hipStream_t stream)
{
    DS_REQUIRE(ctx && verts && colors && (faces || M == 0) && cameras && workspace && out, DS_EINVAL, "%s: null argument", who);
    DS_REQUIRE(N > 0 && M >= 0 && F > 0 && H > 0 && W > 0, DS_EINVAL, "%s: bad shape N=%lld M=%lld F=%d H=%d W=%d", who, (long long)N, (long long)M,
               F, H, W);
    DS_REQUIRE(s >= 1 && s <= 4, DS_EINVAL, "%s: s %d outside 1..4", who, s);
    DS_REQUIRE(isfinite(near) && near > 0.0, DS_EINVAL, "%s: near %g is not a finite number > 0", who, near);
    DS_REQUIRE(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255, DS_EINVAL,
               "%s: background (%d, %d, %d) outside 0..255", who, bg_r, bg_g, bg_b);
    DS_REQUIRE(small_cap >= 0 && small_cap <= MR_CAP_MAX, DS_EINVAL, "%s: small_cap %d outside 0..%d", who, small_cap, MR_CAP_MAX);
    DS_REQUIRE(group >= 1 && group <= F, DS_EINVAL, "%s: group %d outside 1..F=%d", who, group, F);
    DS_REQUIRE(((uintptr_t)workspace & 255) == 0 && (((uintptr_t)verts | (uintptr_t)cameras) & 7) == 0 && ((uintptr_t)faces & 3) == 0, DS_EINVAL,
               "%s: workspace must be 256-byte aligned, verts and cameras 8-byte, faces 4-byte aligned", who);
    // the size limits come before the overlap test: below them every byte count fits 64 bits
    DS_REQUIRE(mr_sizes_ok(N, M, H, W, s) && F <= 65535, DS_EUNSUPPORTED,
               "%s: s H and s W must be <= %d, N and M < 2^31, F <= 65535, got N=%lld M=%lld F=%d H=%d W=%d s=%d", who, MR_SIDE_MAX, (long long)N,
               (long long)M, F, H, W, s);
    const mr_ws l = mr_layout(N, M, H, W, s, group);
    DS_REQUIRE(l.share <= ((size_t)1 << 31), DS_EUNSUPPORTED, "%s: one frame's workspace is %zu bytes, above 2 GiB (N=%lld M=%lld H=%d W=%d s=%d)", who,
               l.share, (long long)N, (long long)M, H, W, s);
    const size_t plane_px = (size_t)H * W;
    const void *in[4] = {verts, colors, faces, cameras};
    const size_t in_bytes[4] = {24 * (size_t)N, 3 * (size_t)N, 12 * (size_t)M, 48 * (size_t)F};
    void *outs[3] = {out, workspace, out_hits};
    const size_t out_bytes[3] = {3 * plane_px * F, (size_t)group * l.share, plane_px * F};
    for (int o = 0; o < 3; o++) {
        if (!outs[o]) continue;
        for (int i = 0; i < 4; i++)
            DS_REQUIRE(!mr_overlap(outs[o], out_bytes[o], in[i], in_bytes[i]), DS_EINVAL, "%s: an output or the workspace overlaps an input", who);
        for (int q = 0; q < o; q++)
            DS_REQUIRE(!(outs[q] && mr_overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])), DS_EINVAL,
                       "%s: out, out_hits and the workspace overlap", who);
    }
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    char *ws = (char *)workspace;
    const int Hs = s * H, Ws = s * W;
    const uint32_t bg = (uint32_t)bg_r | (uint32_t)bg_g << 8 | (uint32_t)bg_b << 16;
    const unsigned vblocks = (unsigned)((N + MR_THREADS - 1) / MR_THREADS), fblocks = (unsigned)((M + MR_THREADS - 1) / MR_THREADS);     // < 2^23
    const unsigned pblocks = (unsigned)((plane_px + MR_THREADS - 1) / MR_THREADS);
    for (int k0 = 0; k0 < F; k0 += group) {
        const int g = F - k0 < group ? F - k0 : group;
        const double *cams = cameras + 6 * (size_t)k0;
        if (stages & 1) DS_HIP_CHECK(hipMemsetAsync(ws, 0, l.records, stream));                    // the keys and the counter blocks
        if (stages & 2)
            hipLaunchKernelGGL(k_mr_project, dim3(vblocks, g), dim3(MR_THREADS), 0, stream, verts, cams, N, s, near, (int4 *)(ws + l.records),
                               l.rec_stride);
        if ((stages & 4) && M > 0)
            hipLaunchKernelGGL(k_mr_raster, dim3(fblocks, g), dim3(MR_THREADS), 0, stream, faces, N, M, Hs, Ws, small_cap,
                               (const int4 *)(ws + l.records), l.rec_stride, (mr_key *)ws, l.keys_stride, (uint32_t *)(ws + l.counters),
                               (uint32_t *)(ws + l.lists), l.list_stride);
        if ((stages & 8) && M > 0)
            hipLaunchKernelGGL(k_mr_raster_large, dim3(MR_LARGE_BLOCKS, g), dim3(MR_THREADS), 0, stream, faces, N, M, Hs, Ws,
                               (const int4 *)(ws + l.records), l.rec_stride, (mr_key *)ws, l.keys_stride, (const uint32_t *)(ws + l.counters),
                               (const uint32_t *)(ws + l.lists), l.list_stride);
        if (stages & 16)
            hipLaunchKernelGGL(k_mr_resolve, dim3(pblocks, g), dim3(MR_THREADS), 0, stream, colors, faces, N, M, H, W, s, bg,
                               (const int4 *)(ws + l.records), l.rec_stride, (const mr_key *)ws, l.keys_stride, out + 3 * plane_px * k0,
                               out_hits ? out_hits + plane_px * k0 : nullptr);
    }
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_mesh_render_u8(ds_ctx *ctx, const double *verts, const uint8_t *colors, const int32_t *faces, int64_t N, int64_t M,
                             const double *cameras, int F, int H, int W, int s, double near, int bg_r, int bg_g, int bg_b, int small_cap,
                             void *workspace, int group, uint8_t *out, uint8_t *out_hits, void *stream)
{
    return mr_run("ds_mesh_render_u8", MR_STAGE_ALL, ctx, verts, colors, faces, N, M, cameras, F, H, W, s, near, bg_r, bg_g, bg_b, small_cap,
                  workspace, group, out, out_hits, (hipStream_t)stream);
}

DS_API int ds_mesh_render_stages_u8(ds_ctx *ctx, const double *verts, const uint8_t *colors, const int32_t *faces, int64_t N, int64_t M,
                                    const double *cameras, int F, int H, int W, int s, double near, int bg_r, int bg_g, int bg_b, int small_cap,
                                    void *workspace, int group, uint8_t *out, uint8_t *out_hits, int stages, void *stream)
{
    DS_REQUIRE(stages >= 1 && stages <= MR_STAGE_ALL, DS_EINVAL, "ds_mesh_render_stages_u8: stages %d outside 1..%d", stages, MR_STAGE_ALL);
    return mr_run("ds_mesh_render_stages_u8", stages, ctx, verts, colors, faces, N, M, cameras, F, H, W, s, near, bg_r, bg_g, bg_b, small_cap,
                  workspace, group, out, out_hits, (hipStream_t)stream);
}
