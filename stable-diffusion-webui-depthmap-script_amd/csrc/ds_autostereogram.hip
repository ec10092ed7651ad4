// Autostereograms from depth on gfx950: the single-image stereogram of ds_autostereogram_u8.  The reference has no counterpart; the
// definition is the comment of ds_autostereogram_u8 in include/depthstereo.h, tests/autostereogram_cases.py is its NumPy model, and the
// kernel gives the model's bits.  A row of a stereogram is a graph problem: column x links the two columns l and r in which the two
// eyes see it, and a pixel's colour is decided by its connected component.  The textbook algorithm walks a row from one end to the
// other; the definition names the component's LARGEST column as its representative, a maximum, which no schedule can change, so a
// whole workgroup resolves a row in LDS.
//
// k_autostereogram_u8: one workgroup per image row, 256 threads up to 2048 columns and 1024 above, a thread on columns tid, tid + T, ...
// Dynamic LDS: a uint32 label and a uint16 per column, 6 w bytes -- 12 KiB at 2048 columns, 96 KiB at the widest row (16384), of the
// 160 KiB of a CU.
// Phase 1.  The row's nearness is staged in the uint16 array (invert applied).  Per column: the separation s (as_separation);
//   the visibility walk, zt = z + floor(t k / (m P)) kept as an integer part and a remainder that carries, so the walk has no division;
//   it reads two LDS values per step, four steps' reads at a time (they do not depend on zt), and ends behind the first occluder; then
//   s, or 0 for a column that offers no link, is parked in the label array, and after a barrier moved into the uint16 array over the
//   nearness, which nobody needs any more.  label[x] = x.
// Phase 2, rounds until one changes nothing.  Invariant: label[x] is a column of x's component and >= x.
//   Hook: every link whose ends carry different labels a < b raises, by LDS atomicMax, the end that carries a, and column a itself
//   (the root of that end's tree: it belongs to the same component), to b.
//   Jump: label[x] = label[label[label[x]]], legal by the invariant.
//   Labels only grow and are bounded, so the rounds end; at the fixed point the ends of every link agree and every label is its own
//   label, so the label of a component is one of its columns and no smaller than any of them: rep.  "Changed" is one of two LDS flags
//   used in turn, so that a round costs two barriers: the flag of the next round is cleared behind this round's first barrier, when
//   every thread has read it for the last time.
// Phase 3.  Colour from (y, rep): consecutive lanes on consecutive pixels, three byte stores each (any byte address, as in
//   ds_lensblur.hip); mode 2 gathers 3 bytes of the tile.
// No workspace, no global atomics: safe under graph capture.  Nothing is addressed by a value read from global memory except the tile,
// at (y mod ph, rep mod pw).
#include "ds_common.h"

#define AS_SIDE_MAX 16384
#define AS_TILE_MAX 4096
#define AS_A (256u * 65535u)
#define AS_SMALL_THREADS 256
#define AS_LARGE_THREADS 1024
#define AS_SMALL_WIDTH 2048             // rows up to this width run on AS_SMALL_THREADS threads
#define AS_WALK 4                       // steps of the visibility walk whose LDS reads are in flight together

__device__ __forceinline__ uint32_t as_lowbias32(uint32_t v)
{
    v ^= v >> 16;
    v *= 0x7FEB352Du;
    v ^= v >> 15;
    v *= 0x846CA68Bu;
    v ^= v >> 16;
    return v;
}

// s = (2 num + den) / (2 den) with num = 2 P a, a = A - m z < 2^24, den = A + a < 2^25 + 1: a dividend below 2^36 and a quotient <= P.
// The quotient is estimated in float -- a is exact there, den, the sum and the division are each good to 2^-23 or better, so the
// estimate is off by less than 512 * 2^-20 and its floor by at most 1 -- and put right by one exact 64-bit product.
__device__ __forceinline__ int as_separation(uint32_t a, uint32_t den, int P)
{
    const uint64_t u = 4ull * (uint32_t)P * a + den, dd = 2ull * den;
    uint32_t q = (uint32_t)(fmaf((float)(4 * P), (float)a, (float)den) / (float)(2u * den));
    const uint64_t prod = (uint64_t)q * dd;
    if (prod > u)
        q--;
    else if (u - prod >= dd)
        q++;
    return (int)q;
}

__global__ __launch_bounds__(AS_LARGE_THREADS) void k_autostereogram_u8(const uint16_t *__restrict__ depth, int h, int w, int P, int m,
                                                                        int mode, uint32_t seed, const uint8_t *__restrict__ tile, int ph,
                                                                        int pw, int invert, uint8_t *__restrict__ out,
                                                                        uint16_t *__restrict__ rounds)
{
    extern __shared__ uint32_t as_lds[];
    __shared__ int changed[2];
    uint32_t *label = as_lds;                                            // [w]
    uint16_t *zz = (uint16_t *)(as_lds + w);                             // [w]: the nearness, then the separation of a linking column or 0
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t row = blockIdx.x;                                       // image * h + y
    const int y = (int)(row % (uint32_t)h);
    const uint16_t *d = depth + row * w;
#pragma clang loop vectorize(disable) unroll(disable)                    // (vectorised for T == 1, the loop holds 34 more registers)
    for (int x = tid; x < w; x += T) {
        const uint32_t v = d[x];
        zz[x] = (uint16_t)(invert ? 65535u - v : v);
    }
    if (tid < 2) changed[tid] = 0;
    __syncthreads();

    // phase 1
    const uint32_t D = (uint32_t)(m * P);                                // <= 65536
    for (int x = tid; x < w; x += T) {
        const uint32_t z = zz[x];
        const uint32_t k = 2u * AS_A - (uint32_t)m * z;                  // 384 * 65535 <= k <= 512 * 65535
        const int s = as_separation(AS_A - (uint32_t)m * z, k, P);       // <= P
        const int l = x - (s >> 1), r = l + s;
        bool offers = l >= 0 && r < w;
        if (offers) {
            const uint32_t q = k / D, rem = k - q * D;                   // t k / D = t q + t rem / D
            uint32_t zt = z, frac = 0;
            // AS_WALK steps at a time: their 2 AS_WALK reads do not depend on zt and are in flight together; a column outside the row
            // reads as 0, which is below every zt (zt >= q >= 384), and a read past the walk's end is inside the row and unused
            for (int t0 = 1, walking = 1; walking; t0 += AS_WALK) {
                uint32_t za[AS_WALK], zb[AS_WALK];
#pragma unroll
                for (int j = 0; j < AS_WALK; j++) {
                    const int a = x - t0 - j, b = x + t0 + j;
                    const uint32_t va = zz[a < 0 ? 0 : a], vb = zz[b >= w ? w - 1 : b];
                    za[j] = a < 0 ? 0u : va;
                    zb[j] = b >= w ? 0u : vb;
                }
#pragma unroll
                for (int j = 0; j < AS_WALK; j++) {
                    zt += q;
                    frac += rem;
                    if (frac >= D) {
                        frac -= D;
                        zt++;
                    }
                    if (walking && zt >= 65535u) walking = 0;
                    if (walking && (za[j] >= zt || zb[j] >= zt)) {
                        offers = false;
                        walking = 0;
                    }
                }
                if (x - t0 - AS_WALK < 0 && x + t0 + AS_WALK >= w) walking = 0;      // nothing left in the row on either side
            }
        }
        label[x] = offers ? (uint32_t)s : 0u;
    }
    __syncthreads();
    for (int x = tid; x < w; x += T) {
        zz[x] = (uint16_t)label[x];
        label[x] = (uint32_t)x;
    }
    __syncthreads();

    // phase 2
    int made = 0;
    for (int flag = 0;; flag ^= 1) {
        bool raised = false;
        for (int x = tid; x < w; x += T) {
            const int s = zz[x];
            if (!s) continue;
            const int l = x - (s >> 1), r = l + s;
            const uint32_t a = label[l], b = label[r];
            if (a == b) continue;
            raised = true;
            const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
            atomicMax(&label[a < b ? l : r], hi);                        // (the results are unused: the no-return form)
            atomicMax(&label[lo], hi);
        }
        if (raised) changed[flag] = 1;
        __syncthreads();
        if (tid == 0) changed[flag ^ 1] = 0;
        raised = false;
        for (int x = tid; x < w; x += T) {
            const uint32_t a = label[x];
            const uint32_t c = label[label[a]];
            if (c != a) {
                label[x] = c;
                raised = true;
            }
        }
        if (raised) changed[flag] = 1;
        __syncthreads();
        made++;
        if (!changed[flag]) break;
    }
    if (rounds && tid == 0) rounds[row] = (uint16_t)(made < 65535 ? made : 65535);

    // phase 3
    uint8_t *o = out + 3 * row * w;
    const uint32_t hy = seed ^ ((uint32_t)y * 0x9E3779B1u);
    const uint8_t *trow = mode == 2 ? tile + 3 * (size_t)(y % ph) * pw : nullptr;
    for (int x = tid; x < w; x += T) {
        const uint32_t rep = label[x];
        uint8_t c0, c1, c2;
        if (mode == 2) {
            const uint8_t *c = trow + 3 * (rep % (uint32_t)pw);
            c0 = c[0];
            c1 = c[1];
            c2 = c[2];
        } else {
            const uint32_t hash = as_lowbias32(hy ^ (rep * 0x85EBCA77u));
            if (mode == 0) {
                c0 = (uint8_t)hash;
                c1 = (uint8_t)(hash >> 8);
                c2 = (uint8_t)(hash >> 16);
            } else {
                c0 = c1 = c2 = (uint8_t)(255u * (hash >> 31));
            }
        }
        o[3 * x] = c0;
        o[3 * x + 1] = c1;
        o[3 * x + 2] = c2;
    }
}

static bool as_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

static int as_run(const char *who, bool want_rounds, ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int period, int m, int mode,
                  uint32_t seed, const uint8_t *tile, int ph, int pw, int invert, uint8_t *out, uint16_t *rounds, hipStream_t stream)
{
    DS_REQUIRE(ctx && depth && out && (mode != 2 || tile) && (rounds || !want_rounds), DS_EINVAL, "%s: null argument", who);
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    DS_REQUIRE(period >= 16 && period <= 512, DS_EINVAL, "%s: period %d outside 16..512", who, period);
    DS_REQUIRE(m >= 1 && m <= 128, DS_EINVAL, "%s: m %d outside 1..128", who, m);
    DS_REQUIRE(mode >= 0 && mode <= 2, DS_EINVAL, "%s: mode %d outside 0..2", who, mode);
    DS_REQUIRE(mode != 2 || (ph >= 1 && ph <= AS_TILE_MAX && pw >= 1 && pw <= AS_TILE_MAX), DS_EINVAL,
               "%s: tile %d x %d outside 1..%d", who, ph, pw, AS_TILE_MAX);
    DS_REQUIRE((((uintptr_t)depth | (uintptr_t)rounds) & 1) == 0, DS_EINVAL, "%s: depth%s must be 2-byte aligned", who,
               want_rounds ? " and rounds" : "");
    // the size limits come before the overlap test: below them every byte count fits 64 bits
    DS_REQUIRE(n <= 65535 && h <= AS_SIDE_MAX && w <= AS_SIDE_MAX, DS_EUNSUPPORTED, "%s: n must be <= 65535, h and w <= %d, got n=%d h=%d w=%d",
               who, AS_SIDE_MAX, n, h, w);
    const size_t rows = (size_t)n * h, count = rows * w;                 // rows < 2^30
    const size_t tile_bytes = mode == 2 ? 3 * (size_t)ph * pw : 0;
    DS_REQUIRE(!as_overlap(out, 3 * count, depth, 2 * count) && !(tile_bytes && as_overlap(out, 3 * count, tile, tile_bytes)), DS_EINVAL,
               "%s: out overlaps an input", who);
    if (rounds)
        DS_REQUIRE(!as_overlap(rounds, 2 * rows, depth, 2 * count) && !as_overlap(rounds, 2 * rows, out, 3 * count) &&
                       !(tile_bytes && as_overlap(rounds, 2 * rows, tile, tile_bytes)),
                   DS_EINVAL, "%s: rounds overlaps another argument", who);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t lds = 6 * (size_t)w;                                    // <= 96 KiB
    if (lds > 64 * 1024)
        DS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_autostereogram_u8), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         6 * AS_SIDE_MAX));
    const int threads = w <= AS_SMALL_WIDTH ? AS_SMALL_THREADS : AS_LARGE_THREADS;
    hipLaunchKernelGGL(k_autostereogram_u8, dim3((unsigned)rows), dim3(threads), lds, stream, depth, h, w, period, m, mode, seed, tile, ph, pw,
                       invert, out, rounds);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_autostereogram_u8(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int period, int m, int mode, uint32_t seed,
                                const uint8_t *tile, int ph, int pw, int invert, uint8_t *out, void *stream)
{
    return as_run("ds_autostereogram_u8", false, ctx, depth, n, h, w, period, m, mode, seed, tile, ph, pw, invert, out, nullptr,
                  (hipStream_t)stream);
}

DS_API int ds_autostereogram_rounds_u8(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int period, int m, int mode, uint32_t seed,
                                       const uint8_t *tile, int ph, int pw, int invert, uint8_t *out, uint16_t *rounds, void *stream)
{
    return as_run("ds_autostereogram_rounds_u8", true, ctx, depth, n, h, w, period, m, mode, seed, tile, ph, pw, invert, out, rounds,
                  (hipStream_t)stream);
}
