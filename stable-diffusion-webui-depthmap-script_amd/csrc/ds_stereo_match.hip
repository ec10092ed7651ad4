// Depth from stereo pairs on gfx950: four-path semi-global matching (Hirschmueller 2008) on a 5x5 census, ds_stereo_match_u8; with
// eight paths and a speckle filter, ds_stereo_match_ex_u8; the filter alone, ds_speckle_filter_i16.  The reference has no counterpart;
// the definitions are the comments of these entry points in include/depthstereo.h, tests/stereo_match_cases.py and
// tests/stereo_match_ex_cases.py are their NumPy models, and the kernels give the models' bits: everything below is integer min, +,
// compare, so no schedule can change a value.
//
// Per group of images (the workspace holds `group` images; groups follow each other in stream order), six launches; with eight paths two
// more behind the vertical paths (k_sm_paths<DR>, k_sm_paths<DL>: a line is a diagonal, see "the paths" below), and with the speckle
// filter k_sm_winner stops before its fill and k_sp_init, k_sp_merge, k_sp_count, k_sp_write (see "speckle filter" below) and k_sm_fill
// follow it:
//   k_sm_census      one thread per pixel and side: 25 lumas, 24 compares, one uint32 per pixel into the two census planes; the thread
//                    of pixel 0 sets the image's lo / hi words to their initial values.
//   k_sm_paths<H>    a line is an image row.  Lanes are disparities: G = 32 lanes hold a line at D = 32 (two lines per wave), 64 lanes at
//                    D = 64, and at D = 128 a lane holds the two disparities 2 l and 2 l + 1, so that d +- 1 is the lane's own other value
//                    or one __shfl_up / __shfl_down, and D = 128 needs no exchange between waves.  A line's two directions run TOGETHER
//                    in the two halves of a packed uint16 pair: at step i chain a stands on position i and chain b on len - 1 - i, so
//                    one min ladder (__shfl_xor, log2 G rounds of v_pk_min_u16) serves both m_r, and a line takes len steps, not 2 len.
//                    Positions below the middle are STORED into S[y][x][d] (d contiguous: 64..256 bytes per step), the middle one (odd
//                    len) stores La + Lb, positions above it are added to what the other chain stored -- by the same lane, earlier in
//                    program order.  The cost is computed on the fly (one popcount per value); the loads of SM_U steps -- census words,
//                    and in the adding half the old S values -- are issued together ahead of the SM_U dependent steps; a chunk never
//                    straddles the middle, so a prefetched S value is never one this chunk writes.
//   k_sm_paths<V>    a line is an image column; four adjacent columns per 256-thread block (eight at D = 32), so a step of the block
//                    touches 512 contiguous bytes of S.  Both directions at once as above; every position is a read-add-write.
//                    A row-owned and a column-owned launch never share an S element within a launch: stream order is the hand-over.
//   k_sm_winner      one block per image row.  dR by the diagonal read of S; per pixel d*, S1, uniqueness, sub-pixel from two passes
//                    over its D contiguous values; left-right check; then the fill in LDS: a thread owns a segment of the row, the
//                    segments' first / last valid columns go through LDS, and two walks give every invalid pixel its neighbours.
//   k_sm_median      3x3 median, min / max of the image through a block reduction and one global atomicMin / atomicMax per block.
//   k_sm_depth       the uint16 map (only when depth is asked for).
// Nothing is addressed by a value read from memory: every index comes from the launch geometry and the checked arguments.
#include "ds_common.h"

#include <limits.h>

#define SM_SIDE_MAX 16384
#define SM_THREADS 256
#define SM_U 4                          // steps of a path whose loads are in flight together
#define SM_BIG 0x3FFF                   // an absent d +- 1: above every L_r (<= 279), and + 64 stays inside 16 bits
#define SM_OUTSIDE 24                   // the cost of a disparity whose right column lies outside the row
#define SM_NONE 32767                   // "no valid pixel on this side" in the fill: above every disp16 (<= 4072)
#define SM_MEDIAN_PER_THREAD 4
#define SM_STAGE_CENSUS 1               // the `stages` bits of ds_stereo_match_stages_u8, in launch order
#define SM_STAGE_HORIZONTAL 2
#define SM_STAGE_VERTICAL 4
#define SM_STAGE_WINNER 8
#define SM_STAGE_MEDIAN 16
#define SM_STAGE_DEPTH 32
#define SM_STAGE_ALL 63
#define SM_STAGE_DIAGONAL 64             // ds_stereo_match_ex_stages_u8 only: the two diagonal launches (paths = 8)
#define SM_STAGE_SPECKLE 128             // the speckle filter and the fill behind it (speckle_size > 0)
#define SM_STAGE_EX_ALL 255

typedef unsigned short sm_pair __attribute__((ext_vector_type(2)));      // .x: the forward chain, .y: the backward chain

struct sm_ws {
    char *base;                         // the first image's block
    size_t stride;                      // bytes per image: ds_stereo_match_workspace_bytes
    size_t cl, cr, fil, mm;             // byte offsets inside an image's block; S is at 0
    size_t d16, v0, v1, par, cnt;       // with the speckle filter: disp16, valid of step 7, valid of step 7b, links, counters
};

static inline size_t sm_r256(size_t v) { return (v + 255) & ~(size_t)255; }

static sm_ws sm_layout(void *base, int h, int w, int D, bool speckle = false)
{
    const size_t plane = (size_t)h * w;
    sm_ws ws;
    ws.base = (char *)base;
    ws.cl = sm_r256(2 * plane * D);
    ws.cr = ws.cl + sm_r256(4 * plane);
    ws.fil = ws.cr + sm_r256(4 * plane);
    ws.mm = ws.fil + sm_r256(2 * plane);
    ws.stride = ws.mm + 256;
    ws.d16 = ws.v0 = ws.v1 = ws.par = ws.cnt = 0;
    if (speckle) {                                                       // behind the share of ds_stereo_match_u8, which stays as it is
        ws.d16 = ws.stride;
        ws.v0 = ws.d16 + sm_r256(2 * plane);
        ws.v1 = ws.v0 + sm_r256(plane);
        ws.par = ws.v1 + sm_r256(plane);
        ws.cnt = ws.par + sm_r256(4 * plane);
        ws.stride = ws.cnt + sm_r256(4 * plane);
    }
    return ws;
}

__device__ __forceinline__ sm_pair sm_from_bits(int v) { return __builtin_bit_cast(sm_pair, v); }
__device__ __forceinline__ int sm_bits(sm_pair v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ sm_pair sm_min(sm_pair a, sm_pair b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ sm_pair sm_both(int v) { return sm_pair{(unsigned short)v, (unsigned short)v}; }

// ---- census ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sm_luma(const uint8_t *p, int c)
{
    return c == 1 ? (int)p[0] : (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8;
}

__global__ __launch_bounds__(SM_THREADS) void k_sm_census(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right, int h, int w,
                                                           int c, sm_ws ws)
{
    const size_t plane = (size_t)h * w;
    const size_t p = (size_t)blockIdx.x * SM_THREADS + threadIdx.x;
    const int img = blockIdx.y, side = blockIdx.z;
    char *block = ws.base + (size_t)img * ws.stride;
    if (p == 0 && side == 0) {
        int *mm = (int *)(block + ws.mm);
        mm[0] = INT_MAX;
        mm[1] = INT_MIN;
    }
    if (p >= plane) return;
    const int y = (int)(p / (unsigned)w), x = (int)(p - (size_t)y * w);
    const uint8_t *src = (side ? right : left) + (size_t)img * plane * c;
    const int centre = sm_luma(src + p * c, c);
    uint32_t bits = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int yy = min(max(y + dy, 0), h - 1);
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            if (dy == 0 && dx == 0) continue;
            const int xx = min(max(x + dx, 0), w - 1);
            bits = (bits << 1) | (uint32_t)(sm_luma(src + ((size_t)yy * w + xx) * c, c) < centre);
        }
    }
    ((uint32_t *)(block + (side ? ws.cr : ws.cl)))[p] = bits;
}

// ---- the paths ------------------------------------------------------------------------------------------------------------------------
// DIR: SM_DIR_H a line is a row; SM_DIR_V a column; SM_DIR_DR a diagonal whose column grows by one per row (chain a is the direction
// (+1,+1), chain b (-1,-1)); SM_DIR_DL one whose column falls by one per row ((+1,-1) and (-1,+1)).  A diagonal is the vertical pass
// with a moving column: a line is named by its column at row 0, c0 = li - (h - 1) in -(h-1)..w-1 for DR and c0 = li in 0..w+h-2 for
// DL, and is live on the rows y0..y0+len-1 where that column lies inside the image, so its first pixel is the one whose predecessor
// is outside.  Line lengths differ between the lines of a block and, at D = 32, between the two lines of a wave: every shuffle below
// stays inside the G lanes of one line (width G, or an xor below G), and those lanes share every trip count and branch.
#define SM_DIR_H 0
#define SM_DIR_V 1
#define SM_DIR_DR 2
#define SM_DIR_DL 3

template <int G, int DPL, int DIR>
__global__ __launch_bounds__(SM_THREADS) void k_sm_paths(int h, int w, int d0, int P1, int P2, int lines_per_image, int total_lines, sm_ws ws)
{
    constexpr int D = G * DPL;
    constexpr int DX = DIR == SM_DIR_H || DIR == SM_DIR_DR ? 1 : DIR == SM_DIR_DL ? -1 : 0, DY = DIR == SM_DIR_H ? 0 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lg = lane & (G - 1);
    int line = ((int)blockIdx.x * (SM_THREADS / 64) + wave) * (64 / G) + lane / G;
    const bool live = line < total_lines;                                // a line beyond the last repeats the last and stores nothing
    if (!live) line = total_lines - 1;
    const int img = line / lines_per_image, li = line - img * lines_per_image;
    char *block = ws.base + (size_t)img * ws.stride;
    const uint32_t *cl = (const uint32_t *)(block + ws.cl), *cr = (const uint32_t *)(block + ws.cr);
    uint16_t *S = (uint16_t *)block;
    int ys = 0, xs = 0, len;                                             // the line's first position and its length
    if (DIR == SM_DIR_H) {
        ys = li;
        len = w;
    } else if (DIR == SM_DIR_V) {
        xs = li;
        len = h;
    } else if (DIR == SM_DIR_DR) {
        const int c0 = li - (h - 1);
        ys = max(0, -c0);
        xs = c0 + ys;
        len = min(h - 1, w - 1 - c0) - ys + 1;
    } else {
        ys = max(0, li - (w - 1));
        xs = li - ys;
        len = min(h - 1, li) - ys + 1;
    }
    const int dlo = d0 + lg * DPL;                                       // this lane's smallest disparity
    const sm_pair P1v = sm_both(P1), P2v = sm_both(P2), bigv = sm_both(SM_BIG);

    sm_pair L[DPL], m = sm_both(0);
#pragma unroll
    for (int k = 0; k < DPL; k++) L[k] = sm_both(0);

    // three ranges of steps: below the middle, the middle (odd len), above it
    for (int r = 0; r < 3; r++) {
        const int lo = r == 0 ? 0 : r == 1 ? len >> 1 : (len + 1) >> 1;
        const int hi = r == 0 ? len >> 1 : r == 1 ? (len + 1) >> 1 : len;
        const bool loads = DIR != SM_DIR_H || r == 2, mid = r == 1;
        for (int i0 = lo; i0 < hi; i0 += SM_U) {
            sm_pair cost[SM_U][DPL];
            uint32_t old_a[SM_U], old_b[SM_U];                           // DPL uint16 values each
#pragma unroll
            for (int j = 0; j < SM_U; j++) {
                const int i = min(i0 + j, hi - 1);
                const int pa = i, pb = len - 1 - i;
                const int xa = xs + DX * pa, xb = xs + DX * pb;
                const size_t row_a = (size_t)(ys + DY * pa) * w, row_b = (size_t)(ys + DY * pb) * w;
                const uint32_t ca = cl[row_a + xa], cb = cl[row_b + xb];
#pragma unroll
                for (int k = 0; k < DPL; k++) {
                    const int ra = xa - dlo - k, rb = xb - dlo - k;
                    const bool ina = (unsigned)ra < (unsigned)w, inb = (unsigned)rb < (unsigned)w;
                    const uint32_t va = cr[row_a + (ina ? ra : 0)], vb = cr[row_b + (inb ? rb : 0)];
                    cost[j][k] = sm_pair{(unsigned short)(ina ? __popc(ca ^ va) : SM_OUTSIDE), (unsigned short)(inb ? __popc(cb ^ vb) : SM_OUTSIDE)};
                }
                old_a[j] = old_b[j] = 0;
                if (loads) {
                    const size_t ea = (row_a + xa) * D + lg * DPL, eb = (row_b + xb) * D + lg * DPL;
                    if (DPL == 1) {
                        old_a[j] = S[ea];
                        old_b[j] = S[eb];
                    } else {
                        old_a[j] = *(const uint32_t *)(S + ea);
                        old_b[j] = *(const uint32_t *)(S + eb);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < SM_U; j++) {
                const int i = i0 + j;
                if (i >= hi) break;
                if (i == 0) {
#pragma unroll
                    for (int k = 0; k < DPL; k++) L[k] = cost[j][k];
                } else {
                    const int up = __shfl_up(sm_bits(L[DPL - 1]), 1, G), dn = __shfl_down(sm_bits(L[0]), 1, G);
                    const sm_pair upv = lg == 0 ? bigv : sm_from_bits(up), dnv = lg == G - 1 ? bigv : sm_from_bits(dn);
                    const sm_pair cap = m + P2v;
                    sm_pair nl[DPL];
#pragma unroll
                    for (int k = 0; k < DPL; k++) {
                        const sm_pair prev = k == 0 ? upv : L[k - 1], next = k == DPL - 1 ? dnv : L[k + 1];
                        nl[k] = cost[j][k] + sm_min(sm_min(L[k], cap), sm_min(prev, next) + P1v) - m;
                    }
#pragma unroll
                    for (int k = 0; k < DPL; k++) L[k] = nl[k];
                }
                m = L[0];
#pragma unroll
                for (int k = 1; k < DPL; k++) m = sm_min(m, L[k]);
#pragma unroll
                for (int o = G / 2; o > 0; o >>= 1) m = sm_min(m, sm_from_bits(__shfl_xor(sm_bits(m), o, 64)));
                if (live) {
                    const int pa = i, pb = len - 1 - i;
                    const size_t ea = ((size_t)(ys + DY * pa) * w + (xs + DX * pa)) * D + lg * DPL;
                    const size_t eb = ((size_t)(ys + DY * pb) * w + (xs + DX * pb)) * D + lg * DPL;
                    uint32_t out_a = old_a[j], out_b = old_b[j];         // two packed uint16 sums (<= 2232 each: no carry between them)
#pragma unroll
                    for (int k = 0; k < DPL; k++) {
                        out_a += (uint32_t)L[k].x << (16 * k);
                        out_b += (uint32_t)L[k].y << (16 * k);
                    }
                    if (mid) {
#pragma unroll
                        for (int k = 0; k < DPL; k++) out_a += (uint32_t)L[k].y << (16 * k);
                    }
                    if (DPL == 1) {
                        S[ea] = (uint16_t)out_a;
                        if (!mid) S[eb] = (uint16_t)out_b;
                    } else {
                        *(uint32_t *)(S + ea) = out_a;
                        if (!mid) *(uint32_t *)(S + eb) = out_b;
                    }
                }
            }
        }
    }
}

// ---- winner, checks, sub-pixel, fill ----------------------------------------------------------------------------------------------------
// ---- the fill of step 8 for one row in LDS: thread t owns columns x0..x1-1.  disp [w] and val [w] are read, fil [w] is written; every
// thread of the block calls it, behind a barrier that made disp and val whole, and it ends behind a barrier of its own.
__device__ __forceinline__ void sm_fill_row(const int16_t *disp, int16_t *fil, const uint8_t *val, int w, int d0, int *seg_last, int *seg_first)
{
    const int tid = threadIdx.x;
    const int seg = (w + SM_THREADS - 1) / SM_THREADS;
    const int x0 = min(tid * seg, w), x1 = min(x0 + seg, w);
    int last = -1, first = w;
    for (int x = x0; x < x1; x++)
        if (val[x]) {
            if (first == w) first = x;
            last = x;
        }
    seg_last[tid] = last;
    seg_first[tid] = first;
    __syncthreads();
    int left = -1, right = w;                                            // the nearest valid column outside the segment, either side
    for (int t = tid - 1; t >= 0 && left < 0; t--) left = seg_last[t];
    for (int t = tid + 1; t < SM_THREADS && right == w; t++) right = seg_first[t];
    int cur = left < 0 ? SM_NONE : disp[left];
    for (int x = x0; x < x1; x++) {
        if (val[x]) cur = disp[x];
        fil[x] = (int16_t)cur;                                           // (of a valid pixel: its own value)
    }
    cur = right == w ? SM_NONE : disp[right];
    for (int x = x1 - 1; x >= x0; x--) {
        if (val[x]) {
            cur = disp[x];
        } else {
            const int v = min((int)fil[x], cur);
            fil[x] = (int16_t)(v == SM_NONE ? 16 * d0 : v);
        }
    }
    __syncthreads();
}

template <int D>
__global__ __launch_bounds__(SM_THREADS) void k_sm_winner(int h, int w, int d0, int u, int lr, int stop, sm_ws ws, uint8_t *__restrict__ valid_out)
{
    extern __shared__ int16_t sm_lds[];
    __shared__ int seg_last[SM_THREADS], seg_first[SM_THREADS];
    int16_t *disp = sm_lds;                                              // [w] disp16 of step 7
    int16_t *fil = sm_lds + w;                                           // [w] d* until the left-right check is done, then the filled row
    uint8_t *val = (uint8_t *)(sm_lds + 2 * (size_t)w);                  // [w]
    uint8_t *dR = val + w;                                               // [w] 255 = undefined
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;                                       // image * h + y
    const int img = (int)(row / (unsigned)h), y = (int)(row - (size_t)img * h);
    char *block = ws.base + (size_t)img * ws.stride;
    const uint16_t *Srow = (const uint16_t *)block + (size_t)y * w * D;

    if (lr >= 0)
        for (int xr = tid; xr < w; xr += SM_THREADS) {
            uint32_t best = 0xFFFFu;
            int bd = 255;
            for (int d = 0; d < D; d++) {
                const int x = xr + d0 + d;
                if ((unsigned)x < (unsigned)w) {
                    const uint32_t v = Srow[(size_t)x * D + d];
                    if (v < best) {
                        best = v;
                        bd = d;
                    }
                }
            }
            dR[xr] = (uint8_t)bd;
        }
    for (int x = tid; x < w; x += SM_THREADS) {
        const uint4 *s4 = (const uint4 *)(Srow + (size_t)x * D);          // D * 2 bytes, 64-byte aligned
        uint32_t best = 0xFFFFu;
        int bd = 0;
        for (int q = 0; q < D / 8; q++) {
            const uint4 v = s4[q];
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const uint32_t e = (wv[t >> 1] >> (16 * (t & 1))) & 0xFFFFu;
                if (e < best) {
                    best = e;
                    bd = 8 * q + t;
                }
            }
        }
        uint32_t other = 0xFFFFu, a = 0, c = 0;
        for (int q = 0; q < D / 8; q++) {
            const uint4 v = s4[q];
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const uint32_t e = (wv[t >> 1] >> (16 * (t & 1))) & 0xFFFFu;
                const int d = 8 * q + t;
                if (d == bd - 1) a = e;
                if (d == bd + 1) c = e;
                if ((d < bd - 1 || d > bd + 1) && e < other) other = e;
            }
        }
        const bool unique = !(other * (uint32_t)(100 - u) < best * 100u);
        int frac = 0;
        if (bd > 0 && bd < D - 1) {
            const int den = (int)a + (int)c - 2 * (int)best;
            if (den > 0) {
                const int num = 16 * ((int)a - (int)c) + den;
                frac = num >= 0 ? num / (2 * den) : -((-num + 2 * den - 1) / (2 * den));      // a floor
            }
        }
        disp[x] = (int16_t)(16 * (d0 + bd) + frac);
        fil[x] = (int16_t)bd;
        val[x] = (uint8_t)unique;
    }
    __syncthreads();
    if (lr >= 0) {
        for (int x = tid; x < w; x += SM_THREADS) {
            const int bd = fil[x];
            const int xr = x - (d0 + bd);
            bool ok = (unsigned)xr < (unsigned)w;
            if (ok) {
                const int r = dR[xr];
                ok = r != 255 && abs(r - bd) <= lr;
            }
            if (!ok) val[x] = 0;
        }
        __syncthreads();
    }
    if (stop) {                                                          // step 7b follows: k_sm_fill makes the rest of this row
        int16_t *d16 = (int16_t *)(block + ws.d16) + (size_t)y * w;
        uint8_t *v0 = (uint8_t *)(block + ws.v0) + (size_t)y * w;
        for (int x = tid; x < w; x += SM_THREADS) {
            d16[x] = disp[x];
            v0[x] = val[x];
        }
        return;
    }
    if (valid_out)
        for (int x = tid; x < w; x += SM_THREADS) valid_out[row * w + x] = val[x];
    sm_fill_row(disp, fil, val, w, d0, seg_last, seg_first);
    int16_t *out = (int16_t *)(block + ws.fil) + (size_t)y * w;
    for (int x = tid; x < w; x += SM_THREADS) out[x] = fil[x];
}

// step 8 behind the speckle filter: a row's disp16 and its filtered mask come back from the workspace
__global__ __launch_bounds__(SM_THREADS) void k_sm_fill(int h, int w, int d0, sm_ws ws, uint8_t *__restrict__ valid_out)
{
    extern __shared__ int16_t sm_lds[];
    __shared__ int seg_last[SM_THREADS], seg_first[SM_THREADS];
    int16_t *disp = sm_lds, *fil = sm_lds + w;
    uint8_t *val = (uint8_t *)(sm_lds + 2 * (size_t)w);
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int img = (int)(row / (unsigned)h), y = (int)(row - (size_t)img * h);
    char *block = ws.base + (size_t)img * ws.stride;
    const int16_t *d16 = (const int16_t *)(block + ws.d16) + (size_t)y * w;
    const uint8_t *v1 = (const uint8_t *)(block + ws.v1) + (size_t)y * w;
    for (int x = tid; x < w; x += SM_THREADS) {
        disp[x] = d16[x];
        val[x] = v1[x];
        if (valid_out) valid_out[row * w + x] = v1[x];
    }
    __syncthreads();
    sm_fill_row(disp, fil, val, w, d0, seg_last, seg_first);
    int16_t *out = (int16_t *)(block + ws.fil) + (size_t)y * w;
    for (int x = tid; x < w; x += SM_THREADS) out[x] = fil[x];
}

// ---- median, min / max, depth ---------------------------------------------------------------------------------------------------------
#define SM_SORT(a, b)                   \
    {                                   \
        const int lo_ = min(a, b);      \
        b = max(a, b);                  \
        a = lo_;                        \
    }

__global__ __launch_bounds__(SM_THREADS) void k_sm_median(int h, int w, sm_ws ws, int16_t *__restrict__ disparity)
{
    __shared__ int red[2][SM_THREADS / 64];
    const size_t plane = (size_t)h * w;
    const int img = blockIdx.y;
    char *block = ws.base + (size_t)img * ws.stride;
    const int16_t *fil = (const int16_t *)(block + ws.fil);
    int lo = INT_MAX, hi = INT_MIN;
    for (int j = 0; j < SM_MEDIAN_PER_THREAD; j++) {
        const size_t p = ((size_t)blockIdx.x * SM_MEDIAN_PER_THREAD + j) * SM_THREADS + threadIdx.x;
        if (p >= plane) break;
        const int y = (int)(p / (unsigned)w), x = (int)(p - (size_t)y * w);
        int v[9];
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const size_t yy = (size_t)min(max(y + dy, 0), h - 1);
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) v[3 * (dy + 1) + dx + 1] = fil[yy * w + min(max(x + dx, 0), w - 1)];
        }
        SM_SORT(v[1], v[2]) SM_SORT(v[4], v[5]) SM_SORT(v[7], v[8]) SM_SORT(v[0], v[1]) SM_SORT(v[3], v[4]) SM_SORT(v[6], v[7])
        SM_SORT(v[1], v[2]) SM_SORT(v[4], v[5]) SM_SORT(v[7], v[8]) SM_SORT(v[0], v[3]) SM_SORT(v[5], v[8]) SM_SORT(v[4], v[7])
        SM_SORT(v[3], v[6]) SM_SORT(v[1], v[4]) SM_SORT(v[2], v[5]) SM_SORT(v[4], v[7]) SM_SORT(v[4], v[2]) SM_SORT(v[6], v[4])
        SM_SORT(v[4], v[2])
        disparity[(size_t)img * plane + p] = (int16_t)v[4];
        lo = min(lo, v[4]);
        hi = max(hi, v[4]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SM_THREADS / 64; k++) {
            lo = min(lo, red[0][k]);
            hi = max(hi, red[1][k]);
        }
        int *mm = (int *)(block + ws.mm);
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

__global__ __launch_bounds__(SM_THREADS) void k_sm_depth(int h, int w, sm_ws ws, const int16_t *__restrict__ disparity, uint16_t *__restrict__ depth)
{
    const size_t plane = (size_t)h * w;
    const size_t p = (size_t)blockIdx.x * SM_THREADS + threadIdx.x;
    const int img = blockIdx.y;
    if (p >= plane) return;
    const int *mm = (const int *)(ws.base + (size_t)img * ws.stride + ws.mm);
    const int lo = mm[0], hi = mm[1];
    const size_t e = (size_t)img * plane + p;
    uint16_t out = 0;
    if (hi > lo) {
        const uint64_t range = (uint64_t)(hi - lo);
        out = (uint16_t)(((uint64_t)(disparity[e] - lo) * 131070u + range) / (2 * range));
    }
    depth[e] = out;
}

// ---- speckle filter (step 7b, ds_speckle_filter_i16) ------------------------------------------------------------------------------------
// Connected components of the graph "4-neighbours, both nodes, |disp difference| <= t" by union-find on links in the workspace, four
// launches of one thread per pixel:
//   k_sp_init     link[p] = p - 1 when p is linked to its left neighbour, else p; count[p] = 0.  Every link and counter is written here,
//                 so nothing below reads what the caller left in the workspace.
//   k_sp_merge    a pixel linked to its upper neighbour unites the two trees.
//   k_sp_count    link[p] = the root of p (the smallest index of its component); the root's counter gets one per pixel.
//   k_sp_write    size_out = the root's counter, valid_out = (it is above `size`).
// The invariant: link[p] <= p, a stored link only ever falls, and it always names a pixel of p's component.  So a walk along links
// strictly descends and ends at a pixel with link[p] == p after at most p steps, whatever other threads store meanwhile; and in
// sp_unite the larger of the two indices strictly falls from one round to the next (below), so it ends within h w rounds.  No thread
// waits for another: there is no flag, no grid barrier and no cooperative launch.  The components and their counts are properties
// of the graph, so the order in which the links fell cannot show in a result.
struct sp_args {
    const char *disp, *valid;           // int16 / uint8 planes
    char *link, *count, *valid_out, *size_out;                           // int32, uint32, uint8, uint32 (size_out may be null)
    size_t disp_stride, valid_stride, link_stride, count_stride, valid_out_stride, size_out_stride;      // bytes from image to image
    int h, w, t, size;
};

__device__ __forceinline__ int sp_root(const int *link, int p)
{
    for (int q = link[p]; q != p; q = link[p]) p = q;                     // q < p: a strict descent
    return p;
}

__device__ __forceinline__ void sp_unite(int *link, int a, int b)
{
    for (;;) {
        a = sp_root(link, a);
        b = sp_root(link, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = atomicMin(&link[a], b);                          // b < a: the stored link falls
        if (old == a) return;                                            // a was a root and now hangs below b
        a = old;                                                         // another thread hung a below old < a first: old and b remain to
    }                                                                    // be united, and max(old, b) < a
}

__global__ __launch_bounds__(SM_THREADS) void k_sp_init(sp_args a)
{
    const int plane = a.h * a.w;                                         // <= 2^28
    const int p = (int)(blockIdx.x * SM_THREADS + threadIdx.x), img = blockIdx.y;
    if (p >= plane) return;
    const int16_t *disp = (const int16_t *)(a.disp + (size_t)img * a.disp_stride);
    const uint8_t *valid = (const uint8_t *)(a.valid + (size_t)img * a.valid_stride);
    const int x = p % a.w;
    int to = p;
    if (x > 0 && valid[p] && valid[p - 1] && abs((int)disp[p] - (int)disp[p - 1]) <= a.t) to = p - 1;
    ((int *)(a.link + (size_t)img * a.link_stride))[p] = to;
    ((uint32_t *)(a.count + (size_t)img * a.count_stride))[p] = 0;
}

__global__ __launch_bounds__(SM_THREADS) void k_sp_merge(sp_args a)
{
    const int plane = a.h * a.w;
    const int p = (int)(blockIdx.x * SM_THREADS + threadIdx.x), img = blockIdx.y;
    if (p < a.w || p >= plane) return;                                   // row 0 has no upper neighbour
    const int16_t *disp = (const int16_t *)(a.disp + (size_t)img * a.disp_stride);
    const uint8_t *valid = (const uint8_t *)(a.valid + (size_t)img * a.valid_stride);
    const int q = p - a.w;
    if (!(valid[p] && valid[q] && abs((int)disp[p] - (int)disp[q]) <= a.t)) return;
    int *link = (int *)(a.link + (size_t)img * a.link_stride);
    sp_unite(link, p, q);
    const int r = sp_root(link, p);                                      // shorten the walks of the launches behind this one
    atomicMin(&link[p], r);
}

__global__ __launch_bounds__(SM_THREADS) void k_sp_count(sp_args a)
{
    const int plane = a.h * a.w;
    const int p = (int)(blockIdx.x * SM_THREADS + threadIdx.x), img = blockIdx.y;
    const uint8_t *valid = (const uint8_t *)(a.valid + (size_t)img * a.valid_stride);
    int *link = (int *)(a.link + (size_t)img * a.link_stride);
    uint32_t *count = (uint32_t *)(a.count + (size_t)img * a.count_stride);
    int r = -1;                                                          // no thread leaves before the ballot: all 64 lanes take part
    if (p < plane && valid[p]) {
        r = sp_root(link, p);
        link[p] = r;                                                     // (a walk of another thread that passes p meanwhile reads the
    }                                                                    // old link or the root: both lie on its way down)
    // the pixels of a wave mostly share a root: the lanes that share lane 0's add once for all of them
    const int lead = __builtin_amdgcn_readfirstlane(r);
    const bool with_lead = r >= 0 && r == lead;
    const unsigned long long mates = __ballot(with_lead);
    if (with_lead) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)mates) - 1) atomicAdd(&count[r], (uint32_t)__popcll(mates));
    } else if (r >= 0) {
        atomicAdd(&count[r], 1u);
    }
}

__global__ __launch_bounds__(SM_THREADS) void k_sp_write(sp_args a)
{
    const int plane = a.h * a.w;
    const int p = (int)(blockIdx.x * SM_THREADS + threadIdx.x), img = blockIdx.y;
    if (p >= plane) return;
    const uint8_t *valid = (const uint8_t *)(a.valid + (size_t)img * a.valid_stride);
    const int *link = (const int *)(a.link + (size_t)img * a.link_stride);
    const uint32_t *count = (const uint32_t *)(a.count + (size_t)img * a.count_stride);
    const uint32_t s = valid[p] ? count[link[p]] : 0u;                   // link[p]: the root, stored by this pixel's thread of k_sp_count
    (a.valid_out + (size_t)img * a.valid_out_stride)[p] = (char)(s > (uint32_t)a.size);
    if (a.size_out) ((uint32_t *)(a.size_out + (size_t)img * a.size_out_stride))[p] = s;
}

static void sp_launch(hipStream_t stream, int g, const sp_args &a)
{
    const dim3 grid((unsigned)(((size_t)a.h * a.w + SM_THREADS - 1) / SM_THREADS), (unsigned)g);
    hipLaunchKernelGGL(k_sp_init, grid, dim3(SM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_sp_merge, grid, dim3(SM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_sp_count, grid, dim3(SM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(k_sp_write, grid, dim3(SM_THREADS), 0, stream, a);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static bool sm_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

DS_API size_t ds_stereo_match_workspace_bytes(int h, int w, int D)
{
    if (h <= 0 || w <= 0 || h > SM_SIDE_MAX || w > SM_SIDE_MAX || (D != 32 && D != 64 && D != 128)) return 0;
    return sm_layout(nullptr, h, w, D).stride;
}

template <int G, int DPL>
static void sm_launch_paths(hipStream_t stream, int stages, int paths, int g, int h, int w, int d0, int P1, int P2, const sm_ws &ws)
{
    const int per_block = (SM_THREADS / 64) * (64 / G);
    const int rows = g * h, cols = g * w;                                 // < 2^30
    if (stages & SM_STAGE_HORIZONTAL)
        hipLaunchKernelGGL((k_sm_paths<G, DPL, SM_DIR_H>), dim3((unsigned)((rows + per_block - 1) / per_block)), dim3(SM_THREADS), 0, stream, h,
                           w, d0, P1, P2, h, rows, ws);
    if (stages & SM_STAGE_VERTICAL)
        hipLaunchKernelGGL((k_sm_paths<G, DPL, SM_DIR_V>), dim3((unsigned)((cols + per_block - 1) / per_block)), dim3(SM_THREADS), 0, stream, h,
                           w, d0, P1, P2, w, cols, ws);
    if (paths == 8 && (stages & SM_STAGE_DIAGONAL)) {
        const int per_image = h + w - 1, lines = g * per_image;           // <= 65535 * 32767 < 2^31
        const dim3 grid((unsigned)(((size_t)lines + per_block - 1) / per_block));
        hipLaunchKernelGGL((k_sm_paths<G, DPL, SM_DIR_DR>), grid, dim3(SM_THREADS), 0, stream, h, w, d0, P1, P2, per_image, lines, ws);
        hipLaunchKernelGGL((k_sm_paths<G, DPL, SM_DIR_DL>), grid, dim3(SM_THREADS), 0, stream, h, w, d0, P1, P2, per_image, lines, ws);
    }
}

template <int D>
static int sm_launch_winner(hipStream_t stream, int g, int h, int w, int d0, int u, int lr, int stop, const sm_ws &ws, uint8_t *valid)
{
    const size_t lds = 6 * (size_t)w;                                    // <= 96 KiB
    if (lds > 64 * 1024)
        DS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sm_winner<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         6 * SM_SIDE_MAX));
    hipLaunchKernelGGL((k_sm_winner<D>), dim3((unsigned)(g * h)), dim3(SM_THREADS), lds, stream, h, w, d0, u, lr, stop, ws, valid);
    return DS_OK;
}

static int sm_launch_speckle_fill(hipStream_t stream, int g, int h, int w, int d0, int speckle_size, int t, const sm_ws &ws, uint8_t *valid)
{
    sp_args a;
    a.disp = ws.base + ws.d16;
    a.valid = ws.base + ws.v0;
    a.link = ws.base + ws.par;
    a.count = ws.base + ws.cnt;
    a.valid_out = ws.base + ws.v1;
    a.size_out = nullptr;
    a.disp_stride = a.valid_stride = a.link_stride = a.count_stride = a.valid_out_stride = a.size_out_stride = ws.stride;
    a.h = h;
    a.w = w;
    a.t = t;
    a.size = speckle_size;
    sp_launch(stream, g, a);
    const size_t lds = 5 * (size_t)w;                                    // <= 80 KiB
    if (lds > 64 * 1024)
        DS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sm_fill), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * SM_SIDE_MAX));
    hipLaunchKernelGGL(k_sm_fill, dim3((unsigned)(g * h)), dim3(SM_THREADS), lds, stream, h, w, d0, ws, valid);
    return DS_OK;
}

// paths 4, speckle_size 0: ds_stereo_match_u8, launch for launch
static int sm_run(const char *who, int stages, ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0,
                  int P1, int P2, int u, int lr, int paths, int speckle_size, int speckle_range, void *workspace, int group,
                  int16_t *disparity, uint8_t *valid, uint16_t *depth, hipStream_t stream)
{
    DS_REQUIRE(ctx && left && right && workspace && disparity, DS_EINVAL, "%s: null argument", who);
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    DS_REQUIRE(c == 1 || c == 3 || c == 4, DS_EINVAL, "%s: c %d is not 1, 3 or 4", who, c);
    DS_REQUIRE(D == 32 || D == 64 || D == 128, DS_EINVAL, "%s: D %d is not 32, 64 or 128", who, D);
    DS_REQUIRE(d0 >= -128 && d0 <= 127, DS_EINVAL, "%s: d0 %d outside -128..127", who, d0);
    DS_REQUIRE(P1 >= 1 && P1 <= 64 && P2 >= P1 && P2 <= 255, DS_EINVAL, "%s: P1 %d outside 1..64 or P2 %d outside P1..255", who, P1, P2);
    DS_REQUIRE(u >= 0 && u <= 50, DS_EINVAL, "%s: u %d outside 0..50", who, u);
    DS_REQUIRE(lr >= -1 && lr <= 3, DS_EINVAL, "%s: lr %d outside -1..3", who, lr);
    DS_REQUIRE(paths == 4 || paths == 8, DS_EINVAL, "%s: paths %d is not 4 or 8", who, paths);
    DS_REQUIRE(speckle_size >= 0 && speckle_size <= 65535 && speckle_range >= 0 && speckle_range <= 16, DS_EINVAL,
               "%s: speckle_size %d outside 0..65535 or speckle_range %d outside 0..16", who, speckle_size, speckle_range);
    DS_REQUIRE(group >= 1 && group <= n, DS_EINVAL, "%s: group %d outside 1..n=%d", who, group, n);
    DS_REQUIRE(((uintptr_t)workspace & 255) == 0 && (((uintptr_t)disparity | (uintptr_t)depth) & 1) == 0, DS_EINVAL,
               "%s: workspace must be 256-byte aligned, disparity and depth 2-byte aligned", who);
    // the size limits come before the overlap test: below them every byte count fits 64 bits
    DS_REQUIRE(n <= 65535 && h <= SM_SIDE_MAX && w <= SM_SIDE_MAX, DS_EUNSUPPORTED,
               "%s: n must be <= 65535, h and w <= %d, got n=%d h=%d w=%d", who, SM_SIDE_MAX, n, h, w);
    const bool speckle = speckle_size > 0;
    const sm_ws layout = sm_layout(workspace, h, w, D, speckle);
    DS_REQUIRE(layout.stride <= ((size_t)1 << 31), DS_EUNSUPPORTED,
               "%s: one image's workspace is %zu bytes, above 2 GiB (h=%d w=%d D=%d)", who, layout.stride, h, w, D);
    const size_t plane = (size_t)h * w, count = (size_t)n * plane;
    const void *in[2] = {left, right};
    void *outs[4] = {disparity, workspace, valid, depth};
    const size_t out_bytes[4] = {2 * count, layout.stride * (size_t)group, count, 2 * count};
    for (int o = 0; o < 4; o++) {
        if (!outs[o]) continue;
        for (int i = 0; i < 2; i++)
            DS_REQUIRE(!sm_overlap(outs[o], out_bytes[o], in[i], count * c), DS_EINVAL, "%s: an output or the workspace overlaps an input", who);
        for (int q = 0; q < o; q++)
            DS_REQUIRE(!(outs[q] && sm_overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])), DS_EINVAL,
                       "%s: disparity, valid, depth and the workspace overlap", who);
    }
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned pixel_blocks = (unsigned)((plane + SM_THREADS - 1) / SM_THREADS);                                   // <= 2^20
    const unsigned median_blocks = (unsigned)((plane + SM_THREADS * SM_MEDIAN_PER_THREAD - 1) / (SM_THREADS * SM_MEDIAN_PER_THREAD));
    for (int i0 = 0; i0 < n; i0 += group) {
        const int g = n - i0 < group ? n - i0 : group;
        const size_t first = (size_t)i0 * plane;
        uint8_t *valid_g = valid ? valid + first : nullptr;
        if (stages & SM_STAGE_CENSUS)
            hipLaunchKernelGGL(k_sm_census, dim3(pixel_blocks, g, 2), dim3(SM_THREADS), 0, stream, left + first * c, right + first * c, h, w, c,
                               layout);
        int rc = DS_OK;
        if (D == 32) {
            sm_launch_paths<32, 1>(stream, stages, paths, g, h, w, d0, P1, P2, layout);
            if (stages & SM_STAGE_WINNER) rc = sm_launch_winner<32>(stream, g, h, w, d0, u, lr, speckle, layout, valid_g);
        } else if (D == 64) {
            sm_launch_paths<64, 1>(stream, stages, paths, g, h, w, d0, P1, P2, layout);
            if (stages & SM_STAGE_WINNER) rc = sm_launch_winner<64>(stream, g, h, w, d0, u, lr, speckle, layout, valid_g);
        } else {
            sm_launch_paths<64, 2>(stream, stages, paths, g, h, w, d0, P1, P2, layout);
            if (stages & SM_STAGE_WINNER) rc = sm_launch_winner<128>(stream, g, h, w, d0, u, lr, speckle, layout, valid_g);
        }
        if (rc != DS_OK) return rc;
        if (speckle && (stages & SM_STAGE_SPECKLE)) rc = sm_launch_speckle_fill(stream, g, h, w, d0, speckle_size, 16 * speckle_range, layout, valid_g);
        if (rc != DS_OK) return rc;
        if (stages & SM_STAGE_MEDIAN)
            hipLaunchKernelGGL(k_sm_median, dim3(median_blocks, g), dim3(SM_THREADS), 0, stream, h, w, layout, disparity + first);
        if (depth && (stages & SM_STAGE_DEPTH))
            hipLaunchKernelGGL(k_sm_depth, dim3(pixel_blocks, g), dim3(SM_THREADS), 0, stream, h, w, layout, disparity + first, depth + first);
    }
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

DS_API int ds_stereo_match_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1, int P2,
                              int u, int lr, void *workspace, int group, int16_t *disparity, uint8_t *valid, uint16_t *depth, void *stream)
{
    return sm_run("ds_stereo_match_u8", SM_STAGE_ALL, ctx, left, right, n, h, w, c, D, d0, P1, P2, u, lr, 4, 0, 0, workspace, group, disparity,
                  valid, depth, (hipStream_t)stream);
}

DS_API int ds_stereo_match_stages_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1,
                                     int P2, int u, int lr, void *workspace, int group, int16_t *disparity, uint8_t *valid, uint16_t *depth,
                                     int stages, void *stream)
{
    DS_REQUIRE(stages >= 1 && stages <= SM_STAGE_ALL, DS_EINVAL, "ds_stereo_match_stages_u8: stages %d outside 1..%d", stages, SM_STAGE_ALL);
    return sm_run("ds_stereo_match_stages_u8", stages, ctx, left, right, n, h, w, c, D, d0, P1, P2, u, lr, 4, 0, 0, workspace, group, disparity,
                  valid, depth, (hipStream_t)stream);
}

DS_API size_t ds_stereo_match_ex_workspace_bytes(int h, int w, int D, int paths, int speckle_size)
{
    if (h <= 0 || w <= 0 || h > SM_SIDE_MAX || w > SM_SIDE_MAX || (D != 32 && D != 64 && D != 128)) return 0;
    if ((paths != 4 && paths != 8) || speckle_size < 0 || speckle_size > 65535) return 0;
    return sm_layout(nullptr, h, w, D, speckle_size > 0).stride;
}

DS_API int ds_stereo_match_ex_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1,
                                 int P2, int u, int lr, int paths, int speckle_size, int speckle_range, void *workspace, int group,
                                 int16_t *disparity, uint8_t *valid, uint16_t *depth, void *stream)
{
    return sm_run("ds_stereo_match_ex_u8", SM_STAGE_EX_ALL, ctx, left, right, n, h, w, c, D, d0, P1, P2, u, lr, paths, speckle_size, speckle_range,
                  workspace, group, disparity, valid, depth, (hipStream_t)stream);
}

DS_API int ds_stereo_match_ex_stages_u8(ds_ctx *ctx, const uint8_t *left, const uint8_t *right, int n, int h, int w, int c, int D, int d0, int P1,
                                        int P2, int u, int lr, int paths, int speckle_size, int speckle_range, void *workspace, int group,
                                        int16_t *disparity, uint8_t *valid, uint16_t *depth, int stages, void *stream)
{
    DS_REQUIRE(stages >= 1 && stages <= SM_STAGE_EX_ALL, DS_EINVAL, "ds_stereo_match_ex_stages_u8: stages %d outside 1..%d", stages,
               SM_STAGE_EX_ALL);
    return sm_run("ds_stereo_match_ex_stages_u8", stages, ctx, left, right, n, h, w, c, D, d0, P1, P2, u, lr, paths, speckle_size, speckle_range,
                  workspace, group, disparity, valid, depth, (hipStream_t)stream);
}

DS_API size_t ds_speckle_filter_workspace_bytes(int h, int w)
{
    if (h <= 0 || w <= 0 || h > SM_SIDE_MAX || w > SM_SIDE_MAX) return 0;
    return 2 * sm_r256(4 * (size_t)h * w);                                // links, counters
}

DS_API int ds_speckle_filter_i16(ds_ctx *ctx, const int16_t *disp, const uint8_t *valid, int n, int h, int w, int size, int t, void *workspace,
                                 int group, uint8_t *valid_out, uint32_t *size_out, void *stream)
{
    const char *who = "ds_speckle_filter_i16";
    DS_REQUIRE(ctx && disp && valid && workspace && valid_out, DS_EINVAL, "%s: null argument", who);
    DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    DS_REQUIRE(size >= 1 && size <= 65535 && t >= 0 && t <= 65535, DS_EINVAL, "%s: size %d outside 1..65535 or t %d outside 0..65535", who, size, t);
    DS_REQUIRE(group >= 1 && group <= n, DS_EINVAL, "%s: group %d outside 1..n=%d", who, group, n);
    DS_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)disp & 1) == 0 && ((uintptr_t)size_out & 3) == 0, DS_EINVAL,
               "%s: workspace must be 256-byte aligned, disp 2-byte and size_out 4-byte aligned", who);
    DS_REQUIRE(n <= 65535 && h <= SM_SIDE_MAX && w <= SM_SIDE_MAX, DS_EUNSUPPORTED,
               "%s: n must be <= 65535, h and w <= %d, got n=%d h=%d w=%d", who, SM_SIDE_MAX, n, h, w);
    const size_t plane = (size_t)h * w, count = (size_t)n * plane, part = sm_r256(4 * plane), share = 2 * part;
    DS_REQUIRE(share <= ((size_t)1 << 31), DS_EUNSUPPORTED, "%s: one image's workspace is %zu bytes, above 2 GiB (h=%d w=%d)", who, share, h, w);
    const void *in[2] = {disp, valid};
    const size_t in_bytes[2] = {2 * count, count};
    void *outs[3] = {valid_out, workspace, size_out};
    const size_t out_bytes[3] = {count, share * (size_t)group, 4 * count};
    for (int o = 0; o < 3; o++) {
        if (!outs[o]) continue;
        for (int i = 0; i < 2; i++)
            DS_REQUIRE(!sm_overlap(outs[o], out_bytes[o], in[i], in_bytes[i]), DS_EINVAL, "%s: an output or the workspace overlaps an input", who);
        for (int q = 0; q < o; q++)
            DS_REQUIRE(!(outs[q] && sm_overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])), DS_EINVAL,
                       "%s: valid_out, size_out and the workspace overlap", who);
    }
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    for (int i0 = 0; i0 < n; i0 += group) {
        const int g = n - i0 < group ? n - i0 : group;
        const size_t first = (size_t)i0 * plane;
        sp_args a;
        a.disp = (const char *)(disp + first);
        a.valid = (const char *)(valid + first);
        a.link = (char *)workspace;
        a.count = (char *)workspace + part;
        a.valid_out = (char *)(valid_out + first);
        a.size_out = size_out ? (char *)(size_out + first) : nullptr;
        a.disp_stride = 2 * plane;
        a.valid_stride = a.valid_out_stride = plane;
        a.link_stride = a.count_stride = share;
        a.size_out_stride = 4 * plane;
        a.h = h;
        a.w = w;
        a.t = t;
        a.size = size;
        sp_launch((hipStream_t)stream, g, a);
    }
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
