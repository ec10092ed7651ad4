// The pieces every member of the bilateral family shares: the two spatial kernels of ds_bilateral.hip and the temporal one of
// ds_video.hip.  The rules of the family are stated HERE, once; the kernels' comments point here.
//   * Taps are visited in ONE fixed order (raster order of the window; frame order along time), one accumulation chain per pixel.
//   * A tap whose spatial (temporal) weight is exactly 0 does not enter the sums: skipped, or given +0.0, which leaves both sums as
//     they are bit for bit (every term is >= +0.0 and finite).
//   * ds_bl_tap: every product and every sum is rounded on its own -- no fused multiply-add.  This relies on contraction being OFF
//     (the pragma below and the library's -ffp-contract=off), not on __dmul_rn / __dadd_rn, which are plain `*` and `+` here.
//   * ds_bl_finish_u16: ONE IEEE division per output, then round half to even (v_rndne_f64); no clamp, the quotient is a convex
//     combination of uint16 values.
//   * The colour weight's argument is the INTEGER k = |dR| + |dG| + |dB| of two guide pixels, 0..DS_BL_WC - 1: both guide pixels are
//     packed words (R, G, B, 0), so k is ONE v_sad_u8, and it lies inside the table by construction.
#pragma once
#include "ds_common.h"

#pragma clang fp contract(off)

#define DS_BL_WC 766                // 3 * 255 + 1 colour differences: the length of wc

// A guide pixel as the packed word (R, G, B, 0): three byte loads -- any alignment, the fourth byte (alpha, or the next pixel) never read.
__device__ __forceinline__ uint32_t ds_bl_rgb(const uint8_t *px)
{
    return (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
}

// All of wc into LDS, by a workgroup of `threads`; the caller's __syncthreads() publishes it.
__device__ __forceinline__ void ds_bl_stage_wc(double *wc_lds, const double *__restrict__ wc, int tid, int threads)
{
    for (int i = tid; i < DS_BL_WC; i += threads) wc_lds[i] = wc[i];
}

// One tap of one chain: s the spatial (temporal) weight, r the range (colour) weight, v the tap's uint16 depth.
__device__ __forceinline__ void ds_bl_tap(double s, double r, uint32_t v, double &num, double &den)
{
    const double wgt = s * r;
    const double p = wgt * (double)v;
    num = num + p;
    den = den + wgt;
}

__device__ __forceinline__ uint16_t ds_bl_finish_u16(double num, double den)
{
    return (uint16_t)(unsigned)__builtin_rint(num / den);
}
