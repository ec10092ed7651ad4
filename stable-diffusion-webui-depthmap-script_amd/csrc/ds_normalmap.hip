// ds_normalmap: create_normalmap (reference: src/normalmap_generation.py:5-56) on gfx950.
//
// Fused path (uint16, no blur): a lane reads the 3x3 (Sobel) or 4-neighbour (np.gradient) uint16 neighbourhood of one or four
// output pixels, does the float64 arithmetic of :20-54 and writes 3 bytes per pixel.  With inputs that are multiples of 2^-8 every
// sum is exact, so only sqrt and the three divisions round -- and those are correctly rounded IEEE operations on the device, hence
// bit-exact results.
//
// Every other route runs numpy's arithmetic in the dtype numpy uses (NmPrec: float64, float32, float16), with each rule -- the
// np.gradient stencil, normalise, quantise, the separable pass, the Gaussian taps, the host pipeline -- written once: np.gradient
// without blurs on float32 / float16 in one fused pass; Gaussian pre/post blur and Sobel of any size as separable passes over
// planes in the context's scratch, rows first then columns, taps accumulated in order (BORDER_REFLECT_101, or modulo under WRAP).
#include <math.h>

#include <type_traits>

#include "ds_common.h"

// ---- border mode (compile-time WRAP of every kernel that looks across the border) ---------------------------------------------------
// WRAP 0: the reference's borders -- BORDER_REFLECT_101 for cv2.Sobel / cv2.GaussianBlur, one-sided differences at the two ends for
//         np.gradient.
// WRAP 1: the image is one period of a tiling: every tap index is taken modulo the image size (a true modulo: a 63-tap kernel on a
//         5-pixel row is legal), and np.gradient is the halved central difference at every pixel, the two ends included.  Same tap
//         order, operation order and roundings: the result is normalmap(np.pad(d, R, mode='wrap'))[R:R+h, R:R+w] bit for bit (R = the
//         summed radii of the passes), and it commutes with np.roll.  (The reference leaves this open: src/normalmap_generation.py:16,
//         "TODO: Tiling can be improved (gradients could be matched)".)
// The index rules themselves (ds_reflect101, ds_mod, ds_wrap_prev / ds_wrap_next) live in ds_common.h.

// np.gradient (:31) along one axis at position i of n >= 2 samples, as a pair of taps: the value is f[*hi] - f[*lo], halved when the
// function returns true.  Reference borders: one-sided differences at the two ends (f[1] - f[0], f[n-1] - f[n-2]), the halved central
// difference inside.  WRAP: the halved central difference everywhere, neighbours modulo n.  Every np.gradient of this file is this.
template <int WRAP>
__device__ __forceinline__ bool nm_gradient_taps(int i, int n, int *lo, int *hi)
{
    if (WRAP) { *lo = ds_wrap_prev(i, n); *hi = ds_wrap_next(i, n); return true; }
    *lo = i > 0 ? i - 1 : 0;
    *hi = i < n - 1 ? i + 1 : n - 1;
    return i > 0 && i < n - 1;
}

#define NM_BX 64
#define NM_BY 4

// ---- uint16 depth, no blur, Sobel 3 or np.gradient: the fused kernels ---------------------------------------------------------------
// normal = (zx, -zy, 1)/|.| ; (+1)/2*256 clipped to [0, 255.9] ; truncate   (:34-39, :51-54)
// The kernels are bound by float64 VALU issue, not by memory (round 3: ~160 vector instructions per pixel; round 4: 62.8 M vector
// instructions per 32 x 1024^2 launch, 121-140 us against 35-40 us of memory time), so the arithmetic is kept to what the result
// needs (round 6: ~60 instead of ~140 vector instructions per pixel):
//   * the Sobel / np.gradient sums in INTEGERS.  The operands are uint16 / 256: every sum of the reference is exact in float64, so
//     the same real number comes out of  Zx = (e02 - e00) + 2 (e12 - e10) + (e22 - e20)  in int32 and ONE conversion + ONE multiply
//     by +-2^-8 (+-2^-9 for np.gradient's halved interior differences) -- instead of 18 conversions, 36 scalings and 10 float64
//     adds per four pixels;
//   * n^2 = fma(nx, nx, fma(ny, ny, 1)): exact (a multiple of 2^-18 below 2^22), so the two fused operations round nothing;
//   * sqrt and 1 / n WITHOUT the range scaling and the special-case fix-ups of the generic expansions: n^2 lies in [1, 2^22], n in
//     [1, 2^11] -- nm_sqrt / nm_rcp below are the compiler's own Newton / Goldschmidt sequences (AMDGPU lowering of llvm.sqrt.f64 and
//     of the float64 division) minus v_div_scale / v_ldexp / v_div_fixup and their compares and selects: the same instructions on the
//     same operands, bit for bit (tests/test_gpu_parity.py compares them with sqrt() and 1.0 / n on 2^27 operands of the domain);
//   * ONE division, y = 1 / n: it is the z component, and the correctly rounded reciprocal turns the other two quotients into
//     q0 = a y;  r = fma(-q0, n, a);  q = fma(r, y, q0)  -- Markstein's sequence, equal to the correctly rounded a / n for every
//     operand of these kernels (the significand of n is never all ones; enumerated by check_normal_division.c, which the test
//     suite builds and runs). n >= 1: no NaN, no zero divisor.  a = -0.0 gives +0.0 where the division gives -0.0: v + 1 is
//     1.0 either way;
//   * (v + 1) / 2 * 256 = (v + 1) * 128 bit for bit (scaling by a power of two never rounds), as fma(v, 128, 128) (the scaling
//     commutes with the rounding of v + 1), the upper clip as one v_min_f64 instead of compare + two 32-bit selects, and NO lower
//     clip: |q| <= 1 because n >= |nx| (sqrt is monotonic and correctly rounded, |nx| is representable), so the value is never
//     negative;
//   * after the clip the value lies in [0, 255.9]: the float64 -> uint8 cast is one v_cvt_i32_f64, not the general numpy
//     emulation (ds_f64_to_u8: int64 conversion + wrap) the unclipped paths of the stereo kernels need.
// nm_pixel below is that arithmetic, and the ONLY one uint16 maps have: both fused kernels form the integer sums and call it.
__device__ __forceinline__ double nm_sqrt(double x)                 // x in [1, 2^22]: correctly rounded, as sqrt(x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}

__device__ __forceinline__ double nm_rcp(double n)                  // n in [1, 2^11]: correctly rounded, as 1.0 / n
{
    double y = __builtin_amdgcn_rcp(n);
    y = __builtin_fma(y, __builtin_fma(-n, y, 1.0), y);
    y = __builtin_fma(y, __builtin_fma(-n, y, 1.0), y);
    return __builtin_fma(__builtin_fma(-n, y, 1.0), y, y);
}

// one pixel: Zx, Zy = the integer gradient sums, kx, ky = their scales (sign of the inversion included; ky also carries the minus
// sign of (zx, -zy, 1)); three bytes out
__device__ __forceinline__ uint32_t nm_pixel(int Zx, int Zy, double kx, double ky)
{
    const double nx = (double)Zx * kx, ny = (double)Zy * ky;
    const double n = nm_sqrt(__builtin_fma(nx, nx, __builtin_fma(ny, ny, 1.0)));
    const double y = nm_rcp(n);
    const double qx0 = nx * y, qy0 = ny * y;
    const double v[3] = { __builtin_fma(__builtin_fma(-qx0, n, nx), y, qx0), __builtin_fma(__builtin_fma(-qy0, n, ny), y, qy0), y };
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) o |= (uint32_t)(int)__builtin_fmin(__builtin_fma(v[k], 128.0, 128.0), 256.0 - 0.1) << (8 * k);
    return o;
}

// ds_normalmap_selfcheck: nm_sqrt / nm_rcp against the generic operations over a range of the operand domain, n^2 = K / 2^18 for
// K = k0 + stride * i (every n^2 the kernels can form is such a value with K in [2^18, 2^40))
__global__ void k_nm_check_sqrt_rcp(unsigned long long k0, unsigned long long stride, unsigned long long count, unsigned long long *bad)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * blockDim.x) {
        const double x = (double)(k0 + stride * i) * (1.0 / 262144.0);
        const double a = nm_sqrt(x), b = sqrt(x);
        if (a != b || nm_rcp(b) != 1.0 / b) atomicAdd(bad, 1ull);
    }
}

// Four pixels per lane (w % 4 == 0): the three input rows arrive as one aligned 8-byte load each plus the two edge columns,
// the 12 output bytes leave as three aligned 32-bit stores (round 1: one pixel per lane, three single-byte stores -- 0.20 ms
// per 32 x 1024^2 = 10 % of the HBM roofline).
template <int SOBEL3, int WRAP>
__global__ __launch_bounds__(NM_BX * NM_BY) void k_normalmap_fused4(const uint16_t *__restrict__ depth, int h, int w, int invert,
                                                                    uint8_t *__restrict__ out)
{
    const int img = blockIdx.z;
    const int x0 = (blockIdx.x * NM_BX + threadIdx.x) * 4;
    const int y = blockIdx.y * NM_BY + threadIdx.y;
    if (x0 >= w || y >= h) return;
    const uint16_t *d = depth + (size_t)img * h * w;
    const double sgn = invert ? 1.0 : -1.0;                                                 /* :20: depthmap * (-1.0) unless inverted */
    // rows y-1, y, y+1 and columns x0-1 .. x0+4; outside the image: BORDER_REFLECT_101 for Sobel, clamped (unused) for gradient;
    // WRAP: the row / column on the opposite side (x0 and x0 + 3 are inside the image: only x0 - 1 and x0 + 4 can leave it)
    int ry[3], cl, cr;
    if (WRAP) {
        ry[0] = ds_wrap_prev(y, h); ry[2] = ds_wrap_next(y, h);
        cl = x0 > 0 ? x0 - 1 : w - 1; cr = x0 + 4 < w ? x0 + 4 : 0;
    } else if (SOBEL3) {
        ry[0] = ds_reflect101(y - 1, h); ry[2] = ds_reflect101(y + 1, h);
        cl = ds_reflect101(x0 - 1, w); cr = ds_reflect101(x0 + 4, w);
    } else {
        ry[0] = y > 0 ? y - 1 : 0; ry[2] = y < h - 1 ? y + 1 : h - 1;
        cl = x0 > 0 ? x0 - 1 : 0; cr = x0 + 4 < w ? x0 + 4 : w - 1;
    }
    ry[1] = y;
    int e[3][6];                                                                            /* depth codes: value = sgn * e / 256 (:20-21) */
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const uint16_t *row = d + (size_t)ry[r] * w;
        const uint2 q = *reinterpret_cast<const uint2 *>(row + x0);
        e[r][0] = row[cl]; e[r][1] = (int)(q.x & 0xffffu); e[r][2] = (int)(q.x >> 16);
        e[r][3] = (int)(q.y & 0xffffu); e[r][4] = (int)(q.y >> 16); e[r][5] = row[cr];
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int x = x0 + i;
        int Zx, Zy;
        double kx = sgn * (1.0 / 256.0), ky = -kx;
        if (SOBEL3) {
            Zx = (e[0][i + 2] - e[0][i]) + 2 * (e[1][i + 2] - e[1][i]) + (e[2][i + 2] - e[2][i]);        /* cv2.Sobel dx, ksize 3 */
            Zy = (e[2][i] - e[0][i]) + 2 * (e[2][i + 1] - e[0][i + 1]) + (e[2][i + 2] - e[0][i + 2]);    /* cv2.Sobel dy, ksize 3 */
        } else if (WRAP) {                                                                               /* halved central differences everywhere */
            Zx = e[1][i + 2] - e[1][i]; kx *= 0.5;
            Zy = e[2][i + 1] - e[0][i + 1]; ky *= 0.5;
        } else {                                                                                         /* np.gradient, :31 */
            if (x == 0) Zx = e[1][i + 2] - e[1][i + 1];
            else if (x == w - 1) Zx = e[1][i + 1] - e[1][i];
            else { Zx = e[1][i + 2] - e[1][i]; kx *= 0.5; }
            if (y == 0) Zy = e[2][i + 1] - e[1][i + 1];
            else if (y == h - 1) Zy = e[1][i + 1] - e[0][i + 1];
            else { Zy = e[2][i + 1] - e[0][i + 1]; ky *= 0.5; }
        }
        o[i] = nm_pixel(Zx, Zy, kx, ky);
    }
    uint32_t *dst = reinterpret_cast<uint32_t *>(out + ((size_t)img * h * w + (size_t)y * w + x0) * 3);
    dst[0] = o[0] | (o[1] << 24);
    dst[1] = (o[1] >> 8) | (o[2] << 16);
    dst[2] = (o[2] >> 16) | (o[3] << 8);
}

// One pixel per lane: every shape and alignment fused4 does not take -- w % 4 != 0, a misaligned pointer, and the single-row and
// single-column Sobel maps (h == 1 or w == 1: ds_reflect101 and the wrap steps both return index 0 for n == 1).  The same integer
// sums and scales as fused4 and the same nm_pixel, so the two kernels agree bit for bit by construction.
template <int SOBEL3, int WRAP>
__global__ __launch_bounds__(NM_BX * NM_BY) void k_normalmap_fused(const uint16_t *__restrict__ depth, int h, int w, int invert,
                                                                   uint8_t *__restrict__ out)
{
    const int img = blockIdx.z;
    const int x = blockIdx.x * NM_BX + threadIdx.x;
    const int y = blockIdx.y * NM_BY + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint16_t *d = depth + (size_t)img * h * w;
    const double sgn = invert ? 1.0 : -1.0;                                     /* :20: depthmap * (-1.0) unless inverted */
#define NME(yy, xx) ((int)d[(size_t)(yy) * w + (xx)])                           /* depth code: value = sgn * e / 256 (:20-21) */
    int Zx, Zy;
    double kx = sgn * (1.0 / 256.0), ky = -kx;
    if (SOBEL3) {
        const int xm = WRAP ? ds_wrap_prev(x, w) : ds_reflect101(x - 1, w), xp = WRAP ? ds_wrap_next(x, w) : ds_reflect101(x + 1, w);
        const int ym = WRAP ? ds_wrap_prev(y, h) : ds_reflect101(y - 1, h), yp = WRAP ? ds_wrap_next(y, h) : ds_reflect101(y + 1, h);
        const int e00 = NME(ym, xm), e01 = NME(ym, x), e02 = NME(ym, xp);
        const int e10 = NME(y, xm), e12 = NME(y, xp);
        const int e20 = NME(yp, xm), e21 = NME(yp, x), e22 = NME(yp, xp);
        Zx = (e02 - e00) + 2 * (e12 - e10) + (e22 - e20);                       /* cv2.Sobel dx, ksize 3 */
        Zy = (e20 - e00) + 2 * (e21 - e01) + (e22 - e02);                       /* cv2.Sobel dy, ksize 3 */
    } else {                                                                    /* np.gradient, :31 */
        int lo, hi;
        if (nm_gradient_taps<WRAP>(x, w, &lo, &hi)) kx *= 0.5;
        Zx = NME(y, hi) - NME(y, lo);
        if (nm_gradient_taps<WRAP>(y, h, &lo, &hi)) ky *= 0.5;
        Zy = NME(hi, x) - NME(lo, x);
    }
#undef NME
    const uint32_t o = nm_pixel(Zx, Zy, kx, ky);
    uint8_t *dst = out + ((size_t)img * h * w + (size_t)y * w + x) * 3;
    dst[0] = (uint8_t)o; dst[1] = (uint8_t)(o >> 8); dst[2] = (uint8_t)(o >> 16);
}

// ---- every other route: numpy's arithmetic in the dtype numpy uses, stated once ---------------------------------------------------
// NmPrec<S> is the precision of a route: S the storage type of the depth map and of the planes, C the type the operations run in,
// rnd() what becomes of the result of EVERY operation, hi() np.clip's upper bound 256 - 0.1 in the array's dtype (NEP 50), root()
// and div() the correctly rounded sqrt and division.  The library is built with -ffp-contract=off and without fast-math, so each
// C++ operator below is one IEEE operation.
//   double    any dtype the reference promotes to float64 (:20-21), and uint16 maps that need a blur or another Sobel size.
//   float     float32 depth with np.gradient (:31), the one combination the reference runs in float32 from end to end: `depthmap *
//             (-1.0) / 256.0` keeps float32, np.gradient, np.dstack, np.linalg.norm (x * x element-wise, the three squares added
//             left to right, sqrt), the three divisions and `+= 1; /= 2; * 256; clip` are float32 operations, each correctly
//             rounded.  With blurs the reference hands float32 arrays to cv2.GaussianBlur (:24 the depth plane, :43 the
//             three-channel normal), which filters CV_32F data with CV_32F coefficients and float32 accumulators.  OpenCV's own
//             summation order inside the separable filter is not reproducible without the library (cv2 is absent from the image:
//             the blur arithmetic is a stand-in, tests hold it to one LSB); the structure is the reference's.
//   _Float16  float16 depth with np.gradient and no blur (round 6): numpy keeps float16 from end to end (`* (-1.0)` and `/ 256.0`
//             with Python scalars do not promote; np.gradient allocates its output in the input's inexact dtype; np.dstack,
//             np.linalg.norm, the in-place divisions and the quantisation stay float16).  numpy's float16 loops convert the
//             operands to float32, operate, and round the float32 result to half: that IS the correctly rounded half operation for
//             + - * / sqrt (24 >= 2 * 11 + 2 bits), hence C = float and rnd = the rounding to half.  np.linalg.norm's add.reduce over
//             the three squares is the one multi-operand step: HALF_add's reduce loop keeps a FLOAT32 accumulator, adds the squares
//             left to right and rounds to half once (established on numpy 2.2 with operand triples on which (s0 + s1) + s2,
//             s0 + (s1 + s2) and the half-rounded chain differ: a CPU test holds numpy to it) -- nm_normalize is written that way
//             for all three precisions; with the identity rounding it is the plain left-to-right sum.
template <typename S> struct NmPrec;
template <> struct NmPrec<double> {
    typedef double S; typedef double C;
    __device__ static __forceinline__ C rnd(C x) { return x; }
    __device__ static __forceinline__ C hi() { return 256.0 - 0.1; }
    __device__ static __forceinline__ C root(C x) { return sqrt(x); }
    __device__ static __forceinline__ C div(C a, C b) { return a / b; }
};
template <> struct NmPrec<float> {
    typedef float S; typedef float C;
    __device__ static __forceinline__ C rnd(C x) { return x; }
    __device__ static __forceinline__ C hi() { return (float)(256 - 0.1); }
    __device__ static __forceinline__ C root(C x) { return __fsqrt_rn(x); }
    __device__ static __forceinline__ C div(C a, C b) { return __fdiv_rn(a, b); }
};
template <> struct NmPrec<_Float16> {
    typedef _Float16 S; typedef float C;
    __device__ static __forceinline__ C rnd(C x) { return (float)(_Float16)x; }
    __device__ static __forceinline__ C hi() { return (float)(_Float16)(256 - 0.1); }                 // 255.875
    __device__ static __forceinline__ C root(C x) { return __fsqrt_rn(x); }
    __device__ static __forceinline__ C div(C a, C b) { return __fdiv_rn(a, b); }
};

// depthmap * (-1.0 unless inverted) / 256.0   (:20-21)
template <typename P>
__device__ __forceinline__ typename P::C nm_scale(typename P::C v, typename P::C sgn)
{
    return P::rnd(P::rnd(v * sgn) / (typename P::C)256);
}

// (a) np.gradient (:31) along one axis: f(j) is the sample at index j of that axis.  numpy divides the one-sided differences by the
// spacing 1.0 and the central one by 2.0.
template <typename P, int WRAP, typename F>
__device__ __forceinline__ typename P::C nm_gradient1(int i, int n, F f)
{
    typedef typename P::C C;
    int lo, hi;
    const bool halved = nm_gradient_taps<WRAP>(i, n, &lo, &hi);
    const C d = P::rnd(f(hi) - f(lo));
    return P::rnd(halved ? d / (C)2 : d / (C)1);
}

// (b) v / |v| as np.linalg.norm and the three divisions do it (:34-39, :45-48): the squares rounded, added left to right in C with
// ONE rounding of the sum, sqrt, three divisions
template <typename P>
__device__ __forceinline__ void nm_normalize(typename P::C v[3])
{
    typedef typename P::C C;
    C s = P::rnd(v[0] * v[0]);
    s = s + P::rnd(v[1] * v[1]);
    s = s + P::rnd(v[2] * v[2]);
    const C n = P::rnd(P::root(P::rnd(s)));
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = P::rnd(P::div(v[k], n));
}

// (c) one component to its byte (:51-54): + 1, / 2, * 256, np.clip(., 0, 256 - 0.1), astype(uint8) -- inside [0, 255.9] that is a
// plain truncation; a NaN (it passes both clips) gives 0
template <typename P>
__device__ __forceinline__ uint8_t nm_quantize(typename P::C v)
{
    typedef typename P::C C;
    C t = P::rnd(v + (C)1);
    t = P::rnd(t / (C)2);
    t = P::rnd(t * (C)256);
    t = t < (C)0 ? (C)0 : t;
    t = t > P::hi() ? P::hi() : t;
    return (t == t) ? (uint8_t)(int)t : (uint8_t)0;
}

// np.gradient at pixel (y, x) of an h x w plane whose sample (yy, xx) is ld(yy, xx), and the first normalisation: v = the unit
// normal (gx, -gy, 1) / |.|   (:31-39)
template <typename P, int WRAP, typename L>
__device__ __forceinline__ void nm_gradient_normal(L ld, int y, int x, int h, int w, typename P::C v[3])
{
    typedef typename P::C C;
    v[0] = nm_gradient1<P, WRAP>(x, w, [&](int j) { return ld(y, j); });
    v[1] = -nm_gradient1<P, WRAP>(y, h, [&](int j) { return ld(j, x); });
    v[2] = (C)1;
    nm_normalize<P>(v);
}

// np.gradient without blurs on float32 / float16 depth: one fused pass from the depth map to the bytes
template <typename S, int WRAP>
__global__ __launch_bounds__(256) void k_nm_gradient_fused(const S *__restrict__ depth, int h, int w, int invert, uint8_t *__restrict__ out)
{
    typedef NmPrec<S> P;
    typedef typename P::C C;
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const S *p = depth + (size_t)img * h * w;
    const C sgn = invert ? (C)1 : (C)-1;
    C v[3];
    nm_gradient_normal<P, WRAP>([&](int yy, int xx) { return nm_scale<P>((C)p[(size_t)yy * w + xx], sgn); }, y, x, h, w, v);
    uint8_t *o = out + ((size_t)img * h * w + (size_t)y * w + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = nm_quantize<P>(v[k]);
}

// ---- planes path (Gaussian pre / post blur, Sobel of any size, float64 np.gradient): separable passes over planes of T ------------
#define NM_MAXK 63
template <typename T> struct NmKernel { T cf[NM_MAXK]; int n; };

template <typename Tin, typename T>
__global__ __launch_bounds__(256) void k_nm_load(const Tin *__restrict__ depth, int64_t count, int invert, T *__restrict__ plane)
{
    const T sgn = invert ? (T)1 : (T)-1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
        plane[i] = nm_scale<NmPrec<T> >((T)depth[i], sgn);
}

// one separable pass along x (AXIS 0) or y (AXIS 1): out = sum_k cf[k] * in[reflect101(pos + k - r)]
// (WRAP: in[(pos + k - r) mod size] -- one modulo for the first tap, then a step with a wrap per tap)
template <typename T, int AXIS, int WRAP>
__global__ __launch_bounds__(256) void k_nm_sep(const T *__restrict__ in, T *__restrict__ out, int h, int w, NmKernel<T> K)
{
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const T *p = in + (size_t)img * h * w;
    const int r = K.n / 2;
    T acc = (T)0;
    if (WRAP) {
        const int size = AXIS == 0 ? w : h;
        int j = ds_mod((AXIS == 0 ? x : y) - r, size);
        for (int k = 0; k < K.n; k++) {
            const T v = AXIS == 0 ? p[(size_t)y * w + j] : p[(size_t)j * w + x];
            acc = acc + K.cf[k] * v;
            j = ds_wrap_next(j, size);
        }
    } else {
        for (int k = 0; k < K.n; k++) {
            T v;
            if (AXIS == 0) v = p[(size_t)y * w + ds_reflect101(x + k - r, w)];
            else v = p[(size_t)ds_reflect101(y + k - r, h) * w + x];
            acc = acc + K.cf[k] * v;
        }
    }
    out[(size_t)img * h * w + (size_t)y * w + x] = acc;
}

// np.gradient (:31) of the (blurred) plane and the first normalisation (:33-39): planes n0, n1, n2 out
template <typename T, int WRAP>
__global__ __launch_bounds__(256) void k_nm_gradnorm(const T *__restrict__ in, T *__restrict__ n0, T *__restrict__ n1, T *__restrict__ n2,
                                                     int h, int w)
{
    const int img = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const T *p = in + (size_t)img * h * w;
    T v[3];
    nm_gradient_normal<NmPrec<T>, WRAP>([&](int yy, int xx) { return p[(size_t)yy * w + xx]; }, y, x, h, w, v);
    const size_t o = (size_t)img * h * w + (size_t)y * w + x;
    n0[o] = v[0]; n1[o] = v[1]; n2[o] = v[2];
}

// Sobel route: planes n0 = zx, n1 = zy (in) -> unit normal components in n0, n1, n2  (:34-39)
__global__ __launch_bounds__(256) void k_nm_normalize_first(double *__restrict__ n0, double *__restrict__ n1, double *__restrict__ n2, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        double v[3] = { n0[i], -n1[i], 1.0 };
        nm_normalize<NmPrec<double> >(v);
        n0[i] = v[0]; n1[i] = v[1]; n2[i] = v[2];
    }
}

// optional renormalise (:45-48) then quantise (:51-54)
template <typename T>
__global__ __launch_bounds__(256) void k_nm_finish(const T *__restrict__ n0, const T *__restrict__ n1, const T *__restrict__ n2,
                                                   int64_t count, int renorm, uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        T v[3] = { n0[i], n1[i], n2[i] };
        if (renorm) nm_normalize<NmPrec<T> >(v);
        for (int k = 0; k < 3; k++) out[i * 3 + k] = nm_quantize<NmPrec<T> >(v[k]);
    }
}

// cv2.getGaussianKernel(ksize, sigma > 0, CV_64F or CV_32F): exp(-x^2/(2 sigma^2)) rounded to T, summed in double in order, scaled
// by the double reciprocal of the sum and rounded to T again (for T = double the two casts do nothing)
template <typename T>
static void nm_gaussian(int ksize, double sigma, NmKernel<T> *K)
{
    K->n = ksize;
    const double scale2x = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < ksize; i++) {
        const double x = (double)i - (double)(ksize - 1) * 0.5;
        K->cf[i] = (T)exp(scale2x * x * x);
        sum += K->cf[i];
    }
    const double inv = 1.0 / sum;
    for (int i = 0; i < ksize; i++) K->cf[i] = (T)(K->cf[i] * inv);
}

// cv2.getDerivKernels / getSobelKernels for one axis (order 0 = smoothing, 1 = derivative)
static int nm_sobel(int ksize, int order, NmKernel<double> *K)
{
    if (ksize == 1) {
        if (order == 0) { K->n = 1; K->cf[0] = 1.0; }
        else { K->n = 3; K->cf[0] = -1.0; K->cf[1] = 0.0; K->cf[2] = 1.0; }
        return 0;
    }
    if (ksize == 3) {
        K->n = 3;
        if (order == 0) { K->cf[0] = 1.0; K->cf[1] = 2.0; K->cf[2] = 1.0; }
        else { K->cf[0] = -1.0; K->cf[1] = 0.0; K->cf[2] = 1.0; }
        return 0;
    }
    if (ksize + 1 > NM_MAXK) return -1;
    double ker[NM_MAXK + 1];
    for (int i = 0; i <= ksize; i++) ker[i] = 0.0;
    ker[0] = 1.0;
    for (int i = 0; i < ksize - order - 1; i++) {
        double oldv = ker[0];
        for (int j = 1; j <= ksize; j++) { const double nv = ker[j] + ker[j - 1]; ker[j - 1] = oldv; oldv = nv; }
    }
    for (int i = 0; i < order; i++) {
        double oldv = -ker[0];
        for (int j = 1; j <= ksize; j++) { const double nv = ker[j - 1] - ker[j]; ker[j - 1] = oldv; oldv = nv; }
    }
    K->n = ksize;
    for (int i = 0; i < ksize; i++) K->cf[i] = ker[i];
    return 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// The argument checks of every entry point, `name` in front of the messages.  GRADIENT_ONLY: the three ds_normalmap_gradient_*
// families (np.gradient is their only derivative: one DS_EINVAL covers n and the shape); otherwise ds_normalmap[_f64][_wrap].
// Negative kernel sizes mean "off" and come back as 0.
template <int GRADIENT_ONLY>
static int nm_check(const char *name, const ds_ctx *ctx, const void *depth, const void *out, int n, int h, int w, int *pre_blur,
                    int *sobel_ksize, int *post_blur)
{
    DS_REQUIRE(ctx && depth && out, DS_EINVAL, "%s: null argument", name);
    if (GRADIENT_ONLY) {
        DS_REQUIRE(n > 0 && n <= 65535 && h >= 2 && w >= 2, DS_EINVAL, "%s: np.gradient needs at least 2 samples per axis (n=%d h=%d w=%d)", name, n, h, w);
    } else {
        DS_REQUIRE(n > 0 && h > 0 && w > 0, DS_EINVAL, "%s: bad shape n=%d h=%d w=%d", name, n, h, w);
        DS_REQUIRE(n <= 65535, DS_EUNSUPPORTED, "%s: n must be <= 65535", name);
    }
    if (*pre_blur < 0) *pre_blur = 0;
    if (*post_blur < 0) *post_blur = 0;
    if (*sobel_ksize < 0) *sobel_ksize = 0;
    DS_REQUIRE((*pre_blur == 0 || (*pre_blur & 1)) && (*post_blur == 0 || (*post_blur & 1)), DS_EINVAL,
               "%s: Gaussian kernel sizes must be odd (cv2.GaussianBlur asserts)", name);
    DS_REQUIRE(*sobel_ksize == 0 || (*sobel_ksize & 1), DS_EINVAL, "%s: Sobel kernel size must be odd", name);
    DS_REQUIRE(*pre_blur <= NM_MAXK && *post_blur <= NM_MAXK && *sobel_ksize < NM_MAXK, DS_EUNSUPPORTED,
               "%s: kernel sizes above %d are not supported", name, NM_MAXK);
    if (!GRADIENT_ONLY && *sobel_ksize == 0) DS_REQUIRE(h >= 2 && w >= 2, DS_EINVAL, "%s: np.gradient needs at least 2 samples per axis", name);
    return DS_OK;
}

// The planes pipeline (arguments checked, device set): load, pre-blur, gradient, first normalisation, post-blur, finish, over 5
// planes of T in the context's scratch.  T = double takes Sobel of any size or np.gradient, T = float np.gradient only.
template <typename Tin, typename T, int WRAP>
static int nm_planes(ds_ctx *ctx, const char *name, const Tin *depth, int n, int h, int w, int pre_blur, int sobel_ksize, int post_blur,
                     int invert, uint8_t *out, hipStream_t st)
{
    const int64_t count = (int64_t)n * h * w;
    int rc = ds_ctx_reserve(ctx, &ctx->tmp_a, &ctx->tmp_a_bytes, (size_t)count * sizeof(T) * 5);
    if (rc) return rc;
    T *A = (T *)ctx->tmp_a, *B = A + count, *C = B + count, *D = C + count, *E = D + count;
    int nb = (int)((count + 1023) / 1024); if (nb > 4096) nb = 4096;
    dim3 g2((w + 63) / 64, (h + 3) / 4, n);
    DS_REQUIRE(g2.y <= 65535, DS_EUNSUPPORTED, "%s: image too tall", name);
    hipLaunchKernelGGL((k_nm_load<Tin, T>), dim3(nb), dim3(256), 0, st, depth, count, invert ? 1 : 0, A);
    NmKernel<T> G;
    if (pre_blur > 0) {                                            // :23-24
        nm_gaussian(pre_blur, (double)pre_blur, &G);
        hipLaunchKernelGGL((k_nm_sep<T, 0, WRAP>), g2, dim3(256), 0, st, A, B, h, w, G);
        hipLaunchKernelGGL((k_nm_sep<T, 1, WRAP>), g2, dim3(256), 0, st, B, A, h, w, G);
    }
    // unit normal of the gradients -> C, D, E
    if constexpr (std::is_same<T, double>::value) {
        if (sobel_ksize > 0) {                                     // :27-29: zx -> C, zy -> D
            NmKernel<double> KD, KS;
            DS_REQUIRE(nm_sobel(sobel_ksize, 1, &KD) == 0 && nm_sobel(sobel_ksize, 0, &KS) == 0, DS_EUNSUPPORTED, "%s: Sobel size", name);
            hipLaunchKernelGGL((k_nm_sep<T, 0, WRAP>), g2, dim3(256), 0, st, A, B, h, w, KD);
            hipLaunchKernelGGL((k_nm_sep<T, 1, WRAP>), g2, dim3(256), 0, st, B, C, h, w, KS);
            hipLaunchKernelGGL((k_nm_sep<T, 0, WRAP>), g2, dim3(256), 0, st, A, B, h, w, KS);
            hipLaunchKernelGGL((k_nm_sep<T, 1, WRAP>), g2, dim3(256), 0, st, B, D, h, w, KD);
            hipLaunchKernelGGL(k_nm_normalize_first, dim3(nb), dim3(256), 0, st, C, D, E, count);
        }
    }
    if (sobel_ksize <= 0) hipLaunchKernelGGL((k_nm_gradnorm<T, WRAP>), g2, dim3(256), 0, st, A, C, D, E, h, w);        // :31
    if (post_blur > 0) {                                           // :42-48
        nm_gaussian(post_blur, (double)post_blur, &G);
        T *planes[3] = { C, D, E };
        for (int k = 0; k < 3; k++) {
            hipLaunchKernelGGL((k_nm_sep<T, 0, WRAP>), g2, dim3(256), 0, st, planes[k], B, h, w, G);
            hipLaunchKernelGGL((k_nm_sep<T, 1, WRAP>), g2, dim3(256), 0, st, B, planes[k], h, w, G);
        }
    }
    hipLaunchKernelGGL(k_nm_finish<T>, dim3(nb), dim3(256), 0, st, C, D, E, count, post_blur > 0 ? 1 : 0, out);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// ds_normalmap[_f64][_wrap]: uint16 maps without blur and with Sobel 3 or np.gradient take a fused kernel, everything else the planes
template <typename Tin, int WRAP>
static int nm_run(ds_ctx *ctx, const Tin *depth, int n, int h, int w, int pre_blur, int sobel_ksize, int post_blur, int invert,
                  uint8_t *out, void *stream)
{
    int rc = nm_check<0>("ds_normalmap", ctx, depth, out, n, h, w, &pre_blur, &sobel_ksize, &post_blur);
    if (rc) return rc;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if constexpr (std::is_same<Tin, uint16_t>::value) {
        if (pre_blur == 0 && post_blur == 0 && (sobel_ksize == 3 || sobel_ksize == 0)) {
            dim3 grid((w + NM_BX - 1) / NM_BX, (h + NM_BY - 1) / NM_BY, n), block(NM_BX, NM_BY);
            DS_REQUIRE(grid.y <= 65535, DS_EUNSUPPORTED, "ds_normalmap: image too tall");
            if ((w & 3) == 0 && w >= 4 && h >= 2 && (((uintptr_t)depth) & 7) == 0 && (((uintptr_t)out) & 3) == 0) {
                dim3 grid4((w / 4 + NM_BX - 1) / NM_BX, grid.y, n);
                const int kt = ds_kt_begin(ctx, DS_KT_NORMALMAP, st);
                if (sobel_ksize == 3) hipLaunchKernelGGL((k_normalmap_fused4<1, WRAP>), grid4, block, 0, st, depth, h, w, invert ? 1 : 0, out);
                else hipLaunchKernelGGL((k_normalmap_fused4<0, WRAP>), grid4, block, 0, st, depth, h, w, invert ? 1 : 0, out);
                ds_kt_end(ctx, DS_KT_NORMALMAP, kt, st);
            } else if (sobel_ksize == 3) {
                hipLaunchKernelGGL((k_normalmap_fused<1, WRAP>), grid, block, 0, st, depth, h, w, invert ? 1 : 0, out);
            } else {
                hipLaunchKernelGGL((k_normalmap_fused<0, WRAP>), grid, block, 0, st, depth, h, w, invert ? 1 : 0, out);
            }
            DS_HIP_CHECK(hipGetLastError());
            return DS_OK;
        }
    }
    return nm_planes<Tin, double, WRAP>(ctx, "ds_normalmap", depth, n, h, w, pre_blur, sobel_ksize, post_blur, invert, out, st);
}

// ds_normalmap_gradient_f32 / _f16 [_wrap], and ds_normalmap_gradient_blur_f32[_wrap] with both blurs off
template <typename S, int WRAP>
static int nm_gradient_fused(ds_ctx *ctx, const char *name, const void *depth, int n, int h, int w, int invert, uint8_t *out, void *stream)
{
    int off[3] = { 0, 0, 0 };
    int rc = nm_check<1>(name, ctx, depth, out, n, h, w, &off[0], &off[1], &off[2]);
    if (rc) return rc;
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    dim3 g2((w + 63) / 64, (h + 3) / 4, n);
    DS_REQUIRE(g2.y <= 65535, DS_EUNSUPPORTED, "%s: image too tall", name);
    hipLaunchKernelGGL((k_nm_gradient_fused<S, WRAP>), g2, dim3(256), 0, (hipStream_t)stream, (const S *)depth, h, w, invert ? 1 : 0, out);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

template <int WRAP>
static int nm_gradient_blur_f32(ds_ctx *ctx, const float *depth, int n, int h, int w, int pre_blur, int post_blur, int invert,
                                uint8_t *out, void *stream)
{
    int sobel_ksize = 0;
    int rc = nm_check<1>("ds_normalmap_gradient_blur_f32", ctx, depth, out, n, h, w, &pre_blur, &sobel_ksize, &post_blur);
    if (rc) return rc;
    if (pre_blur == 0 && post_blur == 0) return nm_gradient_fused<float, WRAP>(ctx, "ds_normalmap_gradient_f32", depth, n, h, w, invert, out, stream);
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    return nm_planes<float, float, WRAP>(ctx, "ds_normalmap_gradient_blur_f32", depth, n, h, w, pre_blur, 0, post_blur, invert, out, (hipStream_t)stream);
}

// ---- the ten entry points (include/depthstereo.h): one instantiation each, so a _wrap entry point's shape rules, error codes and
// timer bracket are its twin's by construction
DS_API int ds_normalmap(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int pre_blur,
                        int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream)
{
    return nm_run<uint16_t, 0>(ctx, depth, n, h, w, pre_blur, sobel_ksize, post_blur, invert, out, stream);
}

DS_API int ds_normalmap_wrap(ds_ctx *ctx, const uint16_t *depth, int n, int h, int w, int pre_blur,
                             int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream)
{
    return nm_run<uint16_t, 1>(ctx, depth, n, h, w, pre_blur, sobel_ksize, post_blur, invert, out, stream);
}

// Any other real dtype of the reference's `depthmap` argument (:20-21 promote it to float64; the host casts): the separable
// float64 passes for every kernel size (general float64 data has no exact 3x3 shortcut).
DS_API int ds_normalmap_f64(ds_ctx *ctx, const double *depth, int n, int h, int w, int pre_blur,
                            int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream)
{
    return nm_run<double, 0>(ctx, depth, n, h, w, pre_blur, sobel_ksize, post_blur, invert, out, stream);
}

DS_API int ds_normalmap_f64_wrap(ds_ctx *ctx, const double *depth, int n, int h, int w, int pre_blur,
                                 int sobel_ksize, int post_blur, int invert, uint8_t *out, void *stream)
{
    return nm_run<double, 1>(ctx, depth, n, h, w, pre_blur, sobel_ksize, post_blur, invert, out, stream);
}

DS_API int ds_normalmap_gradient_f32(ds_ctx *ctx, const float *depth, int n, int h, int w, int invert, uint8_t *out, void *stream)
{
    return nm_gradient_fused<float, 0>(ctx, "ds_normalmap_gradient_f32", depth, n, h, w, invert, out, stream);
}

DS_API int ds_normalmap_gradient_f32_wrap(ds_ctx *ctx, const float *depth, int n, int h, int w, int invert, uint8_t *out, void *stream)
{
    return nm_gradient_fused<float, 1>(ctx, "ds_normalmap_gradient_f32", depth, n, h, w, invert, out, stream);
}

DS_API int ds_normalmap_gradient_f16(ds_ctx *ctx, const void *depth, int n, int h, int w, int invert, uint8_t *out, void *stream)
{
    return nm_gradient_fused<_Float16, 0>(ctx, "ds_normalmap_gradient_f16", depth, n, h, w, invert, out, stream);
}

DS_API int ds_normalmap_gradient_f16_wrap(ds_ctx *ctx, const void *depth, int n, int h, int w, int invert, uint8_t *out, void *stream)
{
    return nm_gradient_fused<_Float16, 1>(ctx, "ds_normalmap_gradient_f16", depth, n, h, w, invert, out, stream);
}

DS_API int ds_normalmap_gradient_blur_f32(ds_ctx *ctx, const float *depth, int n, int h, int w, int pre_blur, int post_blur, int invert,
                                          uint8_t *out, void *stream)
{
    return nm_gradient_blur_f32<0>(ctx, depth, n, h, w, pre_blur, post_blur, invert, out, stream);
}

DS_API int ds_normalmap_gradient_blur_f32_wrap(ds_ctx *ctx, const float *depth, int n, int h, int w, int pre_blur, int post_blur, int invert,
                                               uint8_t *out, void *stream)
{
    return nm_gradient_blur_f32<1>(ctx, depth, n, h, w, pre_blur, post_blur, invert, out, stream);
}

DS_API int ds_normalmap_selfcheck(ds_ctx *ctx, unsigned long long k0, unsigned long long stride, unsigned long long count,
                                  unsigned long long *mismatches, void *stream)
{
    DS_REQUIRE(ctx && mismatches, DS_EINVAL, "ds_normalmap_selfcheck: null argument");
    DS_REQUIRE(k0 >= (1ull << 18) && stride >= 1 && count >= 1 && k0 + stride * (count - 1) < (1ull << 40), DS_EINVAL,
               "ds_normalmap_selfcheck: K = k0 + stride * i must stay in [2^18, 2^40)");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *d_bad = nullptr;
    DS_HIP_CHECK(hipMalloc(&d_bad, sizeof(*d_bad)));
    DS_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(*d_bad), st));
    hipLaunchKernelGGL(k_nm_check_sqrt_rcp, dim3(4096), dim3(256), 0, st, k0, stride, count, d_bad);
    hipError_t e = hipMemcpyAsync(mismatches, d_bad, sizeof(*d_bad), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_bad);
    DS_HIP_CHECK(e);
    return DS_OK;
}
