"""Shared helpers for the tests: golden fixtures and synthetic inputs (no reference tree needed)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def load_stereo_golden():
    z = np.load(os.path.join(GOLDEN, "stereo_cases.npz"))
    index = json.loads(bytes(z["__index__"]).decode())
    return z, index


def load_funnel_golden():
    z = np.load(os.path.join(GOLDEN, "funnel_cases.npz"))
    index = json.loads(bytes(z["__index__"]).decode())
    return z, index


def load_normalmap_golden():
    """tests/golden/make_golden_normalmap.py: outputs of the reference's own create_normalmap (stub cv2, see there)."""
    z = np.load(os.path.join(GOLDEN, "normalmap_cases.npz"))
    index = json.loads(bytes(z["__index__"]).decode())
    return z, index


def golden_inputs(case):
    import make_golden as mg        # pure-numpy generators; importing it does not touch /root/reference
    return mg.gen_inputs(case)


def survey_inputs(H, W, seed, n=1):
    """SURVEY.md Appendix A / section 8(d) synthetic input (integer-only depth pattern)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    d = (xx * 30000) // (W - 1) + ((xx // 8 + yy // 8) % 2) * 8000
    d[H // 4: H // 2, W // 3: 2 * W // 3] = 60000
    d[(3 * H) // 4:, : W // 5] = 1000
    dep = np.repeat(d.astype(np.uint16)[None], n, axis=0)
    return img, dep


def smooth_depth(H, W, seed):
    """Smooth float field with a few occluders -- stands in for a model prediction."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.zeros((H, W))
    for _ in range(6):
        cx, cy, s, a = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(W / 16, W / 3), rng.uniform(-1, 1)
        f += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    f += 0.3 * xx / W
    x0, y0 = int(rng.uniform(0, W / 2)), int(rng.uniform(0, H / 2))
    f[y0:y0 + H // 4, x0:x0 + W // 3] += 1.0
    return f.astype(np.float32)


# ---- exact-integer operands and per-element rounding bounds for the half-precision GEMM / convolution tests ------------------------
MANTISSA_BITS = {"float16": 10, "bfloat16": 7, "float32": 23}
MIN_NORMAL_EXP = {"float16": -14, "bfloat16": -126, "float32": -126}


def ternary(g, shape, density):
    """float64 tensor of {-1, 0, +1}: nonzero with probability `density`, both signs equally likely (generator g, CPU)."""
    import torch
    keep = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return torch.where(keep, sign, torch.zeros_like(sign)).double()


def small_ints(g, shape, bound):
    """float64 tensor of integers drawn uniformly from [-bound, bound]."""
    import torch
    return torch.randint(-bound, bound + 1, shape, generator=g).double()


def ulp_spacing(ref64, dtype):
    """Spacing of `dtype` (float16 / bfloat16 / float32) at the float64 values rounded to it: 2^(floor(log2 |r|) - mantissa bits), and the
    subnormal spacing below the smallest normal number (the construction of test_gpu_midas_small._f16_within_bound, for both types)."""
    import torch
    name = str(dtype).replace("torch.", "")
    r = ref64.to(dtype).double().abs()
    _, e = torch.frexp(r.clamp(min=2.0 ** MIN_NORMAL_EXP[name]))          # |r| = m 2^e with m in [1/2, 1)
    return torch.ldexp(torch.ones_like(r), e - 1 - MANTISSA_BITS[name])


def ulp_distance(got, ref64, floor=0.0):
    """Distance between every element of got and the float64 value rounded to got's type, in units in the last place of that
    type at the rounded value -- a whole number.  floor > 0: the unit is never finer than `floor` (bfloat16 keeps float32's
    exponent range, so near zero its ulp says nothing about an fp32 computation; float16's ends at its subnormal spacing 2^-24)."""
    g = got.detach().cpu()
    r = ref64.to(g.dtype).double()
    return (g.double() - r).abs() / ulp_spacing(ref64, g.dtype).clamp(min=floor)


def rounding_bound_ratio(got, ref64, abs_terms, k_total):
    """Single-rounding bound of a half-precision GEMM with fp32 accumulation and an fp32 epilogue, per element:
        |got - ref64| <= 1/2 ulp_out(ref64) + 2 (k_total + 4) 2^-24 abs_terms,
    abs_terms = sum_k |x_k w_k| + |bias| + ... the same formula on the absolute values.  One fp32 rounding per accumulation step
    and epilogue operation, a FULL ulp (2^-24 relative, not half) each since the MFMA's internal rounding of its partial sums is
    not documented as round-to-nearest.  Returns (worst error / bound, outputs more than one ulp from ref64 rounded)."""
    g = got.detach().cpu()
    err = (g.double() - ref64).abs()
    bound = 0.5 * ulp_spacing(ref64, g.dtype) + 2.0 * (k_total + 4) * 2.0 ** -24 * abs_terms
    return float((err / bound).max()), int((ulp_distance(g, ref64) > 1).sum())


def bilinear_taps(n_in, n_out, align_corners=True):
    """One axis of the bilinear upsample as include/depthstereo.h defines it (ds_upsample_bilinear_nhwc, ds_dpt_head_tail), in
    float32 like the kernels and torch: s = (n_in - 1) / (n_out - 1) as a float32 quotient (0 when n_out == 1), f = s * o -- or
    s = n_in / n_out, f = max(s * (o + 0.5) - 0.5, 0) without align_corners --, i0 = min(int(f), n_in - 1), i1 = min(i0 + 1,
    n_in - 1), t = f - i0.  Returns (i0, i1, t): int64, int64 and float32 arrays of n_out entries."""
    f32 = np.float32
    o = np.arange(n_out, dtype=np.float32)
    if align_corners:
        s = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0.0)
        f = s * o
    else:
        s = f32(n_in) / f32(n_out)
        f = np.maximum(s * (o + f32(0.5)) - f32(0.5), f32(0.0))
    assert f.dtype == np.float32
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, f - i0.astype(np.float32)


def bilinear_ref(x, size, align_corners=True, taps_x=None):
    """Bilinear resize of a float64 NHWC tensor x [B, H, W, C] to size (oh, ow): the four weights (1 - ty) (1 - tx), (1 - ty) tx,
    ty (1 - tx), ty tx are float32 products of bilinear_taps (part of the definition), everything after that is float64 and nothing
    is rounded.  taps_x replaces bilinear_taps along x (a test that corrupts its own reference).  Returns (u, sum |weight * value|)."""
    import torch
    oh, ow = size
    y0, y1, ty = bilinear_taps(x.shape[1], oh, align_corners)
    x0, x1, tx = taps_x if taps_x is not None else bilinear_taps(x.shape[2], ow, align_corners)
    one = np.float32(1.0)
    wy, wx = ((one - ty)[:, None], ty[:, None]), ((one - tx)[None, :], tx[None, :])
    u, s = 0.0, 0.0
    for iy, a in ((y0, wy[0]), (y1, wy[1])):
        for ix, b in ((x0, wx[0]), (x1, wx[1])):
            w = a * b
            assert w.dtype == np.float32
            w64 = torch.from_numpy(w.astype(np.float64))[None, :, :, None]
            v = x[:, torch.from_numpy(iy)[:, None], torch.from_numpy(ix)[None, :]]          # [B, oh, ow, C]
            u, s = u + w64 * v, s + w64 * v.abs()
    return u, s


def bicubic_taps(n_in, n_out):
    """One axis of the bicubic resize as include/depthstereo.h (ds_preprocess_bicubic) and pre_cubic (csrc/ds_common.h) define it, in
    float32 like the kernels (the coordinate and weight arithmetic is part of the definition, every multiply and add rounded on its
    own): s = n_in / n_out, f = s * (o + 0.5) - 0.5, t = f - floor(f), the four weights of the cubic convolution kernel with
    A = -0.75 in pre_cubic's order of operations, indices clamp(floor(f) - 1 + k, 0, n_in - 1).  Returns (int64 [n_out, 4],
    float32 [n_out, 4])."""
    f32 = np.float32
    o = np.arange(n_out, dtype=np.float32)
    s = f32(n_in) / f32(n_out)
    f = s * (o + f32(0.5)) - f32(0.5)
    f0 = np.floor(f)
    t = f - f0
    a = f32(-0.75)
    x0, x3, x2 = t + f32(1.0), f32(2.0) - t, f32(1.0) - t
    c = np.stack([((a * x0 - f32(5.0) * a) * x0 + f32(8.0) * a) * x0 - f32(4.0) * a,
                  ((a + f32(2.0)) * t - (a + f32(3.0))) * t * t + f32(1.0),
                  ((a + f32(2.0)) * x2 - (a + f32(3.0))) * x2 * x2 + f32(1.0),
                  ((a * x3 - f32(5.0) * a) * x3 + f32(8.0) * a) * x3 - f32(4.0) * a], axis=1)
    assert f.dtype == np.float32 and c.dtype == np.float32
    idx = np.clip(f0.astype(np.int64)[:, None] - 1 + np.arange(4, dtype=np.int64)[None, :], 0, n_in - 1)
    return idx, c


def triple(v):
    """A scalar or three values -> float32 [3] (what the binding of ds_preprocess_bicubic passes to the library)."""
    return np.asarray(tuple(v) if hasattr(v, "__len__") else (v,) * 3, dtype=np.float32)


def preprocess_ref(img_u8, size, mean, std, flip):
    """ds_preprocess_bicubic in float64: out[b, c] = (sum_ky sum_kx cy cx (px / 255) - mean_c) / std_c over the taps of bicubic_taps,
    px the byte of image channel 2 - c (flip) or c; mean / std are the float32 values the binding passes, widened.  img_u8: uint8
    [B, H, W, 3] (numpy or CPU tensor).  Returns (out, S) as float64 tensors [B, 3, oh, ow], S = sum |cy cx| px / 255."""
    import torch
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 4 and img.shape[3] == 3
    oh, ow = size
    iy, cy = bicubic_taps(img.shape[1], oh)
    ix, cx = bicubic_taps(img.shape[2], ow)
    px = img.astype(np.float64) / 255.0
    if flip:
        px = px[..., ::-1]
    acc = np.zeros((img.shape[0], oh, ow, 3))
    s = np.zeros_like(acc)
    for ky in range(4):
        for kx in range(4):
            w = cy[:, ky].astype(np.float64)[:, None] * cx[:, kx].astype(np.float64)[None, :]
            v = px[:, iy[:, ky][:, None], ix[:, kx][None, :]]                       # [B, oh, ow, 3]
            acc += w[None, :, :, None] * v
            s += np.abs(w)[None, :, :, None] * v
    out = (acc - triple(mean).astype(np.float64)) / triple(std).astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 3, 1, 2))), torch.from_numpy(np.ascontiguousarray(s.transpose(0, 3, 1, 2)))


def gelu64(x):
    """The exact GELU 0.5 x (1 + erf(x / sqrt 2)) of a float64 tensor, written with erfc (1 + erf(z) = erfc(-z)) so that the left
    tail keeps its relative precision."""
    import torch
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / 2.0 ** 0.5)


def first_mismatches(got, want, limit=5):
    """"<count> of <total> differ: (index, got, want) ..." for two tensors of one shape (a readable failure of torch.equal)."""
    import torch
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    bad = torch.nonzero(g != w)
    rows = ["(%s: got %g, want %g)" % (", ".join(str(int(i)) for i in ix), g[tuple(ix)], w[tuple(ix)]) for ix in bad[:limit]]
    return "%d of %d differ: %s" % (bad.shape[0], g.numel(), " ".join(rows))
