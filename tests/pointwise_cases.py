"""Cases, operands, float64 references and checkers of the pointwise, resize and grouped-convolution kernels, shared by
tests/test_gpu_pointwise_exact.py (the kernels on the device) and tests/test_pointwise_model_cpu.py (their float32 restatements of
tools/pointwise_model.py and its mutants).  Everything here runs on the CPU; nothing comes from the kernels.

Layouts: bias_act operands are [pixels, channels] rows, read-out operands [B, N, C] / [B, C], images uint8 [B, H, W, 3], the
preprocess results logical [B, 3, oh, ow], the grouped convolution's activations NHWC [B, H, W, C] with torch's [C, cpg, 3, 3] weight.

The four bars ("Per-element bars of the pointwise, resize and grouped-convolution kernels"):
    bias_act      operands on a grid q, |v| <= 16: the float32 sum of four terms is exact, so the result is the float64 sum (after the
                  ReLU) rounded ONCE to the type -- torch.equal.
    read-out      |got - gelu64(x)| <= 1/2 ulp_T + 8 2^-24 (|x| + |gelu64(x)|), x = round_T(proj + cls) (exact operands again).
    preprocess    |got - ref64| <= 1/2 ulp_out + 16 2^-24 (S + |mean_c|) / std_c, S = sum |cy cx| px / 255.
    gconv3x3      exact integers: torch.equal; impulses: every output is the code of the tap that reached it; real operands:
                  |got - ref64| <= (9 cpg + 2) 2^-24 sum |terms|."""
import numpy as np
import torch
import torch.nn.functional as F

from util import bicubic_taps, first_mismatches, gelu64, preprocess_ref, small_ints, ternary, triple, ulp_spacing  # noqa: F401

HALF = [torch.float16, torch.bfloat16]
Q = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
DT_CODE = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}          # DS_DTYPE_* of include/depthstereo.h
SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0)


def grid_values(g, shape, dtype, bound):
    """Values of `dtype` that are multiples of Q[dtype] with |v| <= bound: draw, round to the type, then round(v / q) * q (float32
    arithmetic on powers of two and small integers: exact).  The result is still representable -- where the type's spacing is finer
    than q the value has at most 2^mantissa steps of q."""
    q = Q[dtype]
    v = (torch.randn(shape, generator=g) * (bound / 3.0)).clamp_(-bound, bound).to(dtype).float()
    v = torch.round(v / q) * q
    out = v.to(dtype)
    assert torch.equal(out.float(), v)
    return out


# ---- ds_bias_act_nhwc ---------------------------------------------------------------------------------------------------------------
BIAS_ACT_SHAPES = [(3, 8, 4, 4), (2, 64, 5, 7), (1, 264, 3, 5)]           # (B, C, H, W): C8 = 1, 8, 33
BIAS_ACT_STRIDE_SHAPE = (2, 1024, 41, 200)                                # 2,099,200 vectors of 8 > 8192 workgroups x 256 lanes
BIAS_ACT_COMBOS = [(relu, nres) for relu in (False, True) for nres in (0, 1, 2)]


def bias_act_operands(dtype, shape, seed=0):
    b, c, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed + c + 7 * h)
    p = b * h * w
    return {"x": grid_values(g, (p, c), dtype, 16.0), "bias": grid_values(g, (c,), dtype, 16.0),
            "r1": grid_values(g, (p, c), dtype, 16.0), "r2": grid_values(g, (p, c), dtype, 16.0)}


def bias_act_sums(ops, wide):
    """(x + bias, + r1, + r2) accumulated in that order in `wide` (float64: the definition; float32: what the kernel does)."""
    s0 = ops["x"].to(wide) + ops["bias"].to(wide)[None, :]
    s1 = s0 + ops["r1"].to(wide)
    return s0, s1, s1 + ops["r2"].to(wide)


def bias_act_wants(ops):
    """{(relu, nres): the float64 sum, after the ReLU, rounded once to the type}.  The sums are exact in float32 (the premise test), so
    the conversion goes through float32 without a second rounding."""
    dtype = ops["x"].dtype
    sums = bias_act_sums(ops, torch.float64)
    return {(relu, nres): (sums[nres].clamp(min=0.0) if relu else sums[nres]).float().to(dtype) for relu, nres in BIAS_ACT_COMBOS}


def bias_act_args(ops, nres):
    return ops["x"], ops["bias"], ops["r1"] if nres >= 1 else None, ops["r2"] if nres >= 2 else None


def check_bias_act(got, want, tag):
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    assert torch.equal(got, want), f"{tag}: {first_mismatches(got, want)}"


def bias_act_special_operands(dtype):
    """(2, 64, 5, 7) with NaN, +Inf, -Inf and -0.0 in x (pixel 0), in r1 (pixel 1), in r2 (pixel 2) and in the bias (channels
    24 .. 27: whole columns), +Inf in x against -Inf in r1 at one element (NaN by the sum alone), and a NaN under a negative sum."""
    ops = bias_act_operands(dtype, (2, 64, 5, 7), seed=5)
    sp = torch.tensor(SPECIALS).to(dtype)
    ops["x"][0, 0:4] = sp
    ops["r1"][1, 8:12] = sp
    ops["r2"][2, 16:20] = sp
    ops["bias"][24:28] = sp
    ops["x"][3, 40], ops["r1"][3, 40] = float("inf"), float("-inf")
    ops["x"][4, 41], ops["bias"][41] = float("nan"), -8.0
    return ops


def bias_act_special_want(ops, relu, nres):
    """torch on the CPU, float32: relu(x + b + r1 + r2) (finite sums are exact, so the cast to the type is the one rounding)."""
    f = bias_act_sums(ops, torch.float32)[nres]
    return (torch.relu(f) if relu else f).to(ops["x"].dtype)


def check_specials(got, want, tag):
    got = got.detach().cpu()
    assert bool(torch.isnan(want).any()), tag
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{tag}: NaN at {int(torch.isnan(got).sum())} outputs, torch has {int(torch.isnan(want).sum())}"
    a, b = torch.nan_to_num(got.float(), 7.0), torch.nan_to_num(want.float(), 7.0)
    assert torch.equal(a, b), f"{tag}: {first_mismatches(a, b)}"


# ---- ds_reassemble_readout ------------------------------------------------------------------------------------------------------------
READOUT_SHAPES = [(2, 2, 8), (3, 5, 64), (1, 577, 264)]                  # (B, N, C): one output row and C8 = 1; batch 3; C8 = 33
READOUT_STRIDE_SHAPE = (2, 8200, 1024)                                   # 2,098,944 vectors of 8


def readout_operands(dtype, shape, seed=0):
    """proj [B, N, C] and cls [B, C] on the grid with |v| <= 8 (proj + cls is exact in float32); the cls row of proj is NaN: the
    kernel must not read it.  Every image has its own cls vector."""
    b, n, c = shape
    g = torch.Generator().manual_seed(2000 + seed + c + 3 * n)
    proj = grid_values(g, (b, n, c), dtype, 8.0)
    proj[:, 0] = float("nan")
    cls = grid_values(g, (b, c), dtype, 8.0)
    assert all(not torch.equal(cls[i], cls[j]) for i in range(b) for j in range(i))
    return {"proj": proj, "cls": cls}


def readout_sum(ops, wide):
    return ops["proj"][:, 1:].to(wide) + ops["cls"].to(wide)[:, None, :]


def check_readout(got, ops, tag):
    """|got - gelu64(x)| <= 1/2 ulp_T(want) + 8 2^-24 (|x| + |want|) per element, ulp_T floored at 2^-24; no NaN.  Returns (worst
    error / bound, outputs that are not gelu64(x) rounded to the type)."""
    dtype = ops["proj"].dtype
    got = got.detach().cpu()
    x = readout_sum(ops, torch.float64).float().to(dtype).double()          # exact sum (premise), ONE rounding to the storage type
    want = gelu64(x)
    assert got.shape == want.shape and got.dtype == dtype, tag
    assert not bool(torch.isnan(got).any()), f"{tag}: {int(torch.isnan(got).sum())} NaN outputs (the cls row of proj was read?)"
    bound = 0.5 * ulp_spacing(want, dtype).clamp(min=2.0 ** -24) + 8.0 * 2.0 ** -24 * (x.abs() + want.abs())
    ratio = (got.double() - want).abs() / bound
    worst = int(ratio.argmax())
    off = int((got != want.to(dtype)).sum())
    report = (f"{tag}: worst error / bound {float(ratio.max()):.4f} at x = {float(x.flatten()[worst])!r} (got {float(got.flatten()[worst])!r}, "
              f"gelu64 {float(want.flatten()[worst])!r}); {off} of {got.numel()} outputs are not gelu64 rounded")
    assert float(ratio.max()) <= 1.0, report
    return float(ratio.max()), off, report


# ---- ds_preprocess_bicubic --------------------------------------------------------------------------------------------------------------
PRE_SHAPES = [((1, 1), (3, 5)), ((2, 3), (7, 5)), ((1, 9), (4, 20)), ((5, 7), (1, 1)), ((33, 41), (33, 41)), ((20, 30), (32, 48)),
              ((45, 70), (32, 48)), ((300, 40), (32, 48))]
PRE_IDENTITY = ((33, 41), (33, 41))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
PRE_NORMS = [(0.5, 0.5), IMAGENET]
PRE_BATCH = 3
PRE_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# ds_preprocess_bicubic_rows on three of the shapes: (input, output, patch, n_pad) as in test_gpu_forward_ends.PRE_CASES
PRE_ROWS_CASES = [((20, 30), (32, 48), 16, 8), ((45, 70), (32, 48), 16, 16), ((300, 40), (32, 48), 16, 8)]


def pre_image(kind, in_hw, seed=0):
    """uint8 [3, H, W, 3] (numpy): random bytes, or a constant 255."""
    shape = (PRE_BATCH, in_hw[0], in_hw[1], 3)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    return np.random.default_rng(3000 + seed + 31 * in_hw[0] + in_hw[1]).integers(0, 256, shape, dtype=np.uint8)


def check_preprocess(got, ref, s, mean, std, tag):
    """|got - ref| <= 1/2 ulp_out(ref) + 16 2^-24 (S + |mean_c|) / std_c per element.  Returns worst error / bound."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tag, got.shape, ref.shape)
    m = torch.from_numpy(triple(mean).astype(np.float64)).view(1, 3, 1, 1)
    sd = torch.from_numpy(triple(std).astype(np.float64)).view(1, 3, 1, 1)
    bound = 0.5 * ulp_spacing(ref, got.dtype) + 16.0 * 2.0 ** -24 * (s + m.abs()) / sd
    ratio = (got.double() - ref).abs() / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert float(ratio.max()) <= 1.0, (f"{tag}: worst error / bound {float(ratio.max()):.4f} at (b, c, y, x) = {tuple(int(i) for i in worst)}: "
                                       f"got {float(got[worst])!r}, float64 {float(ref[worst])!r}")
    return float(ratio.max())


def pre_identity_want(img, mean, std, flip):
    """Equal input and output sizes: the weights are exactly (0, 1, 0, 0), the output is (float32(px) / 255 - mean) * (1 / std) in
    float32, logical [B, 3, H, W]."""
    f32 = np.float32
    px = img.astype(np.float32) / f32(255.0)
    if flip:
        px = px[..., ::-1]
    o = (px - triple(mean)) * (f32(1.0) / triple(std))
    assert o.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(o.transpose(0, 3, 1, 2)))


def rows_ungather(rows, p, out_hw):
    """[B, n_pad, kpad] patch rows (include/depthstereo.h: ds_preprocess_bicubic_rows: row 1 + gy * gw + gx holds patch (gy, gx) as
    (py, px, c)) -> (the logical [B, 3, gh * p, gw * p] image they hold, mask of the positions that must be zero)."""
    b = rows.shape[0]
    gh, gw = out_hw[0] // p, out_hw[1] // p
    body = rows[:, 1:1 + gh * gw, :p * p * 3].reshape(b, gh, gw, p, p, 3).permute(0, 5, 1, 3, 2, 4).reshape(b, 3, gh * p, gw * p)
    zero = torch.ones(rows.shape, dtype=torch.bool)
    zero[:, 1:1 + gh * gw, :p * p * 3] = False
    return body, zero


# ---- ds_gconv3x3_nhwc_f32 -----------------------------------------------------------------------------------------------------------------
GCONV_SHAPES = [(1, 32, 1, 1), (1, 32, 8, 32), (2, 64, 9, 33), (3, 96, 17, 70)]          # (B, C, H, W); tile 8 x 32 pixels, 32 channels
GCONV_CPGS = (8, 16, 32)


def weight_image(w, groups):
    from src import _native
    return _native.gconv_weight_image(w, groups)


def gconv_ref64(x, w, bias, cpg, relu=False):
    """float64 grouped convolution on the CPU: x NHWC, torch's weight [C, cpg, 3, 3], zero padding 1.  Returns NHWC float64."""
    c = x.shape[3]
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double(), 1, 1, 1, c // cpg)
    y = y.permute(0, 2, 3, 1).contiguous()
    return y.clamp(min=0.0) if relu else y


def gconv_int_operands(shape, cpg, seed=0):
    """x and w in {-1, 0, 1}, bias in [-8, 8]: K = 9 cpg <= 288 products, every partial sum an integer below 2^24."""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(4000 + seed + c + 5 * h + cpg)
    return {"x": ternary(g, (b, h, w, c), 0.7).float(), "w": ternary(g, (c, cpg, 3, 3), 0.7).float(), "bias": small_ints(g, (c,), 8).float()}


def gconv_real_operands(shape, cpg, seed=0):
    b, c, h, w = shape
    g = torch.Generator().manual_seed(5000 + seed + c + 5 * h + cpg)
    return {"x": torch.randn((b, h, w, c), generator=g), "w": torch.randn((c, cpg, 3, 3), generator=g) * (9 * cpg) ** -0.5,
            "bias": torch.randn((c,), generator=g)}


def check_gconv_exact(got, ops, cpg, use_bias, relu, tag):
    want = gconv_ref64(ops["x"], ops["w"], ops["bias"] if use_bias else None, cpg, relu)
    assert float(want.abs().max()) < 2.0 ** 24
    got = got.detach().cpu()
    assert torch.equal(got, want.float()), f"{tag}: {first_mismatches(got, want)}"


def check_gconv_bound(got, ops, cpg, use_bias, relu, tag):
    """|got - ref64| <= (9 cpg + 2) 2^-24 sum |terms|: a chain of 9 cpg FMAs behind the bias, one rounding each (the ReLU is
    1-Lipschitz: the bound of the sum holds behind it).  Returns worst error / bound."""
    b = ops["bias"] if use_bias else None
    ref = gconv_ref64(ops["x"], ops["w"], b, cpg, relu)
    terms = gconv_ref64(ops["x"].abs(), ops["w"].abs(), None if b is None else b.abs(), cpg)
    got = got.detach().cpu()
    ratio = (got.double() - ref).abs() / ((9 * cpg + 2) * 2.0 ** -24 * terms)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    assert float(ratio.max()) <= 1.0, f"{tag}: worst error / bound {float(ratio.max()):.4f}"
    return float(ratio.max())


def impulse_weight(c, cpg):
    """w[co, ci, ky, kx] = 1 + ((ky * 3 + kx) * cpg + ci) * cpg + co % cpg <= 9217: the code names tap, input and output channel."""
    co, ci = torch.arange(c).view(c, 1, 1, 1), torch.arange(cpg).view(1, cpg, 1, 1)
    tap = (torch.arange(3).view(1, 1, 3, 1) * 3 + torch.arange(3).view(1, 1, 1, 3))
    return (1 + (tap * cpg + ci) * cpg + co % cpg).float()


def impulse_sites(shape):
    """(image, channel, y, x) of the single 1.0: the two corners, both sides of the seam of the first pixel tile and channel block,
    and the interior (coordinates beyond a small tensor fold onto its last element; duplicates dropped)."""
    b, c, h, w = shape
    sites = [(0, 0, 0, 0), (b - 1, c - 1, h - 1, w - 1), (b - 1, min(31, c - 1), min(7, h - 1), min(31, w - 1)),
             (b - 1, min(32, c - 1), min(8, h - 1), min(32, w - 1)), (0, c // 2 + 1, h // 2, w // 2)]
    return sorted(set(sites))


def impulse_x(shape, site):
    b, c, h, w = shape
    x = torch.zeros((b, h, w, c))
    x[site[0], site[2], site[3], site[1]] = 1.0
    return x


def impulse_want(shape, cpg, site):
    """By index arithmetic, not by a convolution: output (oy, ox) = (iy + 1 - ky, ix + 1 - kx) of the impulse's image holds, in the
    channels of the impulse's group, the code of (tap ky * 3 + kx, the impulse's channel within the group, co % cpg); all else is 0."""
    b, c, h, w = shape
    n, ch, iy, ix = site
    g, ci = ch // cpg, ch % cpg
    want = torch.zeros((b, h, w, c))
    for ky in range(3):
        for kx in range(3):
            oy, ox = iy + 1 - ky, ix + 1 - kx
            if 0 <= oy < h and 0 <= ox < w:
                want[n, oy, ox, g * cpg:(g + 1) * cpg] = 1.0 + ((ky * 3 + kx) * cpg + ci) * cpg + torch.arange(cpg).float()
    return want


def check_gconv_impulse(got, shape, cpg, site, tag):
    got, want = got.detach().cpu(), impulse_want(shape, cpg, site)
    assert torch.equal(got, want), f"{tag}: impulse at (image, channel, y, x) = {site}: {first_mismatches(got, want)}"
