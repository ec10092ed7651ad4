"""GPU tests of the kernels that compute statistics -- ds_group_norm_nchw, ds_residual_layernorm, ds_row_stats and the online softmax
of ds_attention_fwd -- on the inputs where statistics go wrong: a large common mode, zero spread, one outlier, massive channels,
logits far apart.  Every kernel is compared with a float64 computation on the same rounded operands, element by element, against a
bar in units of the output type's ulp at the float64 value:

    |got - want| <= 2 ulp_T(want) + floor

One rounding of the output costs half an ulp; the floor is the float32 arithmetic each kernel does on purpose (its statistics or its
epilogue), written out per test in units of u = 2^-24.  Every case also checks that the outputs are finite and that a repeated launch
gives identical bits."""
import zlib

import pytest
import torch

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
U32 = 2.0 ** -24                     # unit roundoff of float32


def ulp(want, dtype):
    """Spacing of dtype at |want| (float64 tensor in, float64 tensor out); below the smallest normal, the subnormal spacing."""
    mant, emin = {F16: (10, -14), BF16: (7, -126), torch.float32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(want.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


def ulp_check(got, want, dtype, floor):
    """(worst |got - want| / (2 ulp + floor), worst error in ulps of the output type where |want| >= 1, i.e. away from the floor):
    the first must be <= 1."""
    g = got.double()
    assert torch.isfinite(g).all()
    err = (g - want).abs()
    u = ulp(want, dtype)
    big = want.abs() >= 1.0
    return (err / (2 * u + floor)).max().item(), ((err / u)[big].max().item() if big.any() else 0.0)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------
# Which launch form a shape takes (csrc/ds_encoder_ops.hip, ds_group_norm_nchw): the single-launch k_gn_fused when
# group_len / 8 <= 1024 x 10 (the group fits one workgroup's registers) and images x groups <= 512; the k_gn_moments + k_gn_apply pair
# otherwise, with splits = group_len / 4096 moment slices (at most 32) and chunks = group_len / 8192 apply chunks (at most 64) per group.
GN_SHAPES = {
    # (n, c, h, w), groups
    "fused_2ch_48x48": ((1, 64, 48, 48), 32),              # fused, group_len 4608
    "fused_32ch_48x48": ((1, 1024, 48, 48), 32),           # fused, group_len 73728 (the largest group of the stem at 384^2)
    "fused_8200": ((2, 32, 8, 1025), 32),                  # fused, group_len 8200 = 2 x 4096 + 8
    # pair because images x groups = 544 > 512; group_len 8200: 2 slices of 513 / 512 vectors, one apply chunk
    "pair_many_8200": ((17, 32, 8, 1025), 32),
    # pair because images x groups = 640; group_len 20488 = 5 x 4096 + 8: slices of 513 x 4 + 509 vectors (the last one short);
    # 2 x 8192 + 8: apply chunks of 1281 / 1280 vectors (ragged)
    "pair_many_20488": ((20, 32, 8, 2561), 32),
    # pair because the group (98312 values) exceeds the registers: 98312 = 24 x 4096 + 8 = 12 x 8192 + 8 -> 24 slices, the last one
    # 490 vectors instead of 513; 12 apply chunks, the last one 1014 vectors instead of 1025
    "pair_large_98312": ((1, 4, 8, 12289), 4),
}
# (With splits = group_len / 4096 <= 32 every moments slice holds at least one vector: k_gn_apply still merges an empty one as nothing.)

# (name, mean / std, std): the common-mode sweep, then magnitudes near a quarter of float16's maximum (16384)
GN_OFFSETS = [("ratio0", 0.0, 1.7), ("ratio30", 30.0, 1.0), ("ratio100", 100.0, 1.0), ("ratio300", 300.0, 1.0),
              ("ratio1000", 1000.0, 1.0), ("quarter_max_spread", 0.0, 5000.0), ("quarter_max_offset", 1024.0, 16.0)]
# bfloat16 holds 8 significant bits: at 300 standard deviations its spacing is 2 std, at 1000 it is 8 -- a handful of levels, no longer
# a distribution.  Its sweep stops at 100 (spacing 0.5 std).
GN_OFFSETS_BF16 = ["ratio0", "ratio30", "ratio100", "quarter_max_spread"]
EPILOGUES = [("plain", False, False), ("relu", True, False), ("res", False, True), ("res_relu", True, True)]


def _gn_inputs(kind, shape, groups, dtype, g):
    n, c, h, w = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    for name, ratio, std in GN_OFFSETS:
        if kind == name:
            x = x * std + ratio * std
    if kind in ("constant", "constant_big"):
        # every group constant (a different value per group): variance exactly 0
        x = torch.linspace(-7.25, 11.5, n * groups, dtype=torch.float64).reshape(n, groups, 1)
        if kind == "constant_big":
            x = x * 137.0 + 1000.0
        x = x.expand(n, groups, c // groups * h * w).reshape(shape)
    if kind == "constant_outlier":
        # constant groups with one outlier each, at a different position per group (the first element of one of them)
        x = torch.full((n, groups, c // groups * h * w), 300.0, dtype=torch.float64)
        gl = x.shape[-1]
        for k in range(n * groups):
            x[k // groups, k % groups, (k * 7919) % gl if k else 0] = 300.0 + 2.0 * (1 + k % 5)
        x = x.reshape(shape)
    return x.to(dtype)


def _gn_reference(x, groups, wt, bs, eps, relu, res):
    """float64 GroupNorm of the rounded operands: two-pass mean / population variance, rstd = 1 / sqrt(var + eps) with eps as the
    kernel receives it (float32); returns (y, floor) with the floor of the float32 epilogue (see test_group_norm_statistics)."""
    n, c, h, w = x.shape
    xd = x.double().reshape(n, groups, -1)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    ch = lambda t: t.double().reshape(1, c, 1, 1)        # noqa: E731
    a = (rstd.expand_as(xd).reshape(x.shape)) * ch(wt)
    meanx = mean.expand_as(xd).reshape(x.shape)
    d = x.double() - meanx
    y = d * a + ch(bs)
    if res is not None:
        y = y + res.double()
    if relu:
        y = y.clamp_min(0.0)
    # mean and rstd reach the epilogue as float32: the mean's rounding is exact when the mean is a float32 value (a constant group)
    mean_err = torch.where(meanx.float().double() == meanx, torch.zeros_like(meanx), 2 * U32 * meanx.abs())
    floor = mean_err * a.abs() + 4 * U32 * ((d * a).abs() + ch(bs).abs() + (res.double().abs() if res is not None else 0.0))
    return y, floor


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("form", list(GN_SHAPES))
def test_group_norm_statistics(gpu, dtype, form):
    """ds_group_norm_nchw against a float64 GroupNorm on offset, constant and extreme groups, every epilogue, both launch forms.

    Expected error: the statistics are float64 sums of x - x[0], fed by float32 sums around a nearby value (a wave's first value in
    k_gn_fused, each vector's first in k_gn_moments): the variance is good to ~1e-7 of the local spread, nothing at the scale of the
    common mode -- so what is left is the float32 epilogue y = (x - mean) * (rstd gamma) + beta [+ res] and one rounding
    to the output type.  The epilogue's float32 error, the floor (u = 2^-24):
        |fl32(mean) - mean| |a|                 mean handed over as float32 (<= 2u |mean| |a|; 0 when the mean is a float32 value)
      + 4u (|(x - mean) a| + |beta| + |res|)    rounding of rstd, a = rstd gamma, x - mean, the FMA and the residual add
    with a = rstd gamma.  A constant group has x - mean = 0 exactly: its output is beta (or relu(beta + res)) to the output's rounding.
    At mean / std = 1000 the floor is ~2.4e-4 (0.12 float16 ulp near 3); the float32 E[x^2] - mean^2 moments this replaces missed by
    ~1e-7 (mean / std)^2 relative in the variance -- 10 float16 ulps near 3 at a ratio of 300."""
    from src import _native
    shape, groups = GN_SHAPES[form]
    g = torch.Generator().manual_seed(zlib.crc32(f"{form} {dtype}".encode()))
    c = shape[1]
    kinds = [k for k, _, _ in GN_OFFSETS if dtype == F16 or k in GN_OFFSETS_BF16] + ["constant", "constant_big", "constant_outlier"]
    failures, report = [], []
    for ki, kind in enumerate(kinds):
        x = _gn_inputs(kind, shape, groups, dtype, g).cuda()
        assert _native.group_norm_supported(x, groups)
        wt = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).to(dtype).cuda()
        bs = torch.randn(c, generator=g, dtype=torch.float64).to(dtype).cuda()
        res = (torch.randn(shape, generator=g, dtype=torch.float64) * 2.0).to(dtype).cuda()
        eps = 1e-5 if ki % 2 == 0 else 1e-6
        worst_ulp, worst_bar = 0.0, 0.0
        for ep, relu, use_res in EPILOGUES:
            r = res if use_res else None
            got = _native.group_norm(x, groups, wt, bs, eps, relu=relu, res=r)
            assert got.shape == x.shape and got.dtype == dtype
            want, floor = _gn_reference(x, groups, wt, bs, eps, relu, r)
            ratio, in_ulp = ulp_check(got, want, dtype, floor)
            worst_ulp, worst_bar = max(worst_ulp, in_ulp), max(worst_bar, ratio)
            if ratio > 1.0:
                failures.append((kind, ep, eps, round(ratio, 2), round(in_ulp, 1)))
            assert torch.equal(_native.group_norm(x, groups, wt, bs, eps, relu=relu, res=r), got), (kind, ep)
            if kind.startswith("constant") and kind != "constant_outlier" and not use_res:
                b = bs.double().reshape(1, c, 1, 1).expand(shape)
                if not torch.equal(got.double(), b.clamp_min(0.0) if relu else b):                 # beta, bit for bit
                    failures.append((kind, ep, "output is not beta"))
        report.append(f"{kind}: {worst_ulp:.2f} ulp where |y| >= 1, {worst_bar:.2f} of the bar")
    print(f"\n[group_norm {form} {dtype}] " + "; ".join(report))
    assert not failures, (form, str(dtype), failures)


# ---- residual + LayerNorm, row statistics ---------------------------------------------------------------------------------------------
def _ln_rows(kind, rows, c, g):
    x = torch.randn((rows, c), generator=g, dtype=torch.float64)
    if kind.startswith("offset"):
        ratio = float(kind[6:])
        x = x + ratio                          # std 1, mean / std = ratio
    elif kind == "constant":
        x = torch.linspace(-300.0, 900.0, rows, dtype=torch.float64)[:, None].expand(rows, c).clone()
    elif kind == "massive":
        # the "massive activation" pattern of ViT residual streams: one or two channels 100-1000 times the rest
        x[:, 7] = 250.0 * (1 + torch.arange(rows, dtype=torch.float64) % 4)
        x[::2, c - 3] = -900.0
    return x


LN_KINDS = ["offset0", "offset100", "offset300", "offset1000", "constant", "massive"]
EPL = {384: 6, 768: 12, 1024: 16}                # values per lane of the one-wave-per-row kernels


def _ln_reference(v, w, b, eps):
    """float64 LayerNorm of the rounded row values v: (h, mean, rstd)."""
    vd = v.double()
    mean = vd.mean(-1, keepdim=True)
    var = ((vd - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    return (vd - mean) * rstd * w.double() + b.double(), mean, rstd


def _ln_floor(v, mean, rstd, w, b, c):
    """Float32 error of k_residual_layernorm's statistics and epilogue (u = 2^-24), K = values per lane + 6 shuffle levels:
        mean: a float32 sum of c values, at most K additions deep, then one multiply  ->  |dmean| <= (K + 1) u mean|v|
        h = ((v - mean) rstd) w + b: the centred sum of squares (K deep, relative), rsqrtf, three roundings -> (K + 4) u |(v - mean) rstd w|
              plus the sum's shift: |dmean| rstd |w|, and the bias add: u |b|."""
    k = EPL[c] + 6
    dmean = (k + 1) * U32 * v.double().abs().mean(-1, keepdim=True)
    return dmean * rstd * w.double().abs() + (k + 4) * U32 * ((v.double() - mean) * rstd * w.double()).abs() + U32 * b.double().abs()


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("c", [384, 768, 1024])
def test_residual_layernorm_statistics(gpu, dtype, c):
    """ds_residual_layernorm against a float64 LayerNorm of the residual stream it stores, on rows with a common mode up to 1000 std,
    constant rows, massive channels, and a branch that cancels the residual.

    Expected error: x_out = x + gamma * branch is float32 then rounded (<= 2 ulp: half an ulp plus the float32 product's rounding).
    h = LayerNorm(x_out): the statistics are float32 over the rounded row (mean, then the centred sum of squares), so the bar is
    2 ulp + the floor of _ln_floor.  At a common mode of 1000 std (c = 1024) that floor is ~1.4e-3 absolute; the centred variance keeps
    rstd to K u relative.  A constant row has v - mean = 0 (its sum is exact and so is the mean): h = ln_bias bit for bit."""
    from src import _native
    g = torch.Generator().manual_seed(c * 7 + (dtype == BF16))
    rows = 37
    eps = 1e-6
    w = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).to(dtype).cuda()
    b = (torch.randn(c, generator=g, dtype=torch.float64) * 0.3).to(dtype).cuda()
    failures = []
    cases = [(k, _ln_rows(k, rows, c, g), None, None) for k in LN_KINDS]
    # a branch that cancels the residual: gamma * branch = -x exactly (gamma = 1, branch = -x): x_out = 0, h = ln_bias; and one that
    # leaves a small remainder of the residual (x_out a few ulps of x: a row of rounding-level values, normalised)
    x0 = (torch.randn((rows, c), generator=g, dtype=torch.float64) * 40.0).to(dtype)
    cases.append(("cancel_exact", x0.double(), -x0.double(), torch.ones(c, dtype=torch.float64)))
    gam = torch.full((c,), 0.998, dtype=torch.float64).to(dtype).double()
    cases.append(("cancel_near", x0.double(), -x0.double(), gam))
    for kind, xv, br, gm in cases:
        x = xv.to(dtype).cuda()
        branch = None if br is None else br.to(dtype).cuda()
        gamma = None if gm is None else gm.to(dtype).cuda()
        x_out, h = _native.residual_layernorm(x, branch, gamma, w, b, eps)
        if branch is not None:
            xr = x.double() + gamma.double() * branch.double()
            # float32 product and sum before the rounding to the output type: 2u (|x| + |gamma branch|)
            r, _ = ulp_check(x_out, xr, dtype, 2 * U32 * (x.double().abs() + (gamma.double() * branch.double()).abs()))
            if r > 1.0:
                failures.append((kind, "x_out", round(r, 2)))
            v = x_out
        else:
            v = x
        want, mean, rstd = _ln_reference(v, w, b, eps)
        r, in_ulp = ulp_check(h, want, dtype, _ln_floor(v, mean, rstd, w, b, c))
        if r > 1.0:
            failures.append((kind, "h", round(r, 2), round(in_ulp, 1)))
        if kind in ("constant", "cancel_exact"):
            assert torch.equal(h, b.expand_as(h)), kind                  # ln_bias, bit for bit
        x_out2, h2 = _native.residual_layernorm(x, branch, gamma, w, b, eps)
        assert torch.equal(h2, h) and torch.equal(x_out2, x_out), kind
        # ds_row_stats on the same rows: {rstd, -mean * rstd} in float32
        st = _native.row_stats(v.contiguous(), eps)
        assert st.shape == (rows, 2) and torch.isfinite(st).all()
        assert torch.equal(_native.row_stats(v.contiguous(), eps), st), kind
        k = EPL[c] + 6
        dmean = (k + 1) * U32 * v.double().abs().mean(-1)
        rs, nm = rstd[:, 0], -mean[:, 0] * rstd[:, 0]
        r1, _ = ulp_check(st[:, 0], rs, torch.float32, (k + 3) * U32 * rs)
        r2, _ = ulp_check(st[:, 1], nm, torch.float32, dmean * rs + (k + 4) * U32 * nm.abs())
        if max(r1, r2) > 1.0:
            failures.append((kind, "row_stats", round(r1, 2), round(r2, 2)))
    assert not failures, (c, str(dtype), failures)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_row_stats_rows_of_every_size(gpu, dtype):
    """ds_row_stats alone at the networks' channel counts on offset and massive rows, many rows (several workgroups, a partial last one).
    Bars as test_residual_layernorm_statistics: rstd to 2 ulp + (K + 3) u relative; -mean rstd to 2 ulp + the mean's float32 sum."""
    from src import _native
    g = torch.Generator().manual_seed(17 + (dtype == BF16))
    eps = 1e-6
    for c in (384, 768, 1024):
        k = EPL[c] + 6
        for kind in ("offset1000", "massive", "constant"):
            v = _ln_rows(kind, 1027, c, g).to(dtype).cuda()
            _, mean, rstd = _ln_reference(v, torch.ones(c, device="cuda"), torch.zeros(c, device="cuda"), eps)
            st = _native.row_stats(v, eps)
            rs, nm = rstd[:, 0], -mean[:, 0] * rstd[:, 0]
            r1, _ = ulp_check(st[:, 0], rs, torch.float32, (k + 3) * U32 * rs)
            r2, _ = ulp_check(st[:, 1], nm, torch.float32, (k + 1) * U32 * v.double().abs().mean(-1) * rs + (k + 4) * U32 * nm.abs())
            assert r1 <= 1.0 and r2 <= 1.0, (c, kind, r1, r2)
            assert torch.equal(_native.row_stats(v, eps), st)


# ---- online softmax of the fused attention ----------------------------------------------------------------------------------------------
ATT_SHAPES = [(1, 1, 2, 8), (2, 65, 2, 72), (1, 1025, 2, 1032), (1, 4097, 2, 4104)]     # (b, n_valid, heads, token stride)


def _att_operands(scenario, b, n, h, npad, dtype, g):
    """qk [b, npad, 2, h, 64], vt [b, h*64, npad] and a bias [h, n, n] (natural units) whose logits realise the scenario.  Query
    channel 0 is 8 and the scale 0.125, so key channel 0 IS the logit, plus a small term from the other 63 channels (|.| ~ 0.06)."""
    q = torch.randn((b, npad, h, 64), generator=g, dtype=torch.float64) * 0.25
    k = torch.randn((b, npad, h, 64), generator=g, dtype=torch.float64) * 0.25
    v = torch.randn((b, h * 64, npad), generator=g, dtype=torch.float64)
    q[..., 0] = 8.0
    bias = torch.zeros((h, n, n), dtype=torch.float64)
    keys = torch.arange(npad, dtype=torch.float64)
    if scenario == "spread":
        # one key per (batch, head) 115+ above every other: all others underflow, the output is that key's V row
        k[..., 0] = -110.0 - 20.0 * torch.rand((b, npad, h), generator=g, dtype=torch.float64)
        top = torch.randint(0, n, (b, h), generator=g)
        for bi in range(b):
            for hi in range(h):
                k[bi, top[bi, hi], hi, 0] = 5.0
    elif scenario == "equal":
        # every key identical: all logits equal (and large), the output is the mean of V
        k[:, :] = k[:, :1]
        k[..., 0] = 60.0
    elif scenario == "last_tile":
        # the row maximum sits in the last 64-key tile, every earlier tile about 50 below it
        last = (n - 1) // 64 * 64
        k[..., 0] = 20.0 - 50.0 + 2.0 * torch.randn((b, npad, h), generator=g, dtype=torch.float64)
        k[:, last:, :, 0] = 20.0 + torch.randn((b, npad - last, h), generator=g, dtype=torch.float64)
    elif scenario == "masked":
        # ordinary logits; a bias of -1e4 on chosen keys (the first, the last, one in the middle, and each head's strongest key)
        k[..., 0] = 3.0 * torch.randn((b, npad, h), generator=g, dtype=torch.float64)
        strongest = k[0, :n, :, 0].argmax(0)
        for hi in range(h):
            for j in {0, n - 1, n // 2, int(strongest[hi])}:
                bias[hi, :, j] = -1.0e4
    # pad keys (token stride > n_valid) carry the largest logit and large V: any leak shows
    k[:, n:, :, 0] = 300.0
    v[:, :, n:] = -250.0
    qk = torch.stack([q, k], dim=2).to(dtype)
    return qk, v.to(dtype), bias


def _att_reference(qk, vt, n, bias, npad):
    from src import vit_mi355x as vm
    full = None
    if bias is not None:
        full = torch.zeros((bias.shape[0], npad, npad), dtype=torch.float64, device="cuda")
        full[:, :n, :n] = torch.where(bias <= -1.0e4, float("-inf"), bias).cuda()      # -1e4 in the kernel = the key removed
    want = vm.attention_reference(qk.double(), vt.double(), n, 0.125, full)
    mag = vm.attention_reference(qk.double(), vt.double().abs(), n, 0.125, full)      # sum_j p_j |v_j|
    return want[:, :n], mag[:, :n]


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("scenario,with_bias", [("spread", False), ("spread", True), ("equal", False), ("equal", True),
                                                ("last_tile", False), ("last_tile", True), ("masked", True)])
def test_attention_online_softmax(gpu, dtype, with_bias, scenario):
    """ds_attention_fwd (the default generation for each shape) against a float64 softmax attention of the same rounded operands.

    Expected error: P = exp2(.) is rounded to the operand type for the P.V MFMA (relative u_P = 2^-11 float16, 2^-8 bfloat16) while the
    normaliser sums it in float32, so out = sum p v / sum p is off by at most u_P (sum p |v| / sum p + |out|); one rounding of the
    output on top: the bar is 2 ulp + u_P (S + |want|) with S = sum_j p_j |v_j| in float64.  Where every live p is exactly
    representable -- one key left ("spread": p = 1, the rest underflow to 0) or all logits equal (p = 1 for every key) -- the P
    rounding is gone and only float32 accumulation remains: the bar is 2 ulp + 2^-16 (S + |want|) (at most 65 tiles of sequential
    float32 adds and the exponent's FMA residue, ~100 u).  "masked" needs the bias operand: keys at -1e4 must act as removed keys
    (the float16 operand holds bias / scale, and -8e4 is past float16's range: the pack saturates it instead of storing -inf, which
    the bias MFMA's identity operand turned into a row of NaN)."""
    from src import _native
    g = torch.Generator().manual_seed(zlib.crc32(f"{scenario} {with_bias} {dtype}".encode()))
    u_p = 2.0 ** -11 if dtype == F16 else 2.0 ** -8
    exact_p = scenario in ("spread", "equal")
    failures = []
    for (b, n, h, npad) in ATT_SHAPES:
        if scenario == "masked" and n < 8:
            continue                                   # masking four keys of a one-key sequence leaves nothing to attend to
        qk, vt, bias = _att_operands(scenario, b, n, h, npad, dtype, g)
        qk, vt = qk.cuda(), vt.cuda()
        packed = _native.attention_bias_pack(bias.cuda(), npad, dtype) if with_bias else None
        got = _native.attention_fwd(qk, vt, n, 0.125, packed)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(_native.attention_fwd(qk, vt, n, 0.125, packed), got)
        want, mag = _att_reference(qk, vt, n, bias if with_bias else None, npad)
        floor = (2.0 ** -16 if exact_p else u_p) * (mag + want.abs())
        r, in_ulp = ulp_check(got[:, :n], want, dtype, floor)
        if r > 1.0:
            failures.append((n, round(r, 2), round(in_ulp, 1)))
        if scenario == "spread":
            # the output IS the surviving key's V row, to the output's rounding
            top = qk[:, :n, 1, :, 0].double().argmax(1)                         # [b, h]
            rows = torch.stack([torch.stack([vt[bi, hi * 64:(hi + 1) * 64, top[bi, hi]] for hi in range(h)]) for bi in range(b)])
            assert torch.equal(got[:, :n].reshape(b, n, h, 64), rows.reshape(b, 1, h, 64).expand(b, n, h, 64)), n
    assert not failures, (scenario, with_bias, str(dtype), failures)
