"""The GEMM / implicit-GEMM convolution family of csrc/ds_linear.hip against references that leave no tolerance to hide in.

Part A -- exact integers.  Operands from {-1, 0, +1}, small integer bias / residuals, gamma a power of two: every product, every
partial sum in any order and the result are exactly representable, so the kernel must reproduce a float64 reference BIT FOR BIT,
whatever its tile schedule, MFMA shape, K split or summation order.  A dropped, duplicated or misplaced term is a whole-number
difference.  test_exact_cases_stay_in_the_exact_range (no GPU needed) proves the premise for every case of this file.

Part B -- real-valued operands, per element: |got - ref64| <= 1/2 ulp_out + 2 (K + 4) 2^-24 sum |terms| (util.rounding_bound_ratio),
the single-rounding definition of include/depthstereo.h (fp32 accumulation, fp32 epilogue, one rounding to the output type).

Which kernel renders a tile follows ln_launch (csrc/ds_linear.hip), with T = ceil(M / 256) * (N / 256) tiles on a grid of G
workgroups (G = one per CU: 256 on an MI355X, or DS_LIN_GRID rounded down to a multiple of 8):
    ragged = T % G             if T > G and DS_LIN_RAGGED_DEN (4) * (T % G) <= G, else 0: the last `ragged` tiles of the list
    thin   = ragged == N / 256 and (ceil(M / 256) - 1) % 8 == 0 and DS_LIN_RAGGED_KSPLIT <= 1 (dense, bias / residual epilogues only)
    deep   = DS_LIN_RAGGED_RING == 6, or 8 * ragged <= G when the switch is unset (6-slot ring; otherwise 3 slots)
    K split (ragged, not thin, deep): the largest 2^s <= DS_LIN_RAGGED_KSPLIT with 8 * ragged * 2^s <= G, (K / 64) % 2^s == 0,
                                      K / 64 / 2^s >= _KEEP and K / 64 >= _MIN
The convolution (CONV != 0) has no ragged round: its tiles are walked by the persistent kernel alone."""
import contextlib
import functools
import os
import zlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conftest  # noqa: F401
from util import first_mismatches, rounding_bound_ratio, small_ints, ternary, ulp_distance

GPU = pytest.mark.gpu
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
EXACT_MAX = {"f16": 2048, "bf16": 256}          # integers of at most this magnitude are exact in the type
# erf-GELU of an exact integer pre-activation, distance from float64 erf-GELU rounded to the type, in ulps of the type but never
# finer than 2^-24 (util.ulp_distance: float16's own subnormal spacing; bfloat16 keeps float32's exponents, and in its ulps the
# clamp of ln_gelu beyond |v| = 6, GELU(-8) -> -5.9e-9 instead of -5e-15, would read as 10^4 ulps of nothing).  float16: the bar of
# test_linear_gelu_polynomial_against_erf_everywhere.  bfloat16: the worst distance measured on an MI355X over every GELU case of
# this file, 0.099 (that clamp: 5.9e-9 / 2^-24; every output above 2^-17 in magnitude is the correctly rounded one), plus one ulp
# -- DESIGN.md 3.10.1
GELU_ULPS = {"f16": 1.0, "bf16": 1.099}
ENV = ("DS_LIN_GRID", "DS_LIN_RAGGED", "DS_LIN_RAGGED_THIN", "DS_LIN_RAGGED_RING", "DS_LIN_RAGGED_PIPE", "DS_LIN_RAGGED_DEN",
       "DS_LIN_RAGGED_KSPLIT", "DS_LIN_RAGGED_KSPLIT_MIN", "DS_LIN_RAGGED_KSPLIT_KEEP")


@pytest.fixture
def lin_env(gpu):
    """src._native with every DS_LIN_* switch restored afterwards."""
    from src import _native
    old = {k: os.environ.get(k) for k in ENV}
    try:
        yield _native
    finally:
        _native.linear_env(**old)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _density(dt, k_total):
    """Nonzero fraction d of both operands: the sum of k_total products has variance k_total d^2.  float16: 0.5 (K = 4096: max |sum|
    about 160 of 2048).  bfloat16 holds integers to 256 only: d = sqrt(60 / K) keeps the standard deviation at 7.7 (0.12 at K = 4096
    or 9 x 512 channels, 0.23 at 9 x 128), capped at 0.5 for short contractions."""
    return 0.5 if dt == "f16" else min(0.5, (60.0 / k_total) ** 0.5)


def _gamma(g, n):
    return torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dtype=torch.float64)[torch.randint(0, 6, (n,), generator=g)]


class Want:
    """What one launch must produce: `pre` the float64 value in front of the activation, `act` None / "relu" / "gelu", `bound` an
    upper bound of every partial accumulator in any summation order (the same formula on absolute values)."""

    def __init__(self, pre, act, bound):
        self.pre, self.act, self.bound = pre, act, float(bound.max())

    @property
    def value(self):
        return self.pre.clamp(min=0) if self.act == "relu" else self.pre


def _dev(t, dt):
    return t.to(DT[dt]).cuda()


def _check(got, want, dt, what):
    """Part A: bit for bit (GELU: within GELU_ULPS of float64 erf-GELU of the exact pre-activation, rounded to the type)."""
    if want.act == "gelu":
        ref = F.gelu(want.pre)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        d = float(ulp_distance(got, ref, floor=2.0 ** -24).max())
        print(f"{what}: erf-GELU of exact integers, worst distance {d:.3f} {dt} ulps")
        assert d <= GELU_ULPS[dt], (what, d)
        return
    ref = want.value.to(DT[dt])
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    assert torch.equal(got.cpu(), ref), (what, first_mismatches(got, ref))


# ---- the dense chain ------------------------------------------------------------------------------------------------------------------
# name: (M, N, K, (channels, batch, tokens) of the V^T launch on the same K).  Default grid (256 workgroups): T <= 256, no ragged round.
DENSE = {
    "k128": (256, 256, 128, (256, 2, 128)),            # one tile, ONE K iteration (an iteration is 128 wide)
    "k384_m300": (300, 256, 384, (300, 2, 128)),       # three K iterations (odd), last row panel shifted up to end at row 300
    "k4096": (256, 256, 4096, (256, 1, 256)),          # 32 K iterations: the longest contraction of the encoders
    "m77": (77, 512, 256, None),                       # rows < 256: padded to one panel by the wrapper; two column panels
    "m2100": (2100, 768, 128, (600, 2, 384)),          # 9 x 3 tiles, shifted last panel; V^T: token panels that straddle two images
    # DS_LIN_GRID=8: 9 x 2 = 18 tiles, 18 % 8 = 2 = N / 256 and (9 - 1) % 8 == 0: ragged AND thin-eligible (4 * 2 <= 8); 8 * 2 > 8: the
    # 3-slot ring unless DS_LIN_RAGGED_RING=6.  V^T: 2 x 5 = 10 tiles, 10 % 8 = 2 ragged (never thin)
    "sched": (2100, 512, 384, (512, 4, 320)),
    # DS_LIN_GRID=64, DEN=2, KSPLIT=8, MIN=1, KEEP=2: 33 x 2 = 66 tiles, 66 % 64 = 2, 2 * 2 <= 64: ragged = 2; KSPLIT > 1: not thin;
    # 8 * 2 <= 64: deep; K / 64 = 8 K-tiles: s = 2 (8 * 2 * 4 = 64 <= 64, 8 / 4 = 2 >= KEEP; 8 * 2 * 8 > 64): a 4-way split.  V^T alike
    "ksplit": (33 * 256, 512, 512, (33 * 256, 2, 256)),
}
DENSE_OPS = ("lin", "lin_nobias", "relu", "relu_nobias", "gelu", "res_gamma", "res", "vt")


@functools.lru_cache(maxsize=None)
def dense_case(name, dt):
    m, n, k, vt = DENSE[name]
    g, d = _gen("dense", name, dt), _density(dt, k)
    o = {"x": ternary(g, (m, k), d), "w": ternary(g, (n, k), d), "b": small_ints(g, (n,), 16), "res": small_ints(g, (m, n), 16),
         "gam": _gamma(g, n)}
    acc, aabs = o["x"] @ o["w"].T, o["x"].abs() @ o["w"].abs().T
    ab = aabs + o["b"].abs()
    want = {"lin": Want(acc + o["b"], None, ab), "lin_nobias": Want(acc, None, aabs), "relu": Want(acc + o["b"], "relu", ab),
            "relu_nobias": Want(acc, "relu", aabs), "gelu": Want(acc + o["b"], "gelu", ab)}
    if m >= 256:
        want["res_gamma"] = Want(o["res"] + o["gam"] * (acc + o["b"]), None, o["res"].abs() + o["gam"].abs() * ab)
        want["res"] = Want(o["res"] + acc + o["b"], None, o["res"].abs() + ab)
    if vt:
        c, b, t = vt
        o["wv"], o["h"] = ternary(g, (c, k), d), ternary(g, (b, t, k), d)
        want["vt"] = Want(o["wv"] @ o["h"].transpose(1, 2), None, o["wv"].abs() @ o["h"].abs().transpose(1, 2))          # [b, c, t]
    return o, want


def _raw_linear(nat, x, w, b, act):
    """ds_linear through the raw entry point (the wrapper exposes act 0 / 1 only); rows >= 256."""
    out = torch.empty((x.shape[0], w.shape[0]), dtype=x.dtype, device=x.device)
    rc = nat.lib().ds_linear(nat.ctx_for(torch.cuda.current_device()), x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                             out.data_ptr(), x.shape[0], w.shape[0], x.shape[1], w.shape[0], act, 1 if x.dtype == torch.float16 else 2, None)
    assert rc == 0, nat.lib().ds_last_error()
    return out


def _run_dense(nat, o, want, dt):
    dv = {k: _dev(v, dt) for k, v in o.items()}
    x, w, b = dv["x"], dv["w"], dv["b"]
    rows = x.shape[0]
    xp = x if rows >= 256 else torch.cat([x, x.new_zeros((256 - rows, x.shape[1]))])         # what the wrapper does for act 0 / 1
    got = {"lin": nat.linear(x, w, b), "lin_nobias": nat.linear(x, w, None), "gelu": nat.linear(x, w, b, True),
           "relu": _raw_linear(nat, xp, w, b, 2)[:rows], "relu_nobias": _raw_linear(nat, xp, w, None, 2)[:rows]}
    if "res" in want:
        got["res_gamma"] = nat.linear_residual(x, w, b, dv["gam"], dv["res"])
        got["res"] = nat.linear_residual(x, w, b, None, dv["res"])
    if "vt" in want:
        got["vt"] = nat.linear_vt(dv["wv"], dv["h"])
    return got


RAGGED_KINDS = {"linear+ragged": ("lin", "lin_nobias", "relu", "relu_nobias"), "linear_gelu+ragged": ("gelu",),
                "linear_residual+ragged": ("res_gamma", "res"), "linear_vt+ragged": ("vt",)}


@contextlib.contextmanager
def _ragged_launches(nat, counts):
    """Fills `counts` with the number of ragged-round launches per timer kind made inside the block (ds_kernel_timer_read)."""
    dev = torch.cuda.current_device()
    torch.cuda.synchronize()
    nat.kernel_timer_enable(dev, True)
    try:
        yield
        for kind in RAGGED_KINDS:
            counts[kind] = nat.kernel_timer_read(dev, kind)[0]
            counts[kind.split("+")[0]] = nat.kernel_timer_read(dev, kind.split("+")[0])[0]
    finally:
        nat.kernel_timer_enable(dev, False)


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["k128", "k384_m300", "k4096", "m77", "m2100"])
def test_dense_chain_is_exact_on_integers(lin_env, name, dt):
    o, want = dense_case(name, dt)
    counts = {}
    with _ragged_launches(lin_env, counts):
        got = _run_dense(lin_env, o, want, dt)
    assert all(counts[k] == 0 for k in RAGGED_KINDS), counts            # at most 27 tiles on one workgroup per CU: the persistent walk alone
    for op in want:
        _check(got[op], want[op], dt, f"dense {name} {dt} {op}")


SCHEDULES = {   # switches on top of DS_LIN_GRID=8, and whether the ragged timer must tick
    "walk": (dict(DS_LIN_RAGGED="0"), False),
    "thin": (dict(DS_LIN_RAGGED="1", DS_LIN_RAGGED_THIN="1"), True),
    "ring6_pipelined": (dict(DS_LIN_RAGGED="1", DS_LIN_RAGGED_THIN="0", DS_LIN_RAGGED_RING="6", DS_LIN_RAGGED_PIPE="1"), True),
    "ring6_plain": (dict(DS_LIN_RAGGED="1", DS_LIN_RAGGED_THIN="0", DS_LIN_RAGGED_RING="6", DS_LIN_RAGGED_PIPE="0"), True),
    "ring3": (dict(DS_LIN_RAGGED="1", DS_LIN_RAGGED_THIN="0", DS_LIN_RAGGED_RING="3"), True),
}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_every_schedule_is_exact_on_integers(lin_env, schedule, dt):
    """Every kernel that can render a tile, on the shape whose last two tiles are the ragged round of a grid of 8 (DENSE["sched"]): the
    persistent walk alone, k_linear_thin, k_linear_ragged with the 6-slot ring (pipelined and plain) and the 3-slot ring.  The ragged
    timer kind (ds_kernel_timer_read) says that a second kernel was launched behind the main one -- or, for the walk, that none was.
    (It does not tell the three ragged kernels apart: that part rests on the dispatch code quoted in the module docstring.)"""
    nat = lin_env
    o, want = dense_case("sched", dt)
    switches, ragged = SCHEDULES[schedule]
    nat.linear_env(DS_LIN_GRID="8", **switches)
    counts = {}
    with _ragged_launches(nat, counts):
        got = _run_dense(nat, o, want, dt)
    for kind, ops in RAGGED_KINDS.items():
        assert counts[kind.split("+")[0]] == len(ops), (schedule, counts)
        assert counts[kind] == (len(ops) if ragged else 0), (schedule, counts)
    for op in want:
        _check(got[op], want[op], dt, f"{schedule} {dt} {op}")


KSPLIT = dict(DS_LIN_GRID="64", DS_LIN_RAGGED_KSPLIT="8", DS_LIN_RAGGED_KSPLIT_MIN="1", DS_LIN_RAGGED_KSPLIT_KEEP="2", DS_LIN_RAGGED_DEN="2")


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_k_split_of_the_ragged_round_is_exact_on_integers(lin_env, dt):
    """The 4-way K split of two ragged tiles (DENSE["ksplit"]): fp32 partials of integers add up exactly in any order."""
    nat = lin_env
    o, want = dense_case("ksplit", dt)
    nat.linear_env(**KSPLIT)
    counts = {}
    with _ragged_launches(nat, counts):
        got = _run_dense(nat, o, want, dt)
    for kind, ops in RAGGED_KINDS.items():
        assert counts[kind] == len(ops), counts
    for op in want:
        _check(got[op], want[op], dt, f"ksplit {dt} {op}")


# ---- scatter / gather front ends ------------------------------------------------------------------------------------------------------
SHUFFLE = {   # name: (stride, out_channels, in_channels, has_bias); two images of 13 x 11 pixels (286 rows: two panels, width % 8 != 0)
    "s2_c64": (2, 64, 128, True), "s4_c256": (4, 256, 256, True), "s2_c256": (2, 256, 128, False), "s4_c64": (4, 64, 128, True),
}


@functools.lru_cache(maxsize=None)
def shuffle_case(name, dt):
    s, co, ci, has_bias = SHUFFLE[name]
    g, d = _gen("shuffle", name, dt), _density(dt, ci)
    o = {"x": ternary(g, (2, ci, 13, 11), d), "w": ternary(g, (ci, co, s, s), d), "b": small_ints(g, (co,), 16) if has_bias else None}
    pre = F.conv_transpose2d(o["x"], o["w"], o["b"], stride=s)
    bound = F.conv_transpose2d(o["x"].abs(), o["w"].abs(), None if o["b"] is None else o["b"].abs(), stride=s)
    return o, {"shuffle": Want(pre, None, bound)}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(SHUFFLE))
def test_conv_transpose_shuffle_is_exact_on_integers(lin_env, name, dt):
    """ds_linear_shuffle against F.conv_transpose2d in float64 on the same integers: every output pixel of every tap."""
    s, co, ci, has_bias = SHUFFLE[name]
    o, want = shuffle_case(name, dt)
    layer = nn.ConvTranspose2d(ci, co, s, stride=s, bias=has_bias).cuda()
    with torch.no_grad():
        layer.weight.copy_(o["w"])
        if has_bias:
            layer.bias.copy_(o["b"])
    x = _dev(o["x"], dt).contiguous(memory_format=torch.channels_last)
    assert lin_env.conv_transpose_shuffle_supported(layer, x)
    got = lin_env.conv_transpose_shuffle(layer, x)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _check(got, want["shuffle"], dt, f"shuffle {name} {dt}")


READOUT = {"n258": (320, 258, 128, 256), "n320": (320, 320, 256, 512)}        # tokens_padded, tokens, K, N; two images
PAD_FILL = 1024.0          # exact in both types; a pad row that leaked would add 1024 * (a sum of weights) to an output


@functools.lru_cache(maxsize=None)
def readout_case(name, dt):
    npad, n, k, nf = READOUT[name]
    g, d = _gen("readout", name, dt), _density(dt, k)
    o = {"x": ternary(g, (2, npad, k), d), "w": ternary(g, (nf, k), d), "cls": small_ints(g, (2, nf), 4)}
    o["x"][:, n:] = PAD_FILL
    pre = o["x"][:, 1:n] @ o["w"].T + o["cls"][:, None]
    bound = o["x"].abs() @ o["w"].abs().T + o["cls"].abs()[:, None]                # the cls and pad rows are accumulated too
    return o, {"readout": Want(pre, "gelu", bound)}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(READOUT))
def test_linear_readout_on_integers(lin_env, name, dt):
    """ds_linear_readout: erf-GELU of an exact integer per output; the cls row and the pad rows (filled with 1024) reach no output row."""
    npad, n, k, nf = READOUT[name]
    o, want = readout_case(name, dt)
    got = lin_env.linear_readout(_dev(o["x"], dt), n, _dev(o["w"], dt), _dev(o["cls"], dt))
    assert tuple(got.shape) == (2, n - 1, nf)
    _check(got, want["readout"], dt, f"readout {name} {dt}")


LN = {"m300": (300, 256, 384), "m2100": (2100, 512, 128)}
LN_VT = {"c300": (300, 2, 128, 384)}                                          # channels, batch, tokens, K


def _ln_stats(g, rows, dt):
    """{rstd, -mean rstd} per row as the caller of ds_linear_ln supplies them: rstd = 2^-j, an integer second member -- the folded
    expression rstd * acc + (-mean rstd) * colsum + bias is then a multiple of 2^-j (j <= 2 for float16, <= 1 for bfloat16)."""
    j = torch.randint(0, 3 if dt == "f16" else 2, (rows,), generator=g).double()
    return torch.stack([2.0 ** -j, small_ints(g, (rows,), 3)], 1)


@functools.lru_cache(maxsize=None)
def ln_case(name, dt):
    m, n, k = LN[name]
    g, d = _gen("ln", name, dt), _density(dt, k)
    o = {"x": ternary(g, (m, k), d), "w": ternary(g, (n, k), d), "colsum": small_ints(g, (n,), 4), "b": small_ints(g, (n,), 8),
         "stats": _ln_stats(g, m, dt)}
    acc, aabs = o["x"] @ o["w"].T, o["x"].abs() @ o["w"].abs().T
    folded = o["stats"][:, :1] * acc + o["stats"][:, 1:] * o["colsum"]
    fabs = aabs + o["stats"][:, 1:].abs() * o["colsum"].abs()
    return o, {"ln": Want(folded + o["b"], None, fabs + o["b"].abs()), "ln_nobias": Want(folded, None, fabs),
               "ln_gelu": Want(folded + o["b"], "gelu", fabs + o["b"].abs())}


@functools.lru_cache(maxsize=None)
def ln_vt_case(name, dt):
    c, b, t, k = LN_VT[name]
    g, d = _gen("ln_vt", name, dt), _density(dt, k)
    o = {"wv": ternary(g, (c, k), d), "x": ternary(g, (b, t, k), d), "colsum": small_ints(g, (c,), 4), "stats": _ln_stats(g, b * t, dt)}
    rstd, nm = o["stats"][:, 0].view(b, 1, t), o["stats"][:, 1].view(b, 1, t)
    pre = rstd * (o["wv"] @ o["x"].transpose(1, 2)) + nm * o["colsum"].view(1, c, 1)
    bound = o["wv"].abs() @ o["x"].abs().transpose(1, 2) + nm.abs() * o["colsum"].abs().view(1, c, 1)
    return o, {"vt_ln": Want(pre, None, bound)}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(LN))
def test_linear_ln_is_exact_on_integers(lin_env, name, dt):
    """ds_linear_ln with caller-made statistics: rstd * acc + (-mean rstd) * colsum + bias, exact; its GELU form within GELU_ULPS."""
    o, want = ln_case(name, dt)
    x, w, b = _dev(o["x"], dt), _dev(o["w"], dt), _dev(o["b"], dt)
    colsum, stats = o["colsum"].float().cuda(), o["stats"].float().cuda().contiguous()
    _check(lin_env.linear_ln(x, w, colsum, b, stats), want["ln"], dt, f"ln {name} {dt}")
    _check(lin_env.linear_ln(x, w, colsum, None, stats), want["ln_nobias"], dt, f"ln {name} {dt} no bias")
    _check(lin_env.linear_ln(x, w, colsum, b, stats, True), want["ln_gelu"], dt, f"ln {name} {dt} gelu")


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_linear_vt_ln_is_exact_on_integers(lin_env, dt):
    o, want = ln_vt_case("c300", dt)
    got = lin_env.linear_vt_ln(_dev(o["wv"], dt), o["colsum"].float().cuda(), _dev(o["x"], dt), o["stats"].float().cuda().contiguous())
    _check(got, want["vt_ln"], dt, f"vt_ln {dt}")


# ---- ds_conv3x3_nhwc: the implicit GEMM ---------------------------------------------------------------------------------------------
CONV = {   # name: (batch, height, width, in_channels, out_channels); a tile is 256 consecutive pixels of the NHWC image list
    "one_tile": (1, 16, 16, 128, 256),           # one image is exactly one tile
    "three_images": (3, 11, 9, 256, 512),        # 297 pixels: image seams at 99 and 198 inside tile 0, tile 1 shifted up to end at 297
    "seam": (2, 19, 23, 512, 256),               # 874 pixels: the seam at 437 in the middle of tile 1, ragged last tile
    "row": (1, 1, 300, 256, 128),                # every pixel is a border pixel (no row above or below); 256 x 128 tiles
    "column": (1, 300, 1, 128, 384),             # every pixel is a border pixel (no neighbour left or right); three 128-column tiles
    "seam_c128": (2, 19, 23, 256, 128),          # the head's 256 -> 128 shape class on the seam map
    "three_images_c128": (3, 11, 9, 128, 128),
}
CONV_EPILOGUES = {   # name: (bias, relu, res1, res2, relu_in)
    "none": (False, False, False, False, False), "bias": (True, False, False, False, False), "bias_relu": (True, True, False, False, False),
    "bias_res1_res2": (True, False, True, True, False), "bias_res1_relu": (True, True, True, False, False),
    "relu_in": (True, True, False, False, True),
}


def conv_ref(x, w):
    """3 x 3, stride 1, zero padding 1: x [B, H, W, C], w [O, 3, 3, C] (float64) -> [B, H, W, O], as nine shifted views and one product."""
    b, h, wd, c = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, ky:ky + h, kx:kx + wd] for ky in range(3) for kx in range(3)], dim=3)          # [B, H, W, 9 C], (ky, kx, c)
    return (cols.reshape(-1, 9 * c) @ w.reshape(w.shape[0], -1).T).view(b, h, wd, -1)


def _conv_epilogues(cout):
    return [e for e, (_, _, r1, _, rin) in CONV_EPILOGUES.items() if cout % 256 == 0 or not (r1 or rin)]


@functools.lru_cache(maxsize=None)
def conv_case(name, dt):
    b, h, wd, cin, cout = CONV[name]
    g, d = _gen("conv", name, dt), _density(dt, 9 * cin)
    o = {"x": ternary(g, (b, h, wd, cin), d), "w": ternary(g, (cout, 3, 3, cin), d), "b": small_ints(g, (cout,), 16),
         "r1": small_ints(g, (b, h, wd, cout), 16), "r2": small_ints(g, (b, h, wd, cout), 16)}
    # relu_in: x rectified inside the K loop.  A denser x (its negative half disappears), and exact zeros of both signs among it
    xz = ternary(g, (b, h, wd, cin), min(1.0, 2 * d))
    flat = xz.view(-1)
    flat[::7] = -0.0
    flat[3::11] = 0.0
    o["xz"] = xz
    acc, aabs = conv_ref(o["x"], o["w"]), conv_ref(o["x"].abs(), o["w"].abs())
    acc_z, aabs_z = conv_ref(xz.clamp(min=0), o["w"]), conv_ref(xz.clamp(min=0), o["w"].abs())
    want = {}
    for e in _conv_epilogues(cout):
        bias, relu, r1, r2, rin = CONV_EPILOGUES[e]
        pre, bound = (acc_z, aabs_z) if rin else (acc, aabs)
        for use, t in ((bias, o["b"]), (r1, o["r1"]), (r2, o["r2"])):
            if use:
                pre, bound = pre + t, bound + t.abs()
        want[e] = Want(pre, "relu" if relu else None, bound)
    return o, want


def _conv_modules(o, cin, cout):
    mods = {}
    for has_bias in (False, True):
        m = nn.Conv2d(cin, cout, 3, padding=1, bias=has_bias).cuda()
        with torch.no_grad():
            m.weight.copy_(o["w"].permute(0, 3, 1, 2))
            if has_bias:
                m.bias.copy_(o["b"])
        mods[has_bias] = m
    return mods


def _nchw(t, dt):
    """NHWC float64 -> the logical NCHW view of a channels_last device tensor."""
    return _dev(t, dt).permute(0, 3, 1, 2)


def _run_conv(nat, o, mods, e, dt):
    bias, relu, r1, r2, rin = CONV_EPILOGUES[e]
    got = nat.conv3x3(mods[bias], _nchw(o["xz"] if rin else o["x"], dt), relu=relu, res1=_nchw(o["r1"], dt) if r1 else None,
                      res2=_nchw(o["r2"], dt) if r2 else None, relu_in=rin)
    assert got.is_contiguous(memory_format=torch.channels_last)
    return got.permute(0, 2, 3, 1)


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("grid", [None, "8"])
@pytest.mark.parametrize("name", list(CONV))
def test_conv3x3_is_exact_on_integers(lin_env, name, grid, dt):
    """Every epilogue of ds_conv3x3_nhwc on every map, one workgroup per CU and 8 workgroups walking all tiles: bit for bit the
    convolution of the integers -- each tap of each 64-channel K-tile counted once, the zero line where a neighbour is missing and
    only there, no neighbour from the image next door."""
    b, h, wd, cin, cout = CONV[name]
    o, want = conv_case(name, dt)
    mods = _conv_modules(o, cin, cout)
    lin_env.linear_env(DS_LIN_GRID=grid)
    if "relu_in" in want:
        bits = _dev(o["xz"], dt).view(torch.int16)
        assert bool((bits == -32768).any()) and bool((bits == 0).any())          # -0.0 and +0.0 both reach the kernel
    for e in want:
        _check(_run_conv(lin_env, o, mods, e, dt), want[e], dt, f"conv {name} grid {grid} {dt} {e}")


@functools.lru_cache(maxsize=None)
def impulse_case():
    """Zero input except a single 1 at each image's four corners and the midpoint of its top edge, in channel 77; weights 1 + 3 ky + kx
    for that channel: every nonzero output names the tap that produced it."""
    b, h, wd, cin, cout = CONV["three_images"]
    x, w = torch.zeros((b, h, wd, cin), dtype=torch.float64), torch.zeros((cout, 3, 3, cin), dtype=torch.float64)
    for (yy, xx) in ((0, 0), (0, wd - 1), (h - 1, 0), (h - 1, wd - 1), (0, wd // 2)):
        x[:, yy, xx, 77] = 1.0
    w[:, :, :, 77] = 1.0 + 3.0 * torch.arange(3.0).view(3, 1) + torch.arange(3.0).view(1, 3)
    return {"x": x, "w": w}, Want(conv_ref(x, w), None, conv_ref(x, w))


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_conv3x3_impulses_name_their_taps(lin_env, dt):
    b, h, wd, cin, cout = CONV["three_images"]
    o, want = impulse_case()
    m = nn.Conv2d(cin, cout, 3, padding=1, bias=False).cuda()
    with torch.no_grad():
        m.weight.copy_(o["w"].permute(0, 3, 1, 2))
    got = lin_env.conv3x3(m, _nchw(o["x"], dt)).permute(0, 2, 3, 1)
    ref = want.value.to(DT[dt])
    if not torch.equal(got.cpu(), ref):
        maps = "\n".join(f"image {i}: got\n{got[i, :, :, 0].cpu().int()}\nwant\n{ref[i, :, :, 0].int()}" for i in range(b))
        pytest.fail(f"impulse map (output channel 0; tap = 1 + 3 ky + kx):\n{maps}\n{first_mismatches(got, ref)}")


CONV1X1 = (2, 256, 256, 13, 11)          # batch, in, out, height, width: 286 rows (two panels, the second shifted)


@functools.lru_cache(maxsize=None)
def conv1x1_case(dt):
    b, cin, cout, h, wd = CONV1X1
    g, d = _gen("conv1x1", dt), _density(dt, cin)
    o = {"x": ternary(g, (b, h, wd, cin), d), "w": ternary(g, (cout, cin), d), "b": small_ints(g, (cout,), 16)}
    return o, {"conv1x1": Want(o["x"] @ o["w"].T + o["b"], None, o["x"].abs() @ o["w"].abs().T + o["b"].abs())}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_conv1x1_through_the_gemm_is_exact_on_integers(lin_env, dt):
    """A 1x1 convolution by the route of test_conv1x1_through_the_in_tree_gemm (vit_mi355x.conv_module -> ds_linear on the NHWC rows)."""
    from src import vit_mi355x as vm
    b, cin, cout, h, wd = CONV1X1
    o, want = conv1x1_case(dt)
    layer = nn.Conv2d(cin, cout, 1).cuda()
    with torch.no_grad():
        layer.weight.copy_(o["w"].view(cout, cin, 1, 1))
        layer.bias.copy_(o["b"])
    layer = layer.to(DT[dt])
    x = _nchw(o["x"], dt)
    assert vm.conv1x1_hip_ok(layer, x)
    before = lin_env.CALLS["ds_linear"]
    with torch.no_grad():
        got = vm.conv_module(layer, x)
    assert lin_env.CALLS["ds_linear"] == before + 1
    _check(got.permute(0, 2, 3, 1), want["conv1x1"], dt, f"conv1x1 {dt}")


# ---- the premise of Part A, checked without a GPU -----------------------------------------------------------------------------------
def _exact_cases():
    for dt in DT:
        for name in DENSE:
            yield f"dense {name} {dt}", dt, dense_case(name, dt)[1]
        for name in SHUFFLE:
            yield f"shuffle {name} {dt}", dt, shuffle_case(name, dt)[1]
        for name in READOUT:
            yield f"readout {name} {dt}", dt, readout_case(name, dt)[1]
        for name in LN:
            yield f"ln {name} {dt}", dt, ln_case(name, dt)[1]
        for name in LN_VT:
            yield f"ln_vt {name} {dt}", dt, ln_vt_case(name, dt)[1]
        for name in CONV:
            yield f"conv {name} {dt}", dt, conv_case(name, dt)[1]
        yield f"conv1x1 {dt}", dt, conv1x1_case(dt)[1]


def test_exact_cases_stay_in_the_exact_range():
    """For every Part A case: every partial accumulator, in any order, stays below 2^24 (bounded by the same sum on absolute values);
    the value in front of the activation is exact in fp32, and -- unless GELU follows -- at most 2048 (float16) / 256 (bfloat16) in
    magnitude and exactly representable in the output type (gamma = 1/2 and rstd = 2^-j make binary fractions, so the round trip is
    checked, not only the magnitude); more than 90 % of these values are nonzero, and a ReLU both keeps and clamps a fair share."""
    for what, dt, wants in _exact_cases():
        for op, w in wants.items():
            assert w.bound < 2.0 ** 24, (what, op, w.bound)
            assert torch.equal(w.pre.float().double(), w.pre), (what, op)
            nonzero = float((w.pre != 0).double().mean())
            assert nonzero > 0.9, (what, op, nonzero)
            if w.act == "gelu":
                assert float(w.pre.abs().max()) <= EXACT_MAX[dt], (what, op)
                continue
            assert float(w.pre.abs().max()) <= EXACT_MAX[dt], (what, op, float(w.pre.abs().max()))
            assert torch.equal(w.pre.to(DT[dt]).double(), w.pre), (what, op)
            if w.act == "relu":
                kept = float((w.pre > 0).double().mean())
                assert 0.25 < kept < 0.75, (what, op, kept)
    o, w = impulse_case()
    assert float(w.pre.max()) == 9.0 and int((w.pre[..., 0] != 0).sum()) == 3 * (4 * 4 + 6)          # corners see 4 pixels, the edge midpoint 6


# ---- Part B: per-element rounding bound on real-valued operands -------------------------------------------------------------------
def _randn(g, shape, dt, scale=1.0, offset=0.0):
    """randn * scale + offset, ROUNDED to the type (the reference is evaluated on what the kernel reads), as float64."""
    return (torch.randn(shape, generator=g) * scale + offset).to(DT[dt]).double()


def _report(what, got, ref64, abs_terms, k_total):
    ratio, beyond = rounding_bound_ratio(got, ref64, abs_terms, k_total)
    print(f"{what}: worst error / bound {ratio:.3f}, {beyond} of {ref64.numel()} outputs more than one ulp from the float64 value")
    assert ratio <= 1.0, (what, ratio)


ROUNDING_DENSE = {   # name: (shape of DENSE, op, offset of x and w, scale of the residual)
    "dense": ("m2100", "lin", 0.0, 1.0), "residual_gamma": ("k128", "res_gamma", 0.0, 1.0), "vt": ("k384_m300", "vt", 0.0, 1.0),
    "offset3": ("k384_m300", "lin", 3.0, 1.0),                    # same-sign sums of about 9 K = 3456
    "residual100": ("k384_m300", "res_gamma", 0.0, 100.0),        # the residual stream late in BEiT-L against a branch of about 1
    "ksplit": ("ksplit", "lin", 0.0, 1.0),                        # fp32 partials of four workgroups through the workspace
}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(ROUNDING_DENSE))
def test_dense_rounding_bound(lin_env, name, dt):
    nat = lin_env
    shape, op, offset, res_scale = ROUNDING_DENSE[name]
    m, n, k, (c, b, t) = DENSE[shape]
    g = _gen("round", name, dt)
    if name == "ksplit":
        nat.linear_env(**KSPLIT)
    if op == "vt":
        wv, h = _randn(g, (c, k), dt, k ** -0.5), _randn(g, (b, t, k), dt)
        got = nat.linear_vt(_dev(wv, dt), _dev(h, dt))
        ref, terms = wv @ h.transpose(1, 2), wv.abs() @ h.abs().transpose(1, 2)
    else:
        x, w, bias = _randn(g, (m, k), dt, 1.0, offset), _randn(g, (n, k), dt, k ** -0.5, offset), _randn(g, (n,), dt)
        ref, terms = x @ w.T + bias, x.abs() @ w.abs().T + bias.abs()
        if op == "lin":
            got = nat.linear(_dev(x, dt), _dev(w, dt), _dev(bias, dt))
        else:
            gam, res = _randn(g, (n,), dt), _randn(g, (m, n), dt, res_scale)
            got = nat.linear_residual(_dev(x, dt), _dev(w, dt), _dev(bias, dt), _dev(gam, dt), _dev(res, dt))
            ref, terms = res + gam * ref, res.abs() + gam.abs() * terms
    if name == "ksplit":
        nat.linear_env(DS_LIN_RAGGED_KSPLIT="1")
        unsplit = nat.linear(_dev(x, dt), _dev(w, dt), _dev(bias, dt))
        differ = int((unsplit != got).sum())
        print(f"ksplit {dt}: {differ} outputs differ between the 4-way split and the single chain")
        # another fp32 summation order (include/depthstereo.h: ds_linear_reload_env): the one observable that tells the split from
        # the unsplit ragged round -- bit-reproducible, so this is not a matter of luck from run to run
        assert differ > 0 and torch.equal(unsplit[:32 * 256], got[:32 * 256])          # ... and only ragged tiles can differ
    _report(f"rounding {name} {dt}", got, ref, terms, k)


ROUNDING_CONV = {"res1_res2": ("seam_c256", "bias_res1_res2"), "c128": ("seam_c128", "bias")}
CONV_B = {"seam_c256": (2, 19, 23, 256, 256), "seam_c128": CONV["seam_c128"]}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(ROUNDING_CONV))
def test_conv3x3_rounding_bound(lin_env, name, dt):
    shape, e = ROUNDING_CONV[name]
    b, h, wd, cin, cout = CONV_B[shape]
    g = _gen("round conv", name, dt)
    o = {"x": _randn(g, (b, h, wd, cin), dt), "w": _randn(g, (cout, 3, 3, cin), dt, (9 * cin) ** -0.5), "b": _randn(g, (cout,), dt),
         "r1": _randn(g, (b, h, wd, cout), dt), "r2": _randn(g, (b, h, wd, cout), dt)}
    got = _run_conv(lin_env, o, _conv_modules(o, cin, cout), e, dt)
    ref, terms = conv_ref(o["x"], o["w"]) + o["b"], conv_ref(o["x"].abs(), o["w"].abs()) + o["b"].abs()
    if e == "bias_res1_res2":
        ref, terms = ref + o["r1"] + o["r2"], terms + o["r1"].abs() + o["r2"].abs()
    _report(f"rounding conv {name} {dt}", got, ref, terms, 9 * cin)
