"""Per-element tests of four single-pass kernels that every forward goes through, against float64 definitions on the CPU:

    ds_bias_act_nhwc        exact operands (multiples of 2^-10 / 2^-7, |v| <= 16): torch.equal to the float64 sum rounded once;
                            NaN / Inf / -0.0 like torch's relu(x + b + r1 + r2); a shape beyond one grid stride; return codes
    ds_reassemble_readout   exact proj + cls, then |got - gelu64(x)| <= 1/2 ulp + 8 2^-24 (|x| + |gelu64(x)|) per element
    ds_preprocess_bicubic   (and _rows) |got - ref64| <= 1/2 ulp + 16 2^-24 (S + |mean|) / std per element, from 1 x 1 inputs up
    ds_gconv3x3_nhwc_f32    exact integers bit for bit, impulses that name tap / channel / group, a rounding bound on real operands

Cases, references and checkers are tests/pointwise_cases.py; tests/test_pointwise_model_cpu.py shows on the CPU that those checkers
reject thirteen plausible mistakes.  Every operand of the device is a slice of a larger buffer: inputs lie in NaN (a read outside
the operand shows in the output; uint8 images lie in bytes that a second run inverts: equal bits), outputs in a sentinel that must
survive on both sides.  The kernels are called through _native.lib() so that the test owns every buffer."""
import ctypes

import numpy as np
import pytest
import torch

import conftest  # noqa: F401
import pointwise_cases as pc
from util import preprocess_ref, triple

GPU = pytest.mark.gpu
GUARD = 1024                 # elements on either side of every operand (a multiple of 16 bytes for every type)
SENTINEL = -1536.0           # exact in float16 / bfloat16 / float32; no result of these tests takes it
NAN = float("nan")
IDS = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}


def _inside(t, fill):
    """CPU tensor -> (device buffer filled with `fill`, view of t's shape GUARD elements inside it holding t)."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), fill, dtype=t.dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(t.shape)
    view.copy_(t)
    return buf, view


def _out(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_hold(buf, fill, what):
    for side in (buf[:GUARD], buf[-GUARD:]):
        ok = torch.isnan(side).all() if fill != fill else (side == fill).all()
        assert bool(ok), f"{what}: a store outside the operand"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ctx(nat):
    return nat.ctx_for(torch.cuda.current_device())


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- ds_bias_act_nhwc -------------------------------------------------------------------------------------------------------------------
def _bias_act(nat, x, bias, r1, r2, out, relu):
    rc = nat.lib().ds_bias_act_nhwc(_ctx(nat), x.data_ptr(), bias.data_ptr(), _ptr(r1), _ptr(r2), out.data_ptr(), x.numel(), x.shape[1],
                                    1 if relu else 0, pc.DT_CODE[x.dtype], _stream())
    assert rc == 0, nat.lib().ds_last_error()


def _bias_act_every_way(nat, ops, check):
    """All six (relu, residuals) combinations out of place and in place; check(got, relu, nres, how) judges each result."""
    dtype = ops["x"].dtype
    dev = {k: _inside(v, NAN) for k, v in ops.items()}
    xbuf, x = dev["x"]
    x_clean = x.clone()
    for relu, nres in pc.BIAS_ACT_COMBOS:
        _, bias, r1, r2 = pc.bias_act_args({k: v[1] for k, v in dev.items()}, nres)
        obuf, out = _out(tuple(x.shape), dtype)
        _bias_act(nat, x, bias, r1, r2, out, relu)
        torch.cuda.synchronize()
        check(out, relu, nres, "out of place")
        _guards_hold(obuf, SENTINEL, "out")
        assert torch.equal(x.view(torch.int16), x_clean.view(torch.int16)), "x changed by an out-of-place call"
        _bias_act(nat, x, bias, r1, r2, x, relu)
        torch.cuda.synchronize()
        check(x, relu, nres, "in place")
        _guards_hold(xbuf, NAN, "x (in place)")
        x.copy_(x_clean)
    for k in ("bias", "r1", "r2"):
        assert torch.equal(dev[k][1].view(torch.int16).cpu(), ops[k].view(torch.int16)), f"{k} changed"


@GPU
@pytest.mark.parametrize("dtype", pc.HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", pc.BIAS_ACT_SHAPES + [pc.BIAS_ACT_STRIDE_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_bias_act_is_the_float64_sum_rounded_once(gpu, dtype, shape):
    """(2, 1024, 41, 200) has 2,099,200 vectors of 8: the grid-stride loop makes a second trip and c8 wraps inside it."""
    from src import _native
    ops = pc.bias_act_operands(dtype, shape)
    wants = pc.bias_act_wants(ops)
    _bias_act_every_way(_native, ops, lambda got, relu, nres, how: pc.check_bias_act(
        got, wants[(relu, nres)], f"ds_bias_act_nhwc {IDS[dtype]} {shape} relu={relu} residuals={nres} {how}"))


@GPU
@pytest.mark.parametrize("dtype", pc.HALF, ids=["f16", "bf16"])
def test_bias_act_specials_like_torch(gpu, dtype):
    """NaN, +Inf, -Inf and -0.0 in x, in each residual and in the bias: the NaN mask of torch's relu(x + b + r1 + r2) on the CPU, and
    equal values everywhere else.  relu(NaN) is NaN."""
    from src import _native
    ops = pc.bias_act_special_operands(dtype)
    _bias_act_every_way(_native, ops, lambda got, relu, nres, how: pc.check_specials(
        got, pc.bias_act_special_want(ops, relu, nres), f"ds_bias_act_nhwc specials {IDS[dtype]} relu={relu} residuals={nres} {how}"))


@GPU
def test_bias_act_argument_checks(gpu):
    from src import _native
    L, ctx = _native.lib(), _ctx(_native)
    x = torch.zeros((35, 64), dtype=torch.float16, device="cuda")
    y, r, b = torch.empty_like(x), torch.zeros_like(x), torch.zeros(64, dtype=torch.float16, device="cuda")

    def call(xp=x.data_ptr(), bp=b.data_ptr(), r1=r.data_ptr(), r2=None, yp=y.data_ptr(), n=35 * 64, c=64, dt=1):
        return L.ds_bias_act_nhwc(ctx, xp, bp, r1, r2, yp, n, c, 1, dt, _stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert call(c=12) == -1 and call(c=0) == -1 and call(n=35 * 60, c=60) == -1                 # channels % 8
    assert call(n=35 * 64 - 8) == -1 and call(n=0) == -1                                          # elements % channels
    for name in ("xp", "bp", "r1", "yp"):                                                         # 16-byte alignment of every operand
        assert call(**{name: x.data_ptr() + 2}) == -1, name
    assert call(r2=r.data_ptr() + 8) == -1
    assert call(dt=0) == -1 and call(dt=3) == -1                                                  # f16 / bf16 only
    assert call(xp=None) == -1 and call(yp=None) == -1 and call(bp=None) == -1


def test_exact_cases_stay_in_the_exact_range():
    """No GPU.  The premise of the torch.equal tests, for every case: operands are multiples of q with |v| <= 16 (8 for the
    read-out), and every float32 sum the kernels form -- x + bias, + res1, + res2; proj + cls -- equals the float64 sum, so the
    single rounding to the storage type is the only one.  The integer convolutions stay below 2^24."""
    for dtype in pc.HALF:
        q = pc.Q[dtype]
        for shape in pc.BIAS_ACT_SHAPES + [pc.BIAS_ACT_STRIDE_SHAPE]:
            ops = pc.bias_act_operands(dtype, shape)
            for v in ops.values():
                assert float(v.float().abs().max()) <= 16.0 and torch.equal(torch.round(v.float() / q) * q, v.float())
            for s32, s64 in zip(pc.bias_act_sums(ops, torch.float32), pc.bias_act_sums(ops, torch.float64)):
                assert torch.equal(s32.double(), s64), (dtype, shape)
        ops = pc.bias_act_special_operands(dtype)
        for s32, s64 in zip(pc.bias_act_sums(ops, torch.float32), pc.bias_act_sums(ops, torch.float64)):
            assert torch.equal(torch.nan_to_num(s32.double(), 7.0), torch.nan_to_num(s64, 7.0)) and torch.equal(torch.isnan(s32), torch.isnan(s64))
        for shape in pc.READOUT_SHAPES + [pc.READOUT_STRIDE_SHAPE]:
            ops = pc.readout_operands(dtype, shape)
            assert bool(torch.isnan(ops["proj"][:, 0]).all()) and float(ops["proj"][:, 1:].float().abs().max()) <= 8.0
            assert float(ops["cls"].float().abs().max()) <= 8.0
            for v in (ops["proj"][:, 1:], ops["cls"]):
                assert torch.equal(torch.round(v.float() / q) * q, v.float())
            assert torch.equal(pc.readout_sum(ops, torch.float32).double(), pc.readout_sum(ops, torch.float64)), (dtype, shape)
    for shape in pc.GCONV_SHAPES:
        for cpg in pc.GCONV_CPGS:
            ops = pc.gconv_int_operands(shape, cpg)
            terms = pc.gconv_ref64(ops["x"].abs(), ops["w"].abs(), ops["bias"].abs(), cpg)
            assert float(terms.max()) <= 9 * cpg + 8 < 2 ** 24 and torch.equal(terms, terms.round())
            assert float(pc.impulse_weight(shape[1], cpg).max()) == 1 + (8 * cpg + cpg - 1) * cpg + cpg - 1 <= 9217


# ---- ds_reassemble_readout ----------------------------------------------------------------------------------------------------------------
def _readout(nat, proj, cls, out):
    b, n, c = proj.shape
    rc = nat.lib().ds_reassemble_readout(_ctx(nat), proj.data_ptr(), cls.data_ptr(), out.data_ptr(), b, n, c, pc.DT_CODE[proj.dtype], _stream())
    assert rc == 0, nat.lib().ds_last_error()


@GPU
@pytest.mark.parametrize("dtype", pc.HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", pc.READOUT_SHAPES + [pc.READOUT_STRIDE_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_readout_is_the_erf_gelu_of_the_rounded_sum(gpu, dtype, shape):
    """The cls row of proj is NaN and every image has its own cls vector (pointwise_cases.readout_operands); (2, 8200, 1024) has
    2,098,944 vectors of 8, one grid stride and a bit."""
    from src import _native
    ops = pc.readout_operands(dtype, shape)
    (_, proj), (_, cls) = _inside(ops["proj"], NAN), _inside(ops["cls"], NAN)
    b, n, c = shape
    (buf1, out1), (buf2, out2) = _out((b, n - 1, c), dtype), _out((b, n - 1, c), dtype)
    _readout(_native, proj, cls, out1)
    _readout(_native, proj, cls, out2)
    torch.cuda.synchronize()
    ratio, off, report = pc.check_readout(out1, ops, f"ds_reassemble_readout {IDS[dtype]} {shape}")
    print(report)
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16)), "two calls on the same operands differ"
    _guards_hold(buf1, SENTINEL, "out")
    _guards_hold(buf2, SENTINEL, "out (second call)")


@GPU
def test_readout_argument_checks(gpu):
    from src import _native
    L, ctx = _native.lib(), _ctx(_native)
    proj = torch.zeros((2, 5, 64), dtype=torch.float16, device="cuda")
    cls, out = torch.zeros((2, 64), dtype=torch.float16, device="cuda"), torch.empty((2, 4, 64), dtype=torch.float16, device="cuda")

    def call(pp=proj.data_ptr(), cp=cls.data_ptr(), op=out.data_ptr(), n=5, c=64, dt=1):
        return L.ds_reassemble_readout(ctx, pp, cp, op, 2, n, c, dt, _stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert call(n=1) == -1 and call(n=0) == -1                              # nothing but the cls row
    assert call(c=60) == -1 and call(c=4) == -1 and call(c=0) == -1         # channels % 8
    for name in ("pp", "cp", "op"):
        assert call(**{name: proj.data_ptr() + 2}) == -1, name
    assert call(dt=0) == -1 and call(dt=3) == -1


# ---- ds_preprocess_bicubic ----------------------------------------------------------------------------------------------------------------
def _floats(v):
    return (ctypes.c_float * 3)(*[float(f) for f in triple(v)])


def _image_inside(img, seed, invert):
    """uint8 image (numpy) GUARD bytes inside a buffer of random bytes (inverted: the same buffer with the surroundings flipped)."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randint(0, 256, (img.size + 2 * GUARD,), generator=g, dtype=torch.uint8)
    if invert:
        flat = 255 - flat
    flat[GUARD:GUARD + img.size] = torch.from_numpy(img).flatten()
    return flat.cuda()[GUARD:GUARD + img.size].view(img.shape)


def _preprocess(nat, img, out_hw, mean, std, flip, dtype):
    """-> (guard buffer, logical [B, 3, oh, ow] view of the NHWC output)."""
    b, ih, iw, _ = img.shape
    buf, out = _out((b, out_hw[0], out_hw[1], 3), dtype)
    rc = nat.lib().ds_preprocess_bicubic(_ctx(nat), img.data_ptr(), out.data_ptr(), b, ih, iw, out_hw[0], out_hw[1], 1 if flip else 0,
                                         _floats(mean), _floats(std), pc.DT_CODE[dtype], _stream())
    assert rc == 0, nat.lib().ds_last_error()
    torch.cuda.synchronize()
    return buf, out.permute(0, 3, 1, 2)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@GPU
@pytest.mark.parametrize("in_hw,out_hw", pc.PRE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_preprocess_within_the_float32_chain_of_the_float64_resize(gpu, in_hw, out_hw):
    """Batch 3, random bytes and a constant 255, scalar 0.5 / 0.5 and the ImageNet triples, flip on and off, float32 / float16 /
    bfloat16 outputs.  Inputs of 1 x 1, 2 x 3 and 1 x 9 clamp all or most taps; equal sizes give weights (0, 1, 0, 0) exactly."""
    from src import _native
    worst = {}
    for kind in ("random", "white"):
        img = pc.pre_image(kind, in_hw)
        dev, dev_inv = _image_inside(img, 9, False), _image_inside(img, 9, True)
        for mean, std in pc.PRE_NORMS:
            for flip in (True, False):
                ref, s = preprocess_ref(img, out_hw, mean, std, flip)
                for dtype in pc.PRE_DTYPES:
                    tag = f"ds_preprocess_bicubic {in_hw} -> {out_hw} {kind} flip={flip} mean={mean} {IDS[dtype]}"
                    buf, got = _preprocess(_native, dev, out_hw, mean, std, flip, dtype)
                    buf2, got2 = _preprocess(_native, dev_inv, out_hw, mean, std, flip, dtype)
                    worst[dtype] = max(worst.get(dtype, 0.0), pc.check_preprocess(got, ref, s, mean, std, tag))
                    assert torch.equal(_bits(got), _bits(got2)), f"{tag}: the bytes around the image change the output"
                    _guards_hold(buf, SENTINEL, tag)
                    _guards_hold(buf2, SENTINEL, tag)
                    if (in_hw, out_hw) == pc.PRE_IDENTITY and dtype == torch.float32:
                        want = pc.pre_identity_want(img, mean, std, flip)
                        assert torch.equal(got.cpu(), want), f"{tag}: {pc.first_mismatches(got, want)}"
    print(f"ds_preprocess_bicubic {in_hw} -> {out_hw}: worst error / bound " + ", ".join(f"{IDS[d]} {v:.4f}" for d, v in worst.items()))


@GPU
@pytest.mark.parametrize("dtype", pc.HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("in_hw,out_hw,p,n_pad", pc.PRE_ROWS_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_preprocess_rows_against_the_float64_resize(gpu, in_hw, out_hw, p, n_pad, dtype):
    """ds_preprocess_bicubic_rows against the float64 reference directly (test_gpu_forward_ends holds it bit-equal to
    ds_preprocess_bicubic): the patch rows hold the resized image within the same bar, every other element is zero."""
    from src import _native
    kpad = (3 * p * p + 127) // 128 * 128
    gh, gw = out_hw[0] // p, out_hw[1] // p
    assert n_pad >= 1 + gh * gw
    img = pc.pre_image("random", in_hw)
    dev = _image_inside(img, 10, False)
    worst = 0.0
    for (mean, std), flip in zip(pc.PRE_NORMS, (True, False)):
        ref, s = preprocess_ref(img, out_hw, mean, std, flip)
        buf, out = _out((pc.PRE_BATCH, n_pad, kpad), dtype)
        got = _native.preprocess_bicubic_rows(dev, out_hw, mean, std, p, n_pad, kpad, flip=flip, dtype=dtype, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        body, zero = pc.rows_ungather(got.cpu(), p, out_hw)
        tag = f"ds_preprocess_bicubic_rows {in_hw} -> {out_hw} flip={flip} {IDS[dtype]}"
        worst = max(worst, pc.check_preprocess(body, ref[:, :, :gh * p, :gw * p], s[:, :, :gh * p, :gw * p], mean, std, tag))
        assert not bool(got.cpu()[zero].any()), f"{tag}: a non-zero element outside the patch rows"
        _guards_hold(buf, SENTINEL, tag)
    print(f"ds_preprocess_bicubic_rows {in_hw} -> {out_hw} {IDS[dtype]}: worst error / bound {worst:.4f}")


# ---- ds_gconv3x3_nhwc_f32 -------------------------------------------------------------------------------------------------------------------
def _gconv(nat, x, wimg, bias, out, cpg, relu):
    b, h, w, c = x.shape
    rc = nat.lib().ds_gconv3x3_nhwc_f32(_ctx(nat), x.data_ptr(), wimg.data_ptr(), _ptr(bias), out.data_ptr(), b, h, w, c, cpg, 1 if relu else 0, _stream())
    assert rc == 0, nat.lib().ds_last_error()
    torch.cuda.synchronize()


@GPU
@pytest.mark.parametrize("cpg", pc.GCONV_CPGS)
@pytest.mark.parametrize("shape", pc.GCONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gconv3x3_exact_integers_impulses_and_rounding_bound(gpu, shape, cpg):
    from src import _native
    b, c, h, w = shape
    groups = c // cpg

    def run(x, weight, bias, relu):
        (_, xd), (_, wd) = _inside(x, NAN), _inside(pc.weight_image(weight, groups), NAN)
        bd = None if bias is None else _inside(bias, NAN)[1]
        obuf, out = _out((b, h, w, c), torch.float32)
        _gconv(_native, xd, wd, bd, out, cpg, relu)
        _guards_hold(obuf, SENTINEL, "y")
        return out

    ops = pc.gconv_int_operands(shape, cpg)
    for use_bias, relu in ((True, True), (False, False), (True, False)):
        got = run(ops["x"], ops["w"], ops["bias"] if use_bias else None, relu)
        pc.check_gconv_exact(got, ops, cpg, use_bias, relu, f"ds_gconv3x3_nhwc_f32 exact {shape} cpg={cpg} bias={use_bias} relu={relu}")
    codes = pc.impulse_weight(c, cpg)
    for site in pc.impulse_sites(shape):
        pc.check_gconv_impulse(run(pc.impulse_x(shape, site), codes, None, False), shape, cpg, site, f"ds_gconv3x3_nhwc_f32 {shape} cpg={cpg}")
    ops = pc.gconv_real_operands(shape, cpg)
    worst = 0.0
    for use_bias, relu in ((True, True), (False, False)):
        got = run(ops["x"], ops["w"], ops["bias"] if use_bias else None, relu)
        worst = max(worst, pc.check_gconv_bound(got, ops, cpg, use_bias, relu, f"ds_gconv3x3_nhwc_f32 bound {shape} cpg={cpg} bias={use_bias} relu={relu}"))
    print(f"ds_gconv3x3_nhwc_f32 {shape} cpg={cpg}: worst error / bound {worst:.4f}")


@GPU
def test_gconv3x3_argument_checks(gpu):
    from src import _native
    L, ctx = _native.lib(), _ctx(_native)
    x = torch.zeros((1, 4, 4, 64), device="cuda")
    y, wt, bias = torch.empty_like(x), torch.zeros((64 * 9 * 64,), device="cuda"), torch.zeros(64, device="cuda")

    def call(xp=x.data_ptr(), wp=wt.data_ptr(), yp=y.data_ptr(), c=64, cpg=8):
        return L.ds_gconv3x3_nhwc_f32(ctx, xp, wp, bias.data_ptr(), yp, 1, 4, 4, c, cpg, 1, _stream())
    assert call() == 0 and call(cpg=16) == 0 and call(cpg=32) == 0
    torch.cuda.synchronize()
    assert call(cpg=4) == -2 and call(cpg=64) == -2 and call(cpg=0) == -2            # DS_EUNSUPPORTED: 8, 16 or 32 channels per group
    assert call(c=48) == -2 and call(c=16) == -2                                     # channels % 32
    assert call(c=0) == -1
    assert call(yp=x.data_ptr()) == -1                                               # y aliases x
    for name in ("xp", "wp", "yp"):
        assert call(**{name: x.data_ptr() + 4}) == -1, name                          # 16-byte alignment
    assert call(xp=None) == -1 and call(yp=None) == -1 and call(wp=None) == -1
