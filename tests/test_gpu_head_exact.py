"""The fused DPT head tail (ds_dpt_head_tail, ds_dpt_head_tail_circular) and the bilinear upsample (ds_upsample_bilinear_nhwc) of
csrc/ds_encoder_ops.hip against references that leave no tolerance to hide in -- the scheme of tests/test_gpu_gemm_exact.py.

Part A -- exact.  All three head-tail kernels compute the upsampled activation in float32, round it ONCE to the operand type into
LDS, accumulate the 3x3 convolution in fp32 on the matrix cores and do bias, ReLU, the 32 -> 1 dot product, bias and ReLU in fp32; the
output is rounded once.  The source coordinate is fy = sy * oy with sy = (float)(ih - 1) / (float)(oh - 1) (0 when oh == 1).  With
oh - 1 = 2^j (ih - 1), 2^-j or identity every bilinear weight is a dyadic fraction; with inputs from {-1, 0, +1} the upsampled values
are multiples of 1/4 or 1/16 in [-1, 1], exact in float16 AND bfloat16; with ternary 3x3 weights and small-integer biases every
product and every partial sum in any order is exact in fp32.  So every kernel, mode, variant, segment length and MFMA order must
reproduce a float64 reference BIT FOR BIT (the stream kernel's FMA chain and the tile kernel's multiply and add included).
test_exact_cases_stay_in_the_exact_range (no GPU) proves the premise for every case;
test_the_exact_comparison_rejects_a_corrupted_reference (no GPU) shows that a dropped MFMA term, two swapped channels and one wrong
bilinear weight at a producer seam do not pass.

Part B -- real-valued operands, per output element |got - ref64| <= bound, the bound derived from the kernels' arithmetic:
    upsampled activation  e_u = 1/2 ulp_T(|u|) + 2 (4 + 4) 2^-24 sum |w v|
    conv3 channel         e_3 = sum |W| e_u + 2 (1152 + 4) 2^-24 (sum |W| |u| + |b|)
    output                1/2 ulp_T(|out|) + sum |w3| e_3 + 2 (32 + 4) 2^-24 (sum |w3| relu(conv3) + |b3|)        (ReLU is 1-Lipschitz)
The reference computes the source coordinates and the four weights in float32 exactly as include/depthstereo.h defines them
(util.bilinear_taps; torch does the same) and everything after that in float64, the upsampled map NOT rounded.  The term
sum |W| e_u charges every one of the 1152 roundings of an activation at its worst sign, so the bound is slack by construction -- so
slack that one missing MFMA term (bfloat16) or a bilinear weight off by 2^-6 passes it.  The kernels are therefore held to a
second, sharper bound as well (head_sharp_bound): against the float64 chain on the map ROUNDED to the type, where every activation
whose rounding the float32 error cannot change (over 99 % of them) is charged nothing.
test_the_rounding_bound_rejects_a_corrupted_reference (no GPU) shows what each of the two rejects.

Dispatch of ds_dpt_head_tail (ht_head_tail): DS_HEAD_MODE=stream (the default) runs k_dpt_head_tail_s<BF16, DS_HEAD_VARIANT> on work
items (image, 32-column strip, segment of DS_HEAD_SEG rows) unless 3 sy >= 1.99 or 8 sx >= 4.99, which takes k_dpt_head_tail_p like
DS_HEAD_MODE=persist (8 x 32 tiles); DS_HEAD_MODE=tile runs k_dpt_head_tail<BF16, RPW, 0> (4 RPW x 32 tiles, RPW from DS_HEAD_RPW,
read once per process); padding_mode='circular' is always k_dpt_head_tail<BF16, RPW, 1>.  The head tail has no kernel-timer kind,
so which kernel ran rests on this arithmetic, quoted per case."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import conftest  # noqa: F401
from test_gpu_gemm_exact import DT, EXACT_MAX, _dev, _gen, _randn
from util import (bilinear_ref, bilinear_taps, first_mismatches, rounding_bound_ratio, small_ints, ternary, ulp_distance,
                  ulp_spacing)

GPU = pytest.mark.gpu
HEAD_ENV = ("DS_HEAD_MODE", "DS_HEAD_VARIANT", "DS_HEAD_SEG", "DS_HEAD_PERSIST")
CONFIGS = {   # what a configuration sets (everything else of HEAD_ENV is unset), and whether the 3x3 convolution pads circularly
    "stream0": (dict(DS_HEAD_MODE="stream", DS_HEAD_VARIANT="0"), False),
    "stream1": (dict(DS_HEAD_MODE="stream", DS_HEAD_VARIANT="1"), False),
    "persist": (dict(DS_HEAD_MODE="persist"), False),
    "tile": (dict(DS_HEAD_MODE="tile"), False),
    "default": ({}, False),
    "circular": ({}, True),
}


@pytest.fixture
def head_env(gpu, monkeypatch):
    """src._native and a function that selects one of CONFIGS (plus DS_HEAD_SEG); the switches are read per call."""
    from src import _native

    def select(config, seg=None):
        for k in HEAD_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in CONFIGS[config][0].items():
            monkeypatch.setenv(k, v)
        if seg is not None:
            monkeypatch.setenv("DS_HEAD_SEG", str(seg))
        return CONFIGS[config][1]
    return _native, select


# ---- float64 references ---------------------------------------------------------------------------------------------------------------
def conv3_ref(u, w, circular, drop=None):
    """3 x 3, stride 1, padding 1 (zeros, or circular on the UPSAMPLED map): u [B, H, W, 128], w [32, 3, 3, 128] (float64) ->
    [B, H, W, 32], one product per tap.  drop = (channel, tap, slice): that channel loses the 16 input channels of one tap."""
    b, h, wd, c = u.shape
    if circular:
        up = torch.cat([u[:, -1:], u, u[:, :1]], 1)
        up = torch.cat([up[:, :, -1:], up, up[:, :, :1]], 2)
    else:
        up = torch.zeros((b, h + 2, wd + 2, c), dtype=u.dtype)
        up[:, 1:-1, 1:-1] = u
    acc = torch.zeros((b * h * wd, w.shape[0]), dtype=u.dtype)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        v = up[:, ky:ky + h, kx:kx + wd].reshape(-1, c)
        acc += v @ w[:, ky, kx].T
        if drop is not None and drop[1] == tap:
            k = slice(16 * drop[2], 16 * drop[2] + 16)
            acc[:, drop[0]] -= v[:, k] @ w[drop[0], ky, kx, k]
    return acc.view(b, h, wd, -1)


class HeadWant:
    """What the head tail must produce on operands o: u the upsampled map (unrounded) with s_u = sum |weight * value|, pre3 the
    3x3 convolution + bias in front of the inner ReLU, pre1 the value in front of the outer ReLU."""

    def __init__(self, u, s_u, pre3, pre1):
        self.u, self.s_u, self.pre3, self.pre1 = u, s_u, pre3, pre1

    def value(self, relu_out):
        return self.pre1.clamp(min=0) if relu_out else self.pre1


def head_ref(o, size, circular=False, corrupt=None, round_to=None):
    """upsample (align_corners) -> conv3x3 + bias -> ReLU -> conv1x1 + bias.  corrupt (the tests on corrupted references below):
    ("drop", channel, tap, slice), ("swap", channel, channel) before the 1x1 convolution, or ("tx", column, delta).  round_to: the
    upsampled map is rounded to that type in front of the convolution, as the kernels round it into LDS."""
    kind = corrupt[0] if corrupt else None
    taps_x = None
    if kind == "tx":
        x0, x1, tx = bilinear_taps(o["x"].shape[2], size[1])
        tx = tx.copy()
        tx[corrupt[1]] += np.float32(corrupt[2])
        taps_x = (x0, x1, tx)
    u, s_u = bilinear_ref(o["x"], size, True, taps_x)
    if round_to is not None:
        u = u.to(DT[round_to]).double()
    pre3 = conv3_ref(u, o["w"], circular, corrupt[1:] if kind == "drop" else None) + o["b"]
    if kind == "swap":
        idx = list(range(32))
        idx[corrupt[1]], idx[corrupt[2]] = corrupt[2], corrupt[1]
        pre3 = pre3[..., idx]
    return HeadWant(u, s_u, pre3, pre3.clamp(min=0) @ o["w1"] + o["b1"])


def head_bound(o, want, dt, circular, relu_out):
    """The per-output bound of Part B (module docstring) for a reference `want` of operands o."""
    wabs, w1abs = o["w"].abs(), o["w1"].abs()
    e_u = 0.5 * ulp_spacing(want.u, DT[dt]) + 2.0 * (4 + 4) * 2.0 ** -24 * want.s_u
    e_3 = conv3_ref(e_u, wabs, circular) + 2.0 * (1152 + 4) * 2.0 ** -24 * (conv3_ref(want.u.abs(), wabs, circular) + o["b"].abs())
    return (0.5 * ulp_spacing(want.value(relu_out), DT[dt]) + e_3 @ w1abs
            + 2.0 * (32 + 4) * 2.0 ** -24 * (want.pre3.clamp(min=0) @ w1abs + abs(o["b1"])))


def head_sharp_bound(o, want, sharp, dt, circular, relu_out):
    """The second bound of Part B, against `sharp` = head_ref(..., round_to=dt).  The kernel's float32 activation lies within
    d = 2 (4 + 4) 2^-24 sum |w v| of the float64 one (want.u), and rounding is monotone: where u - d and u + d round to the same
    number of the type as u does, the kernel holds exactly that number and the activation carries NO error; elsewhere (u within d
    of a rounding boundary, well under 1 % of the activations) it is off by at most the distance to the farther of the two
    roundings.  The rest is the issue's chain: fp32 accumulation of 1152 exact products, bias, ReLU, 32 terms, one rounding."""
    wabs, w1abs, T = o["w"].abs(), o["w1"].abs(), DT[dt]
    d = 2.0 * (4 + 4) * 2.0 ** -24 * want.s_u
    e_u = torch.maximum((want.u + d).to(T).double() - sharp.u, sharp.u - (want.u - d).to(T).double())
    assert float(e_u.min()) >= 0.0
    e_3 = conv3_ref(e_u, wabs, circular) + 2.0 * (1152 + 4) * 2.0 ** -24 * (conv3_ref(sharp.u.abs(), wabs, circular) + o["b"].abs())
    return (0.5 * ulp_spacing(sharp.value(relu_out), T) + e_3 @ w1abs
            + 2.0 * (32 + 4) * 2.0 ** -24 * (sharp.pre3.clamp(min=0) @ w1abs + abs(o["b1"])))


def _exact_equal(got64, want64, dt):
    """The comparison of Part A on two float64 tensors: equal bit for bit once rounded to the type."""
    return torch.equal(got64.to(DT[dt]), want64.to(DT[dt]))


def _bound_ratio(got, ref64, bound):
    return float(((got.detach().cpu().double() - ref64).abs() / bound).max())


# ---- Part A: the cases ---------------------------------------------------------------------------------------------------------------
# name: (b, ih, iw, oh, ow, grain of the upsampled values).  A strip / tile is 32 columns wide; sy = (ih - 1) / (oh - 1)
HEAD = {
    "seam": (2, 9, 17, 17, 33, 0.25),          # x2 - 1: second strip ONE column wide; oh = 17 is no multiple of 4 (nor of 8: persist)
    # 3 strips x 9 (SEG=4) or 3 (SEG=12) segments x 24 images = 648 / 216 stream items, several per workgroup on 256 CUs.  SEG=4:
    # nsteps = 1, a segment made of its lead-in and the "last step's row" code alone.  SEG=12: nsteps = 3, odd: the parity of the
    # partner-exchange buffer flips from item to item.  persist: 3 x 5 x 24 = 360 tiles of 8 x 32, more than one per workgroup
    "items": (24, 17, 33, 33, 65, 0.25),
    "tiny_3x3": (3, 2, 2, 3, 3, 0.25),         # oh < 4: one step whose rows 3 .. are outside; a 2 x 2 source
    "tiny_row": (1, 1, 5, 1, 9, 0.25),         # oh = 1: sy = 0; a single source row (y1 clamps onto y0 everywhere)
    "x4": (1, 5, 9, 17, 33, 0.0625),           # weights in quarters; the 4 x 7 staging tile covers 3 columns (its narrow end)
    # sy = sx = 1: 3 sy = 3 >= 1.99, so the default mode must take the persist kernel; every weight is 0 or 1
    "identity": (2, 19, 37, 19, 37, 1.0),
    "half": (1, 37, 69, 19, 35, 1.0),          # sy = sx = 2: 3 sy = 6 >= 1.99, the persist fallback; ty = tx = 0 on every second source pixel
    "column": (1, 5, 1, 9, 1, 0.25),           # circular only: ow = 1 (sx = 0), the columns left and right are the column itself
}
# (case, configuration, DS_HEAD_SEG)
RUNS = ([("seam", c, None) for c in ("stream0", "stream1", "persist", "tile", "circular")]
        + [("items", c, s) for c in ("stream0", "stream1") for s in (4, 12)] + [("items", "persist", None)]
        + [(n, c, None) for n in ("tiny_3x3", "tiny_row", "x4") for c in ("stream0", "stream1", "tile")]
        + [("identity", "default", None), ("identity", "tile", None), ("half", "default", None), ("column", "circular", None)])
# (case, type): salt of the generator where the first draw misses a condition of the premise test: the share that the outer ReLU
# keeps is a coarse number on 9 or 27 outputs, and one draw of 32 biases and 16 signs shifts it for a whole case
SEEDS = {("items", "f16"): 2, ("tiny_3x3", "f16"): 1, ("tiny_3x3", "bf16"): 1, ("tiny_row", "bf16"): 1, ("column", "f16"): 1}


@functools.lru_cache(maxsize=None)
def head_case(name, dt):
    """Operands of one Part A case as float64.  x and the 3x3 weights ternary with the density of test_gpu_gemm_exact._density for
    K = 1152, scaled by the grain: bfloat16 holds multiples of 1/4 only below 64 (of 1/16 below 16), the binding constraint for the
    conv3 pre-activations; for the output it is met by thinning conv1.weight (4 taps instead of 16), not by shrinking the shapes."""
    b, ih, iw, oh, ow, grain = HEAD[name]
    g = _gen("head", name, dt, SEEDS.get((name, dt), 0))
    limit = EXACT_MAX[dt] * grain
    d = min(0.5, limit / 6.0 / 1152 ** 0.5)
    n1 = 16 if dt == "f16" else 4
    w1 = torch.zeros(32, dtype=torch.float64)
    where = torch.randperm(32, generator=g)[:n1]
    w1[where] = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(n1 // 2)
    return {"x": ternary(g, (b, ih, iw, 128), d), "w": ternary(g, (32, 3, 3, 128), d),
            "b": small_ints(g, (32,), int(min(16, max(1, limit // 16)))), "w1": w1, "b1": 1.0}


@functools.lru_cache(maxsize=None)
def head_want(name, dt, circular):
    b, ih, iw, oh, ow, grain = HEAD[name]
    return head_ref(head_case(name, dt), (oh, ow), circular)


def _modules(o, circular):
    """Fresh modules per launch: the fragment cache of _native.dpt_head_tail lives on conv3, keyed on data_ptr and _version.
    skip_init: no initial values are drawn, so the global generator stays where the rest of the suite left it."""
    conv3 = nn.utils.skip_init(nn.Conv2d, 128, 32, 3, padding=1, padding_mode="circular" if circular else "zeros", device="cuda")
    conv1 = nn.utils.skip_init(nn.Conv2d, 32, 1, 1, device="cuda")
    with torch.no_grad():
        conv3.weight.copy_(o["w"].permute(0, 3, 1, 2))
        conv3.bias.copy_(o["b"])
        conv1.weight.copy_(o["w1"].view(1, 32, 1, 1))
        conv1.bias.fill_(o["b1"])
    return conv3, conv1


def _run_head(nat, o, size, dt, circular, relu_out):
    conv3, conv1 = _modules(o, circular)
    name = "ds_dpt_head_tail_circular" if circular else "ds_dpt_head_tail"
    before = nat.CALLS[name]
    got = nat.dpt_head_tail(_dev(o["x"], dt).permute(0, 3, 1, 2), size, conv3, conv1, relu_out=relu_out)
    assert nat.CALLS[name] == before + 1
    assert tuple(got.shape) == (o["x"].shape[0], 1) + tuple(size) and got.dtype == DT[dt]
    return got[:, 0]


def _check_exact(got, want64, dt, what):
    ref = want64.to(DT[dt])
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    assert torch.equal(got.cpu(), ref), (what, first_mismatches(got, ref))


# ---- A1 ---------------------------------------------------------------------------------------------------------------------------------
@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name,config,seg", RUNS, ids=[f"{n}-{c}" + (f"-seg{s}" if s else "") for n, c, s in RUNS])
def test_head_tail_is_exact_on_integers(head_env, name, config, seg, dt):
    """Every head-tail kernel on ternary operands, with and without the outer ReLU: bit for bit the float64 reference."""
    nat, select = head_env
    circular = select(config, seg)
    b, ih, iw, oh, ow, grain = HEAD[name]
    if config == "default":
        sy, sx = np.float32(ih - 1) / np.float32(oh - 1), np.float32(iw - 1) / np.float32(ow - 1)
        assert not (np.float32(3) * sy < np.float32(1.99) and np.float32(8) * sx < np.float32(4.99))          # ht_head_tail's guard: persist
    o, want = head_case(name, dt), head_want(name, dt, circular)
    for relu_out in (True, False):
        got = _run_head(nat, o, (oh, ow), dt, circular, relu_out)
        _check_exact(got, want.value(relu_out), dt, f"head {name} {config} seg {seg} {dt} relu_out {relu_out}")


# ---- A2: the channel map ---------------------------------------------------------------------------------------------------------------
CHANNEL_RUNS = [(c, "f16") for c in ("stream0", "stream1", "persist", "tile", "circular")] + [("stream0", "bf16"), ("stream1", "bf16")]


@GPU
@pytest.mark.parametrize("config,dt", CHANNEL_RUNS)
def test_head_tail_channel_map(head_env, config, dt):
    """conv1.weight one-hot on channel c, no bias, no outer ReLU: the output is relu(conv3[c] + b[c]) of the `seam` case, for every c
    -- ch = (r & 3) + 8 (r >> 2) + 4 hi of the accumulator registers, and the fragment packing of _native.dpt_head_tail."""
    nat, select = head_env
    circular = select(config)
    b, ih, iw, oh, ow, grain = HEAD["seam"]
    o, want = dict(head_case("seam", dt)), head_want("seam", dt, circular)
    o["b1"] = 0.0
    for c in range(32):
        o["w1"] = torch.zeros(32, dtype=torch.float64)
        o["w1"][c] = 1.0
        got = _run_head(nat, o, (oh, ow), dt, circular, False)
        _check_exact(got, want.pre3[..., c].clamp(min=0), dt, f"channel {c} {config} {dt}")


# ---- A3: impulses ----------------------------------------------------------------------------------------------------------------------
IMPULSES = ((0, 0, 0), (0, 8, 16), (1, 4, 16), (1, 4, 8))          # (image, source row, source column) on the `seam` shape, see impulse_case
IMPULSE_SEG = 8                                                    # stream: segments [0, 8), [8, 16), [16, 17)
IMPULSE_LIT = {False: 9 + 9 + 15 + 25, True: 28 + 20 + 25}


def impulse_channel(s):
    """Input channel of k-slice s: the slice's upper 8-channel half for odd s (hi = 1), s < 4 in consumer half kh = 0, s >= 4 in kh = 1."""
    return 16 * s + 8 * (s & 1) + (3 * s) % 8


@functools.lru_cache(maxsize=None)
def impulse_case(s, dt, circular):
    """One input channel of k-slice s holds a single 1 at four pixels of the `seam` shape (x2 - 1: source (y, x) is output (2y, 2x),
    its bilinear footprint the 3 x 3 block 1/4 1/2 1/4; 1/2 1 1/2; 1/4 1/2 1/4 around it):
        image 0 (0, 0)     the corner: footprint 2 x 2, 3 x 3 outputs (zero padding)
        image 0 (8, 16)    the opposite corner, in the one-column strip and the one-row last segment: 3 x 3 outputs
        image 1 (4, 16)    output (8, 32): first row of the second segment (DS_HEAD_SEG=8), the strip seam column: 5 x 3 outputs
        image 1 (4, 8)     output (8, 8): the segment seam row at the first producer seam (columns 0 .. 8 | 9 ..): 5 x 5 outputs
    (circular padding: the corners' outputs wrap, 16 each with 4 shared, and the strip-seam impulse gains column 0: IMPULSE_LIT).
    3x3 weights of that input channel: 1 + tap + 9 (co % m), tap = 3 ky + kx, m = 8 (float16) or 2 (bfloat16: sums of quarters must
    stay below 64); conv1.weight one-hot on channel (5 s + 3) % 32, no biases: every output is the footprint x taps pattern of ONE
    named channel, zero elsewhere."""
    b, ih, iw, oh, ow, grain = HEAD["seam"]
    ci, co = impulse_channel(s), (5 * s + 3) % 32
    x, w = torch.zeros((b, ih, iw, 128), dtype=torch.float64), torch.zeros((32, 3, 3, 128), dtype=torch.float64)
    for img, yy, xx in IMPULSES:
        x[img, yy, xx, ci] = 1.0
    w[:, :, :, ci] = (1.0 + torch.arange(9.0).view(1, 3, 3) + 9.0 * (torch.arange(32) % (8 if dt == "f16" else 2)).view(32, 1, 1)).double()
    w1 = torch.zeros(32, dtype=torch.float64)
    w1[co] = 1.0
    o = {"x": x, "w": w, "b": torch.zeros(32, dtype=torch.float64), "w1": w1, "b1": 0.0}
    return o, head_ref(o, (oh, ow), circular)


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("config", ["stream0", "stream1", "persist", "tile", "circular"])
def test_head_tail_impulses_name_their_taps(head_env, config, dt):
    nat, select = head_env
    circular = select(config, IMPULSE_SEG)
    b, ih, iw, oh, ow, grain = HEAD["seam"]
    for s in range(8):
        o, want = impulse_case(s, dt, circular)
        got = _run_head(nat, o, (oh, ow), dt, circular, False)
        ref = want.pre1.to(DT[dt])
        if not torch.equal(got.cpu(), ref):
            maps = "\n".join(f"image {i}: got\n{got[i].cpu().float()}\nwant\n{ref[i].float()}" for i in range(b))
            pytest.fail(f"impulse map, k-slice {s} (input channel {impulse_channel(s)}) {config} {dt}:\n{maps}\n{first_mismatches(got, ref)}")


# ---- A4: the stand-alone upsample on ternary inputs ------------------------------------------------------------------------------------
# name: (b, c, ih, iw, oh, ow, align_corners).  A workgroup renders output rows 2 y and 2 y + 1 and keeps the source rows of the first
# for the second (py0 / py1); a row of ow * c / 8 lanes is cut into blocks of 256
UPSAMPLE = {
    "x2": (2, 64, 5, 7, 9, 13, True),                # oh odd: the last workgroup has one row; row pairs (2k, 2k + 1) share their top source row
    "x4": (1, 8, 3, 4, 9, 13, True),                 # both rows of a pair between the same two source rows; 13 lanes of a block of 256
    "identity": (3, 8, 9, 13, 9, 13, True),          # ty = 0: "the previous bottom row is this top row" on every second row
    "half": (1, 16, 17, 9, 9, 5, True),              # downsampling: no source row is shared, both rows load four pieces
    "one_row": (1, 8, 1, 6, 1, 11, True),            # oh = 1: sy = 0, y1 == y0 at the clamp, r = 1 breaks off
    "even_rows": (1, 24, 4, 5, 4, 9, True),          # oh even, identity in y, x2 - 1 in x; 24 channels
    "c136": (1, 136, 3, 16, 5, 31, True),            # ow * C8 = 31 * 17 = 527 lanes: three blocks, the last one ragged
    "x2_half_pixel": (2, 32, 10, 6, 20, 12, False),  # weights 1/4 and 3/4, fy clamped to 0 in the first row; oh even
    "half_half_pixel": (1, 8, 12, 10, 6, 5, False),  # weights 1/2: every output the mean of four sources
}
SENTINEL = -23.0          # exact in both types, outside [-1, 1]


@functools.lru_cache(maxsize=None)
def upsample_case(name):
    b, c, ih, iw, oh, ow, ac = UPSAMPLE[name]
    x = ternary(_gen("upsample", name), (b, ih, iw, c), 0.7)
    return x, bilinear_ref(x, (oh, ow), ac)[0]


def _raw_upsample(nat, x, out, oh, ow, ac):
    """ds_upsample_bilinear_nhwc into caller-owned memory: x [B, ih, iw, C] contiguous, out a flat slice of a larger buffer."""
    b, ih, iw, c = x.shape
    rc = nat.lib().ds_upsample_bilinear_nhwc(nat.ctx_for(torch.cuda.current_device()), x.data_ptr(), out.data_ptr(), b, c, ih, iw, oh, ow,
                                             1 if ac else 0, 1 if x.dtype == torch.float16 else 2, nat._stream(x))
    assert rc == 0, nat.lib().ds_last_error()


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(UPSAMPLE))
def test_upsample_is_exact_on_ternary_inputs(gpu, name, dt):
    """Bit for bit the float64 interpolation, through _native.upsample_bilinear and through the raw entry point writing into the
    middle of a buffer prefilled with a sentinel: not one byte in front of or behind the output changes."""
    from src import _native as nat
    b, c, ih, iw, oh, ow, ac = UPSAMPLE[name]
    x64, want = upsample_case(name)
    x = _dev(x64, dt)
    got = nat.upsample_bilinear(x.permute(0, 3, 1, 2), size=(oh, ow), align_corners=ac)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _check_exact(got.permute(0, 2, 3, 1), want, dt, f"upsample {name} {dt}")
    n, guard = want.numel(), 4096                                     # elements; 8 KiB on either side keeps the output 16-byte aligned
    buf = torch.full((n + 2 * guard,), SENTINEL, dtype=DT[dt], device="cuda")
    _raw_upsample(nat, x.contiguous(), buf[guard:guard + n], oh, ow, ac)
    torch.cuda.synchronize()
    _check_exact(buf[guard:guard + n].view(b, oh, ow, c), want, dt, f"upsample {name} {dt} (raw)")
    bits, clean = buf.view(torch.int16).cpu(), torch.full((1,), SENTINEL, dtype=DT[dt]).view(torch.int16)
    assert bool((bits[:guard] == clean).all()) and bool((bits[guard + n:] == clean).all()), f"upsample {name} {dt}: guard bands written"


# ---- A5: the premise of Part A, checked without a GPU ---------------------------------------------------------------------------------
def _round_trips(t, dt):
    return torch.equal(t.to(DT[dt]).double(), t)


def test_exact_cases_stay_in_the_exact_range():
    """For every Part A case and type: every upsampled activation, every conv3 pre-activation and every output survives a round
    trip through the type; every partial sum of absolute values stays below 2^24 (bounded by 1152 max |u| max |W| + max |b| and by
    sum |w3| max relu + |b3|); more than 90 % of the conv3 and of the final pre-activations are nonzero; both ReLUs keep between
    25 % and 75 %; the impulse cases light the expected number of outputs."""
    for dt in DT:
        for name, circular in sorted({(n, CONFIGS[c][1]) for n, c, _ in RUNS}):
            what, o, w = (name, circular, dt), head_case(name, dt), head_want(name, dt, circular)
            assert _round_trips(o["x"], dt) and _round_trips(o["w"], dt), what
            for t in (w.u, w.pre3, w.pre1):
                assert _round_trips(t, dt), (what, float(t.abs().max()))
            assert 1152 * float(w.u.abs().max()) * float(o["w"].abs().max()) + float(o["b"].abs().max()) < 2.0 ** 24, what
            assert float(o["w1"].abs().sum()) * float(w.pre3.abs().max()) + abs(o["b1"]) < 2.0 ** 24, what
            for t in (w.pre3, w.pre1):
                nonzero, kept = float((t != 0).double().mean()), float((t > 0).double().mean())
                assert nonzero > 0.9, (what, nonzero)
                assert 0.25 < kept < 0.75, (what, kept)
        for s in range(8):
            for circular in (False, True):
                o, w = impulse_case(s, dt, circular)
                assert _round_trips(w.u, dt) and _round_trips(w.pre3, dt) and _round_trips(w.pre1, dt), (s, dt, circular)
                assert float(o["w"].max()) <= EXACT_MAX[dt] and _round_trips(o["w"], dt)
                assert int((w.pre1 != 0).sum()) == IMPULSE_LIT[circular], (s, dt, circular, int((w.pre1 != 0).sum()))
    assert sorted(impulse_channel(s) // 16 for s in range(8)) == list(range(8))
    assert {impulse_channel(s) // 8 % 2 for s in range(8)} == {0, 1} and {impulse_channel(s) // 64 for s in range(8)} == {0, 1}
    for name in UPSAMPLE:
        x, want = upsample_case(name)
        for dt in DT:
            assert _round_trips(want, dt), (name, dt)
        assert float((want != 0).double().mean()) > 0.5, name


# ---- Part B: per-element rounding bound on real-valued operands ------------------------------------------------------------------------
ROUNDING = {   # name: (b, ih, iw, oh, ow), non-dyadic ratios
    "x2": (1, 37, 37, 74, 74),                 # sy = 36 / 73
    "ragged": (2, 20, 31, 33, 70),             # sy = 19 / 32, sx = 30 / 69: three strips, the last one 6 columns wide
    "fallback": (1, 100, 100, 150, 161),       # 3 sy = 3 * 99 / 149 = 1.9933 >= 1.99: the default mode takes the persist kernel
}
ROUNDING_RUNS = ([(n, c) for n in ("x2", "ragged") for c in ("stream0", "stream1", "persist", "tile")]
                 + [("fallback", "default"), ("ragged", "circular")])


@functools.lru_cache(maxsize=None)
def rounding_case(name, dt):
    """randn operands rounded to the type first; 3x3 weights scaled by 1152^-1/2, 1x1 weights by 32^-1/2."""
    b, ih, iw, oh, ow = ROUNDING[name]
    g = _gen("head rounding", name, dt)
    return {"x": _randn(g, (b, ih, iw, 128), dt), "w": _randn(g, (32, 3, 3, 128), dt, 1152 ** -0.5), "b": _randn(g, (32,), dt),
            "w1": _randn(g, (32,), dt, 32 ** -0.5), "b1": float(_randn(g, (1,), dt))}


@functools.lru_cache(maxsize=None)
def rounding_want(name, dt, circular):
    b, ih, iw, oh, ow = ROUNDING[name]
    o = rounding_case(name, dt)
    want, sharp = head_ref(o, (oh, ow), circular), head_ref(o, (oh, ow), circular, round_to=dt)
    return (want, {r: head_bound(o, want, dt, circular, r) for r in (True, False)},
            sharp, {r: head_sharp_bound(o, want, sharp, dt, circular, r) for r in (True, False)})


def _rounding_ratios(got, name, dt, circular, relu_out):
    """Worst error / bound of one output against the two checks of Part B: (unrounded map, sum |W| e_u), (rounded map, sharp bound)."""
    want, bounds, sharp, sharp_bounds = rounding_want(name, dt, circular)
    return (_bound_ratio(got, want.value(relu_out), bounds[relu_out]), _bound_ratio(got, sharp.value(relu_out), sharp_bounds[relu_out]))


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name,config", ROUNDING_RUNS, ids=[f"{n}-{c}" for n, c in ROUNDING_RUNS])
def test_head_tail_rounding_bound(head_env, name, config, dt):
    nat, select = head_env
    circular = select(config)
    b, ih, iw, oh, ow = ROUNDING[name]
    o = rounding_case(name, dt)
    want, sharp = rounding_want(name, dt, circular)[0], rounding_want(name, dt, circular)[2]
    for relu_out in (True, False):
        got = _run_head(nat, o, (oh, ow), dt, circular, relu_out)
        ref = want.value(relu_out)
        ratio, ratio_sharp = _rounding_ratios(got, name, dt, circular, relu_out)
        beyond, beyond_sharp = int((ulp_distance(got, ref) > 1).sum()), int((ulp_distance(got, sharp.value(relu_out)) > 1).sum())
        print(f"rounding head {name} {config} {dt} relu_out {relu_out}: worst error / bound {ratio:.3f}, {beyond} of {ref.numel()} "
              f"outputs more than one ulp from the float64 value; rounded map: {ratio_sharp:.3f}, {beyond_sharp}")
        assert ratio <= 1.0, (name, config, dt, relu_out, ratio)
        assert ratio_sharp <= 1.0, (name, config, dt, relu_out, ratio_sharp)


UPSAMPLE_B = {"ac": (2, 32, 10, 10, 37, 23, True), "half_pixel": (2, 32, 10, 10, 37, 23, False), "dav2": (1, 128, 37, 66, 74, 132, True)}


@GPU
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(UPSAMPLE_B))
def test_upsample_rounding_bound(gpu, name, dt):
    """|got - ref64| <= 1/2 ulp_T + 2 (4 + 4) 2^-24 sum |w v|: util.rounding_bound_ratio with K = 4."""
    from src import _native as nat
    b, c, ih, iw, oh, ow, ac = UPSAMPLE_B[name]
    x = _randn(_gen("upsample rounding", name, dt), (b, ih, iw, c), dt)
    ref, terms = bilinear_ref(x, (oh, ow), ac)
    got = nat.upsample_bilinear(_dev(x, dt).permute(0, 3, 1, 2), size=(oh, ow), align_corners=ac).permute(0, 2, 3, 1)
    ratio, beyond = rounding_bound_ratio(got, ref, terms, 4)
    print(f"rounding upsample {name} {dt}: worst error / bound {ratio:.3f}, {beyond} of {ref.numel()} outputs more than one ulp from "
          f"the float64 value")
    assert ratio <= 1.0, (name, dt, ratio)


# ---- A6: the power of the two checks, shown on corrupted references (no GPU) -----------------------------------------------------------
def _corruption(kind, o):
    """(i) one (tap, 16-channel slice) term -- one MFMA -- missing from the conv3 channel with the largest |conv1.weight|; (ii) the conv3
    channels with the largest and the smallest conv1.weight swapped in front of the 1x1 convolution; (iii) the bilinear tx of the single
    column ox = 0 + 8, where the column ranges of the first two producer waves meet, off by 2^-6."""
    if kind == "drop":
        return ("drop", int(o["w1"].abs().argmax()), 4, 3)
    if kind == "swap":
        return ("swap", int(o["w1"].argmax()), int(o["w1"].argmin()))
    return ("tx", 8, 2.0 ** -6)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["drop", "swap", "tx"])
def test_the_exact_comparison_rejects_a_corrupted_reference(kind, dt):
    """The comparison of test_head_tail_is_exact_on_integers (`seam` case) does not accept the float64 reference with one fault built
    in, with or without the outer ReLU -- the faults that err < tol * (1 + max |want|) on white noise lets through."""
    b, ih, iw, oh, ow, grain = HEAD["seam"]
    o, want = head_case("seam", dt), head_want("seam", dt, False)
    bad = head_ref(o, (oh, ow), False, _corruption(kind, o))
    for relu_out in (True, False):
        assert _exact_equal(want.value(relu_out), want.value(relu_out), dt)
        assert not _exact_equal(bad.value(relu_out), want.value(relu_out), dt), (kind, dt, relu_out)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["drop", "swap", "tx"])
def test_the_rounding_bound_rejects_a_corrupted_reference(kind, dt):
    """The two bounds of test_head_tail_rounding_bound (`x2` case) against the same three faults.  The output of a faulty kernel is
    modelled as the float64 chain with the fault built in, the upsampled map rounded to the type as the kernels round it, the result
    rounded to the type; the same chain without a fault must pass both bounds, with a fault it must exceed one of them somewhere.

    The bound on the unrounded map alone (sum |W| 1/2 ulp_T(|u|): each of the 1152 activation roundings of a channel at its worst
    sign, about 5e-3 per channel in float16 and 4e-2 in bfloat16 on these operands, and each of the 32 channels at its worst sign
    again) rejects the swap in both types and the dropped term in float16, and nothing else: worst error / bound
                 no fault   drop     swap     tx
        float16  0.03       3.6     60       0.6
        bfloat16 0.04       0.5     11       0.1
    (one missing MFMA term moves ONE channel by about 0.07 and the output by |conv1.weight| <= 0.45 times that; a tx off by 2^-6
    moves an activation by less than bfloat16's own rounding step).  That is why Part B holds the kernels to head_sharp_bound as
    well, which knows what almost every activation rounds to and charges nothing for it; its ratios are printed here."""
    b, ih, iw, oh, ow = ROUNDING["x2"]
    o = rounding_case("x2", dt)
    fault = _corruption(kind, o)
    worst = {}
    for what, corrupt in (("no fault", None), (kind, fault)):
        ratios = [_rounding_ratios(head_ref(o, (oh, ow), False, corrupt, round_to=dt).value(r).to(DT[dt]), "x2", dt, False, r) for r in (True, False)]
        worst[what] = (max(a for a, _ in ratios), max(b_ for _, b_ in ratios))
        print(f"rounding bounds on a modelled kernel output, {what} {dt}: worst error / bound {worst[what][0]:.3f} (unrounded map), "
              f"{worst[what][1]:.3f} (rounded map)")
    assert max(worst["no fault"]) <= 1.0, (dt, worst)
    assert max(worst[kind]) > 1.0, (kind, dt, worst)


# ---- A7: DS_HEAD_RPW=2, read once per process: one fresh child ------------------------------------------------------------------------
RPW2_SELECT = "test_head_tail_is_exact_on_integers and tile"
RPW2_SECONDS = 300          # the child's own time limit: interpreter start, GPU context, 10 small launches take well under a minute


@GPU
def test_two_rows_per_wave_in_a_child_process(gpu):
    """k_dpt_head_tail<BF16, RPW = 2, 0> (8 x 32 tiles, two accumulators per wave) on the tile-mode cases of
    test_head_tail_is_exact_on_integers: ONE child process with DS_HEAD_RPW=2 (one more GPU context), which must pass every one of
    them and skip none.  A child that dies on a signal or at its time limit fails this test, and nothing is started after it."""
    expected = 2 * sum(1 for n, c, s in RUNS if c == "tile")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", RPW2_SELECT],
                           env=dict(os.environ, DS_HEAD_RPW="2"), cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=RPW2_SECONDS)
    tail = child.stdout[-4000:]
    assert child.returncode == 0, f"child exit status {child.returncode}\n{tail}"
    summary = re.search(r"(\d+) passed", child.stdout)
    assert summary and int(summary.group(1)) == expected and " skipped" not in child.stdout.splitlines()[-1], tail
