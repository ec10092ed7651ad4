"""ds_dpt_head_front: refinenet1's x2 bilinear upsample and the head's 256 -> 128 convolution in one kernel
(csrc/ds_head_front.hip).  Its contract is "the same bits as ds_upsample_bilinear_nhwc followed by ds_conv3x3_nhwc", so the
reference of every comparison here is those two launches, and every comparison is on bit patterns.

Tile of the kernel: 8 x 32 output pixels, all 128 channels; a workgroup walks its tiles in 64-channel chunks.  The shapes are the
smallest at which it can go wrong (low-resolution height x width, batch):
    5 x 7, 2      partial tiles in both directions, an image seam inside the tile list, every border tap
    4 x 16, 1     exactly one tile
    9 x 20, 1     3 x 2 tiles, the last ones partial
    9 x 20, 50    300 tiles: more than one per workgroup on a 256-CU chip (the workgroup is persistent, one per CU)
    1 x 1, 64     sy = sx = 0, one source pixel under everything.  Batch 64, not 3: ds_conv3x3_nhwc, the reference, takes no
                  fewer than 256 pixels, and 64 images of 2 x 2 are the fewest that reach it
    2 x 33, 1     a row longer than two tiles and shorter than three
The whole-network tests run dpt_beit_large_512 and Depth-Anything-V2 ViT-L with the route on against off."""
import pytest
import torch
import torch.nn as nn

import conftest  # noqa: F401
import model_weights as mw

pytestmark = pytest.mark.gpu
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CASES = [(5, 7, 2), (4, 16, 1), (9, 20, 1), (9, 20, 50), (1, 1, 64), (2, 33, 1)]
NAMES = ("ds_dpt_head_front", "ds_conv3x3_nhwc", "ds_upsample_bilinear_nhwc")


def _conv(dtype, bias, seed=5):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(256, 128, kernel_size=3, stride=1, padding=1, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / 48)
        if bias:
            conv.bias.copy_(torch.randn(128, generator=g))
    return conv.cuda().to(dtype)


def _x(b, ih, iw, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((b, 256, ih, iw), generator=g).cuda().to(dtype).contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.permute(0, 2, 3, 1).contiguous().view(torch.int16)


def _two_launches(nat, conv, x):
    return nat.conv3x3(conv, nat.upsample_bilinear(x, scale_factor=2, align_corners=True))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_b%d" % c)
def test_same_bits_as_the_two_launches(gpu, case, dt, bias):
    from src import _native as nat
    ih, iw, b = case
    conv, x = _conv(DT[dt], bias), _x(b, ih, iw, DT[dt], seed=100 * ih + iw)
    before = {n: nat.CALLS[n] for n in NAMES}
    got = nat.dpt_head_front(x, conv)
    assert {n: nat.CALLS[n] - before[n] for n in NAMES} == {n: 1 for n in NAMES}
    want = _two_launches(nat, conv, x)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (b, 128, 2 * ih, 2 * iw) and got.is_contiguous(memory_format=torch.channels_last)
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().mean()) > 0.1
    assert torch.equal(got, want), f"{int((_bits(got) != _bits(want)).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("dt", list(DT))
def test_nan_and_inf_in_border_pixels_land_where_the_upsample_puts_them(gpu, dt):
    """A NaN and an Inf in two corners of the source image: the halo beside them is the convolution's zero padding, literal zeros,
    not a product with a zero weight -- so exactly the outputs of the two launches are NaN / Inf, and the bit patterns agree."""
    from src import _native as nat
    conv, x = _conv(DT[dt], True), _x(2, 5, 7, DT[dt], seed=9)
    x[0, 3, 0, 0] = float("nan")
    x[0, 70, 0, 0] = float("inf")
    x[1, 200, 4, 6] = float("-inf")
    x[1, 129, 4, 0] = float("nan")
    got, want = nat.dpt_head_front(x, conv), _two_launches(nat, conv, x)
    torch.cuda.synchronize()
    assert bool(torch.isnan(want.float()).any()) and bool(torch.isfinite(want.float()).any())
    assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} bit patterns differ"


@pytest.mark.parametrize("dt", list(DT))
def test_nothing_outside_out_is_written(gpu, dt):
    """The raw entry point writing into the middle of a buffer prefilled with a sentinel (as tests/test_gpu_head_exact.py does for
    the upsample): the slice holds the two launches' result, the bytes in front of and behind it are unchanged."""
    from src import _native as nat
    sentinel = -1234.0
    conv, x = _conv(DT[dt], True), _x(2, 5, 7, DT[dt], seed=3)
    want = _two_launches(nat, conv, x).permute(0, 2, 3, 1).contiguous()
    n, guard = want.numel(), 4096                                     # elements; 8 KiB on either side keeps the output 16-byte aligned
    buf = torch.full((n + 2 * guard,), sentinel, dtype=DT[dt], device="cuda")
    nat.dpt_head_front(x, conv, out=buf[guard:guard + n])
    torch.cuda.synchronize()
    assert torch.equal(buf[guard:guard + n].view(want.shape), want)
    bits, clean = buf.view(torch.int16).cpu(), torch.full((1,), sentinel, dtype=DT[dt]).view(torch.int16)
    assert bool((bits[:guard] == clean).all()) and bool((bits[guard + n:] == clean).all()), "guard bands written"


def test_unsupported_shapes_are_refused(gpu):
    """Other channel counts and an upsample too weak for the staging tile return DS_EUNSUPPORTED (the caller runs the two launches)."""
    from src import _native as nat
    x = _x(1, 8, 40, torch.float16, seed=1).permute(0, 2, 3, 1).contiguous()
    w = torch.zeros((256, 9, 256), dtype=torch.float16, device="cuda")
    out = torch.zeros((1 * 16 * 80 * 256,), dtype=torch.float16, device="cuda")

    def rc(oh, ow, n):
        return nat.lib().ds_dpt_head_front(nat.ctx_for(torch.cuda.current_device()), x.data_ptr(), w.data_ptr(), None, out.data_ptr(),
                                           1, 8, 40, oh, ow, 256, n, 1, nat._stream(x))
    assert rc(16, 80, 256) == -2 and rc(16, 80, 64) == -2             # DS_EUNSUPPORTED: out_channels != 128
    assert rc(8, 40, 128) == -2                                       # no upsample at all: 10 rows of source under a patch
    assert rc(16, 80, 128) == 0
    torch.cuda.synchronize()


def _run(m, x, vm, nat, monkeypatch, on, **kw):
    monkeypatch.setattr(vm, "HEAD_FRONT", on)
    before = {n: nat.CALLS[n] for n in NAMES}
    with torch.no_grad():
        y = m(x, **kw)
    torch.cuda.synchronize()
    return y, {n: nat.CALLS[n] - before[n] for n in NAMES}


def _check_routes(calls1, calls0):
    assert calls1["ds_dpt_head_front"] == 1 and calls0["ds_dpt_head_front"] == 0, (calls1, calls0)
    for n in ("ds_conv3x3_nhwc", "ds_upsample_bilinear_nhwc"):
        assert calls1[n] == calls0[n] > 0, (n, calls1, calls0)


def test_dpt_beit_large_512_keeps_its_bits(gpu, monkeypatch):
    """512^2, batch 2, float16: DS_HEAD_FRONT on against off, eager and replayed from a hipGraph; the counters tell the routes apart
    while the numbers of in-tree convolutions and upsamples read the same.  With taps (features={}) the fused entry point is not
    reached and the taps are unchanged."""
    from dmidas.dpt_depth import DPTDepthModel
    from src import _native as nat
    from src import vit_mi355x as vm
    from src.hip_graph import GraphedForward
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    m = m.cuda().half()
    base = mw.synthetic_image((1, 3, 512, 512), seed=31)
    x = torch.cat([base, base.roll(17, dims=3)]).cuda().half().contiguous(memory_format=torch.channels_last)
    y1, calls1 = _run(m, x, vm, nat, monkeypatch, True)
    y0, calls0 = _run(m, x, vm, nat, monkeypatch, False)
    _check_routes(calls1, calls0)
    assert bool(torch.isfinite(y1.float()).all()) and float(y1.float().std()) > 0
    assert torch.equal(y1, y0), "the fused head front changed the prediction"
    f1, f0 = {}, {}
    t1, c1 = _run(m, x, vm, nat, monkeypatch, True, features=f1)
    t0, c0 = _run(m, x, vm, nat, monkeypatch, False, features=f0)
    assert c1["ds_dpt_head_front"] == 0 and c1 == c0, (c1, c0)
    assert torch.equal(t1, t0) and sorted(f1) == sorted(f0) and all(torch.equal(f1[k], f0[k]) for k in f0)
    assert f1["r1"].shape[2:] == (256, 256)                           # the tap is path_1 itself, upsampled
    monkeypatch.setattr(vm, "HEAD_FRONT", True)
    before = nat.CALLS["ds_dpt_head_front"]
    with torch.no_grad():
        gf = GraphedForward(lambda t: m(t))
        yg = gf(x)
        yg = gf(x)
    torch.cuda.synchronize()
    assert gf.graphs, "the forward was not captured"
    assert nat.CALLS["ds_dpt_head_front"] > before
    assert torch.equal(yg, y0), "the replayed forward differs"


def test_depth_anything_v2_vitl_keeps_its_bits(gpu, monkeypatch):
    """ViT-L at 518^2, batch 1, float16: 148 x 148 -> 296 x 296 in front of output_conv1 (9.25 tiles across, 37 down)."""
    from ddepth_anything_v2 import DepthAnythingV2
    from src import _native as nat
    from src import vit_mi355x as vm
    m = DepthAnythingV2('vitl', features=256, out_channels=[256, 512, 1024, 1024]).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.cuda().half()
    x = mw.synthetic_image((1, 3, 518, 518), seed=32).cuda().half()
    y1, calls1 = _run(m, x, vm, nat, monkeypatch, True)
    y0, calls0 = _run(m, x, vm, nat, monkeypatch, False)
    _check_routes(calls1, calls0)
    assert bool(torch.isfinite(y1.float()).all()) and float(y1.float().std()) > 0
    assert torch.equal(y1, y0), "the fused head front changed the prediction"
