"""GPU tests of MiDaS v2.1 small (model id 6): ds_dwconv_nhwc against its float64 definition, the network in float32 against the
reference's own module (tests/golden/midas_small_cases.npz) and in float16 against the project's half-precision bar, the
DS_DWCONV=0 route, the funnel with a hipGraph replay, and Boost."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401
import model_weights as mw

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "midas_small_cases.npz")
CASES = {"b2_96x128": ((2, 3, 96, 128), 31), "b1_256x192": ((1, 3, 256, 192), 32)}
WIDTHS = (32, 144, 192, 288, 576, 816, 1392)          # every depthwise width of EfficientNet-Lite3


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _pads(k, s, choice, h, w):
    """(pad_top, pad_left, out_h, out_w): TF "same", symmetric (k - 1) / 2 with a floor division, or k - 1 before and none after."""
    def same(n):
        total = max((-(-n // s) - 1) * s + k - n, 0)
        return total // 2, total - total // 2
    if choice == "same":
        (pt, pb), (pl, pr) = same(h), same(w)
    elif choice == "sym":
        pt = pb = pl = pr = (k - 1) // 2
    else:
        pt, pb, pl, pr = k - 1, 0, k - 1, 0
    return pt, pl, (h + pt + pb - k) // s + 1, (w + pl + pr - k) // s + 1


def _definition(x, w_taps, bias_in, bias, k, s, pt, pl, oh, ow, clamp=True):
    """include/depthstereo.h: ds_dwconv_nhwc in float64 on the CPU (x logical NCHW; clamp=False: without the output ReLU6)."""
    x = x.detach().cpu().double()
    c, h, w = x.shape[1:]
    a = (x + bias_in.cpu().double().view(1, -1, 1, 1)).clamp(0, 6)
    pb, pr = (oh - 1) * s + k - pt - h, (ow - 1) * s + k - pl - w
    a = F.pad(a, (pl, max(pr, 0), pt, max(pb, 0)))
    y = F.conv2d(a, w_taps.cpu().double().t().reshape(c, 1, k, k), bias.cpu().double(), stride=s, groups=c)[:, :, :oh, :ow]
    return y.clamp(0, 6) if clamp else y


def _operands(g, b, c, h, w, k, dtype):
    x = (torch.randn((b, c, h, w), generator=g) * 3 + 1).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    w_taps = (torch.randn((k * k, c), generator=g) / k).cuda()
    return x, w_taps, torch.randn((c,), generator=g).cuda(), (torch.randn((c,), generator=g) + 1).cuda()


def _f16_ulps(got, ref64):
    """distance in f16 ulps between every output and the float64 value rounded to f16 (all values lie in [0, 6])."""
    a = got.detach().cpu().abs().view(torch.int16).int()
    b = ref64.abs().half().view(torch.int16).int()
    return (a - b).abs()


def _f16_within_bound(got, ref64, x, w_taps, bias_in, bias, k, s, pt, pl, oh, ow):
    """Every output equals the float64 value rounded to f16 or is one f16 ulp from it -- unless the sum cancels: an fp32
    accumulation of k^2 products and the bias is exact to (k^2 + 1) 2^-24 sum |terms|, which can exceed half an f16 ulp of a
    small result.  Such outputs may differ by that bound plus one ulp.  Returns (#outputs beyond one ulp, all within bound)."""
    ulps = _f16_ulps(got, ref64)
    terms = _definition(x, w_taps.abs(), bias_in, bias.abs(), k, s, pt, pl, oh, ow, clamp=False)       # sum |w a| + |bias|
    r16 = ref64.half().double()
    spacing = torch.where(r16 >= 2.0 ** -14, 2.0 ** (torch.floor(torch.log2(r16.clamp(min=2.0 ** -14))) - 10), torch.full_like(r16, 2.0 ** -24))
    slack = (k * k + 1) * 2.0 ** -24 * terms + spacing
    ok = (ulps <= 1) | ((got.detach().cpu().double() - ref64).abs() <= slack)
    return int((ulps > 1).sum()), bool(ok.all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_dwconv_matches_float64_definition(gpu, dtype):
    from src import _native
    g = torch.Generator().manual_seed(7)
    sizes = [(7, 9), (8, 12), (15, 16), (16, 11)]
    beyond, total = 0, 0
    for k in (3, 5):
        for s in (1, 2):
            for i, c in enumerate(WIDTHS):
                h, w = sizes[(i + k + s) % len(sizes)]
                choice = ("same", "sym", "edge")[i % 3]
                b = (1, 3)[i % 2]
                pt, pl, oh, ow = _pads(k, s, choice, h, w)
                x, wt, bi, bo = _operands(g, b, c, h, w, k, dtype)
                y = _native.dwconv(x, wt, bi, bo, k, s, pt, pl, (oh, ow))
                ref = _definition(x, wt, bi, bo, k, s, pt, pl, oh, ow)
                case = (k, s, c, h, w, choice, b)
                assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last), case
                xa = x.float() + bi.view(1, -1, 1, 1)
                assert bool((xa < 0).any()) and bool((xa > 6).any()), case          # the input tail clamps at both ends
                if dtype == torch.float32:
                    err = (y.cpu().double() - ref).abs().max().item()
                    assert err <= 1e-5 * ref.abs().max().item(), (case, err)
                else:
                    n, ok = _f16_within_bound(y, ref, x, wt, bi, bo, k, s, pt, pl, oh, ow)
                    beyond, total = beyond + n, total + ref.numel()
                    assert ok, case
    if dtype == torch.float16:
        print(f"ds_dwconv_nhwc f16: {beyond} of {total} outputs more than one ulp from the float64 value (cancellation)")
        assert beyond <= 1e-3 * total


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_dwconv_batch_invariance(gpu, dtype):
    """image 2 of a batch of 3 equals the same image alone, bit for bit (the launch picks its tile from the batch size)."""
    from src import _native
    g = torch.Generator().manual_seed(8)
    for k, s, c, h, w in [(5, 2, 816, 36, 64), (3, 1, 1392, 8, 8), (3, 2, 144, 144, 256), (5, 1, 576, 18, 32)]:
        pt, pl, oh, ow = _pads(k, s, "same", h, w)
        x, wt, bi, bo = _operands(g, 3, c, h, w, k, dtype)
        y3 = _native.dwconv(x, wt, bi, bo, k, s, pt, pl, (oh, ow))
        y1 = _native.dwconv(x[2:3].contiguous(memory_format=torch.channels_last), wt, bi, bo, k, s, pt, pl, (oh, ow))
        assert torch.equal(y3[2:3], y1), (k, s, c, h, w)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_nan_reaches_exactly_the_windows_that_hold_it(gpu, dtype, k):
    """One NaN input element gives NaN at exactly the outputs of its channel whose window holds it -- ReLU6 propagates NaN like the
    reference's nn.ReLU6 (hardtanh) and like the clamp of _definition; every other output keeps the bits of the run without it."""
    from src import _native
    g = torch.Generator().manual_seed(9)
    for s, (b, c, h, w), (n, ch, iy, ix) in [(1, (2, 32, 9, 12), (1, 5, 4, 6)), (2, (3, 144, 11, 10), (2, 143, 0, 9)), (1, (1, 192, 8, 8), (0, 64, 7, 0))]:
        pt, pl, oh, ow = _pads(k, s, "same", h, w)
        x, wt, bi, bo = _operands(g, b, c, h, w, k, dtype)
        clean = _native.dwconv(x, wt, bi, bo, k, s, pt, pl, (oh, ow))
        x[n, ch, iy, ix] = float("nan")
        y = _native.dwconv(x, wt, bi, bo, k, s, pt, pl, (oh, ow)).cpu()
        oy, ox = torch.arange(oh).view(-1, 1), torch.arange(ow).view(1, -1)
        hit = (oy * s - pt <= iy) & (iy < oy * s - pt + k) & (ox * s - pl <= ix) & (ix < ox * s - pl + k)
        want = torch.zeros((b, c, oh, ow), dtype=torch.bool)
        want[n, ch] = hit
        case = (k, s, (b, c, h, w), (n, ch, iy, ix))
        assert bool(hit.any()) and torch.equal(torch.isnan(y), want), (case, int(torch.isnan(y).sum()), int(want.sum()))
        assert torch.equal(torch.isnan(_definition(x, wt, bi, bo, k, s, pt, pl, oh, ow)), want), case
        assert torch.equal(y[~want], clean.cpu()[~want]), case


def test_dwconv_argument_checks(gpu):
    from src import _native
    L = _native.lib()
    x, wt, bi, bo = _operands(torch.Generator().manual_seed(1), 1, 32, 8, 8, 3, torch.float16)
    y = torch.empty_like(x)
    ctx = _native.ctx_for(torch.cuda.current_device())

    def call(xp=x.data_ptr(), yp=y.data_ptr(), c=32, oh=8, ow=8, k=3, s=1, pt=1, pl=1, dt=1):
        return L.ds_dwconv_nhwc(ctx, xp, wt.data_ptr(), bi.data_ptr(), bo.data_ptr(), yp, 1, 8, 8, c, oh, ow, k, s, pt, pl, dt, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert call(dt=2) == -2                                   # bf16: DS_EUNSUPPORTED
    assert call(dt=0) == -1 and call(dt=4) == -1
    assert call(k=4) == -1 and call(k=7) == -1 and call(s=3) == -1 and call(s=0) == -1
    assert call(pt=3) == -1 and call(pl=-1) == -1             # pads outside [0, kernel)
    assert call(c=12) == -1 and call(c=0) == -1               # channels % 8
    assert call(yp=x.data_ptr()) == -1 and call(yp=x.data_ptr() + 16) == -1      # y aliases x
    assert call(oh=10) == -1 and call(ow=3) == -1             # outputs that do not follow from the input
    assert call(xp=x.data_ptr() + 2) == -1                    # 16-byte alignment


def _model(dtype=torch.float32):
    from dmidas.midas_net_custom import MidasNet_small
    m = MidasNet_small(path=None, features=64, backbone="efficientnet_lite3", exportable=True, non_negative=True,
                       blocks={'expand': True}).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    return m.cuda().to(dtype)


def test_network_float32_matches_reference_module(gpu):
    from src import _native
    gold = np.load(GOLD)
    m = _model()
    for tag, (shape, seed) in CASES.items():
        x = mw.synthetic_image(shape, seed).cuda()
        before = _native.CALLS["ds_dwconv_nhwc"]
        with torch.no_grad():
            y = m(x).cpu().numpy()
        assert _native.CALLS["ds_dwconv_nhwc"] - before == 24          # every depthwise convolution in-tree
        err = _rel(y, gold[f"{tag}_out"])
        print(f"midas_small {tag} float32: {err:.3e} of the reference module's output")
        assert err < 1e-4, err


def test_network_float16_within_half_precision_bar(gpu):
    """max(2e-2, 1.3 x the error of the same network under vm.stock_routing() in float16) -- DESIGN.md's rule for dpt_hybrid --
    for the in-tree route and for DS_DWCONV=0."""
    from dmidas.backbones import efficientnet_lite as effl
    from src import vit_mi355x as vm
    gold = np.load(GOLD)
    m = _model(torch.float16)
    for tag, (shape, seed) in CASES.items():
        ref = gold[f"{tag}_out"]
        x = mw.synthetic_image(shape, seed).cuda().half().contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            e16 = _rel(m(x).float().cpu().numpy(), ref)
            with vm.stock_routing():
                e_stock = _rel(m(x).float().cpu().numpy(), ref)
            saved = effl.DWCONV_HIP
            effl.DWCONV_HIP = False
            try:
                e_lib = _rel(m(x).float().cpu().numpy(), ref)
            finally:
                effl.DWCONV_HIP = saved
        bound = max(2e-2, 1.3 * e_stock)
        print(f"midas_small {tag} float16: in-tree {e16:.3e}, DS_DWCONV=0 {e_lib:.3e}, stock torch {e_stock:.3e}, bound {bound:.3e}")
        assert np.isfinite(e16) and e16 <= bound and e_lib <= bound


def test_funnel_and_graph_replay(gpu):
    """core_generation_funnel with model_type 6 (random init) for two same-size images and one other size: depth, stereo pair and
    normal map; then one shape four times through predict_batch: the fourth call is a hipGraph replay equal to the eager forward."""
    from PIL import Image
    import src.core as core
    core.model_holder.allow_random_init = True
    try:
        # torch's default initialisation leaves this network's head dead (a constant depth map): name-seeded weights instead
        core.model_holder.ensure_models(6, torch.device('cuda', torch.cuda.current_device()), False)
        net = core.model_holder.depth_model.net
        net.load_state_dict(mw.fill_state_dict(net.state_dict()), strict=True)
        rng = np.random.default_rng(4)
        imgs = [Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)) for _ in range(2)]
        imgs.append(Image.fromarray(rng.integers(0, 256, (80, 112, 3), dtype=np.uint8)))
        res = list(core.core_generation_funnel(None, imgs, None, None, {'model_type': 6, 'net_width': 256, 'net_height': 256,
                                                                        'gen_stereo': True, 'stereo_modes': ['left-right'],
                                                                        'gen_normalmap': True}))
        for i, im in enumerate(imgs):
            kinds = [k for j, k, _ in res if j == i]
            assert 'depth' in kinds and 'left-right' in kinds and 'normalmap' in kinds, kinds
            d = np.asarray([r for j, k, r in res if j == i and k == 'depth'][0])
            assert d.shape == (im.height, im.width) and d.max() > d.min()
        pred = core.model_holder.depth_model
        assert next(pred.net.parameters()).dtype == torch.float16
        pred.hip_graphs = "auto"
        pred._graphed.clear()
        u8 = torch.from_numpy(np.stack([np.asarray(im) for im in imgs[:2]])).cuda()
        outs = [pred.predict_batch(u8, 256, 256) for _ in range(4)]
        gf = pred._graphed[(256, 256)]
        assert (tuple(u8.shape), u8.dtype, u8.device) in gf.graphs and not gf.failed
        eager = pred._predict_batch_eager(u8, 256, 256)
        assert torch.equal(outs[3], eager) and torch.equal(outs[2], eager)
    finally:
        core.model_holder.allow_random_init = False
        core.model_holder.unload_models()


def test_boost_on_midas_small(gpu):
    from PIL import Image
    from src.depthmap_generation import ModelHolder
    mh = ModelHolder()
    mh.allow_random_init = True
    mh.ensure_models(6, 'cuda', True)
    assert next(mh.depth_model.net.parameters()).dtype == torch.float32        # Boost never runs MiDaS in half (reference :271)
    img = Image.fromarray(np.random.default_rng(5).integers(0, 256, (768, 1024, 3), dtype=np.uint8))
    raw, invert = mh.get_raw_prediction(img, 256, 256)
    raw = torch.as_tensor(raw)
    assert tuple(raw.shape) == (768, 1024) and bool(torch.isfinite(raw).all()) and not invert
    mh.unload_models()
