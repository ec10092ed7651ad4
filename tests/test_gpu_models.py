"""GPU tests of the model path: the fused MFMA attention kernel against its float32 definition, and the half-precision
Depth-Anything-V2 forward (HIP attention inside) against the float32 reference outputs committed under tests/golden."""
import os

import numpy as np
import pytest
import torch

import conftest  # noqa: F401
import model_weights as mw

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_cases.npz")


def _case(b, n_valid, h, dtype, seed, with_bias, stride=None):
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(seed)
    npad = vm.pad_len(n_valid) if stride is None else stride
    qk = (torch.randn((b, npad, 2, h, 64), generator=g) * 1.5).to(dtype).cuda()
    vt = torch.randn((b, h * 64, npad), generator=g).to(dtype).cuda()
    # the bias is defined on the valid tokens only ([H, n, n], natural units), like the reference's relative position bias
    bias = (torch.randn((h, n_valid, n_valid), generator=g) * 2.0).cuda() if with_bias else None
    return qk, vt, bias, npad


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("with_bias", [False, True])
def test_attention_kernel_matches_definition(gpu, dtype, with_bias):
    from src import vit_mi355x as vm
    from src import _native
    for (b, n_valid, h, seed) in [(1, 1, 1, 1), (2, 63, 2, 2), (1, 64, 3, 3), (2, 131, 6, 4), (1, 577, 12, 5), (1, 1370, 16, 6),
                                  (3, 200, 1, 7)]:
        qk, vt, bias, npad = _case(b, n_valid, h, dtype, seed, with_bias)
        packed, padded = None, None
        if bias is not None:
            packed = _native.attention_bias_pack(bias, npad, dtype)
            padded = torch.zeros((h, npad, npad), device='cuda')
            padded[:, :n_valid, :n_valid] = bias
            # the pack kernel against its layout definition (include/depthstereo.h): [H][Np/32][Np/64][4][64 lanes][8];
            # chunk c = 2 kb + s holds, for lane (hi, l31), bias[query 16 s + 8 hi + t][key 32 kb + l31] / scale (t = 0..7):
            # the A fragments of the MFMAs that add the bias to the logits
            t = packed.data.float().view(h, npad // 32, npad // 64, 4, 64, 8)
            lane = torch.arange(64, device='cuda')
            c = torch.arange(4, device='cuda')
            j = torch.arange(8, device='cuda')
            qq = (16 * (c[:, None, None] & 1) + 8 * (lane[None, :, None] >> 5) + j[None, None, :]).expand(4, 64, 8)
            key = (32 * (c[:, None, None] >> 1) + (lane & 31)[None, :, None]).expand(4, 64, 8)
            mul = 8.0
            for qb in (0, npad // 32 - 1):
                for kt in (0, npad // 64 - 1):
                    exact = (padded[:, qb * 32:(qb + 1) * 32, kt * 64:(kt + 1) * 64] * mul)[:, qq, key]
                    # correctly rounded to the operand type (the kernel rounds the product once)
                    ulp = 2.0 ** (-10 if dtype == torch.float16 else -7)
                    assert ((t[:, qb, kt] - exact).abs() <= 0.5 * ulp * exact.abs() * 1.001 + 1e-30).all()
        got = _native.attention_fwd(qk, vt, n_valid, 0.125, packed)
        want = vm.attention_reference(qk.float(), vt.float(), n_valid, 0.125, padded)
        err = (got.float()[:, :n_valid] - want[:, :n_valid]).abs().max().item()
        # P and the output are rounded to the 11 / 8 bit mantissa; the bias operand (values of a few units, in log2
        # units) is rounded to it as well
        tol = (2e-3 if dtype == torch.float16 else 1.6e-2) if bias is None else (5e-3 if dtype == torch.float16 else 8e-2)
        assert err < tol, (dtype, with_bias, b, n_valid, h, err)
        assert torch.isfinite(got.float()).all()               # pad query rows must stay finite


@pytest.mark.parametrize("b,n_valid,h,with_bias,stride", [
    (32, 1025, 16, True, 1032),       # dpt_beit_large_512 at batch 32 with the tight pad vm.pad_len(1025, 32): 129 row panels
    (8, 2443, 16, False, 2464),       # Depth-Anything-V2 ViT-L, 1080p, batch 8
    (3, 131, 2, True, 136), (2, 577, 12, False, 584), (2, 60, 1, True, 64), (1, 200, 3, True, 200),
])
def test_attention_tight_token_stride(gpu, b, n_valid, h, with_bias, stride):
    """The token stride of the operands only has to be a multiple of 8: the kernel walks whole 64-key tiles, rows between the
    stride and the next multiple of 64 do not exist (K reads end at the batch element, V^T columns alias the next row, both
    masked; query rows there are neither loaded nor stored).  Against the float32 definition on the same strided operands;
    the neighbouring batch elements are poisoned where a stray read or store would show."""
    from src import vit_mi355x as vm
    from src import _native
    assert stride % 8 == 0 and stride >= n_valid
    dtype = torch.float16
    qk, vt, bias, npad = _case(b, n_valid, h, dtype, 4000 + n_valid, with_bias, stride=stride)
    packed, padded = None, None
    if bias is not None:
        packed = _native.attention_bias_pack(bias, npad, dtype)
        assert packed.npad == (npad + 63) // 64 * 64
        padded = torch.zeros((h, npad, npad), device='cuda')
        padded[:, :n_valid, :n_valid] = bias
    # pad rows of every batch element carry large finite junk in K and V (a real pad row holds whatever the GEMM wrote)
    if npad > n_valid:
        qk[:, n_valid:, 1] = 300.0
        vt[:, :, n_valid:] = -250.0
    got = _native.attention_fwd(qk, vt, n_valid, 0.125, packed)
    tol = 2e-3 if bias is None else 1e-2
    worst = 0.0
    for b0 in range(0, b, 4):
        want = vm.attention_reference(qk[b0:b0 + 4].float(), vt[b0:b0 + 4].float(), n_valid, 0.125, padded)
        worst = max(worst, (got[b0:b0 + 4].float()[:, :n_valid] - want[:, :n_valid]).abs().max().item())
    assert worst < tol, (b, n_valid, stride, worst)
    assert got.shape == (b, npad, h * 64) and torch.isfinite(got.float()).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("b,n_valid,h,with_bias,stride", [
    (2, 1025, 16, True, 1032),        # the metric's shape (one (batch, head) = 4 full workgroups + one with a single live row)
    (1, 2443, 16, False, 2448),       # config 5: the last workgroup has three live waves, 11 keys in the last tile
    (1, 4097, 4, True, 4104),         # NET_SIZE_MATCH: 65 tiles
    (2, 577, 12, False, 584), (1, 1370, 16, False, 1376),
    (3, 1, 1, True, 8), (2, 63, 2, False, 64), (1, 64, 3, True, 64), (2, 65, 2, True, 72), (2, 128, 1, False, 128),
    (1, 129, 2, True, 136), (2, 256, 2, True, 256), (1, 257, 2, False, 264), (1, 300, 3, True, 304), (2, 191, 6, True, 192),
])
def test_attention_generation4_is_generation2_reordered(gpu, dtype, b, n_valid, h, with_bias, stride):
    """Generation 4 of the attention kernel (csrc/ds_attention4.hip: one wave per SIMD, two query sub-blocks skewed by half a tile
    inside the wave; opt-in, DS_ATT_GEN=4) restates generation 2's arithmetic in another order of INDEPENDENT operations: with
    the tiled path on every block (DS_ATT_TAIL=0) the outputs are bit-identical, pad rows included, on every tile-count corner
    (one tile, one key in the last tile, a full last tile, one live row in the last workgroup, dead waves), with keys far
    above the rest in several tiles (the deferred maximum is raised mid-sequence) and junk in the pad rows.  With the GEMV
    tail blocks (the default, ds_attention.h: at_tail_rows) both meet the float32 definition
    (dmidas/backbones/beit.py:65-91)."""
    from src import vit_mi355x as vm
    from src import _native
    qk, vt, bias, npad = _case(b, n_valid, h, dtype, 6000 + n_valid, with_bias, stride=stride)
    packed, padded = None, None
    if bias is not None:
        packed = _native.attention_bias_pack(bias, npad, dtype)
        padded = torch.zeros((h, npad, npad), device='cuda')
        padded[:, :n_valid, :n_valid] = bias
    if npad > n_valid:
        qk[:, n_valid:, 1] = 300.0
        vt[:, :, n_valid:] = -250.0
    for t in range(0, n_valid, 97):
        qk[:, t, 1] *= 3.0
    out = {}
    try:
        for gen, tail in ((2, 0), (4, 0), (2, 1), (4, 1)):
            # generation 2 with 32 rows per wave: the instantiation the metric's shape runs
            _native.attention_env(DS_ATT_GEN=gen, DS_ATT_TAIL=tail, DS_ATT_NQB=1 if gen == 2 else None)
            out[gen, tail] = _native.attention_fwd(qk, vt, n_valid, 0.125, packed).clone()
    finally:
        _native.attention_env(DS_ATT_GEN=None, DS_ATT_TAIL=None, DS_ATT_NQB=None)
    assert torch.equal(out[2, 0].view(torch.int16), out[4, 0].view(torch.int16)), (out[2, 0].float() - out[4, 0].float()).abs().max().item()
    want = vm.attention_reference(qk.float(), vt.float(), n_valid, 0.125, padded)
    tol = (4e-3 if dtype == torch.float16 else 3e-2) if bias is None else (1e-2 if dtype == torch.float16 else 1e-1)
    for key, got in out.items():
        assert torch.isfinite(got.float()).all(), key
        err = (got.float()[:, :n_valid] - want[:, :n_valid]).abs().max().item()
        assert err < tol, (key, dtype, n_valid, err)


def test_attention_masks_pad_keys(gpu):
    """Changing K / V^T of the pad keys must not change any real row."""
    from src import _native
    qk, vt, _, npad = _case(1, 100, 2, torch.float16, 9, False)
    a = _native.attention_fwd(qk, vt, 100, 0.125)
    qk2, vt2 = qk.clone(), vt.clone()
    qk2[:, 100:, 1] = 7.0
    vt2[:, :, 100:] = -3.0
    b = _native.attention_fwd(qk2, vt2, 100, 0.125)
    assert torch.equal(a[:, :100], b[:, :100])


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-2), (torch.bfloat16, 8e-2)])
def test_dav2_half_forward_vs_reference_fp32(gpu, dtype, tol):
    """Half-precision forward on the GPU (the reference's default for Depth-Anything-V2, src/depthmap_generation.py:
    273-275) against the reference's float32 outputs.  The float32 bar (1e-4) is tests/test_models_cpu.py; here the
    bound is what 10-11 bit arithmetic through 12 blocks allows."""
    from ddepth_anything_v2 import DepthAnythingV2
    gold = np.load(GOLD)
    m = DepthAnythingV2('vits', features=64, out_channels=[48, 96, 192, 384]).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.cuda().to(dtype)
    x = mw.synthetic_image((2, 3, 140, 182), seed=11).cuda().to(dtype)
    with torch.no_grad():
        y = m(x).float().cpu().numpy()
    ref = gold["dav2_vits_140x182_out"]
    rel = np.abs(y - ref).max() / np.abs(ref).max()
    assert rel < tol, rel


def test_dav2_fp32_gpu_matches_reference(gpu):
    from ddepth_anything_v2 import DepthAnythingV2
    gold = np.load(GOLD)
    m = DepthAnythingV2('vits', features=64, out_channels=[48, 96, 192, 384]).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.cuda()
    x = mw.synthetic_image((2, 3, 140, 182), seed=11).cuda()
    prev = torch.backends.cuda.matmul.allow_tf32
    with torch.no_grad():
        y = m(x).cpu().numpy()
    ref = gold["dav2_vits_140x182_out"]
    assert np.abs(y - ref).max() / np.abs(ref).max() < 1e-4


def test_dav2_infer_batch_shapes(gpu):
    from ddepth_anything_v2 import DepthAnythingV2
    m = DepthAnythingV2('vits', features=64, out_channels=[48, 96, 192, 384]).eval().cuda().half()
    img = torch.randint(0, 256, (2, 96, 160, 3), dtype=torch.uint8, device='cuda')
    d = m.infer_batch(img, input_size=70)
    assert tuple(d.shape) == (2, 96, 160) and d.dtype == torch.float32 and torch.isfinite(d).all()


def test_dpt_beit_half_forward_vs_reference_fp32(gpu):
    """fp16 BEiT-DPT on the GPU (fused attention WITH the relative-position bias operand) against the float32 outputs of the
    reference's own dmidas code (tests/golden/model_cases.npz)."""
    from dmidas.dpt_depth import DPTDepthModel
    gold = np.load(GOLD)
    m = DPTDepthModel(path=None, backbone="beitb16_384", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    x = mw.synthetic_image((2, 3, 160, 224), seed=13).cuda()
    ref = gold["dpt_beitb_160x224_out"]
    with torch.no_grad():
        y32 = m.cuda()(x).cpu().numpy()
    assert np.abs(y32 - ref).max() / np.abs(ref).max() < 1e-4
    with torch.no_grad():
        y16 = m.half()(x.half().contiguous(memory_format=torch.channels_last)).float().cpu().numpy()
    assert np.abs(y16 - ref).max() / np.abs(ref).max() < 2e-2


def test_funnel_with_built_model_family(gpu):
    """core_generation_funnel end to end with a built network (random init: no checkpoints offline): depth + stereo."""
    from PIL import Image
    import src.core as core
    core.model_holder.allow_random_init = True
    try:
        img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (96, 128, 3), dtype=np.uint8))
        res = list(core.core_generation_funnel(None, [img], None, None,
                                               {'model_type': 12, 'net_width': 70, 'net_height': 70, 'gen_stereo': True,
                                                'stereo_modes': ['left-right']}))
        kinds = [k for _, k, _ in res]
        assert 'depth' in kinds and 'left-right' in kinds, kinds
        sbs = [r for _, k, r in res if k == 'left-right'][0]
        assert sbs.size == (256, 96)
    finally:
        core.model_holder.allow_random_init = False
        core.unload_models()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_residual_layernorm_kernel(gpu, dtype):
    from src import _native
    g = torch.Generator().manual_seed(5)
    for rows, c in [(3, 384), (70, 768), (1408, 1024), (5, 1536)]:
        x = torch.randn((rows, c), generator=g).to(dtype).cuda()
        o = torch.randn((rows, c), generator=g).to(dtype).cuda()
        gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype).cuda()
        w = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype).cuda()
        b = (0.1 * torch.randn(c, generator=g)).to(dtype).cuda()
        x_out, h = _native.residual_layernorm(x, o, gamma, w, b, 1e-6)
        xr = (x.float() + gamma.float() * o.float()).to(dtype)
        hr = torch.nn.functional.layer_norm(xr.float(), (c,), w.float(), b.float(), 1e-6)
        tol = 4e-3 if dtype == torch.float16 else 3e-2
        assert (x_out.float() - xr.float()).abs().max().item() <= (1e-3 if dtype == torch.float16 else 1.6e-2) * (1 + xr.float().abs().max().item())
        assert (h.float() - hr).abs().max().item() < tol * (1 + hr.abs().max().item())
        _, h0 = _native.residual_layernorm(x, None, None, w, b, 1e-6)
        h0r = torch.nn.functional.layer_norm(x.float(), (c,), w.float(), b.float(), 1e-6)
        assert (h0.float() - h0r).abs().max().item() < tol * (1 + h0r.abs().max().item())


def test_boost_blend_kernel_vs_restatement(gpu, oracle):
    """ds_boost_blend (all patches, one launch) against the sequential numpy restatement of estimateboost's per-patch loop
    (oracle.boost_blend): overlapping rectangles in a fixed order, non-square rectangles, rectangles at the border."""
    from src import _native
    rng = np.random.default_rng(3)
    H, W, S, M = 150, 220, 64, 97
    dst = rng.random((H, W), dtype=np.float32)
    rects = [(10, 5, 120, 120), (60, 20, 140, 100), (0, 0, 50, 70), (100, 90, 120, 60), (30, 40, 90, 90), (199, 129, 21, 21)]
    coefs = [(float(rng.uniform(0.5, 1.5)), float(rng.uniform(-0.2, 0.2))) for _ in rects]
    preds = rng.random((len(rects), S, S), dtype=np.float32)
    yy, xx = np.mgrid[0:M, 0:M]
    mask = np.exp(-(((xx - M / 2) ** 2 + (yy - M / 2) ** 2) / (2 * (M / 5) ** 2))).astype(np.float32)
    want = oracle.boost_blend(dst, rects, coefs, preds, mask)
    d = torch.from_numpy(dst.copy()).cuda()
    _native.boost_blend(d, rects, coefs, torch.from_numpy(preds).cuda(), torch.from_numpy(mask).cuda())
    got = d.cpu().numpy()
    assert np.abs(got - want).max() < 2e-6, float(np.abs(got - want).max())
    untouched = np.ones((H, W), bool)
    for (x0, y0, w, h) in rects:
        untouched[y0:y0 + h, x0:x0 + w] = False
    assert np.array_equal(got[untouched], dst[untouched])
    # order matters: reversing the list changes the result where rectangles overlap
    d2 = torch.from_numpy(dst.copy()).cuda()
    _native.boost_blend(d2, rects[::-1], coefs[::-1], torch.from_numpy(preds[::-1].copy()).cuda(), torch.from_numpy(mask).cuda())
    assert np.abs(d2.cpu().numpy() - got).max() > 1e-3


def test_boost_pipeline_runs_end_to_end(gpu):
    """estimateboost with LeReS + the pix2pix merge network (random init: no checkpoints offline) on a 1200x1600 image:
    resolution search, double estimation, patch selection, batched patch estimation, one-launch blend."""
    from src import boost
    from lib.multi_depth_model_woauxi import RelDepthModel
    from pix2pix.models.pix2pix4depth_model import Pix2Pix4DepthModel
    torch.manual_seed(0)
    net = RelDepthModel('resnext101').eval().cuda()
    p2p = Pix2Pix4DepthModel().eval().cuda()
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:1200, 0:1600]
    img = (127 + 60 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + rng.normal(0, 25, (1200, 1600, 3))).clip(0, 255).astype(np.uint8)
    stats = {}
    out = boost.estimateboost(torch.from_numpy(img).cuda(), net, 0, p2p, whole_size_threshold=1600, stats=stats)
    assert tuple(out.shape) == (1200, 1600) and out.dtype == torch.float32 and torch.isfinite(out).all()
    assert stats["patches"] >= 1 and 448 <= stats["whole_image_optimal_size"] <= 1600, stats


def test_boost_end_to_end_vs_reference_estimateboost(gpu):
    """Boost end to end ON THE DEVICE (float32 networks, device-side Sobel / resizes / selection, batched patch estimation,
    the one-launch HIP blend) against the reference's OWN estimateboost run on the CPU (tests/golden/make_golden_boost.py;
    src/depthmap_generation.py:774-941, LeReS + pix2pix with name-seeded weights, 480 x 640 image): the same 18 patches, final
    depth within north_star's 1e-4 of full scale and 2e-5 on average.  MEASURED on the device: 9.5e-5 against the round-4 golden
    (profiles/round5_parity_probe_boost.json), and the golden regenerated in round 5 with float32 stand-ins for cv2's float32
    resizes sits 1.7e-5 closer to the product's arithmetic (CPU twin 9.5e-5 -> 7.8e-5, tests/test_models_cpu.py); the device adds
    1.4-1.6e-5 to its CPU twin (per-stage budget in the next test).  Noise floor of the comparison: one ulp on every weight moves
    the output by 3.3e-5 (profiles/round5_boost_conditioning.txt).  What stays unpinned: OpenCV's own resize / blur arithmetic
    (numpy restatements in the golden)."""
    from lib.multi_depth_model_woauxi import RelDepthModel
    from pix2pix.models.pix2pix4depth_model import Pix2Pix4DepthModel
    from src import boost
    z = np.load(os.path.join(os.path.dirname(GOLD), "boost_cases.npz"))
    net = RelDepthModel('resnext101').eval()
    net.load_state_dict(mw.fill_state_dict(net.state_dict()), strict=True)
    p2p = Pix2Pix4DepthModel().eval()
    p2p.netG.load_state_dict(mw.fill_state_dict(p2p.netG.state_dict()), strict=True)
    stats = {}
    out = boost.estimateboost(torch.from_numpy(z["image"]).cuda(), net.cuda(), 0, p2p.cuda(), whole_size_threshold=int(z["rmax"][0]),
                              stats=stats).cpu().numpy()
    want = z["depth_s2"]
    got = out[::2, ::2]
    assert stats["patches"] == 18 and stats["whole_image_optimal_size"] == 896, stats
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"boost on the device vs the reference's estimateboost: max {rel:.3e}, mean {float(np.abs(got - want).mean()):.3e}")
    assert rel < 1e-4 and np.abs(got - want).mean() < 2e-5, (rel, float(np.abs(got - want).mean()))


def test_boost_gpu_error_budget_per_stage(gpu):
    """Where the GPU twin of Boost leaves its CPU twin (which holds 9.5e-5 against the reference's own estimateboost,
    tests/test_models_cpu.py): estimateboost on the device (MIOpen float32 convolutions, HIP blend) against the stage outputs
    of the SAME code on the CPU (torch float32, the blend through the oracle; tests/golden/make_golden_boost_stages.py) --
    whole-image double estimate (2 LeReS forwards + the merge network), base at merge size, the 18 merged patches (2 x 18 LeReS
    forwards + 2 x 18 merge-network forwards), their polyfit coefficients, the blend, the final resize.  Every stage is a float32
    network output renormalised to [0, 1] (pix2pix4depth_model.py:100-104 min-max normalises its inputs; doubleestimate
    :1046-1048 its output): a stage's error is the convolutions' summation-order noise of a ~100-layer float32 ResNeXt times the
    gain of that renormalisation, and the stages do not compound beyond the merge network's own sensitivity."""
    from lib.multi_depth_model_woauxi import RelDepthModel
    from pix2pix.models.pix2pix4depth_model import Pix2Pix4DepthModel
    from src import boost
    import make_golden_boost_stages as mk
    z = np.load(os.path.join(os.path.dirname(GOLD), "boost_cases.npz"))
    want = np.load(os.path.join(os.path.dirname(GOLD), "boost_stage_cases.npz"))
    net = RelDepthModel('resnext101').eval()
    net.load_state_dict(mw.fill_state_dict(net.state_dict()), strict=True)
    p2p = Pix2Pix4DepthModel().eval()
    p2p.netG.load_state_dict(mw.fill_state_dict(p2p.netG.state_dict()), strict=True)
    trace = {}
    out = boost.estimateboost(torch.from_numpy(z["image"]).cuda(), net.cuda(), 0, p2p.cuda(), whole_size_threshold=int(z["rmax"][0]), trace=trace)
    trace["out"] = out.cpu()
    budget = {}
    for k in mk.STRIDES:
        a, b = want[k].astype(np.float64), mk.subsample(k, trace[k]).astype(np.float64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        budget[k] = float(np.abs(a - b).max() / np.abs(a).max())
    print("boost GPU-vs-CPU error budget (max |difference| / max |value| per stage):", {k: f"{v:.2e}" for k, v in budget.items()})
    scratch = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(scratch):                                   # kept with the GPU call's outputs (copied to profiles/ by hand)
        import json
        with open(os.path.join(scratch, "boost_error_budget.json"), "w") as f:
            json.dump({"what": "estimateboost on the GPU vs the same code on the CPU (float32), max |difference| / max |value| per stage",
                       "image": "tests/golden/boost_cases.npz (480 x 640, 18 patches)", "budget": budget}, f, indent=1)
    # measured (profiles/round4_boost_error_budget.json, both twins run on one box): whole estimate 2.5e-5, base 1.8e-5, merged
    # patches 7.6e-5, polyfit coefficients 2e-6, blended and final depth 1.6e-5
    assert budget["whole_estimate"] < 1e-4 and budget["base"] < 1e-4, budget
    assert budget["mapped"] < 3e-4 and budget["coef"] < 1e-4, budget
    assert budget["blended"] < 1e-4 and budget["out"] < 1e-4, budget


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_upsample_bilinear_nhwc_kernel(gpu, dtype):
    from src import _native
    g = torch.Generator().manual_seed(8)
    for (b, c, ih, iw, oh, ow, ac) in [(2, 64, 5, 7, 10, 14, True), (1, 256, 16, 16, 32, 32, True), (3, 8, 9, 13, 20, 27, True),
                                        (2, 32, 10, 10, 37, 23, False), (1, 128, 37, 66, 518, 924, True)]:
        x = torch.randn((b, c, ih, iw), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
        got = _native.upsample_bilinear(x, size=(oh, ow), align_corners=ac)
        want = torch.nn.functional.interpolate(x.float(), size=(oh, ow), mode="bilinear", align_corners=ac)
        tol = 2e-3 if dtype == torch.float16 else 1.6e-2
        assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert (got.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())


@pytest.mark.parametrize("mode", ["persist", "tile"])
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)])
def test_dpt_head_tail_kernel(gpu, dtype, tol, mode, monkeypatch):
    """ds_dpt_head_tail against the torch sequence upsample -> conv3x3 -> ReLU -> conv1x1 -> ReLU in float32: the two older
    kernels (DS_HEAD_MODE=persist is also the fallback of the default for upsamples below ~1.6; the streaming default has its
    own test below)."""
    from src import _native
    monkeypatch.setenv("DS_HEAD_MODE", mode)
    import torch.nn as nn
    import torch.nn.functional as F
    torch.manual_seed(4)
    conv3 = nn.Conv2d(128, 32, 3, padding=1).cuda()
    conv1 = nn.Conv2d(32, 1, 1).cuda()
    with torch.no_grad():
        conv1.bias.fill_(0.05)
    for (b, ih, iw, oh, ow, relu) in [(2, 9, 13, 18, 26, True), (1, 37, 37, 518 // 7, 518 // 7, True), (3, 16, 16, 32, 32, False),
                                      (1, 20, 31, 33, 70, True)]:
        x = torch.randn((b, 128, ih, iw), device='cuda')
        with torch.no_grad():
            up = F.interpolate(x.to(dtype).float(), size=(oh, ow), mode="bilinear", align_corners=True)
            y = conv1(F.relu(conv3(up)))
            want = F.relu(y) if relu else y
            got = _native.dpt_head_tail(x.to(dtype).contiguous(memory_format=torch.channels_last), (oh, ow),
                                        conv3.to(dtype), conv1.to(dtype), relu_out=relu).float()
        conv3.float(); conv1.float()
        assert got.shape == want.shape
        err = (got - want).abs().max().item()
        assert err < tol * (1 + want.abs().max().item()), (b, ih, iw, oh, ow, err)


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)])
def test_dpt_head_tail_stream_kernel(gpu, dtype, tol, monkeypatch):
    """The streaming kernel of ds_dpt_head_tail (the default: column strips, producer / consumer waves, a ring of upsampled
    rows in LDS) against the float32 torch sequence, on shapes with one and several segments per strip, several work items
    per workgroup (forced with DS_HEAD_SEG), ragged right / bottom edges, the two production shapes (256^2 -> 512^2 of DPT,
    296 x 528 -> 518 x 924 of Depth-Anything-V2 at 1080p), both consumer schedules, and one shape that takes the fallback."""
    from src import _native
    import torch.nn as nn
    import torch.nn.functional as F
    torch.manual_seed(4)
    conv3 = nn.Conv2d(128, 32, 3, padding=1).cuda()
    conv1 = nn.Conv2d(32, 1, 1).cuda()
    with torch.no_grad():
        conv1.bias.fill_(0.05)
    monkeypatch.delenv("DS_HEAD_MODE", raising=False)
    for ci, (b, ih, iw, oh, ow, relu, seg) in enumerate([(2, 9, 13, 18, 26, True, None), (1, 37, 37, 518 // 7, 518 // 7, True, None), (3, 16, 16, 32, 32, False, 8),
                                           (1, 20, 31, 33, 70, True, None), (2, 64, 64, 128, 128, True, 16), (1, 37, 66, 518, 924, True, None),
                                           (40, 48, 40, 97, 80, True, 12), (2, 256, 256, 512, 512, True, None), (1, 296, 528, 518, 924, True, None),
                                           (1, 100, 100, 150, 161, True, None)]):
        monkeypatch.setenv("DS_HEAD_VARIANT", str(ci & 1))
        if seg is None:
            monkeypatch.delenv("DS_HEAD_SEG", raising=False)
        else:
            monkeypatch.setenv("DS_HEAD_SEG", str(seg))
        x = torch.randn((b, 128, ih, iw), device='cuda')
        with torch.no_grad():
            up = F.interpolate(x.to(dtype).float(), size=(oh, ow), mode="bilinear", align_corners=True)
            y = conv1(F.relu(conv3(up)))
            want = F.relu(y) if relu else y
            got = _native.dpt_head_tail(x.to(dtype).contiguous(memory_format=torch.channels_last), (oh, ow),
                                        conv3.to(dtype), conv1.to(dtype), relu_out=relu).float()
        conv3.float(); conv1.float()
        assert got.shape == want.shape
        assert torch.isfinite(got).all(), (b, ih, iw, oh, ow)
        err = (got - want).abs().max().item()
        assert err < tol * (1 + want.abs().max().item()), (b, ih, iw, oh, ow, err)


def test_video_two_pass_pipeline_single_rank(gpu, oracle):
    """gen_frames_sharded on one rank: network -> global normalisation -> uint16 -> stereo, against the same steps done by
    hand (process_predicitons on the host, the stereo oracle)."""
    from src import video_mode
    from ddepth_anything_v2 import DepthAnythingV2
    torch.manual_seed(0)
    net = DepthAnythingV2('vits', features=64, out_channels=[48, 96, 192, 384]).eval().cuda().half()
    rng = np.random.default_rng(2)
    frames = torch.from_numpy(rng.integers(0, 256, (5, 56, 84, 3), dtype=np.uint8))
    seen = []           # the predictions the pipeline itself consumed: two float16 forwards of the same frames are not
                        # bit-identical (the library GEMMs under them sum in arrival order, tools/determinism_check.py),
                        # and what this test pins is everything AFTER the network

    def predict(b):
        out = net.infer_batch(b, 70)
        seen.append(out.float().cpu())
        return out
    res = video_mode.gen_frames_sharded(frames, predict, {'stereo_modes': ['left-right']}, 'none', batch=2)
    assert set(res.keys()) == {'depth', 'left-right'} and tuple(res['left-right'].shape) == (5, 56, 168, 3)
    preds = torch.cat(seen).numpy()
    assert preds.shape[0] == 5
    again = torch.cat([net.infer_batch(frames[i:i + 2].cuda(), 70) for i in range(0, 5, 2)]).float().cpu().numpy()
    assert np.abs(again - preds).max() <= 2e-2 * np.abs(preds).max()
    norm = video_mode.process_predicitons([p for p in preds], 'none')
    for i in range(5):
        d16 = oracle.convert_to_i16(norm[i])
        assert np.array_equal(res['depth'][i].cpu().numpy(), d16)
        want = oracle.create_stereoimages_arrays(frames[i].numpy(), d16, 2.5, 0.0, ['left-right'], 0.0, 1.0, 'polylines_sharp')[0]
        assert np.array_equal(res['left-right'][i].cpu().numpy(), want)


@pytest.mark.parametrize("tag,kind", [("n", "zoedepth_n"), ("k", "zoedepth_k"), ("nk", "zoedepth_nk")])
def test_zoedepth_gpu_vs_reference_fp32(gpu, tag, kind):
    """ZoeDepth (ids 7, 8, 9; 8 and 9 run in half on a GPU, src/depthmap_generation.py:266-272) on the device against the outputs of
    the reference's own ZoeDepth code (tests/golden/zoedepth_cases.npz): float32 at north_star's 1e-4, float16 (fused kernels
    inside the DPT core) at 2e-2.  MEASURED (profiles/round5_parity_probe.json, tools/parity_probe.py): float32 6.5e-7 (N), 8.3e-7
    (K), 7.6e-7 (NK) -- the device is as close to the golden as the float64 evaluation of the same network is (8e-7 .. 1.1e-6), no
    stage above 1.1e-5; float16 2.9e-4 / 2.2e-3 / 2.6e-4, the same as the network's stock-torch half twin (3.0e-4 / 2.3e-3 /
    2.2e-4).  (Rounds 1-4 held 5e-4 / 5e-2 here without a measured value.)"""
    from dzoedepth import build_zoedepth
    z = np.load(os.path.join(os.path.dirname(GOLD), "zoedepth_cases.npz"))
    m, _ = build_zoedepth(kind, midas_model_type="DPT_BEiT_B_384")
    m = m.eval()
    m.load_state_dict(mw.fill_state_dict_zoe(m.state_dict()), strict=True)
    m = m.cuda()
    x = torch.rand((1, 3, 88, 120), generator=torch.Generator().manual_seed(21)).cuda()
    m.core.set_net_size(160, 128)
    ref = z[f"{tag}_88x120_infer"]
    with torch.no_grad():
        y32 = m.infer(x).cpu().numpy()
    e32 = np.abs(y32 - ref).max() / np.abs(ref).max()
    assert e32 < 1e-4, e32
    with torch.no_grad():
        y16 = m.half().infer(x.half()).float().cpu().numpy()
    assert np.isfinite(y16).all()
    e16 = np.abs(y16 - ref).max() / np.abs(ref).max()
    assert e16 < 2e-2, e16


def test_funnel_with_zoedepth(gpu):
    """ids 7 (float32 by the reference's rule) and 9 through ModelHolder / the funnel with random weights: plumbing only
    (PIL -> ToTensor scaling -> padded + flipped inference -> inverted depth -> uint16)."""
    from PIL import Image
    import src.core as core
    core.model_holder.allow_random_init = True
    try:
        rng = np.random.default_rng(3)
        img = Image.fromarray(rng.integers(0, 256, (96, 128, 3), dtype=np.uint8))
        for mt in (7, 9):
            got = list(core.core_generation_funnel(None, [img], None, None,
                                                   {'model_type': mt, 'net_width': 128, 'net_height': 96, 'net_size_match': False}))
            assert [k for _, k, _ in got] == ['depth']
            d = np.asarray(got[0][2])
            assert d.shape == (96, 128) and d.dtype == np.uint16 and d.max() > d.min()
            net = core.model_holder.depth_model.net
            assert next(net.parameters()).dtype == (torch.float32 if mt == 7 else torch.float16)
    finally:
        core.model_holder.allow_random_init = False
        core.model_holder.unload_models()


# ---- parity at the BENCHMARKED shapes ---------------------------------------------------------------------------------
GOLD_LARGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_cases_large.npz")


@pytest.mark.parametrize("b,n_valid,h,with_bias,dtype", [
    (32, 1025, 16, True, torch.float16),      # dpt_beit_large_512 at batch 32: the launch bench.py's roofline is quoted on
    (4, 2443, 16, False, torch.float16),      # Depth-Anything-V2 ViT-L on a 1080p frame (BASELINE config 5)
    (2, 4097, 16, True, torch.float16),       # dpt_beit_large_512 with NET_SIZE_MATCH at 1024^2 (net 1024)
    (2, 1025, 16, True, torch.bfloat16),
    (1, 577, 12, False, torch.float16),       # dpt_hybrid_384 (BASELINE config 2)
])
def test_attention_kernel_at_benchmark_shapes(gpu, b, n_valid, h, with_bias, dtype):
    """k_attention_fwd2 against its float32 definition (vit_mi355x.attention_reference, query-tiled so the B x H x N x N
    logits never exceed 1 GiB) at the exact launch shapes of the networks BASELINE.json names -- every batch element,
    every head, every valid row.  dmidas/backbones/beit.py:65-91, dinov2_layers/attention.py:49-62."""
    from src import vit_mi355x as vm
    from src import _native
    qk, vt, bias, npad = _case(b, n_valid, h, dtype, 1000 + n_valid, with_bias)
    packed, padded = None, None
    if bias is not None:
        packed = _native.attention_bias_pack(bias, npad, dtype)
        padded = torch.zeros((h, npad, npad), device='cuda')
        padded[:, :n_valid, :n_valid] = bias
    got = _native.attention_fwd(qk, vt, n_valid, 0.125, packed)
    # with a bias: its values (a few units) are rounded to the 11 / 8 bit operand type -- 4e-3 / 3e-2 of absolute error on a
    # logit, i.e. that relative error on a probability, times |V| ~ 3 at the 4 sigma tail of 5 * 10^8 outputs
    tol = (2e-3 if dtype == torch.float16 else 1.6e-2) if bias is None else (1e-2 if dtype == torch.float16 else 8e-2)
    worst = 0.0
    for b0 in range(0, b, 4):                       # the definition in float32, four batch elements at a time
        want = vm.attention_reference(qk[b0:b0 + 4].float(), vt[b0:b0 + 4].float(), n_valid, 0.125, padded)
        worst = max(worst, (got[b0:b0 + 4].float()[:, :n_valid] - want[:, :n_valid]).abs().max().item())
    assert worst < tol, (b, n_valid, h, with_bias, dtype, worst)
    assert torch.isfinite(got.float()).all()


def test_attention_rescale_branch_is_exercised(gpu):
    """The online softmax only rescales O when a running maximum moves; spike one key per 64-key tile so that every tile
    moves it for some query, and make the LAST tile hold the row maximum for others (cdna_hip_programming.md rule 26)."""
    from src import vit_mi355x as vm
    from src import _native
    qk, vt, _, npad = _case(2, 1025, 4, torch.float16, 77, False)
    for t in range(0, 1025, 64):
        qk[:, t + (t // 64) % 50, 1] *= 6.0          # a strong key in every tile, stronger towards the end
    qk[:, 1024, 1] = qk[:, 3, 0] * 3.0               # the last valid key matches query 3
    got = _native.attention_fwd(qk, vt, 1025, 0.125)
    want = vm.attention_reference(qk.float(), vt.float(), 1025, 0.125)
    assert (got.float()[:, :1025] - want[:, :1025]).abs().max().item() < 4e-3


def test_dpt_beit_large_512_forward_vs_reference(gpu):
    """dpt_beit_large_512 (BASELINE config 3's network, 24 blocks, 1025 tokens, relative-position bias) on the GPU against
    the float32 output of the reference's own dmidas code at the same size (make_golden_models_large.py):
    float32 at 1e-4 (north_star's depth tolerance), then float16 -- the precision bench.py runs and the reference's own GPU
    default (src/depthmap_generation.py:268-275) -- at 2e-2: fused attention with the packed bias, fused residual +
    LayerNorm, fused head tail."""
    from dmidas.dpt_depth import DPTDepthModel
    gold = np.load(GOLD_LARGE)
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    x = mw.synthetic_image((1, 3, 512, 512), seed=31).cuda()
    ref = gold["dpt_beitl512_512x512_out_s2"]
    m = m.cuda()
    with torch.no_grad():
        y32 = m(x)[:, ::2, ::2].cpu().numpy()
        taps = m.pretrained(x)
    scale = np.abs(ref).max()
    assert np.abs(y32 - ref).max() / scale < 1e-4, np.abs(y32 - ref).max() / scale
    t4 = taps[3][:, ::4].float().cpu().numpy()
    g4 = gold["dpt_beitl512_512x512_layer4_s"]
    assert np.abs(t4 - g4).max() / np.abs(g4).max() < 1e-4
    with torch.no_grad():
        y16 = m.half()(x.half().contiguous(memory_format=torch.channels_last))[:, ::2, ::2].float().cpu().numpy()
    assert np.abs(y16 - ref).max() / scale < 2e-2, np.abs(y16 - ref).max() / scale


def test_dpt_beit_large_512_net1024_forward_vs_reference(gpu):
    """The metric's network in its second form (NET_SIZE_MATCH on a 1024 x 1024 frame, net 1024, 4097 tokens; reference
    src/core.py:177-181, dmidas/backbones/beit.py:38-63 interpolate the relative-position tables to the 64 x 64 window) against the
    float32 output of the reference's own dmidas code at that size (tests/golden/make_golden_models_net1024.py): float32 at 1e-4,
    float16 -- what bench.py's c3match leg runs -- at 2e-2, plus the reassembled tap of block 23."""
    from dmidas.dpt_depth import DPTDepthModel
    gold = np.load(os.path.join(os.path.dirname(GOLD_LARGE), "model_cases_net1024.npz"))
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    x = mw.synthetic_image((1, 3, 1024, 1024), seed=33).cuda()
    ref = gold["dpt_beitl512_1024x1024_out_s4"]
    m = m.cuda()
    with torch.no_grad():
        y32 = m(x)[:, ::4, ::4].cpu().numpy()
        taps = m.pretrained(x)
    scale = np.abs(ref).max()
    assert np.abs(y32 - ref).max() / scale < 1e-4, np.abs(y32 - ref).max() / scale
    t4 = taps[3][:, ::4].float().cpu().numpy()
    g4 = gold["dpt_beitl512_1024x1024_layer4_s"]
    assert t4.shape == g4.shape and np.abs(t4 - g4).max() / np.abs(g4).max() < 1e-4
    del taps
    with torch.no_grad():
        y16 = m.half()(x.half().contiguous(memory_format=torch.channels_last))[:, ::4, ::4].float().cpu().numpy()
    assert np.abs(y16 - ref).max() / scale < 2e-2, np.abs(y16 - ref).max() / scale


def test_dav2_vitl_1080p_forward_vs_reference(gpu):
    """Depth-Anything-V2 ViT-L at 518 x 924 (a 1080p frame at input_size 518: 2443 tokens, BASELINE config 5) against the
    float32 outputs of the reference's own modules: encoder taps and depth, float32 at 1e-4 and float16 at 2e-2."""
    from ddepth_anything_v2 import DepthAnythingV2
    gold = np.load(GOLD_LARGE)
    m = DepthAnythingV2('vitl', features=256, out_channels=[256, 512, 1024, 1024]).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.cuda()
    x = mw.synthetic_image((1, 3, 518, 924), seed=32).cuda()
    ref = gold["dav2_vitl_518x924_out_s2"]
    scale = np.abs(ref).max()
    with torch.no_grad():
        y32 = m(x)[:, ::2, ::2].cpu().numpy()
        taps = m.pretrained.get_intermediate_layers(x, [4, 11, 17, 23], return_class_token=True)
    assert np.abs(y32 - ref).max() / scale < 1e-4, np.abs(y32 - ref).max() / scale
    for i, key in ((1, "dav2_vitl_518x924_tap1_s"), (3, "dav2_vitl_518x924_tap3_s")):
        g = gold[key]
        t = taps[i][0][:, ::8, ::4].float().cpu().numpy()
        assert np.abs(t - g).max() / np.abs(g).max() < 1e-4, (key, np.abs(t - g).max() / np.abs(g).max())
    with torch.no_grad():
        mh = m.half()
        y16 = mh(x.half())[:, ::2, ::2].float().cpu().numpy()
        t16 = mh.pretrained.get_intermediate_layers(x.half(), [4, 11, 17, 23], return_class_token=True)[3][0][:, ::8, ::4].float().cpu().numpy()
    g = gold["dav2_vitl_518x924_tap3_s"]
    assert np.abs(t16 - g).max() / np.abs(g).max() < 3e-2
    assert np.abs(y16 - ref).max() / scale < 2e-2, np.abs(y16 - ref).max() / scale


def test_leres_and_hybrid_gpu_fp32_vs_reference(gpu):
    """LeReS res101 (BatchNorm folded) and dpt_hybrid_384 on the GPU in float32 against the reference modules' outputs
    (tests/golden/model_cases.npz), 1e-4; dpt_hybrid also in float16 (BASELINE config 2's precision) at 2e-2."""
    from dmidas.dpt_depth import DPTDepthModel
    from lib.multi_depth_model_woauxi import RelDepthModel
    gold = np.load(GOLD)
    m = RelDepthModel(backbone='resnext101').eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    x5 = mw.synthetic_image((2, 3, 96, 160), seed=15).cuda()
    with torch.no_grad():
        y = m.cuda().depth_model(x5).cpu().numpy()
    ref = gold["leres_96x160_out"]
    assert np.abs(y - ref).max() / np.abs(ref).max() < 1e-4, np.abs(y - ref).max() / np.abs(ref).max()
    m = DPTDepthModel(path=None, backbone="vitb_rn50_384", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    x4 = mw.synthetic_image((2, 3, 160, 224), seed=14).cuda()
    ref = gold["dpt_hybrid_160x224_out"]
    with torch.no_grad():
        y32 = m.cuda()(x4).cpu().numpy()
    assert np.abs(y32 - ref).max() / np.abs(ref).max() < 1e-4, np.abs(y32 - ref).max() / np.abs(ref).max()
    # float16: this network with name-seeded weights loses 4-5e-2 in half precision WHATEVER runs it -- measured (profiles/
    # round5_parity_probe.json): in-tree kernels 4.1e-2 / 4.8e-2 (two runs: the library's split-K convolutions are not
    # bit-reproducible), every GEMM / convolution through the libraries 4.6e-2, the stock-torch twin (no in-tree kernel at all:
    # the arithmetic the reference's own modules run in half) 4.8e-2; stage by stage the two agree (the four taps: 4e-3, 1.4e-2,
    # 7.9e-2, 7.0e-2 against 5e-3, 1.7e-2, 7.5e-2, 6.9e-2: the loss is made inside the ViT-B blocks on the ResNetV2 stem's
    # output, by half precision itself).  The 2e-2 rule therefore cannot hold for this network; the bar is the stock twin's own
    # error with a margin for the run-to-run spread, and 2e-2 wherever the stock twin itself meets it.
    from src import vit_mi355x as vm
    mh = m.half()
    xh = x4.half().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y16 = mh(xh).float().cpu().numpy()
        with vm.stock_routing():
            y16_stock = mh(xh).float().cpu().numpy()
    e16 = np.abs(y16 - ref).max() / np.abs(ref).max()
    e16_stock = np.abs(y16_stock - ref).max() / np.abs(ref).max()
    print(f"dpt_hybrid float16 vs the reference's float32 output: in-tree {e16:.3e}, stock-torch half twin {e16_stock:.3e}")
    assert e16 < max(2e-2, 1.3 * e16_stock), (e16, e16_stock)
    assert e16_stock < 1e-1, e16_stock                      # the yardstick itself is a half-precision forward, not garbage


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_reassemble_readout_kernel(gpu, dtype, tol):
    """ds_reassemble_readout against its definition, and ProjectReadout (split GEMM + fused epilogue) against the
    reference's formulation cat(tokens, cls) -> Linear(2C -> C) -> GELU (dmidas/backbones/utils.py:28-39)."""
    from src import _native
    from dmidas.backbones.beit import ProjectReadout
    g = torch.Generator().manual_seed(12)
    for (b, n, c) in [(2, 5, 64), (3, 1025, 1024), (1, 577, 768)]:
        proj = torch.randn((b, n, c), generator=g).to(dtype).cuda()
        cls = torch.randn((b, c), generator=g).to(dtype).cuda()
        got = _native.reassemble_readout(proj, cls)
        want = torch.nn.functional.gelu((proj[:, 1:].float() + cls[:, None].float()).to(dtype).float())
        assert tuple(got.shape) == (b, n - 1, c)
        assert (got.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())
    torch.manual_seed(5)
    ro = ProjectReadout(256).cuda()
    x = torch.randn((2, 101, 256), device='cuda')
    with torch.no_grad():
        ref = ro.project(torch.cat((x[:, 1:], x[:, 0].unsqueeze(1).expand_as(x[:, 1:])), -1))     # the reference's forward
        y32 = ro(x)
        y16 = ro.to(dtype)(x.to(dtype)).float()
    assert (y32 - ref).abs().max().item() < 1e-5 * (1 + ref.abs().max().item())
    assert (y16 - ref).abs().max().item() < 4 * tol * (1 + ref.abs().max().item())


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_bias_act_kernel_and_residual_conv_unit(gpu, dtype, tol):
    """ds_bias_act_nhwc against its definition (all optional operands, in place and out of place), and the fused residual
    convolution unit against the reference's sequence conv(relu) -> conv(relu) -> + x (dmidas/blocks.py:352-377) in float32."""
    import torch.nn as nn
    import torch.nn.functional as F
    from src import _native
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(21)
    for (b, c, h, w) in [(2, 64, 5, 7), (1, 256, 33, 17), (3, 8, 4, 4)]:
        mk = lambda: torch.randn((b, c, h, w), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
        x, r1, r2 = mk(), mk(), mk()
        bias = torch.randn(c, generator=g).to(dtype).cuda()
        for relu in (False, True):
            for a, bb in ((None, None), (r1, None), (r1, r2)):
                want = x.float() + bias.float().view(1, -1, 1, 1)
                if a is not None:
                    want = want + a.float()
                if bb is not None:
                    want = want + bb.float()
                if relu:
                    want = F.relu(want)
                got = _native.bias_act(x, bias, relu=relu, res1=a, res2=bb, inplace=False)
                assert got.is_contiguous(memory_format=torch.channels_last)
                assert (got.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())
        y = x.clone(memory_format=torch.channels_last)
        assert _native.bias_act(y, bias, relu=True).data_ptr() == y.data_ptr()
        assert torch.equal(y, _native.bias_act(x, bias, relu=True, inplace=False))
    torch.manual_seed(3)
    c1, c2 = nn.Conv2d(64, 64, 3, padding=1).cuda(), nn.Conv2d(64, 64, 3, padding=1).cuda()
    x = torch.randn((2, 64, 19, 23), device='cuda')
    skip = torch.randn((2, 64, 19, 23), device='cuda')
    with torch.no_grad():
        ref = c2(F.relu(c1(F.relu(x)))) + x
        got32 = vm.residual_conv_unit(c1, c2, x)
        assert (got32 - ref).abs().max().item() < 1e-5 * (1 + ref.abs().max().item())
        c1h, c2h = c1.to(dtype), c2.to(dtype)
        xh = x.to(dtype).contiguous(memory_format=torch.channels_last)
        got = vm.residual_conv_unit(c1h, c2h, xh).float()
        got_s = vm.residual_conv_unit(c1h, c2h, xh, skip=skip.to(dtype)).float()
    assert (got - ref).abs().max().item() < 6 * tol * (1 + ref.abs().max().item())
    assert (got_s - (ref + skip)).abs().max().item() < 6 * tol * (1 + ref.abs().max().item())


def test_hip_graph_replay_equals_eager_forward(gpu):
    """src/hip_graph.GraphedForward: the captured-and-replayed forward (fused attention, residual+LN, read-out, decoder tails,
    head tail and the library kernels inside one hipGraph) returns what the eager forward returns, for new inputs too, and a
    second shape gets its own graph; through ModelHolder's `hip_graphs` setting as well."""
    from ddepth_anything_v2 import DepthAnythingV2
    from dmidas.dpt_depth import DPTDepthModel
    from src.hip_graph import GraphedForward
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(4)
    for net, call in ((DepthAnythingV2('vits', features=64, out_channels=[48, 96, 192, 384]).eval().cuda().half(),
                       lambda m, x: m.infer_batch(x, 70)),
                      (DPTDepthModel(path=None, backbone="vitb_rn50_384", non_negative=True).eval().cuda().half(),
                       lambda m, x: m.infer_batch(x, net_size=128, net_h=96))):
        gf = GraphedForward(lambda x, net=net, call=call: call(net, x))
        for shape in ((1, 96, 128, 3), (1, 96, 128, 3), (2, 64, 96, 3), (1, 96, 128, 3)):
            x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()
            # The library kernels under these small float16 networks are not bit-reproducible run to run (stream-K GEMMs sum
            # in arrival order; measured by tools/determinism_check.py with every in-tree kernel switched off as well: 1e-3 of
            # the maximum for the ViT, 1-7 % for the random-init hybrid, which amplifies it), and inside a capture MIOpen
            # falls back to solvers that need no workspace.  So: the eager noise floor is measured here, and a replay has to
            # agree with the eager forward within a few times that floor -- and follow its input (no stale static buffers).
            runs = [call(net, x) for _ in range(4)]
            want = runs[0]
            noise = max((r - want).abs().max().item() for r in runs[1:])
            tol = 5 * noise + 2e-2 * want.abs().max().item()
            got = gf(x)
            assert got.shape == want.shape and torch.isfinite(got).all()
            assert (got - want).abs().max().item() <= tol, (shape, noise)
            assert (gf(x) - got).abs().max().item() <= tol, (shape, noise)
            x2 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()
            got2 = gf(x2)
            assert (got2 - call(net, x2)).abs().max().item() <= tol, (shape, noise)
            assert (got2 - got).abs().mean().item() > 0
        # every shape was either captured (and validated at capture) or, if the library misbehaved inside the capture, left eager
        assert len(gf.graphs) + len(gf.failed) == 2
        # at most max_graphs shapes keep a graph (each holds its activations' memory pool): the least recently used one is dropped
        gm = GraphedForward(lambda x, net=net, call=call: call(net, x), max_graphs=2)
        for shape in ((1, 96, 128, 3), (1, 64, 96, 3), (1, 96, 128, 3), (1, 128, 160, 3)):
            gm(torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda())
            assert len(gm.graphs) <= 2
        assert (1, 64, 96, 3) not in [k[0] for k in gm.graphs] or len(gm.failed) > 0
        # lazy = 2 (ModelHolder.hip_graphs = "auto", the default): a shape runs eager twice and is captured on its third use
        gl = GraphedForward(lambda x, net=net, call=call: call(net, x), lazy=2)
        x = torch.randint(0, 256, (1, 96, 128, 3), generator=g, dtype=torch.uint8).cuda()
        want = call(net, x)
        for i in range(4):
            got = gl(x)
            assert len(gl.graphs) + len(gl.failed) == (1 if i >= 2 else 0), i
            assert (got - want).abs().max().item() <= 5 * noise + 2e-2 * want.abs().max().item()


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 1.5e-3), (torch.bfloat16, 1.2e-2)])
def test_linear_kernel_matches_float32_and_is_race_free(gpu, dtype, tol):
    """ds_linear (csrc/ds_linear.hip: 256x256 MFMA tiles, LDS-DMA staging, 8-phase K loop, fused bias / erf-GELU) against
    x @ W.T + b [-> GELU] in float32 on the SAME rounded operands.  Shapes cover: one K iteration (K = 128), odd numbers
    of iterations, a ragged last row panel, rows < 256, no bias, several column panels, and the encoder shapes of
    dpt_beit_large_512 (fc1 at one image).  The kernel's synchronisation is counted waits + barriers: a race would show
    as run-to-run differences, so every launch is repeated and must be bit-identical."""
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(31)
    cases = [(256, 256, 128, True, True), (300, 256, 384, True, False), (77, 512, 256, False, True),
             (1088, 4096, 1024, True, True), (1088, 1024, 4096, True, False), (2443, 768, 640, False, False),
             (4352, 2048, 1024, True, False)]
    for (m, n, k, has_bias, gelu) in cases:
        x = torch.randn((m, k), generator=g).to(dtype).cuda()
        w = (torch.randn((n, k), generator=g) * k ** -0.5).to(dtype).cuda()
        b = torch.randn(n, generator=g).to(dtype).cuda() if has_bias else None
        want = x.double() @ w.double().T
        if has_bias:
            want = want + b.double()
        if gelu:
            want = F.gelu(want)
        got = _native.linear(x, w, b, gelu)
        assert got.shape == (m, n) and got.dtype == dtype
        err = (got.double() - want).abs().max().item()
        assert err < tol * (1 + want.abs().max().item()), (m, n, k, has_bias, gelu, err)
        for _ in range(3):
            assert torch.equal(_native.linear(x, w, b, gelu), got), "run-to-run difference: a race in the K loop"
    # the workgroups are persistent (one per CU, each walking a strided list of tiles): a grid of 8 makes every workgroup
    # walk many tiles, with the next tile's prologue issued behind the previous epilogue
    import os
    _native.linear_env(DS_LIN_GRID="8")
    try:
        for (m, n, k, has_bias, gelu) in [(2443, 768, 640, True, True), (4352, 2048, 1024, True, False)]:
            x = torch.randn((m, k), generator=g).to(dtype).cuda()
            w = (torch.randn((n, k), generator=g) * k ** -0.5).to(dtype).cuda()
            b = torch.randn(n, generator=g).to(dtype).cuda()
            want = x.double() @ w.double().T + b.double()
            want = F.gelu(want) if gelu else want
            got = _native.linear(x, w, b, gelu)
            assert (got.double() - want).abs().max().item() < tol * (1 + want.abs().max().item()), (m, n, k)
            assert torch.equal(_native.linear(x, w, b, gelu), got)
    finally:
        _native.linear_env(DS_LIN_GRID=None)
    # a 3-D input and a strided (sliced) weight go through the same entry point
    x3 = torch.randn((2, 130, 256), generator=g).to(dtype).cuda()
    wbig = torch.randn((768, 256), generator=g).to(dtype).cuda()
    got = _native.linear(x3, wbig[:512], None, False)
    want = x3.double() @ wbig[:512].double().T
    assert got.shape == (2, 130, 512) and (got.double() - want).abs().max().item() < tol * (1 + want.abs().max().item())
    # argument errors are reported, not launched
    with pytest.raises(AssertionError):
        _native.linear(x3, wbig[:300], None, False)


def test_linear_gelu_polynomial_against_erf_everywhere(gpu):
    """The fused GELU is a polynomial/exp2 evaluation of the erf form, not the tanh approximation: on a dense sweep of
    pre-activations (identity weight, bias carries the value) it must stay within 1 float16 ulp of erf-GELU computed in
    float64, and agree exactly on > 99.8 % of the sweep."""
    import torch.nn.functional as F
    from src import _native
    n = 256
    w = torch.eye(n, 128, dtype=torch.float16).cuda()                  # x = 0 -> the accumulator is exactly the bias
    x = torch.zeros((256, 128), dtype=torch.float16).cuda()
    vals = torch.cat([torch.linspace(-9, 9, 256 * 255), torch.tensor([0.0] * 256)]).view(256, n)
    bad = 0
    for r in range(vals.shape[0]):
        b = vals[r].half().cuda()
        got = _native.linear(x, w, b, True)[0]
        want = F.gelu(b.double()).half()
        ulp = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
        assert ulp.max().item() <= 1, (r, ulp.max().item())
        bad += int((ulp != 0).sum().item())
    assert bad / vals.numel() < 2e-3, bad


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_conv3x3_kernel_matches_float32_convolution(gpu, dtype, tol):
    """ds_conv3x3_nhwc (the implicit GEMM of csrc/ds_linear.hip) against F.conv2d in float32 on the same rounded operands:
    image borders inside and across 256-pixel tiles, several images per tile, ragged last tile, 128 / 256 / 512 input
    channels, no bias (scratch.layerN_rn), bias + ReLU (first half of a residual unit), bias + residual + skip (second
    half); repeated launches must be bit-identical."""
    import torch.nn as nn
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(41)
    # (out_channels 128 / 384: the 256 x 128 tiles of the head's 256 -> 128 convolution -- no residual operands there)
    cases = [(1, 16, 16, 128, 256, False), (2, 19, 23, 256, 256, True), (3, 11, 9, 256, 512, True), (1, 40, 33, 512, 256, False),
             (2, 19, 23, 256, 128, True), (1, 40, 33, 128, 384, False), (3, 17, 16, 256, 128, True)]
    for (b, h, w, cin, cout, has_bias) in cases:
        conv = nn.Conv2d(cin, cout, 3, padding=1, bias=has_bias).cuda()
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (9 * cin) ** -0.5)
            if has_bias:
                conv.bias.copy_(torch.randn(cout, generator=g))
        mk = lambda c: torch.randn((b, c, h, w), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
        x, r1, r2 = mk(cin), mk(cout), mk(cout)
        wq = conv.weight.detach().to(dtype).float()
        bq = None if not has_bias else conv.bias.detach().to(dtype).float()
        base = F.conv2d(x.float(), wq, bq, padding=1)
        for relu, a, bb in ((False, None, None), (True, None, None), (False, r1, r2), (True, r1, None)):
            if cout % 256 != 0 and a is not None:
                continue
            want = base
            if a is not None:
                want = want + a.float()
            if bb is not None:
                want = want + bb.float()
            if relu:
                want = F.relu(want)
            got = _native.conv3x3(conv, x, relu=relu, res1=a, res2=bb)
            assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
            err = (got.float() - want).abs().max().item()
            assert err < tol * (1 + want.abs().max().item()), (b, h, w, cin, cout, relu, err)
            assert torch.equal(_native.conv3x3(conv, x, relu=relu, res1=a, res2=bb), got)
        if cout % 256 == 0:
            # round 6: conv(relu(x)) with the maximum taken on the MFMA fragments inside the K loop (act 6) -- the same bits as
            # the convolution of a rectified copy of x, signed zeros and the zero padding ring included
            xz = x.clone()
            flat = xz.permute(0, 2, 3, 1).reshape(-1)           # a view of the channels_last memory
            flat[::7] = -0.0
            flat[3::11] = 0.0
            got = _native.conv3x3(conv, xz, relu=True, relu_in=True)
            assert torch.equal(got, _native.conv3x3(conv, F.relu(xz), relu=True)), (b, h, w, cin, cout)
            want = F.relu(F.conv2d(F.relu(xz.float()), wq, bq, padding=1))
            assert (got.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())
    import os
    _native.linear_env(DS_LIN_GRID="8")                 # persistent workgroups walking many tiles (see the linear test)
    try:
        conv = nn.Conv2d(256, 256, 3, padding=1).cuda()
        xr = torch.randn((2, 256, 37, 41), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
        assert torch.equal(_native.conv3x3(conv, xr, relu=True, relu_in=True), _native.conv3x3(conv, F.relu(xr), relu=True))
        x = torch.randn((2, 256, 37, 41), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
        r1 = torch.randn((2, 256, 37, 41), generator=g).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
        want = F.relu(F.conv2d(x.float(), conv.weight.detach().to(dtype).float(), conv.bias.detach().to(dtype).float(), padding=1) + r1.float())
        got = _native.conv3x3(conv, x, relu=True, res1=r1)
        assert (got.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())
        assert torch.equal(_native.conv3x3(conv, x, relu=True, res1=r1), got)
    finally:
        _native.linear_env(DS_LIN_GRID=None)
    # the residual unit of the decoders at a size that takes the in-tree path (both convolutions + fused tails)
    from src import vit_mi355x as vm
    torch.manual_seed(5)
    c1, c2 = nn.Conv2d(256, 256, 3, padding=1).cuda(), nn.Conv2d(256, 256, 3, padding=1).cuda()
    x = torch.randn((2, 256, 128, 128), device='cuda')
    skip = torch.randn((2, 256, 128, 128), device='cuda')
    want = skip + (c2(F.relu(c1(F.relu(x)))) + x)
    xh = x.to(dtype).contiguous(memory_format=torch.channels_last)
    assert vm.conv3x3_hip_ok(c1.to(dtype), xh)
    got = vm.residual_conv_unit(c1.to(dtype), c2.to(dtype), xh, skip=skip.to(dtype))
    assert (got.float() - want).abs().max().item() < 4 * tol * (1 + want.abs().max().item())


@pytest.mark.parametrize("m,n,k,gelu", [(33024, 4096, 1024, True), (33024, 1024, 4096, False), (33024, 2048, 1024, False),
                                        (33024, 1024, 1024, False), (34816, 4096, 1024, True), (34816, 2048, 1024, False)])
def test_linear_kernel_at_benchmark_shapes(gpu, m, n, k, gelu):
    """ds_linear at the shapes ONE encoder block of dpt_beit_large_512 launches at batch 32 (the bench's step): 33 024 rows
    = 32 x 1032 = 129 row panels with the tight token pad (round 4; rounds 1-3 padded to 1088: 34 816 rows = 136 panels),
    i.e. the whole XCD-aware tile list of ~2 000 tiles over all 256 persistent workgroups (the smaller tests walk at most
    17 panels).  Every element against a float32 GEMM of the same rounded operands."""
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(m + n + k)
    x = torch.randn((m, k), generator=g).half().cuda()
    w = (torch.randn((n, k), generator=g) * k ** -0.5).half().cuda()
    b = torch.randn(n, generator=g).half().cuda()
    got = _native.linear(x, w, b, gelu)
    assert got.shape == (m, n) and got.dtype == torch.float16
    worst, scale = 0.0, 0.0
    wf, bf = w.float(), b.float()
    for r0 in range(0, m, 4352):
        want = x[r0:r0 + 4352].float() @ wf.T + bf
        want = F.gelu(want) if gelu else want
        worst = max(worst, (got[r0:r0 + 4352].float() - want).abs().max().item())
        scale = max(scale, want.abs().max().item())
    assert worst < 1.5e-3 * (1 + scale), (m, n, k, worst, scale)
    assert torch.equal(_native.linear(x, w, b, gelu), got), "run-to-run difference at the benchmark shape"


def test_conv3x3_kernel_at_benchmark_shape(gpu):
    """ds_conv3x3_nhwc at refinenet1's shape in the bench's step: 32 x 128 x 128, 256 -> 256, bias + residual
    (2 048 tiles), every output against F.conv2d in float32 on the same rounded operands."""
    import torch.nn as nn
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(43)
    conv = nn.Conv2d(256, 256, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 2304 ** -0.5)
        conv.bias.copy_(torch.randn(256, generator=g))
    mk = lambda: torch.randn((32, 256, 128, 128), generator=g).half().cuda().contiguous(memory_format=torch.channels_last)  # noqa: E731
    x, r1 = mk(), mk()
    got = _native.conv3x3(conv.half(), x, relu=False, res1=r1)
    wq, bq = conv.weight.detach().float(), conv.bias.detach().float()
    worst, scale = 0.0, 0.0
    for i in range(0, 32, 4):
        want = F.conv2d(x[i:i + 4].float(), wq, bq, padding=1) + r1[i:i + 4].float()
        worst = max(worst, (got[i:i + 4].float() - want).abs().max().item())
        scale = max(scale, want.abs().max().item())
    assert worst < 2e-3 * (1 + scale), (worst, scale)
    assert torch.equal(_native.conv3x3(conv, x, relu=False, res1=r1), got)


def test_conv3x3_head_convolution_at_benchmark_shape(gpu):
    """The head's first convolution (dmidas/dpt_depth.py:150: 256 -> 128, bias, no activation) at the bench's shape, 32 x 256 x
    256: 8 192 tiles of 256 x 128 on a persistent grid (small grid too: many tiles per workgroup, the early prologue's store
    count is 8 here), every output against F.conv2d in float32 on the same rounded operands."""
    import torch.nn as nn
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(47)
    conv = nn.Conv2d(256, 128, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 2304 ** -0.5)
        conv.bias.copy_(torch.randn(128, generator=g))
    conv = conv.half()
    x = torch.randn((32, 256, 256, 256), generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    wq, bq = conv.weight.detach().float(), conv.bias.detach().float()
    outs = []
    for grid, early in ((None, "1"), ("16", "1"), ("16", "0")):
        _native.linear_env(DS_LIN_GRID=grid, DS_LIN_EARLY=early)
        got = _native.conv3x3(conv, x)
        outs.append(got)
        assert torch.equal(_native.conv3x3(conv, x), got)
    _native.linear_env(DS_LIN_GRID=None, DS_LIN_EARLY=None)
    assert all(torch.equal(o, outs[0]) for o in outs[1:]), "grid size / prologue order changed the values"
    worst, scale = 0.0, 0.0
    for i in range(0, 32, 4):
        want = F.conv2d(x[i:i + 4].float(), wq, bq, padding=1)
        worst = max(worst, (outs[0][i:i + 4].float() - want).abs().max().item())
        scale = max(scale, want.abs().max().item())
    assert worst < 2e-3 * (1 + scale), (worst, scale)


def test_infer_batch_gpu_vs_reference_get_raw_prediction(gpu):
    """uint8 image -> depth at image size ON THE DEVICE (pre-resize + normalise + forward + bicubic / bilinear back, SURVEY
    8f-1) against the reference's own ModelHolder.get_raw_prediction -> estimatemidas / estimatedepthanything_v2 run on the
    CPU in float32 (tests/golden/make_golden_infer.py; src/depthmap_generation.py:375-403,455-499,548-559): float32 at 1e-4,
    float16 (the reference's GPU default) at 2e-2, also through the product's ModelHolder-level predictor with a batch of 2."""
    import make_golden_infer as mgi
    from ddepth_anything_v2 import DepthAnythingV2
    from dmidas.dpt_depth import DPTDepthModel
    z = np.load(os.path.join(os.path.dirname(GOLD), "infer_cases.npz"))
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    m = DPTDepthModel(path=None, backbone="beitb16_384", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    m = m.cuda()
    for name, h, w, nw, nh, seed in mgi.MIDAS_CASES:
        img = torch.from_numpy(z[f"midas__{name}__image"]).cuda()
        got = m.infer_batch(img[None], net_size=nw, resize_mode="minimal", net_h=nh)[0].cpu().numpy()
        assert got.shape == (h, w) and rel(got, z[f"midas__{name}__pred"]) < 1e-4, (name, rel(got, z[f"midas__{name}__pred"]))
        both = m.infer_batch(torch.stack([img, img.flip(0)]), net_size=nw, resize_mode="minimal", net_h=nh)
        assert rel(both[0].cpu().numpy(), z[f"midas__{name}__pred"]) < 1e-4
    m16 = m.half()
    for name, h, w, nw, nh, seed in mgi.MIDAS_CASES:
        img = torch.from_numpy(z[f"midas__{name}__image"]).cuda()
        got = m16.infer_batch(img[None], net_size=nw, resize_mode="minimal", net_h=nh)[0].cpu().numpy()
        assert rel(got, z[f"midas__{name}__pred"]) < 2e-2, (name, rel(got, z[f"midas__{name}__pred"]))
    d = DepthAnythingV2('vits', features=64, out_channels=[48, 96, 192, 384]).eval()
    d.load_state_dict(mw.fill_state_dict(d.state_dict()), strict=True)
    d = d.cuda()
    for name, h, w, size, seed in mgi.DAV2_CASES:
        img = torch.from_numpy(z[f"dav2__{name}__image"]).cuda()
        got = d.infer_batch(img[None], size)[0].cpu().numpy()
        assert got.shape == (h, w) and rel(got, z[f"dav2__{name}__pred"]) < 1e-4, (name, rel(got, z[f"dav2__{name}__pred"]))
    d16 = d.half()
    for name, h, w, size, seed in mgi.DAV2_CASES:
        img = torch.from_numpy(z[f"dav2__{name}__image"]).cuda()
        got = d16.infer_batch(img[None], size)[0].cpu().numpy()
        assert rel(got, z[f"dav2__{name}__pred"]) < 2e-2, (name, rel(got, z[f"dav2__{name}__pred"]))


def _lin_ref(x, w, b=None, gamma=None, res=None, gelu=False):
    import torch.nn.functional as F
    y = x.double() @ w.double().T
    if b is not None:
        y = y + b.double()
    if gelu:
        y = F.gelu(y)
    if gamma is not None:
        y = y * gamma.double()
    if res is not None:
        y = y + res.double()
    return y


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 1.5e-3), (torch.bfloat16, 1.2e-2)])
def test_linear_ragged_round_vt_and_fused_residual(gpu, dtype, tol):
    """The pieces of csrc/ds_linear.hip added in round 3, at small sizes with a small persistent grid (DS_LIN_GRID) so that
    every path is taken: k_linear_ragged (the last, nearly empty round of tiles rendered as 128 x 64 pieces, one LDS-staged
    GEMM per workgroup; some shapes here also take its two-way K split) behind plain / GELU / LayerScale + residual epilogues, a
    shifted last row panel, K = 128 (two K-tiles); ds_linear_vt (V^T written per batch element by the epilogue) with and without
    a ragged round.  Against float64 on the same rounded operands; repeated launches bit-identical; ragged on == ragged off
    to rounding."""
    import os
    from src import _native
    g = torch.Generator().manual_seed(77)
    mk = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    old = {k: os.environ.get(k) for k in ("DS_LIN_GRID", "DS_LIN_RAGGED", "DS_LIN_EARLY", "DS_LIN_RAGGED_RING", "DS_LIN_RAGGED_PIPE", "DS_LIN_RAGGED_THIN")}
    try:
        # (rows, out, in, grid): tiles % grid <= grid / 4 -> a ragged round of 1 .. 4 tiles
        # (2304, 512, ..) and (2100, 512, ..): the ragged round is the last row panel alone -> k_linear_thin (round 6: 32 x 64 pieces, two
        # K-tiles per step; full panel / 52 new rows in two 32-row blocks, the first reaching into the main rounds' rows; odd step count)
        for (m, n, k, grid) in [(4352, 256, 384, 8), (2304, 512, 1024, 8), (2637, 768, 640, 16), (4352, 256, 128, 8), (8448, 256, 256, 32),
                                (2100, 512, 384, 8), (2304, 256, 128, 8)]:
            _native.linear_env(DS_LIN_GRID=str(grid))
            x, w, b = mk(m, k).to(dtype).cuda(), (mk(n, k) * k ** -0.5).to(dtype).cuda(), mk(n).to(dtype).cuda()
            gam, res = mk(n).to(dtype).cuda(), mk(m, n).to(dtype).cuda()
            for gelu in (False, True):
                want = _lin_ref(x, w, b, gelu=gelu)
                _native.linear_env(DS_LIN_RAGGED="1")
                got = _native.linear(x, w, b, gelu)
                assert (got.double() - want).abs().max().item() < tol * (1 + want.abs().max().item()), (m, n, k, gelu)
                assert torch.equal(_native.linear(x, w, b, gelu), got), "ragged round: run-to-run difference"
                _native.linear_env(DS_LIN_RAGGED="0")
                off = _native.linear(x, w, b, gelu)
                assert (got.double() - off.double()).abs().max().item() < tol * (1 + want.abs().max().item())
                # the two schedules differ only in the summation order of the ragged tiles: most outputs are bit-identical
                assert (got != off).float().mean().item() < 0.2
                assert torch.equal(got, off), "the ragged round and the main rounds sum in different orders"      # round 6: one chain
                _native.linear_env(DS_LIN_RAGGED="1", DS_LIN_RAGGED_THIN="0")
                assert torch.equal(_native.linear(x, w, b, gelu), got), "k_linear_thin differs from k_linear_ragged"
                _native.linear_env(DS_LIN_RAGGED_THIN=None)
            _native.linear_env(DS_LIN_RAGGED="1")
            for gm in (gam, None):
                want = _lin_ref(x, w, b, gamma=gm, res=res)
                got = _native.linear_residual(x, w, b, gm, res)
                assert (got.double() - want).abs().max().item() < tol * (1 + want.abs().max().item()), (m, n, k, gm is None)
                assert torch.equal(_native.linear_residual(x, w, b, gm, res), got)
                _native.linear_env(DS_LIN_RAGGED_THIN="0")
                assert torch.equal(_native.linear_residual(x, w, b, gm, res), got), "k_linear_thin differs from k_linear_ragged"
                _native.linear_env(DS_LIN_RAGGED_THIN=None)
        # schedule switches that must not change a single bit: the order of prologue DMAs and epilogue (DS_LIN_EARLY), the ring
        # depth of the ragged kernel -- on a many-tiles-per-workgroup walk with every epilogue variant
        _native.linear_env(DS_LIN_GRID="8")
        x, w, b = mk(4352, 384).to(dtype).cuda(), (mk(256, 384) * 384 ** -0.5).to(dtype).cuda(), mk(256).to(dtype).cuda()
        gam, res = mk(256).to(dtype).cuda(), mk(4352, 256).to(dtype).cuda()
        outs = []
        import torch.nn as nn
        hv, wv = mk(4, 320, 256).to(dtype).cuda(), (mk(512, 256) * 256 ** -0.5).to(dtype).cuda()
        cv = nn.Conv2d(128, 256, 3, padding=1).to(dtype).cuda()
        xc, rc = (mk(2, c, 37, 41).to(dtype).cuda().contiguous(memory_format=torch.channels_last) for c in (128, 256))
        for early, ring, pipe in (("1", "3", "1"), ("0", "3", "1"), ("1", "6", "1"), ("0", "6", "1"), ("1", "6", "0")):
            _native.linear_env(DS_LIN_EARLY=early, DS_LIN_RAGGED_RING=ring, DS_LIN_RAGGED_PIPE=pipe)
            # every epilogue variant whose store count the early prologue's waits rely on: GELU, plain without a bias, LayerScale +
            # residual, V^T, convolution with ReLU and with two residual operands
            outs.append((_native.linear(x, w, b, True), _native.linear(x, w, None, False), _native.linear_residual(x, w, b, gam, res),
                         _native.linear_vt(wv, hv), _native.conv3x3(cv, xc, relu=True), _native.conv3x3(cv, xc, res1=rc, res2=rc)))
        _native.linear_env(DS_LIN_EARLY=None, DS_LIN_RAGGED_RING=None, DS_LIN_RAGGED_PIPE=None)
        for o in outs[1:]:
            assert all(torch.equal(a, c) for a, c in zip(o, outs[0])), "DS_LIN_EARLY / ring depth changed the values"
        assert (outs[0][1].double() - _lin_ref(x, w)).abs().max().item() < tol * 10
        # V^T: [B, C, Np] out of h [B, Np, K]; (B, Np, C, K, grid)
        for (bb, npad, c, k, grid) in [(4, 320, 512, 256, 8), (2, 640, 256, 384, 256), (6, 128, 768, 128, 8)]:
            _native.linear_env(DS_LIN_GRID=str(grid))
            h, wv = mk(bb, npad, k).to(dtype).cuda(), (mk(c, k) * k ** -0.5).to(dtype).cuda()
            assert _native.linear_vt_supported(wv, h)
            want = torch.einsum("ck,bnk->bcn", wv.double(), h.double())
            got = _native.linear_vt(wv, h)
            assert got.shape == (bb, c, npad) and got.is_contiguous()
            assert (got.double() - want).abs().max().item() < tol * (1 + want.abs().max().item()), (bb, npad, c, k)
            assert torch.equal(_native.linear_vt(wv, h), got)
    finally:
        for k_, v in old.items():
            _native.linear_env(**{k_: v})


@pytest.mark.parametrize("npad", [1032, 1088])
def test_linear_vt_and_fused_fc2_at_benchmark_shapes(gpu, npad):
    """ds_linear_vt and ds_linear_residual at the shapes of ONE encoder block of dpt_beit_large_512 at batch 32 -- token stride
    1032 (round 4's tight pad: 516 tiles = two full rounds on 256 CUs + a ragged round of 4 tiles) and 1088 (544 tiles: + 32)
    -- every element against float32 on the same rounded operands."""
    from src import _native
    g = torch.Generator().manual_seed(91)
    rows = 32 * npad
    h = torch.randn((32, npad, 1024), generator=g).half().cuda()
    wv = (torch.randn((1024, 1024), generator=g) / 32).half().cuda()
    got = _native.linear_vt(wv, h)
    worst = 0.0
    for b in range(32):
        want = wv.float() @ h[b].float().T
        worst = max(worst, (got[b].float() - want).abs().max().item() / (1 + want.abs().max().item()))
    assert worst < 1.5e-3, worst
    assert torch.equal(_native.linear_vt(wv, h), got)
    a = torch.randn((rows, 4096), generator=g).half().cuda()
    w2 = (torch.randn((1024, 4096), generator=g) / 64).half().cuda()
    b2, gam = torch.randn(1024, generator=g).half().cuda(), torch.randn(1024, generator=g).half().cuda()
    res = torch.randn((rows, 1024), generator=g).half().cuda()
    got = _native.linear_residual(a, w2, b2, gam, res)
    worst = 0.0
    for r0 in range(0, rows, 4352):
        want = (a[r0:r0 + 4352].float() @ w2.float().T + b2.float()) * gam.float() + res[r0:r0 + 4352].float()
        worst = max(worst, (got[r0:r0 + 4352].float() - want).abs().max().item() / (1 + want.abs().max().item()))
    assert worst < 1.5e-3, worst
    assert torch.equal(_native.linear_residual(a, w2, b2, gam, res), got)
    # the ragged round's K split (up to 8 workgroups share the K range of a 128 x 64 piece and the last one to arrive adds
    # their fp32 partials in K order): launches of different split factors alternate on the same arrival counters and stay
    # bit-reproducible; against the unsplit kernel only the fp32 summation order of the ragged tiles differs
    x1 = a[:, :1024].contiguous()
    w1, b1 = (torch.randn((4096, 1024), generator=g) / 32).half().cuda(), torch.randn(4096, generator=g).half().cuda()
    first = None
    try:
        _native.linear_env(DS_LIN_RAGGED_KSPLIT="8", DS_LIN_RAGGED_KSPLIT_MIN="1", DS_LIN_RAGGED_KSPLIT_KEEP="2")  # split the K = 1024 launches too (8 / 8 / 4 / 2 ways)
        for _ in range(3):
            outs = (_native.linear_residual(a, w2, b2, gam, res), _native.linear(x1, w1, b1, True), _native.linear_vt(wv, h),
                    _native.linear(x1, w1[:2048].contiguous(), b1[:2048].contiguous(), False))
            if first is None:
                first = outs
            assert all(torch.equal(o, f) for o, f in zip(outs, first)), "K-split ragged round: run-to-run difference"
        _native.linear_env(DS_LIN_RAGGED_KSPLIT="1")
        plain = (_native.linear_residual(a, w2, b2, gam, res), _native.linear(x1, w1, b1, True), _native.linear_vt(wv, h),
                 _native.linear(x1, w1[:2048].contiguous(), b1[:2048].contiguous(), False))
    finally:
        _native.linear_env(DS_LIN_RAGGED_KSPLIT=None, DS_LIN_RAGGED_KSPLIT_MIN=None, DS_LIN_RAGGED_KSPLIT_KEEP=None)
    # the default (round 6): NO K split, and the ragged round runs the main rounds' accumulation chain -- a row's value does not depend
    # on the round its tile falls into: bit-identical to the same launch with every tile sent through the main kernel
    assert torch.equal(_native.linear_residual(a, w2, b2, gam, res), plain[0])
    try:
        _native.linear_env(DS_LIN_RAGGED="0")
        main_only = (_native.linear_residual(a, w2, b2, gam, res), _native.linear(x1, w1, b1, True), _native.linear_vt(wv, h),
                     _native.linear(x1, w1[:2048].contiguous(), b1[:2048].contiguous(), False))
    finally:
        _native.linear_env(DS_LIN_RAGGED=None)
    for o, f in zip(plain, main_only):
        assert torch.equal(o, f), "the ragged round and the main rounds sum in different orders"
    try:                                                     # k_linear_thin (the default for proj / fc2 / qk here) against k_linear_ragged
        _native.linear_env(DS_LIN_RAGGED_THIN="0")
        wide = (_native.linear_residual(a, w2, b2, gam, res), _native.linear(x1, w1, b1, True), _native.linear_vt(wv, h),
                _native.linear(x1, w1[:2048].contiguous(), b1[:2048].contiguous(), False))
    finally:
        _native.linear_env(DS_LIN_RAGGED_THIN=None)
    for o, f in zip(plain, wide):
        assert torch.equal(o, f), "k_linear_thin differs from k_linear_ragged"
    if npad == 1032:                                         # 516 / 1032 / 2064 tiles: ragged rounds of 4 / 8 / 16 tiles
        assert not all(torch.equal(o, f) for o, f in zip(plain, first)), "the K split was not taken at the benchmark shapes"
    for o, f in zip(plain, first):
        assert (o.float() - f.float()).abs().max().item() < 1.5e-3 * (1 + f.float().abs().max().item())
        assert (o != f).float().mean().item() < 0.02         # only ragged tiles (< 1 % of the outputs) may differ at all


def test_preprocess_bicubic_kernel_vs_torch_chain(gpu):
    """ds_preprocess_bicubic (uint8 image -> normalised network input in one pass) against the torch chain it replaces -- flip,
    permute, float / 255, F.interpolate(bicubic, align_corners=False), (x - mean) / std -- for down-, up- and identity scaling,
    non-square shapes, scalar and per-channel mean / std, f32 / f16 / bf16 outputs; then against the reference's own transform
    chain (tests/golden/make_golden_transforms.py: Resize(INTER_CUBIC) / NormalizeImage / PrepareForNet on a numpy cubic stand-in)."""
    import torch.nn.functional as F
    import make_golden_transforms as mgt
    from src import _native
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(3)
    for (b, h, w, oh, ow, mean, std) in [(2, 64, 96, 32, 48, 0.5, 0.5), (1, 50, 70, 96, 128, vm.IMAGENET_MEAN, vm.IMAGENET_STD),
                                        (3, 33, 41, 33, 41, 0.5, 0.5), (1, 1024, 1024, 512, 512, 0.5, 0.5), (2, 135, 240, 266, 476, vm.IMAGENET_MEAN, vm.IMAGENET_STD)]:
        img = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8).cuda()
        x = img.flip(-1).permute(0, 3, 1, 2).float() / 255.0
        x = F.interpolate(x, size=(oh, ow), mode="bicubic", align_corners=False)
        m = torch.tensor(mean if isinstance(mean, tuple) else (mean,) * 3, device="cuda").view(1, 3, 1, 1)
        s = torch.tensor(std if isinstance(std, tuple) else (std,) * 3, device="cuda").view(1, 3, 1, 1)
        want = (x - m) / s
        got = _native.preprocess_bicubic(img, (oh, ow), mean, std, flip=True, dtype=torch.float32)
        assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        # (white-noise images and a non-integer scale are the worst case: torch's build contracts scale * (dst + 0.5) - 0.5 into
        # an FMA, this library is built with -ffp-contract=off -- one ulp of the source coordinate times a pixel step of 255)
        assert (got - want).abs().max().item() < 3e-5 * (1 + want.abs().max().item()), (b, h, w, oh, ow)
        for dt, tol in ((torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)):
            gh = _native.preprocess_bicubic(img, (oh, ow), mean, std, flip=True, dtype=dt)
            assert gh.dtype == dt and (gh.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())
        nf = _native.preprocess_bicubic(img, (oh, ow), mean, std, flip=False, dtype=torch.float32)
        assert (nf - want.flip(1) * s.flip(1) / s - (m.flip(1) - m) / s).abs().max().item() < 1e-4      # same pixels, channels not swapped
    z = np.load(os.path.join(os.path.dirname(GOLD), "transform_cases.npz"))
    from dmidas.dpt_depth import DPTDepthModel
    for name, h, w, nw, nh, method, seed in mgt.CASES:
        x = DPTDepthModel.preprocess(torch.from_numpy(mgt.image(h, w, seed))[None].cuda(), nw, nh, method, 0.5, 0.5)[0].cpu().numpy()
        assert x.shape == z[name].shape and np.abs(x - z[name]).max() < 5e-5, (name, float(np.abs(x - z[name]).max()))


# ---- the route the benchmark runs: every block GEMM and the decoder's 3x3 convolutions in-tree ---------------------------
def _variants(x, count):
    """`count` inputs out of ONE golden image: the image itself first, then flips / rolls of it (distinct units, same
    statistics: a routing bug that mixes batch elements or drops rows cannot cancel)."""
    outs = [x]
    ops = [lambda t: t.flip(-1), lambda t: t.flip(-2), lambda t: t.roll(37, -1), lambda t: t.roll(-53, -2),
           lambda t: t.flip(-1).roll(91, -2), lambda t: t.flip(-2).roll(-17, -1), lambda t: t.roll(11, -1).roll(5, -2)]
    for i in range(count - 1):
        outs.append(ops[i % len(ops)](x))
    return torch.cat(outs, 0)


def _route_calls(before, names):
    """C-ABI calls since `before`; the LayerNorm-folded variants (round 5: ds_linear_ln, ds_linear_vt_ln) count as the GEMM they are."""
    from src import _native
    out = {n: _native.CALLS[n] - before.get(n, 0) for n in names}
    for n, folded in (("ds_linear", "ds_linear_ln"), ("ds_linear_vt", "ds_linear_vt_ln")):
        if n in out:
            out[n] += _native.CALLS[folded] - before.get(folded, 0)
    return out


def test_dpt_beit_large_512_batch8_takes_the_benchmarked_route(gpu):
    """The route bench.py times (dmidas/backbones/beit.py:94-107 + dmidas/blocks.py:352-377 of the reference as in-tree
    kernels: qk / V^T / proj + LayerScale + residual / fc1 + GELU / fc2 + LayerScale + residual through k_linear256, the
    residual convolution units through the implicit-GEMM convolution) needs >= 96 GEMM tiles and >= 128 convolution tiles,
    i.e. a batch: dpt_beit_large_512 at 512^2, batch 8, float16.  Unit 0 is the golden image: 2e-2 against the float32
    output of the reference's own dmidas code.  ALL units: against the same network with every GEMM / 3x3 convolution
    sent to the ROCm libraries (vm.library_routing) at float16 noise level.  The counters of the ctypes binding prove
    that the fused entry points were really reached."""
    from dmidas.dpt_depth import DPTDepthModel
    from src import _native
    from src import vit_mi355x as vm
    gold = np.load(GOLD_LARGE)
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    m = m.cuda().half()
    x = _variants(mw.synthetic_image((1, 3, 512, 512), seed=31), 8).cuda().half().contiguous(memory_format=torch.channels_last)
    names = ("ds_linear", "ds_linear_residual", "ds_linear_vt", "ds_conv3x3_nhwc", "ds_attention_fwd", "ds_linear_readout", "ds_linear_shuffle")
    before = dict(_native.CALLS)
    with torch.no_grad():
        y = m(x).float()
    calls = _route_calls(before, names)
    # 24 blocks: qk + fc1 through ds_linear, proj + fc2 through ds_linear_residual, V^T through ds_linear_vt
    assert calls["ds_linear"] >= 48 and calls["ds_linear_residual"] == 48 and calls["ds_linear_vt"] == 24, calls
    assert calls["ds_conv3x3_nhwc"] >= 4 and calls["ds_attention_fwd"] == 24, calls
    # round 5, the reassemble stage (dmidas/backbones/utils.py:28-39,167-249): four read-out GEMMs on the padded taps, the two
    # transposed convolutions as GEMMs with a pixel-shuffle store, the 1x1 convolutions that fill the chip through ds_linear
    assert calls["ds_linear_readout"] == 4 and calls["ds_linear_shuffle"] == 2 and calls["ds_linear"] >= 50, calls
    before = dict(_native.CALLS)
    with torch.no_grad(), vm.library_routing():
        y_lib = m(x).float()
    calls_lib = _route_calls(before, names)
    assert calls_lib["ds_linear"] == calls_lib["ds_linear_residual"] == calls_lib["ds_linear_vt"] == calls_lib["ds_conv3x3_nhwc"] == 0, calls_lib
    assert calls_lib["ds_linear_readout"] == calls_lib["ds_linear_shuffle"] == 0, calls_lib
    ref = gold["dpt_beitl512_512x512_out_s2"]
    scale = float(np.abs(ref).max())
    e0 = np.abs(y[0:1, ::2, ::2].cpu().numpy() - ref).max() / scale
    assert e0 < 2e-2, e0
    # two float16 routes of the same network: each is within 2e-2 of the float32 reference at its worst pixel, so that is the
    # bar for their worst-pixel difference too; on average they agree far better
    e_lib = ((y - y_lib).abs().flatten(1).max(1).values / y_lib.abs().flatten(1).max(1).values).max().item()
    e_mean = ((y - y_lib).abs().flatten(1).mean(1) / y_lib.abs().flatten(1).max(1).values).max().item()
    assert e_lib < 2e-2 and e_mean < 2e-3, (e_lib, e_mean)
    # the units are distinct images: their outputs must differ (a route that broadcast unit 0 would pass the checks above)
    assert (y[1] - y[0]).abs().max().item() > 1e-3 * scale


def test_full_1080p_frame_on_the_networks_own_prediction_vs_oracle(gpu, oracle):
    """BASELINE config 5's per-pixel leg on what actually feeds it in bench.py: the float16 prediction of a random-initialised
    Depth-Anything-V2 ViT-L on a 1920 x 1080 frame -- noise at every scale: a quarter of the pixel-eyes take the general pass, a row
    or two the exact sweep -- through depth -> uint16 -> create_stereoimages(polylines_sharp, left-right, 2.5 %) and create_normalmap:
    EVERY row of both eyes and the normal map bit for bit against the CPU oracle on the same uint16 depth
    (reference: src/core.py:189-211, src/stereoimage_generation.py:162-283, src/normalmap_generation.py:5-56)."""
    orc = oracle
    from ddepth_anything_v2 import DepthAnythingV2
    from src import _native
    import src.stereoimage_generation as sg
    import src.normalmap_generation as nmg
    torch.manual_seed(1)                                      # bench.py's c5 network: seed 1
    net = DepthAnythingV2(encoder='vitl', features=256, out_channels=[256, 512, 1024, 1024]).eval().cuda().half()
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (1, 1080, 1920, 3), dtype=np.uint8)
    it = torch.from_numpy(img).cuda()
    with torch.no_grad():
        pred = net.infer_batch(it, 518).float()
    assert pred.shape == (1, 1080, 1920) and float(pred.max() - pred.min()) > 0
    d16 = _native.depth_to_u16(pred, False)
    sbs = sg.create_stereoimages_batch(it, d16, 2.5, 0.0, ['left-right'], 0.0, 1.0, 'polylines_sharp')[0]
    exact_rows, general = _native.last_stats(it)
    nmap = nmg.create_normalmap_batch(d16)
    torch.cuda.synchronize()
    d16_np = d16[0].cpu().numpy()
    assert np.array_equal(d16_np, orc.convert_to_i16(orc.depth_normalize01(pred[0].cpu().numpy(), False)))
    want = orc.create_stereoimages_arrays(img[0], d16_np, 2.5, 0.0, ['left-right'], 0.0, 1.0, 'polylines_sharp')[0]
    got = sbs[0].cpu().numpy()
    bad = int((want != got).sum())
    assert bad == 0, (bad, np.argwhere((want != got).any(axis=2))[:5].tolist())
    assert np.array_equal(nmap[0].cpu().numpy(), orc.create_normalmap_array(d16_np))
    assert general > 100000, general                          # the regime the bench's c5 leg is in: a large general pass


def test_dav2_vitl_1080p_batch4_takes_the_benchmarked_route(gpu):
    """Depth-Anything-V2 ViT-L at 518 x 924 (2443 tokens, BASELINE config 5), batch 4, float16: the block route of
    ddepth_anything_v2/depth_anything_v2/dinov2_layers/block.py:82-107 as in-tree GEMMs (156 tiles at 1024 columns).
    Unit 0 against the reference's own float32 output (2e-2), every unit against library routing."""
    from ddepth_anything_v2 import DepthAnythingV2
    from src import _native
    from src import vit_mi355x as vm
    gold = np.load(GOLD_LARGE)
    m = DepthAnythingV2('vitl', features=256, out_channels=[256, 512, 1024, 1024]).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.cuda().half()
    x = _variants(mw.synthetic_image((1, 3, 518, 924), seed=32), 4).cuda().half()
    names = ("ds_linear", "ds_linear_residual", "ds_linear_vt", "ds_conv3x3_nhwc", "ds_attention_fwd")
    before = dict(_native.CALLS)
    with torch.no_grad():
        y = m(x).float()
    calls = _route_calls(before, names)
    assert calls["ds_linear"] >= 48 and calls["ds_linear_residual"] == 48 and calls["ds_linear_vt"] == 24, calls
    assert calls["ds_attention_fwd"] == 24, calls
    with torch.no_grad(), vm.library_routing():
        y_lib = m(x).float()
    ref = gold["dav2_vitl_518x924_out_s2"]
    scale = float(np.abs(ref).max())
    e0 = np.abs(y[0:1, ::2, ::2].cpu().numpy() - ref).max() / scale
    assert e0 < 2e-2, e0
    # two float16 routes of the same network: each is within 2e-2 of the float32 reference at its worst pixel, so that is the
    # bar for their worst-pixel difference too; on average they agree far better
    e_lib = ((y - y_lib).abs().flatten(1).max(1).values / y_lib.abs().flatten(1).max(1).values).max().item()
    e_mean = ((y - y_lib).abs().flatten(1).mean(1) / y_lib.abs().flatten(1).max(1).values).max().item()
    assert e_lib < 2e-2 and e_mean < 2e-3, (e_lib, e_mean)
    assert (y[1] - y[0]).abs().max().item() > 1e-3 * scale


# ---- round 5: the reassemble stage in-tree ----------------------------------------------------------------------------------
@pytest.mark.parametrize("b,cin,cout,h,w,s,grid", [
    (32, 256, 256, 32, 32, 4, None),       # act_postprocess1 of dpt_beit_large_512 at batch 32 (dmidas/backbones/utils.py:196-205)
    (32, 512, 512, 32, 32, 2, None),       # act_postprocess2 (:215-224)
    (8, 256, 256, 37, 66, 4, None),        # Depth-Anything-V2 ViT-L on a 1080p frame (dpt.py:57-64): a non-square grid, 19 536 pixels
    (2, 128, 96, 9, 15, 4, 8),             # out_channels not a power of two (16 * 96 = 1536 columns), 270 pixels, every workgroup walks tiles
    (3, 256, 64, 11, 10, 2, 16),           # 4 * 64 = 256 columns: one column tile
])
def test_linear_shuffle_matches_conv_transpose(gpu, b, cin, cout, h, w, s, grid):
    """ds_linear_shuffle (ConvTranspose2d with kernel == stride as a GEMM with the pixel shuffle in the store address) against
    torch's conv_transpose2d in float32 on the same rounded operands, every output element; the module path
    (vm.conv_module -> _native.conv_transpose_shuffle) with its cached weight image and per-tap bias."""
    import torch.nn as nn
    from src import _native
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(50 + cin + s)
    layer = nn.ConvTranspose2d(cin, cout, s, s, 0).cuda().half()
    with torch.no_grad():
        layer.weight.copy_((torch.randn(layer.weight.shape, generator=g) * cin ** -0.5).half())
        layer.bias.copy_(torch.randn((cout,), generator=g).half())
    x = torch.randn((b, cin, h, w), generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    assert _native.conv_transpose_shuffle_supported(layer, x)
    if grid:
        _native.linear_env(DS_LIN_GRID=grid)
    try:
        before = _native.CALLS["ds_linear_shuffle"]
        y = _native.conv_transpose_shuffle(layer, x)
        y2 = _native.conv_transpose_shuffle(layer, x)
        assert _native.CALLS["ds_linear_shuffle"] == before + 2
    finally:
        if grid:
            _native.linear_env(DS_LIN_GRID=None)
    assert tuple(y.shape) == (b, cout, h * s, w * s) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, y2)
    with torch.no_grad():
        ref = torch.nn.functional.conv_transpose2d(x.float(), layer.weight.float(), layer.bias.float(), stride=s)
    err = (y.float() - ref).abs().max().item()
    assert err < 2e-3 * (1 + ref.abs().max().item()), (err, ref.abs().max().item())
    if not grid and vm.conv_transpose_hip_ok(layer, x):          # what the networks call
        with torch.no_grad():
            y3 = vm.conv_module(layer, x)
        assert torch.equal(y3, y)


@pytest.mark.parametrize("b,npad,n,c,grid", [
    (32, 1032, 1025, 1024, None),          # dpt_beit_large_512 at batch 32: the bench's shape (129 row panels x 4 column tiles)
    (8, 2464, 2443, 1024, None),           # a padded sequence whose pad is longer than one row group
    (3, 136, 130, 256, 8),                 # small: 408 rows, one column tile, every workgroup walks several tiles
    (2, 584, 577, 768, 16),                # ViT-B / hybrid at 384^2 (768 features = 3 column tiles)
])
def test_linear_readout_matches_definition(gpu, b, npad, n, c, grid):
    """ds_linear_readout against the definition of ProjectReadout (dmidas/backbones/utils.py:28-39) + Transpose / Unflatten
    (:165-169) in float32 on the same rounded operands: GELU(tokens @ w_tok^T + (w_cls @ cls + bias)), the cls row and the pad
    rows dropped, token-major output; junk (NaN) in the pad rows must not reach any output row; ProjectReadout.forward_padded
    (the module path) equals ProjectReadout.forward on the unpadded tap within float16 rounding."""
    from dmidas.backbones.beit import ProjectReadout
    from src import _native
    g = torch.Generator().manual_seed(60 + c)
    ro = ProjectReadout(c).cuda().half()
    with torch.no_grad():
        ro.project[0].weight.copy_((torch.randn((c, 2 * c), generator=g) * (2 * c) ** -0.5).half())
        ro.project[0].bias.copy_(torch.randn((c,), generator=g).half())
    xp = torch.randn((b, npad, c), generator=g).half().cuda()
    xp[:, n:] = float("nan")                                        # pad rows: never read as anything that matters
    if grid:
        _native.linear_env(DS_LIN_GRID=grid)
    try:
        before = _native.CALLS["ds_linear_readout"]
        with torch.no_grad():
            if grid:                     # below the routing threshold of the module path (a chip-filling launch): the kernel itself
                w_tok, w_cls = ro._split()
                clsvec = torch.nn.functional.linear(xp[:, 0], w_cls, ro.project[0].bias)
                y = _native.linear_readout(xp, n, w_tok, clsvec)
                y2 = _native.linear_readout(xp, n, w_tok, clsvec)
            else:
                y = ro.forward_padded(xp, n)
                y2 = ro.forward_padded(xp, n)
        assert _native.CALLS["ds_linear_readout"] == before + 2
    finally:
        if grid:
            _native.linear_env(DS_LIN_GRID=None)
    assert tuple(y.shape) == (b, n - 1, c) and y.is_contiguous() and torch.equal(y, y2)
    w = ro.project[0].weight.float()
    x = xp[:, :n].float()
    ref = torch.nn.functional.gelu(x[:, 1:] @ w[:, :c].t() + (x[:, 0] @ w[:, c:].t() + ro.project[0].bias.float())[:, None])
    assert torch.isfinite(y).all()
    err = (y.float() - ref).abs().max().item()
    assert err < 2e-3 * (1 + ref.abs().max().item()), (err, ref.abs().max().item())
    with torch.no_grad():
        y_lib = ro(xp[:, :n])                                        # split library GEMM + ds_reassemble_readout
    assert (y.float() - y_lib.float()).abs().max().item() < 4e-3 * (1 + ref.abs().max().item())


def test_conv1x1_through_the_in_tree_gemm(gpu):
    """1x1 convolutions of the reassemble stage / fusion blocks as ds_linear on the NHWC rows (vm.conv1x1) against the library
    convolution: same values within float16 rounding, channels_last in and out, and the routing rule (chip-filling launches only)."""
    import torch.nn as nn
    from src import _native
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(71)
    for (b, cin, cout, h, w) in [(32, 1024, 256, 32, 32), (32, 256, 256, 64, 64), (8, 1024, 512, 37, 66)]:
        layer = nn.Conv2d(cin, cout, 1).cuda().half()
        x = torch.randn((b, cin, h, w), generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        assert vm.conv1x1_hip_ok(layer, x)
        before = _native.CALLS["ds_linear"]
        with torch.no_grad():
            y = vm.conv_module(layer, x)
            ref = torch.nn.functional.conv2d(x.float(), layer.weight.float(), layer.bias.float())
        assert _native.CALLS["ds_linear"] == before + 1
        assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
        assert (y.float() - ref).abs().max().item() < 2e-3 * (1 + ref.abs().max().item())
    small = torch.randn((1, 256, 16, 16), generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    # one tile: in-tree as well since round 6 (vm.INVARIANT: a unit's depth must not depend on which library solver a launch size
    # picks); with DS_INVARIANT=0 the tile-count rule of rounds 4-5 hands it to the library's small kernels again
    one = nn.Conv2d(256, 256, 1).cuda().half()
    assert vm.conv1x1_hip_ok(one, small) == vm.INVARIANT
    keep = vm.INVARIANT
    try:
        vm.INVARIANT = False
        assert not vm.conv1x1_hip_ok(one, small)
        vm.INVARIANT = True
        assert vm.conv1x1_hip_ok(one, small)
        with torch.no_grad():
            y = vm.conv_module(one, small)
            ref = torch.nn.functional.conv2d(small.float(), one.weight.float(), one.bias.float())
        assert (y.float() - ref).abs().max().item() < 2e-3 * (1 + ref.abs().max().item())
    finally:
        vm.INVARIANT = keep


def test_kernel_timers_bracket_the_launches(gpu):
    """ds_kernel_timer_enable / ds_kernel_timer_read: every timed kind reports the launches made while the timer was on, with a
    plausible duration, and nothing once it is off (bench.py's in-step roofline reads these)."""
    from src import _native
    dev = torch.cuda.current_device()
    x = torch.randn((8192, 1024)).half().cuda()
    w = (torch.randn((4096, 1024)) / 32).half().cuda()
    _native.linear(x, w, None, True)
    torch.cuda.synchronize()
    _native.kernel_timer_enable(dev, True)
    for _ in range(3):
        _native.linear(x, w, None, True)
    _native.linear(x, w, None, False)
    n, ms = _native.kernel_timer_read(dev, "linear_gelu")
    assert n == 3 and 0.01 < ms / n < 5.0, (n, ms)
    n2, ms2 = _native.kernel_timer_read(dev, "linear")
    assert n2 == 1 and ms2 > 0.0
    assert _native.kernel_timer_read(dev, "attention") == (0, 0.0)
    _native.kernel_timer_enable(dev, False)
    _native.linear(x, w, None, True)
    assert _native.kernel_timer_read(dev, "linear_gelu") == (0, 0.0)


def test_linear_ragged_ksplit_stress_small_grid(gpu):
    """The advisor's stress test of the ragged round's K split (its cross-workgroup hand-over is argued on the gfx950 ISA, not on the
    HIP memory model): 60 back-to-back launches on a SMALL grid (every workgroup walks many tiles and the ragged pieces' workgroups
    arrive at their counters at very different times), two shapes alternating on the same counters and workspace -- every launch
    bit-identical to the first of its shape (a stale partial or a torn counter would show as a run-to-run difference), and within
    fp32-summation-order distance of the unsplit result."""
    from src import _native
    g = torch.Generator().manual_seed(97)
    shapes = [(40 * 256 + 256, 1024, 4096), (72 * 256 + 512, 2048, 1024)]          # tiles mod grid leave small ragged rounds
    ops = []
    for rows, n, k in shapes:
        x = torch.randn((rows, k), generator=g).half().cuda()
        w = (torch.randn((n, k), generator=g) * k ** -0.5).half().cuda()
        b = torch.randn((n,), generator=g).half().cuda()
        ops.append((x, w, b))
    try:
        _native.linear_env(DS_LIN_GRID=64, DS_LIN_RAGGED_KSPLIT="8", DS_LIN_RAGGED_KSPLIT_MIN="1", DS_LIN_RAGGED_KSPLIT_KEEP="2", DS_LIN_RAGGED_DEN="2")
        first = [None, None]
        for it in range(60):
            i = it & 1
            y = _native.linear(*ops[i], False)
            if first[i] is None:
                first[i] = y
            else:
                assert torch.equal(y, first[i]), f"K-split ragged round: launch {it} differs from the first of its shape"
        _native.linear_env(DS_LIN_RAGGED_KSPLIT="1")
        plain = [_native.linear(*ops[i], False) for i in range(2)]
    finally:
        _native.linear_env(DS_LIN_GRID=None, DS_LIN_RAGGED_KSPLIT=None, DS_LIN_RAGGED_KSPLIT_MIN=None, DS_LIN_RAGGED_KSPLIT_KEEP=None,
                           DS_LIN_RAGGED_DEN=None)
    for (x, w, b), y, p in zip(ops, first, plain):
        ref = x.float() @ w.float().T + b.float()
        assert (y.float() - ref).abs().max().item() < 1.5e-3 * (1 + ref.abs().max().item())
        assert (y.float() - p.float()).abs().max().item() < 1.5e-3 * (1 + ref.abs().max().item())


def test_dpt_beit_large_512_at_the_metrics_batch_is_pinned_on_three_units(gpu):
    """The metric's batch itself (round-4 verdict, weak 3: the reference-made golden was compared at batch 1 and at unit 0 of batch 8
    only): dpt_beit_large_512 at 512^2, BATCH 32, float16 -- the launch shapes bench.py times (33 024 padded token rows: 129 row
    panels, fc1 2064 tiles with its ragged round, 4096 / 2048-tile transposed convolutions, the read-out on 129 x 4 tiles).  The
    golden image sits at units 0, 13 and 31 (first, middle, last: first / middle / last row panels and the shifted last panel),
    the other units are flips / rolls of it: each of the three against the reference's own float32 output at 2e-2, BIT-IDENTICAL
    to each other (the units of a batch are independent: asserted since round 6), every unit against library routing."""
    from dmidas.dpt_depth import DPTDepthModel
    from src import _native
    from src import vit_mi355x as vm
    gold = np.load(GOLD_LARGE)
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    m = m.cuda().half()
    base = mw.synthetic_image((1, 3, 512, 512), seed=31)
    x = _variants(base, 32)
    x[13], x[31] = base[0], base[0]
    x = x.cuda().half().contiguous(memory_format=torch.channels_last)
    before = dict(_native.CALLS)
    with torch.no_grad():
        y = m(x).float()
    calls = _route_calls(before, ("ds_linear", "ds_linear_residual", "ds_linear_vt", "ds_linear_readout", "ds_linear_shuffle", "ds_conv3x3_nhwc"))
    assert calls["ds_linear_residual"] == 48 and calls["ds_linear_vt"] == 24 and calls["ds_linear_readout"] == 4 and calls["ds_linear_shuffle"] == 2, calls
    assert calls["ds_linear"] >= 48 + 4 and calls["ds_conv3x3_nhwc"] >= 12, calls     # qk + fc1, the reassemble 1x1 convolutions; the decoder
    ref = gold["dpt_beitl512_512x512_out_s2"]
    scale = float(np.abs(ref).max())
    for u in (0, 13, 31):
        e = np.abs(y[u:u + 1, ::2, ::2].cpu().numpy() - ref).max() / scale
        assert e < 2e-2, (u, e)
    # the same image at three positions of the batch comes out BIT-IDENTICAL (round 6): units 0 and 13 sit in full rounds of every
    # GEMM, unit 31's last tokens fall into the ragged round, which now runs the main rounds' accumulation chain (rounds 4-5: a K
    # split and two chains per K-tile -- another fp32 order, 3.2e-3 of the output range after 24 blocks).  The reference processes
    # one image at a time (src/core.py:133): an image's depth must not depend on its neighbours or its position.
    d13, d31 = (y[13] - y[0]).abs().max().item(), (y[31] - y[0]).abs().max().item()
    print(f"same image at units 0 / 13 / 31 of a batch of 32: max |difference| {d13:.3e} / {d31:.3e} of range {scale:.3f}")
    assert d13 == 0.0 and d31 == 0.0, (d13, d31)
    # ... nor on the SIZE of the batch (strong scaling: the same 32 units split over 1 / 2 / 4 / 8 ranks), nor on the
    # launch: the forward of this network has no library convolution or GEMM left (vit_mi355x.INVARIANT: every convolution and the
    # read-out's cls vector through the in-tree GEMM, one accumulation chain per output element) -- units 24..31 alone, as a batch
    # of 8, and a second launch of the batch of 32, bit for bit
    with torch.no_grad():
        y8 = m(x[24:32].contiguous(memory_format=torch.channels_last)).float()
        y_again = m(x).float()
    assert torch.equal(y8, y[24:32]), (y8 - y[24:32]).abs().max().item()
    assert torch.equal(y_again, y), (y_again - y).abs().max().item()
    with torch.no_grad(), vm.library_routing():
        y_lib = m(x[:8]).float()
    e_lib = ((y[:8] - y_lib).abs().flatten(1).max(1).values / y_lib.abs().flatten(1).max(1).values).max().item()
    assert e_lib < 2e-2, e_lib
    assert (y[1] - y[0]).abs().max().item() > 1e-3 * scale


# ---- round 5: LayerNorm folded into the GEMM behind it ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows,c,n,gelu", [(33024, 1024, 2048, False), (33024, 1024, 4096, True), (19712, 1024, 2048, False), (1280, 768, 2304, True),
                                             (516, 384, 768, False)])
def test_linear_ln_matches_layernorm_then_linear(gpu, rows, c, n, gelu):
    """ds_row_stats + ds_linear_ln against LayerNorm -> Linear [-> GELU] in float32 on the same rounded inputs (timm's Block as run by
    dmidas/backbones/beit.py:94-107: norm1 -> qkv, norm2 -> fc1): rows with a large common mode (mean ~ 4 standard deviations, the
    case the folded form's cancellation has to survive), at the benchmark's shapes and small ones; repeated launches bit-identical;
    the statistics against torch's own."""
    from src import _native
    from src import vit_mi355x as vm
    import torch.nn as nn
    g = torch.Generator().manual_seed(80 + c + n)
    x = (torch.randn((rows, c), generator=g) * torch.rand((rows, 1), generator=g).mul(3).add(0.2) + torch.randn((rows, 1), generator=g) * 4).half().cuda()
    ln = nn.LayerNorm(c, eps=1e-6).cuda()
    lin = nn.Linear(c, n).cuda()
    with torch.no_grad():
        ln.weight.copy_(torch.randn((c,), generator=g).mul(0.3).add(1.0))
        ln.bias.copy_(torch.randn((c,), generator=g).mul(0.2))
        lin.weight.copy_(torch.randn((n, c), generator=g) * c ** -0.5)
        lin.bias.copy_(torch.randn((n,), generator=g) * 0.1)
    ln, lin = ln.half(), lin.half()
    st = _native.row_stats(x, 1e-6)
    xf = x.float()
    mean, var = xf.mean(1), xf.var(1, unbiased=False)
    rstd = (var + 1e-6).rsqrt()
    assert (st[:, 0] - rstd).abs().max().item() < 1e-4 * rstd.abs().max().item()
    assert (st[:, 1] + mean * rstd).abs().max().item() < 1e-4 * (1 + (mean * rstd).abs().max().item())
    ws = (lin.weight.float() * ln.weight.float()[None, :]).half().contiguous()
    colsum = ws.float().sum(1).contiguous()
    bias = (lin.bias.float() + lin.weight.float() @ ln.bias.float()).half().contiguous()
    y = _native.linear_ln(x, ws, colsum, bias, st, gelu)
    assert torch.equal(_native.linear_ln(x, ws, colsum, bias, st, gelu), y)
    worst, scale = 0.0, 0.0
    for r0 in range(0, rows, 8192):
        h = torch.nn.functional.layer_norm(xf[r0:r0 + 8192], (c,), ln.weight.float(), ln.bias.float(), 1e-6)
        ref = h @ lin.weight.float().T + lin.bias.float()
        if gelu:
            ref = torch.nn.functional.gelu(ref)
        worst = max(worst, (y[r0:r0 + 8192].float() - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
    # the reference path rounds LN(x) to half before the GEMM (5e-4 relative per element); the folded path does not, but rounds
    # W * ln_weight once: both are float16 forwards of the same float32 map
    assert worst < 4e-3 * (1 + scale), (worst, scale)


@pytest.mark.parametrize("b,npad,c", [(32, 1032, 1024), (8, 2464, 1024), (2, 640, 768)])
def test_linear_vt_ln_matches_layernorm_then_v_transposed(gpu, b, npad, c):
    """ds_linear_vt_ln against (W_v . LN(x)^T) per batch element in float32 (without the constant W_v . ln_bias, which the host folds
    into the projection bias), every element; bit-identical when repeated."""
    from src import _native
    g = torch.Generator().manual_seed(90 + npad)
    x = (torch.randn((b, npad, c), generator=g) * 1.5 + torch.randn((b, npad, 1), generator=g) * 2).half().cuda()
    gamma = torch.randn((c,), generator=g).mul(0.3).add(1.0).cuda()
    wv = (torch.randn((c, c), generator=g) * c ** -0.5).half().cuda()
    st = _native.row_stats(x, 1e-6)
    ws = (wv.float() * gamma[None, :]).half().contiguous()
    colsum = ws.float().sum(1).contiguous()
    vt = _native.linear_vt_ln(ws, colsum, x, st)
    assert tuple(vt.shape) == (b, c, npad) and torch.equal(_native.linear_vt_ln(ws, colsum, x, st), vt)
    worst, scale = 0.0, 0.0
    for i in range(b):
        h = torch.nn.functional.layer_norm(x[i].float(), (c,), gamma, None, 1e-6)
        ref = wv.float() @ h.T
        worst = max(worst, (vt[i].float() - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
    assert worst < 4e-3 * (1 + scale), (worst, scale)


def test_ln_fold_route_equals_layernorm_route(gpu):
    """The whole encoder both ways on one network: dpt_beit_large_512 at batch 8, float16, with the LayerNorms folded into the GEMMs
    (DS_LN_FOLD=1: 48 ds_row_stats, 48 ds_linear_ln, 24 ds_linear_vt_ln, no ds_residual_layernorm in the blocks) and with
    ds_residual_layernorm in front of the GEMMs (the default): the two float16 forwards agree at float16 noise level on every unit,
    and the folded one holds 2e-2 against the reference's float32 golden.  (The folded route is correct and SLOWER -- 789.2 / 790.7
    against 798.7 / 798.3 pairs/s on one box, profiles/round5_ln_fold_ab.txt: the work moved into the GEMMs' epilogues is exposed
    time of a workgroup that owns its CU, the LayerNorm pass it replaces streams at HBM speed -- which is why it is not the default.)"""
    from dmidas.dpt_depth import DPTDepthModel
    from src import _native
    from src import vit_mi355x as vm
    gold = np.load(GOLD_LARGE)
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval()
    m.load_state_dict(mw.fill_state_dict_beit(m.state_dict()), strict=True)
    m = m.cuda().half()
    x = _variants(mw.synthetic_image((1, 3, 512, 512), seed=31), 8).cuda().half().contiguous(memory_format=torch.channels_last)
    names = ("ds_row_stats", "ds_linear_ln", "ds_linear_vt_ln", "ds_residual_layernorm", "ds_linear_residual")
    saved = vm.LN_FOLD
    try:
        vm.LN_FOLD = True
        before = dict(_native.CALLS)
        with torch.no_grad():
            y = m(x).float()
        calls = {n: _native.CALLS[n] - before.get(n, 0) for n in names}
        assert calls == {"ds_row_stats": 48, "ds_linear_ln": 48, "ds_linear_vt_ln": 24, "ds_residual_layernorm": 0, "ds_linear_residual": 48}, calls
        vm.LN_FOLD = False
        before = dict(_native.CALLS)
        with torch.no_grad():
            y_ln = m(x).float()
        calls = {n: _native.CALLS[n] - before.get(n, 0) for n in names}
        assert calls["ds_row_stats"] == 0 and calls["ds_linear_ln"] == 0 and calls["ds_residual_layernorm"] == 48, calls
    finally:
        vm.LN_FOLD = saved
    ref = gold["dpt_beitl512_512x512_out_s2"]
    scale = float(np.abs(ref).max())
    assert np.abs(y[0:1, ::2, ::2].cpu().numpy() - ref).max() / scale < 2e-2
    e = ((y - y_ln).abs().flatten(1).max(1).values / y_ln.abs().flatten(1).max(1).values).max().item()
    e_mean = ((y - y_ln).abs().flatten(1).mean(1) / y_ln.abs().flatten(1).max(1).values).max().item()
    assert e < 2e-2 and e_mean < 2e-3, (e, e_mean)


# ---- round 5: float32 kernels of Boost's base estimator ------------------------------------------------------------------------
@pytest.mark.parametrize("b,c,cpg,h,w", [(8, 256, 8, 224, 224), (8, 512, 16, 112, 112), (8, 1024, 32, 56, 56), (2, 256, 8, 37, 53), (1, 64, 16, 9, 70),
                                         (3, 96, 32, 8, 32)])
def test_gconv3x3_matches_torch_grouped_convolution(gpu, b, c, cpg, h, w):
    """ds_gconv3x3_nhwc_f32 (conv2 + folded bn2 + relu of the ResNeXt bottlenecks, lib/Resnext_torch.py:104-110) against torch's grouped
    float32 convolution on the same operands: at the shapes a batch of eight 896^2 patches sends through layers 1-3, and on ragged
    tiles (sizes that are not multiples of the 8 x 32 pixel tile, a single 32-channel block); with and without bias / ReLU."""
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(40 + c + h)
    x = torch.randn((b, c, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
    wt = (torch.randn((c, cpg, 3, 3), generator=g) * (9 * cpg) ** -0.5).cuda()
    bias = torch.randn((c,), generator=g).cuda()
    assert _native.gconv3x3_supported(x, wt, (1, 1), (1, 1), (1, 1), c // cpg)
    img = _native.gconv_weight_image(wt, c // cpg)
    for use_bias, relu in ((True, True), (False, False)):
        y = _native.gconv3x3(x, img, bias if use_bias else None, relu, cpg)
        ref = F.conv2d(x, wt, bias if use_bias else None, 1, 1, 1, c // cpg)
        if relu:
            ref = F.relu(ref)
        assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
        err = (y - ref).abs().max().item()
        assert err < 2e-5 * (1 + ref.abs().max().item()), (use_bias, relu, err)
        assert torch.equal(_native.gconv3x3(x, img, bias if use_bias else None, relu, cpg), y)
    a, bb = torch.randn((b, c, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last), x
    if a.numel() % 4 == 0:
        assert torch.equal(_native.add_relu(a, bb), F.relu(a + bb))
        # NaN / Inf activations propagate like torch's ReLU (a NaN must reach the output, not become 0)
        a2 = a.clone()
        a2[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0]).cuda()
        got, want = _native.add_relu(a2, torch.zeros_like(a2)), F.relu(a2)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0))
        xn = x.clone()
        xn[0, :, 0, 0] = float("nan")
        yn = _native.gconv3x3(xn, img, None, True, cpg)
        rn = F.relu(F.conv2d(xn, wt, None, 1, 1, 1, c // cpg))
        assert torch.equal(torch.isnan(yn), torch.isnan(rn)) and bool(torch.isnan(yn).any())


def test_leres_takes_the_in_tree_grouped_convolutions(gpu):
    """RelDepthModel (LeReS res101) on the device: the 28 stride-1 grouped convolutions of layers 1-3 go through ds_gconv3x3_nhwc_f32
    (layer 4's 64-wide groups and the strided first blocks stay library calls); round 6: every library convolution runs without its
    bias and ds_bias_act_f32 applies the folded bias, the shortcut add of the 33 bottleneck tails and the ReLU in one pass -- the same
    operations in the same order, so the output is BIT-IDENTICAL to torch's bias pass + add_relu (DS_BIAS_ACT_F32=0).  Against the
    library-only network (DS_GCONV=0 too) the difference is float32 summation order; 1e-4 against the reference's own modules is held
    by test_leres_and_hybrid_gpu_fp32_vs_reference."""
    import lib.multi_depth_model_woauxi as leres
    from src import _native
    m = leres.RelDepthModel(backbone='resnext101').eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    m = m.cuda()
    x = mw.synthetic_image((2, 3, 96, 160), seed=15).cuda()
    before = dict(_native.CALLS)
    with torch.no_grad():
        y = m.depth_model(x)
    assert _native.CALLS["ds_gconv3x3_nhwc_f32"] - before.get("ds_gconv3x3_nhwc_f32", 0) == 3 + 3 + 22
    # stem + 33 x (conv1, conv3 + shortcut) + 4 downsample + 5 library conv2 (3 strided first blocks + layer 4's other two) + the decoder
    assert _native.CALLS["ds_bias_act_f32"] - before.get("ds_bias_act_f32", 0) >= 1 + 66 + 4 + 5
    saved = leres.GCONV_HIP, leres.ADD_RELU_HIP, leres.BIAS_ACT_HIP
    try:
        leres.BIAS_ACT_HIP = False
        before = dict(_native.CALLS)
        with torch.no_grad():
            y_two_pass = m.depth_model(x)
        assert _native.CALLS["ds_bias_act_f32"] == before.get("ds_bias_act_f32", 0)
        assert _native.CALLS["ds_add_relu_f32"] - before.get("ds_add_relu_f32", 0) >= 33
        assert torch.equal(y, y_two_pass), (y - y_two_pass).abs().max().item()
        leres.GCONV_HIP = leres.ADD_RELU_HIP = False
        with torch.no_grad():
            y_lib = m.depth_model(x)
    finally:
        leres.GCONV_HIP, leres.ADD_RELU_HIP, leres.BIAS_ACT_HIP = saved
    assert (y - y_lib).abs().max().item() < 2e-5 * (1 + y_lib.abs().max().item())


def test_bias_act_f32_and_relu_cat_f32_match_torch_bit_for_bit(gpu):
    """ds_bias_act_f32 = [relu]((x + bias) [+ res]) in place and ds_relu_cat_f32 = relu(cat(a, b)) on float32 channels_last activations
    against torch's own passes: equal bits (the same float32 operations in the same order), NaN / Inf / -0.0 included, at a shape of
    layer 1 of a 896^2 patch batch, on ragged sizes, and with more elements than one grid stride."""
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(77)
    for (n, c, h, w) in [(8, 256, 224, 224), (1, 4, 3, 5), (2, 2048, 7, 9), (3, 36, 11, 13)]:
        x = torch.randn((n, c, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
        r = torch.randn((n, c, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
        b = torch.randn((c,), generator=g).cuda()
        x[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0]).cuda()[:min(4, w)] if w >= 4 else x[0, 0, 0, :4]
        for relu, res in ((True, None), (False, None), (True, r), (False, r)):
            want = x + b.view(1, -1, 1, 1)
            if res is not None:
                want = want + res
            if relu:
                want = F.relu(want)
            assert _native.bias_act_f32_ok(x, b, res)
            got = _native.bias_act_f32(x.clone(memory_format=torch.preserve_format), b, relu, res)
            assert got.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0)), (n, c, h, w, relu)
    for (n, ca, cb, h, w) in [(8, 64, 64, 512, 512), (1, 4, 8, 3, 5), (2, 512, 512, 2, 2), (3, 12, 4, 7, 9)]:
        a = torch.randn((n, ca, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
        b = torch.randn((n, cb, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
        a[0, 0, 0, 0], b[0, 0, 0, 0] = float("nan"), float("-inf")
        want = F.relu(torch.cat([a, b], 1))
        got = _native.relu_cat_f32(a, b)
        assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0)), (n, ca, cb, h, w)
    assert not _native.relu_cat_f32_ok(a[:, :3], b) and not _native.bias_act_f32_ok(a.contiguous(), torch.zeros(12).cuda())
    # the U-Net's up path: the skip is channels_last, the transposed convolution's result NCHW, and so is the concatenation (ragged
    # pixel tiles, planes smaller than a tile, the innermost 2 x 2 level)
    for (n, ca, cb, h, w) in [(8, 64, 64, 512, 512), (2, 512, 512, 2, 2), (3, 32, 96, 7, 9), (1, 128, 64, 65, 3)]:
        a = torch.randn((n, ca, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last)
        b = torch.randn((n, cb, h, w), generator=g).cuda()
        a[0, 0, 0, 0], b[0, 0, 0, 0] = float("nan"), float("-inf")
        for aa in (a, a.contiguous()):
            want = F.relu(torch.cat([aa, b], 1))
            assert _native.relu_cat_f32_ok(aa, b)
            got = _native.relu_cat_f32(aa, b)
            assert got.shape == want.shape and got.is_contiguous()
            assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, 7.0), torch.nan_to_num(want, 7.0)), (n, ca, cb, h, w)


def test_pix2pix_unet_takes_relu_cat(gpu):
    """The merge network with its nine skip concatenations written rectified by ds_relu_cat_f32 against the same network with torch.cat
    + F.relu (DS_RELU_CAT=0).  The pass itself is bit-identical to torch's two (test above); the NETWORK's output is compared at float32
    summation-order level, because MIOpen's split-K solvers (`..._gkgs`: atomic adds) make two runs of the same float32 U-Net differ
    in the last bits whatever feeds them."""
    import pix2pix.models.networks as networks
    from src import _native
    torch.manual_seed(3)
    m = networks.UnetGenerator().eval().cuda()
    x = torch.randn((2, 2, 1024, 1024), device="cuda")
    before = _native.CALLS["ds_relu_cat_f32"]
    with torch.no_grad():
        y = m(x)
    assert _native.CALLS["ds_relu_cat_f32"] - before == 9
    saved = networks.RELU_CAT_HIP
    try:
        networks.RELU_CAT_HIP = False
        with torch.no_grad():
            y2 = m(x)
    finally:
        networks.RELU_CAT_HIP = saved
    assert (y - y2).abs().max().item() < 2e-5 * (1 + y2.abs().max().item())


# ---- round 6: GroupNorm of the ResNetV2-50 stem (dpt_hybrid_384, BASELINE config 2) ----------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
def test_group_norm_kernel_matches_float32_group_norm(gpu, dtype, tol):
    """ds_group_norm_nchw (two launches: float32 moments per slice, float64 combine, float32 affine map [+ residual] [+ ReLU]) against
    torch's F.group_norm in float32 on the same rounded operands -- the shapes of the stem at 384 x 384 (64 x 192^2 with 2 channels per
    group ... 1024 x 24^2 with 32), a batch, a plane that is a bare multiple of 8, an offset distribution (mean >> spread: the
    E[x^2] - mean^2 form must survive it), and the routing rule for what it does not take."""
    import torch.nn.functional as F
    from src import _native
    g = torch.Generator().manual_seed(61)
    for (n, c, h, w, shift) in [(1, 64, 192, 192, 0.0), (1, 256, 96, 96, 0.0), (1, 128, 48, 48, 3.0), (2, 1024, 24, 24, 0.0), (3, 64, 4, 6, 0.0),
                                (1, 512, 48, 48, 40.0)]:
        x = (torch.randn((n, c, h, w), generator=g) * 1.7 + shift).to(dtype).cuda()
        res = torch.randn((n, c, h, w), generator=g).to(dtype).cuda()
        wt, bs = (torch.randn(c, generator=g) * 0.5 + 1.0).cuda(), torch.randn(c, generator=g).cuda()
        assert _native.group_norm_supported(x, 32)
        for relu, use_res in ((True, False), (False, False), (True, True)):
            want = F.group_norm(x.float(), 32, wt.to(dtype).float(), bs.to(dtype).float(), 1e-5)
            if use_res:
                want = want + res.float()
            if relu:
                want = F.relu(want)
            got = _native.group_norm(x, 32, wt, bs, 1e-5, relu=relu, res=res if use_res else None)
            assert got.shape == x.shape and got.dtype == dtype
            err = (got.float() - want).abs().max().item()
            assert err < tol * (1 + want.abs().max().item()), (n, c, h, w, shift, relu, use_res, err)
            assert torch.equal(_native.group_norm(x, 32, wt, bs, 1e-5, relu=relu, res=res if use_res else None), got)
    # (the batch of 3 x 32 groups and every group above fit one workgroup's registers: the single-launch kernel; 20 images x 32 groups of
    # 96^2 x 8 values = the moments + apply pair)
    xb = torch.randn((20, 256, 96, 96), generator=g).to(dtype).cuda()
    wt, bs = torch.ones(256).cuda(), torch.zeros(256).cuda()
    got = _native.group_norm(xb, 32, wt, bs, 1e-5, relu=True)
    want = F.relu(F.group_norm(xb.float(), 32, wt, bs, 1e-5))
    assert (got.float() - want).abs().max().item() < tol * (1 + want.abs().max().item())
    assert not _native.group_norm_supported(torch.randn((1, 64, 5, 5)).half().cuda(), 32)            # 25 pixels per plane: torch's kernel
    assert not _native.group_norm_supported(torch.randn((1, 64, 8, 8)).cuda(), 32)                   # float32: torch's kernel


def test_hybrid_stem_takes_the_in_tree_group_norm(gpu):
    """The ResNetV2-50 stem of dpt_hybrid_384 in half precision: 52 GroupNorms per image through ds_group_norm_nchw (the 16 behind
    conv3 with the shortcut add and the ReLU folded in); against the float32 stem it loses no more than the same half-precision stem with
    DS_GROUPNORM off (torch's group_norm + ReLU + add) does."""
    from dmidas.backbones import vit as hv
    from src import _native
    torch.manual_seed(3)
    stem = hv.ResNetV2Stem().eval().cuda().half()
    x = torch.randn((1, 3, 384, 384)).half().cuda()
    before = _native.CALLS["ds_group_norm_nchw"]
    with torch.no_grad():
        got = stem.forward_stages(x)
    assert _native.CALLS["ds_group_norm_nchw"] - before == 1 + 16 * 3 + 3          # stem + three per bottleneck + three downsamples
    keep = hv.GROUPNORM_HIP
    try:
        hv.GROUPNORM_HIP = False
        with torch.no_grad():
            half_torch = stem.forward_stages(x)
    finally:
        hv.GROUPNORM_HIP = keep
    with torch.no_grad():
        want = stem.float().forward_stages(x.float())
    # a random-initialised stem amplifies half-precision rounding stage by stage (16 bottlenecks, no trained scales): the yardstick is the
    # float32 stem, and the in-tree GroupNorm must not lose more against it than torch's own half-precision group_norm does
    for a, b, ref in zip(got, half_torch, want):
        assert a.shape == ref.shape
        scale = ref.abs().max().item()
        e_tree, e_torch = (a.float() - ref).abs().max().item() / scale, (b.float() - ref).abs().max().item() / scale
        e_tree_mean, e_torch_mean = (a.float() - ref).abs().mean().item() / scale, (b.float() - ref).abs().mean().item() / scale
        assert e_tree < 1.5 * e_torch + 5e-3 and e_tree_mean < 1.5 * e_torch_mean + 5e-4, (e_tree, e_torch, e_tree_mean, e_torch_mean)
