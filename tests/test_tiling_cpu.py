"""TILING_MODE without a GPU: the premise of the exact-integer tests of tests/test_gpu_tiling.py, the host routing of circular
layers, and the new golden (tests/golden/make_golden_tiling_heads.py) against this package's own float32 forward."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import conftest  # noqa: F401
import model_weights as mw
import test_gpu_gemm_exact as ge
import test_gpu_tiling as tt

DT = ge.DT
EXACT_MAX = ge.EXACT_MAX


def _exact_cases():
    for dt in DT:
        for name in tt.CONV:
            yield f"circular conv {name} {dt}", dt, tt.conv_case(name, dt)[1]
        for name in tt.STRIDED:
            yield f"circular strided {name} {dt}", dt, tt.strided_case(name, dt)[1]


def test_circular_exact_cases_stay_in_the_exact_range():
    """The argument of test_gpu_gemm_exact.test_exact_cases_stay_in_the_exact_range for the circular cases: every partial
    accumulator, in any order, stays below 2^24 (bounded by the same sum on absolute values); the value in front of the activation
    is exact in fp32, at most 2048 (float16) / 256 (bfloat16) in magnitude and exactly representable in the output type; more than
    90 % of these values are nonzero, and a ReLU both keeps and clamps a fair share."""
    for what, dt, wants in _exact_cases():
        for op, w in wants.items():
            assert w.bound < 2.0 ** 24, (what, op, w.bound)
            assert torch.equal(w.pre.float().double(), w.pre), (what, op)
            assert float((w.pre != 0).double().mean()) > 0.9, (what, op)
            assert float(w.pre.abs().max()) <= EXACT_MAX[dt], (what, op, float(w.pre.abs().max()))
            assert torch.equal(w.pre.to(DT[dt]).double(), w.pre), (what, op)
            if w.act == "relu":
                kept = float((w.pre > 0).double().mean())
                assert 0.25 < kept < 0.75, (what, op, kept)


def test_circular_reference_is_the_circular_convolution():
    """conv_ref_circular (F.pad on the NHWC tensor + nine shifted views) against nn.Conv2d(padding_mode='circular') in float64, also
    on maps of height 1 and width 1 (a pixel wraps onto itself), and against the zero-padding reference away from the border."""
    g = torch.Generator().manual_seed(3)
    for (b, h, wd, c, o) in ((2, 5, 4, 3, 2), (1, 1, 6, 2, 3), (1, 7, 1, 2, 3)):
        x, w = torch.randn((b, h, wd, c), generator=g, dtype=torch.float64), torch.randn((o, 3, 3, c), generator=g, dtype=torch.float64)
        m = nn.Conv2d(c, o, 3, padding=1, bias=False, padding_mode='circular').double()
        with torch.no_grad():
            m.weight.copy_(w.permute(0, 3, 1, 2))
            want = m(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        got = tt.conv_ref_circular(x, w)
        assert torch.allclose(got, want, rtol=0, atol=1e-12), (b, h, wd)
        assert torch.equal(got[:, 1:-1, 1:-1], ge.conv_ref(x, w)[:, 1:-1, 1:-1])


def test_circular_impulse_map_names_the_wrapped_taps():
    """The reference map of the impulse test: images 0 and 2 stay zero; five impulses of nine taps each (sum 1 + .. + 9 = 45); the
    bottom-right corner sees itself through the centre tap (5) and the three other corners through the wrapped taps 9, 8 and 6; the
    bottom row sees the top edge's impulse through the taps of ky = 2."""
    b, h, wd, cin, cout = tt.CONV["three_images"]
    o, w = tt.impulse_case()
    m = w.pre[..., 0]
    assert float(m[0].abs().max()) == 0.0 and float(m[2].abs().max()) == 0.0
    assert float(m[1].sum()) == 5 * 45.0 and torch.equal(w.pre, w.pre[..., :1].expand_as(w.pre))
    assert float(m[1, h - 1, wd - 1]) == 5.0 + 9.0 + 8.0 + 6.0
    assert [float(v) for v in m[1, h - 1, wd // 2 - 1: wd // 2 + 2]] == [9.0, 8.0, 7.0]
    zero = ge.conv_ref(o["x"], o["w"])[..., 0]
    assert float(zero[1, h - 1, wd - 1]) == 5.0 and float(zero[1, h - 1, wd // 2]) == 0.0          # what zero padding would give


def test_host_routing_of_circular_layers(monkeypatch):
    """conv3x3_circular_supported is conv3x3_supported with padding_mode == 'circular' (and the latter still rejects circular
    layers); the switch DS_CONV_CIRCULAR=0 (vit_mi355x.CONV_CIRCULAR_HIP) sends circular layers, and only them, to the library."""
    from src import _native
    from src import vit_mi355x as vm
    x = torch.zeros((1, 128, 16, 16))
    zero, circ = nn.Conv2d(128, 256, 3, padding=1), nn.Conv2d(128, 256, 3, padding=1)
    circ.padding_mode = 'circular'
    assert _native.conv3x3_supported(zero, x) and not _native.conv3x3_circular_supported(zero, x)
    assert _native.conv3x3_circular_supported(circ, x) and not _native.conv3x3_supported(circ, x)
    for bad in (nn.Conv2d(128, 256, 3, padding=1, stride=2), nn.Conv2d(128, 256, 3, padding=0), nn.Conv2d(128, 256, 3, padding=1, groups=2),
                nn.Conv2d(128, 200, 3, padding=1), nn.Conv2d(128, 256, 3, padding=1, dilation=2), nn.Conv2d(128, 256, 1)):
        bad.padding_mode = 'circular'
        assert not _native.conv3x3_circular_supported(bad, x)
    reflect = nn.Conv2d(128, 256, 3, padding=1, padding_mode='reflect')
    assert not _native.conv3x3_circular_supported(reflect, x) and not _native.conv3x3_supported(reflect, x)
    assert not _native.conv3x3_circular_supported(circ, x[:, :, :8])          # fewer than 256 pixels
    assert vm.CONV_CIRCULAR_HIP and vm.circular_hip_ok(circ) and vm.circular_hip_ok(zero)
    monkeypatch.setattr(vm, "CONV_CIRCULAR_HIP", False)
    assert not vm.circular_hip_ok(circ) and vm.circular_hip_ok(zero)
    for name in ("ds_conv3x3_nhwc_circular", "ds_dpt_head_tail_circular"):
        assert name in _native.EXPORTS


def test_tiling_head_golden_matches_this_package_in_float32():
    """The Depth-Anything-V2 of tests/golden/tiling_head_cases.npz (ViT-S encoder, features 256: the decoder width whose head is the
    fused head tail on the GPU) with apply_tiling_mode, float32 on the CPU, against the reference's hijacked module at 1e-4; and
    tiling really changes this output."""
    from ddepth_anything_v2 import DepthAnythingV2
    from src.depthmap_generation import apply_tiling_mode
    z = np.load(os.path.join(tt.GOLDEN, "tiling_head_cases.npz"))
    ref = z["dav2_vits_f256_140x182_out"]
    m = DepthAnythingV2(**tt.DAV2).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    x = mw.synthetic_image((2, 3, 140, 182), seed=11)
    with torch.no_grad():
        plain = m(x).numpy()
    assert apply_tiling_mode(m) == int(z["dav2_vits_f256_n_convs"][0])
    with torch.no_grad():
        y = m(x).numpy()
    scale = np.abs(ref).max()
    assert y.shape == ref.shape and np.abs(y - ref).max() / scale < 1e-4, np.abs(y - ref).max() / scale
    assert np.abs(plain - ref).max() / scale > 1e-2
