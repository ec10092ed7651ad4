"""Routing of the fused head front (vm.head_front_ok, ds_dpt_head_front) without a GPU: the predicate says no wherever the two
launches it replaces would not both be the in-tree kernels, and a CPU forward does not notice the switch."""
import torch
import torch.nn as nn

import conftest  # noqa: F401
import model_weights as mw


def _conv(cin=256, cout=128, **kw):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, **kw)


def test_predicate_says_no(monkeypatch):
    from src import vit_mi355x as vm
    x = torch.zeros((1, 256, 8, 16), dtype=torch.float16)
    assert not vm.head_front_ok(x, _conv())                                # a CPU tensor
    # from here on every tensor counts as "half precision on the GPU", so that each remaining reason is tested on its own
    monkeypatch.setattr(vm, "half_on_gpu", lambda t: t.dtype in (torch.float16, torch.bfloat16) and not vm.STOCK[0])
    assert vm.head_front_ok(x, _conv()) and vm.head_front_ok(x.bfloat16(), _conv(bias=False))
    assert not vm.head_front_ok(x.float(), _conv())                        # float32
    assert not vm.head_front_ok(x, _conv(padding_mode="circular"))         # TILING_MODE
    assert not vm.head_front_ok(x, _conv(cout=256))                        # other widths
    assert not vm.head_front_ok(x[:, :128], _conv(cin=128))
    assert not vm.head_front_ok(x, _conv(cin=128))                         # channels of x and of the convolution disagree
    assert not vm.head_front_ok(x, _conv(), scale_factor=4)
    assert not vm.head_front_ok(x, _conv(), scale_factor=1.5)
    assert not vm.head_front_ok(x, _conv(), align_corners=False)
    assert not vm.head_front_ok(x, nn.Conv2d(256, 128, 3, stride=2, padding=1))
    assert not vm.head_front_ok(x, nn.Conv2d(256, 128, 3, padding=2, dilation=2))
    assert not vm.head_front_ok(x[:, :, :2, :2], _conv())                  # 16 upsampled pixels: the convolution it replaces takes >= 256
    with vm.library_routing():
        assert not vm.head_front_ok(x, _conv())
    with vm.stock_routing():
        assert not vm.head_front_ok(x, _conv())
    assert vm.head_front_ok(x, _conv())
    monkeypatch.setattr(vm, "HEAD_FRONT", False)                           # DS_HEAD_FRONT=0
    assert not vm.head_front_ok(x, _conv())
    monkeypatch.setattr(vm, "HEAD_FRONT", True)
    monkeypatch.setattr(vm, "CONV_HEAD_HIP", False)                        # DS_CONV_HEAD=0: the convolution would be the library's
    assert not vm.head_front_ok(x, _conv())


def test_fusion_block_without_its_upsample():
    """upsample=False returns what the block upsamples: interpolating it gives the block's usual output (both copies of the block)."""
    from ddepth_anything_v2.depth_anything_v2.dpt import FeatureFusionBlock
    from dmidas.dpt_depth import FeatureFusionBlock_custom
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn((1, 16, 5, 6), generator=g), torch.randn((1, 16, 5, 6), generator=g)
    for cls in (FeatureFusionBlock, FeatureFusionBlock_custom):
        blk = cls(16).eval()
        with torch.no_grad():
            full, low = blk(a, b), blk(a, b, upsample=False)
            assert low.shape == a.shape and full.shape == (1, 16, 10, 12)
            assert torch.equal(vm.interpolate_bilinear(low, scale_factor=2, align_corners=True), full)
            assert torch.equal(blk(a, b, size=(7, 9), upsample=False), low)


def test_cpu_forward_does_not_notice_the_switch(monkeypatch):
    from ddepth_anything_v2 import DepthAnythingV2
    from src import _native
    from src import vit_mi355x as vm
    m = DepthAnythingV2('vits', features=256, out_channels=[48, 96, 192, 384]).eval()
    m.load_state_dict(mw.fill_state_dict(m.state_dict()), strict=True)
    assert tuple(m.depth_head.scratch.output_conv1.weight.shape) == (128, 256, 3, 3)
    x = mw.synthetic_image((1, 3, 56, 70), seed=4)
    before = _native.CALLS["ds_dpt_head_front"]
    outs = []
    for on in (True, False):
        monkeypatch.setattr(vm, "HEAD_FRONT", on)
        with torch.no_grad():
            outs.append(m(x))
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    assert _native.CALLS["ds_dpt_head_front"] == before


def test_a_factor_two_upsample_fits_the_staging_tile():
    """ds_dpt_head_front refuses an upsample whose source pixels under a tile's 10 x 34 patch exceed its 6 x 18 staging tile (hf_fits
    in csrc/ds_head_front.hip, restated here in the same float32 arithmetic); the routing sends it every x2 upsample without asking.
    That is safe: no size up to 8192 is refused, for the 8-row tiles or the 32-column ones."""
    import numpy as np

    def fits(in_n, out_n, tile, rows):
        s = np.float32(in_n - 1) / np.float32(out_n - 1)
        t0 = np.arange(0, out_n, tile)
        lo = np.minimum((s * np.maximum(t0 - 1, 0).astype(np.float32)).astype(np.int64), in_n - 1)
        last = np.minimum(t0 + tile, out_n - 1)
        hi = np.minimum(np.minimum((s * last.astype(np.float32)).astype(np.int64), in_n - 1) + 1, in_n - 1)
        return bool((hi - lo <= rows - 1).all())
    assert all(fits(n, 2 * n, 8, 6) and fits(n, 2 * n, 32, 18) for n in range(1, 8193))
    assert not fits(8, 8, 8, 6) and not fits(40, 60, 32, 18)             # no upsample, x1.5: refused
