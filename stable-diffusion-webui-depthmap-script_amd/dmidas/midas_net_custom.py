"""MiDaS v2.1 small (model id 6, `midas_v21_small`), MI355X-first.

Reference: dmidas/midas_net_custom.py (MidasNet_small :12-105), dmidas/blocks.py (_make_encoder :126-128, _make_scratch :136-166,
_make_efficientnet_backbone :179-189, Interpolate :211-243, ResidualConvUnit_custom :322-377, FeatureFusionBlock_custom :382-441) and
its callers estimatemidas (src/depthmap_generation.py:182-193, :455-499) and estimatemidasBoost (:1180-1220).  Checkpoint key names
are the reference's (pretrained.layerN.*, scratch.*).  The encoder is dmidas/backbones/efficientnet_lite.py, a restatement of
gen-efficientnet's tf_efficientnet_lite3 (which the reference loads through torch.hub); its depthwise convolutions run in-tree
(ds_dwconv_nhwc), the rest of the network on the library routes the DPT decoders use (src/vit_mi355x.py).
"""
import torch.nn as nn

from src import vit_mi355x as vm

from .backbones.efficientnet_lite import forward_encoder, make_efficientnet_lite3_backbone
from .dpt_depth import DPTDepthModel, Interpolate, ResidualConvUnit_custom


class FeatureFusionBlock_custom(nn.Module):
    """blocks.py:382-441 with deconv=False, bn=False, ReLU(False); with expand, out_conv halves the width."""

    def __init__(self, features, expand=False, align_corners=True):
        super().__init__()
        self.align_corners = align_corners
        self.out_conv = nn.Conv2d(features, features // 2 if expand else features, kernel_size=1, stride=1, padding=0, bias=True)
        self.resConfUnit1 = ResidualConvUnit_custom(features)
        self.resConfUnit2 = ResidualConvUnit_custom(features)

    def forward(self, *xs):
        output = xs[0]
        if len(xs) == 2:                # skip add fused into the unit's last element-wise pass
            output = vm.residual_conv_unit(self.resConfUnit1.conv1, self.resConfUnit1.conv2, xs[1], skip=output)
        output = self.resConfUnit2(output)
        if output.is_cuda and not vm.STOCK[0]:
            # 1x1 out_conv and bilinear interpolation commute (linear, weights sum to one): conv first, on 4x fewer pixels
            return vm.interpolate_bilinear(vm.conv_module(self.out_conv, output), scale_factor=2, align_corners=self.align_corners)
        output = vm.interpolate_bilinear(output, scale_factor=2, align_corners=self.align_corners)
        return self.out_conv(output)


class MidasNet_small(nn.Module):
    def __init__(self, path=None, features=64, backbone="efficientnet_lite3", non_negative=True, exportable=True, channels_last=False,
                 align_corners=True, blocks={'expand': True}):
        super().__init__()
        if backbone != "efficientnet_lite3":
            raise NotImplementedError(f"MidasNet_small backbone '{backbone}' is not built (built: efficientnet_lite3)")
        # exportable: gen-efficientnet's ONNX-friendly "SAME" convolution; the pads are derived from every input here either way
        self.channels_last = channels_last
        self.blocks = blocks
        self.backbone = backbone
        self.groups = 1
        self.expand = "expand" in blocks and blocks['expand'] == True      # noqa: E712 (the reference's test)
        f1, f2, f3, f4 = (features, features * 2, features * 4, features * 8) if self.expand else (features,) * 4
        self.pretrained = make_efficientnet_lite3_backbone()
        scratch = nn.Module()
        for i, (cin, cout) in enumerate(zip((32, 48, 136, 384), (f1, f2, f3, f4))):      # _make_scratch, blocks.py:126-166
            setattr(scratch, f"layer{i + 1}_rn", nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=False))
        scratch.activation = nn.ReLU(False)
        scratch.refinenet4 = FeatureFusionBlock_custom(f4, self.expand, align_corners)
        scratch.refinenet3 = FeatureFusionBlock_custom(f3, self.expand, align_corners)
        scratch.refinenet2 = FeatureFusionBlock_custom(f2, self.expand, align_corners)
        scratch.refinenet1 = FeatureFusionBlock_custom(f1, False, align_corners)
        scratch.output_conv = nn.Sequential(
            nn.Conv2d(features, features // 2, kernel_size=3, stride=1, padding=1),
            Interpolate(scale_factor=2, mode="bilinear"),      # align_corners=False (midas_net_custom.py:61), unlike the fusion blocks
            nn.Conv2d(features // 2, 32, kernel_size=3, stride=1, padding=1),
            scratch.activation,
            nn.Conv2d(32, 1, kernel_size=1, stride=1, padding=0),
            nn.ReLU(True) if non_negative else nn.Identity(),
            nn.Identity())
        self.scratch = scratch
        if path:
            self.load(path)

    load = DPTDepthModel.load

    @vm.deterministic_forward
    def forward(self, x):               # midas_net_custom.py:73-105
        with vm.size_routed():          # the stem and the 1x1 convolutions are library calls anyway (as for vitb_rn50_384)
            l1, l2, l3, l4 = forward_encoder(self.pretrained, x)
            s = self.scratch
            l1, l2, l3, l4 = vm.conv2d(s.layer1_rn, l1), vm.conv2d(s.layer2_rn, l2), vm.conv2d(s.layer3_rn, l3), vm.conv2d(s.layer4_rn, l4)
            path_4 = s.refinenet4(l4)
            path_3 = s.refinenet3(path_4, l3)
            path_2 = s.refinenet2(path_3, l2)
            path_1 = s.refinenet1(path_2, l1)
            return s.output_conv(path_1).squeeze(dim=1)

    # estimatemidas's device-resident pre / post-processing, shared with the DPT models (resize_mode and ImageNet statistics
    # are the caller's: src/depthmap_generation.py)
    preprocess = staticmethod(DPTDepthModel.preprocess)
    infer_batch = DPTDepthModel.infer_batch
