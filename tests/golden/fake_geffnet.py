"""TEST INFRASTRUCTURE -- a stand-in for gen-efficientnet (rwightman/gen-efficientnet-pytorch), which the reference fetches with
`torch.hub.load(..., "tf_efficientnet_lite3", pretrained=..., exportable=True)` (dmidas/blocks.py:169-176) and which is neither
vendored by the reference nor installed where the goldens are made.  Just enough of `tf_efficientnet_lite3` for the REFERENCE's own
MidasNet_small to run: gen-efficientnet's containers with its attribute names (GenEfficientNet: conv_stem, bn1, act1, blocks;
DepthwiseSeparableConv; InvertedResidual) and their forwards, restated from the published definition (gen_efficientnet.py,
efficientnet_builder.py, conv2d_layers.py).  The head (conv_head, bn2, classifier) is left out: _make_efficientnet_backbone drops it.
The stride-2 convolutions are Conv2dSameExport, the exportable variant, whose zero pad is derived from the FIRST input it sees and
then kept: a golden builds one fresh model per input size.  Written apart from dmidas/backbones/efficientnet_lite.py; what the two
restatements agree on is pinned by the goldens, their fidelity to gen-efficientnet is not.  `pretrained=True` is accepted and
ignored (no weights here: the goldens load name-seeded ones).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

_LITE_ARCH = [['ds_r1_k3_s1_e1_c16'], ['ir_r2_k3_s2_e6_c24'], ['ir_r2_k5_s2_e6_c40'], ['ir_r3_k3_s2_e6_c80'],
              ['ir_r3_k5_s1_e6_c112'], ['ir_r4_k5_s2_e6_c192'], ['ir_r1_k3_s1_e6_c320']]       # _gen_efficientnet_lite


def make_divisible(v, divisor=8, min_value=None):
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def round_channels(channels, multiplier=1.0, divisor=8):
    return make_divisible(channels * multiplier, divisor)


def _same_pad_arg(input_size, kernel_size, stride, dilation):
    ih, iw = input_size
    kh, kw = kernel_size
    pad_h = max((math.ceil(ih / stride[0]) - 1) * stride[0] + (kh - 1) * dilation[0] + 1 - ih, 0)
    pad_w = max((math.ceil(iw / stride[1]) - 1) * stride[1] + (kw - 1) * dilation[1] + 1 - iw, 0)
    return [pad_w // 2, pad_w - pad_w // 2, pad_h // 2, pad_h - pad_h // 2]


class Conv2dSameExport(nn.Conv2d):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, dilation=1, groups=1, bias=True):
        super().__init__(in_channels, out_channels, kernel_size, stride, 0, dilation, groups, bias)
        self.pad = None
        self.pad_input_size = (0, 0)

    def forward(self, x):
        input_size = x.size()[-2:]
        if self.pad is None:
            self.pad = nn.ZeroPad2d(_same_pad_arg(input_size, self.weight.size()[-2:], self.stride, self.dilation))
            self.pad_input_size = input_size
        x = self.pad(x)
        return F.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)


def create_conv2d(in_chs, out_chs, kernel_size, stride=1, depthwise=False):
    """pad_type 'same': static symmetric padding where it is static (stride 1, odd kernel), the exportable dynamic one otherwise."""
    groups = out_chs if depthwise else 1
    if stride == 1 and (kernel_size - 1) % 2 == 0:
        return nn.Conv2d(in_chs, out_chs, kernel_size, stride=1, padding=(kernel_size - 1) // 2, groups=groups, bias=False)
    return Conv2dSameExport(in_chs, out_chs, kernel_size, stride=stride, groups=groups, bias=False)


class DepthwiseSeparableConv(nn.Module):
    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, bn_eps=1e-3):
        super().__init__()
        self.has_residual = stride == 1 and in_chs == out_chs
        self.conv_dw = create_conv2d(in_chs, in_chs, dw_kernel_size, stride=stride, depthwise=True)
        self.bn1 = nn.BatchNorm2d(in_chs, eps=bn_eps)
        self.act1 = nn.ReLU6(inplace=True)
        self.se = nn.Identity()
        self.conv_pw = create_conv2d(in_chs, out_chs, 1)
        self.bn2 = nn.BatchNorm2d(out_chs, eps=bn_eps)
        self.act2 = nn.Identity()

    def forward(self, x):
        residual = x
        x = self.act1(self.bn1(self.conv_dw(x)))
        x = self.se(x)
        x = self.act2(self.bn2(self.conv_pw(x)))
        if self.has_residual:
            x += residual
        return x


class InvertedResidual(nn.Module):
    def __init__(self, in_chs, out_chs, dw_kernel_size=3, stride=1, exp_ratio=1.0, bn_eps=1e-3):
        super().__init__()
        mid_chs = make_divisible(in_chs * exp_ratio)
        self.has_residual = in_chs == out_chs and stride == 1
        self.conv_pw = create_conv2d(in_chs, mid_chs, 1)
        self.bn1 = nn.BatchNorm2d(mid_chs, eps=bn_eps)
        self.act1 = nn.ReLU6(inplace=True)
        self.conv_dw = create_conv2d(mid_chs, mid_chs, dw_kernel_size, stride=stride, depthwise=True)
        self.bn2 = nn.BatchNorm2d(mid_chs, eps=bn_eps)
        self.act2 = nn.ReLU6(inplace=True)
        self.se = nn.Identity()
        self.conv_pwl = create_conv2d(mid_chs, out_chs, 1)
        self.bn3 = nn.BatchNorm2d(out_chs, eps=bn_eps)

    def forward(self, x):
        residual = x
        x = self.act1(self.bn1(self.conv_pw(x)))
        x = self.act2(self.bn2(self.conv_dw(x)))
        x = self.se(x)
        x = self.bn3(self.conv_pwl(x))
        if self.has_residual:
            x += residual
        return x


def _decode_arch(arch_def, depth_multiplier):
    """decode_arch_def(..., depth_trunc='ceil', fix_first_last=True) for one block string per stage."""
    out = []
    for i, (block_str,) in enumerate(arch_def):
        ops = block_str.split('_')
        opt = {o[0]: int(o[1:]) for o in ops[1:]}
        reps = opt['r'] if i in (0, len(arch_def) - 1) else int(math.ceil(opt['r'] * depth_multiplier))
        out.append((ops[0], reps, opt['k'], opt['s'], opt['e'], opt['c']))
    return out


class GenEfficientNet(nn.Module):
    def __init__(self, arch, channel_multiplier, stem_size=32, bn_eps=1e-3):
        super().__init__()
        self.conv_stem = create_conv2d(3, stem_size, 3, stride=2)           # fix_stem: not scaled
        self.bn1 = nn.BatchNorm2d(stem_size, eps=bn_eps)
        self.act1 = nn.ReLU6(inplace=True)
        in_chs, stages = stem_size, []
        for kind, reps, k, s, e, c in arch:
            out_chs = round_channels(c, channel_multiplier)
            blocks = []
            for r in range(reps):
                stride = s if r == 0 else 1
                blocks.append(DepthwiseSeparableConv(in_chs, out_chs, k, stride, bn_eps) if kind == 'ds'
                              else InvertedResidual(in_chs, out_chs, k, stride, e, bn_eps))
                in_chs = out_chs
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)


def tf_efficientnet_lite3(pretrained=False, exportable=True, **kwargs):
    return GenEfficientNet(_decode_arch(_LITE_ARCH, 1.4), channel_multiplier=1.2)


def install():
    """Route torch.hub.load("rwightman/gen-efficientnet-pytorch", "tf_efficientnet_lite3", ...) to the stand-in."""
    def load(repo, model, *args, **kwargs):
        if repo == "rwightman/gen-efficientnet-pytorch" and model == "tf_efficientnet_lite3":
            return tf_efficientnet_lite3(*args, **kwargs)
        raise RuntimeError(f"torch.hub.load({repo!r}, {model!r}) has no stand-in")
    torch.hub.load = load
