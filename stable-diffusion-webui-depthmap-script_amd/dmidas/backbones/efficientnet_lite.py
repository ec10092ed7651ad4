"""EfficientNet-Lite3 encoder of MiDaS v2.1 small (model id 6), MI355X-first.

The reference obtains the network with `torch.hub.load("rwightman/gen-efficientnet-pytorch", "tf_efficientnet_lite3",
exportable=True)` and wraps it with `_make_efficientnet_backbone` (dmidas/blocks.py:169-189).  gen-efficientnet is neither vendored
by the reference nor a dependency of this package, so its containers are restated here from its published definition
(gen_efficientnet.py: `_gen_efficientnet_lite`, `tf_efficientnet_lite3`; efficientnet_builder.py: `round_channels`,
`make_divisible`, `_scale_stage_depth`, `DepthwiseSeparableConv`, `InvertedResidual`; conv2d_layers.py: "same" padding), with its
attribute names, so that the reference's checkpoint keys load: pretrained.layer1.0 / .1 = conv_stem / bn1, layer1.3 / .4 = block
stages 0 / 1, layer2.0 = stage 2, layer3.0 / .1 = stages 3 / 4, layer4.0 / .1 = stages 5 / 6.

Lite arch: stem 32 (not scaled), ReLU6, no squeeze-excite, BatchNorm eps 1e-3; channel multiplier 1.2 (rounded to multiples of 8),
depth multiplier 1.4 with ceil, the first and last stage not scaled:

    stage  block  kernel  first stride  repeats  width  expanded width
    stem   conv   3       2             -        32     -
    0      ds     3       1             1        24     (32)
    1      ir     3       2             3        32     144 / 192
    2      ir     5       2             3        48     192 / 288
    3      ir     3       2             5        96     288 / 576
    4      ir     5       1             5        136    576 / 816
    5      ir     5       2             6        232    816 / 1392
    6      ir     3       1             1        384    1392

TF "SAME" padding: stride-1 convolutions are plain nn.Conv2d with (k - 1) / 2 on both sides (TILING_MODE switches them to circular
padding, like the reference's hijack); stride-2 ones are `Conv2dSame`, a SUBCLASS of nn.Conv2d as in gen-efficientnet (TILING_MODE
leaves them alone), padding total = max((ceil(i / s) - 1) s + k - i, 0), total // 2 before and the rest after, from the input of
every call.

Forward (`forward_encoder`): on the CPU or under vm.stock_routing() the modules' own forwards -- convolution, BatchNorm, ReLU6 as
the reference runs them.  On the GPU every BatchNorm is folded into the convolution in front of it once per weight version, and a
block is: expand 1x1 as a library GEMM without bias -> `ds_dwconv_nhwc` (the expand's bias + ReLU6, the depthwise convolution, its
bias + ReLU6: one pass) -> project 1x1 as a library GEMM with its bias [+ the residual: one ds_bias_act pass].  The stem convolution
is a library call whose bias + ReLU6 go into the first depthwise convolution.  DS_DWCONV=0 sends the depthwise convolutions to the
library (F.conv2d with groups = channels on the folded weights; tools/midas_small_ab.py times the two).
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from src import vit_mi355x as vm

DWCONV_HIP = os.environ.get("DS_DWCONV", "1") != "0"
BN_EPS = 1e-3                                  # gen-efficientnet's BN_EPS_TF_DEFAULT (tf_ variants)
# _gen_efficientnet_lite's arch_def: ds_r1_k3_s1_e1_c16, ir_r2_k3_s2_e6_c24, ir_r2_k5_s2_e6_c40, ir_r3_k3_s2_e6_c80,
# ir_r3_k5_s1_e6_c112, ir_r4_k5_s2_e6_c192, ir_r1_k3_s1_e6_c320 as (block, repeats, kernel, stride, expansion, width)
_ARCH = (("ds", 1, 3, 1, 1, 16), ("ir", 2, 3, 2, 6, 24), ("ir", 2, 5, 2, 6, 40), ("ir", 3, 3, 2, 6, 80), ("ir", 3, 5, 1, 6, 112),
         ("ir", 4, 5, 2, 6, 192), ("ir", 1, 3, 1, 6, 320))


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def same_pads(size, k, s):
    """(before, after) of TF "SAME" padding along one axis of `size` pixels."""
    total = max((math.ceil(size / s) - 1) * s + k - size, 0)
    return total // 2, total - total // 2


class Conv2dSame(nn.Conv2d):
    """gen-efficientnet's Conv2dSame: TF "SAME" padding derived from the input of every call (the stride-2 convolutions)."""

    def __init__(self, cin, cout, k, stride, groups=1):
        super().__init__(cin, cout, k, stride=stride, padding=0, groups=groups, bias=False)

    def pads(self, x):
        """(top, bottom, left, right) for the input x."""
        return same_pads(x.shape[-2], self.kernel_size[0], self.stride[0]) + same_pads(x.shape[-1], self.kernel_size[1], self.stride[1])

    def forward(self, x):
        pt, pb, pl, pr = self.pads(x)
        return F.conv2d(F.pad(x, (pl, pr, pt, pb)), self.weight, self.bias, self.stride, 0, self.dilation, self.groups)


def _conv(cin, cout, k, stride=1, groups=1):
    if stride == 1:                            # gen-efficientnet's static "same" padding
        return nn.Conv2d(cin, cout, k, stride=1, padding=(k - 1) // 2, groups=groups, bias=False)
    return Conv2dSame(cin, cout, k, stride, groups)


class DepthwiseSeparableConv(nn.Module):
    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.has_residual = stride == 1 and cin == cout
        self.conv_dw = _conv(cin, cin, k, stride, groups=cin)
        self.bn1 = nn.BatchNorm2d(cin, eps=BN_EPS)
        self.act1 = nn.ReLU6(inplace=True)
        self.conv_pw = _conv(cin, cout, 1)
        self.bn2 = nn.BatchNorm2d(cout, eps=BN_EPS)

    def forward(self, x):
        y = self.bn2(self.conv_pw(self.act1(self.bn1(self.conv_dw(x)))))
        return y + x if self.has_residual else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, k, stride, exp_ratio):
        super().__init__()
        mid = make_divisible(cin * exp_ratio)
        self.has_residual = stride == 1 and cin == cout
        self.conv_pw = _conv(cin, mid, 1)
        self.bn1 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.act1 = nn.ReLU6(inplace=True)
        self.conv_dw = _conv(mid, mid, k, stride, groups=mid)
        self.bn2 = nn.BatchNorm2d(mid, eps=BN_EPS)
        self.act2 = nn.ReLU6(inplace=True)
        self.conv_pwl = _conv(mid, cout, 1)
        self.bn3 = nn.BatchNorm2d(cout, eps=BN_EPS)

    def forward(self, x):
        y = self.act2(self.bn2(self.conv_dw(self.act1(self.bn1(self.conv_pw(x))))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.has_residual else y


class EfficientNetLite(nn.Module):
    """conv_stem, bn1, act1 and the block stages of gen-efficientnet's GenEfficientNet for tf_efficientnet_lite3 (its head --
    conv_head, bn2, classifier -- is dropped by _make_efficientnet_backbone and not built)."""

    def __init__(self, channel_multiplier=1.2, depth_multiplier=1.4, stem_size=32):
        super().__init__()
        self.conv_stem = _conv(3, stem_size, 3, 2)
        self.bn1 = nn.BatchNorm2d(stem_size, eps=BN_EPS)
        self.act1 = nn.ReLU6(inplace=True)
        stages, cin = [], stem_size
        for i, (kind, reps, k, s, e, c) in enumerate(_ARCH):
            if 0 < i < len(_ARCH) - 1:
                reps = int(math.ceil(reps * depth_multiplier))
            cout = make_divisible(c * channel_multiplier)
            blocks = []
            for r in range(reps):
                stride = s if r == 0 else 1
                blocks.append(DepthwiseSeparableConv(cin, cout, k, stride) if kind == "ds" else InvertedResidual(cin, cout, k, stride, e))
                cin = cout
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)


def make_efficientnet_lite3_backbone():
    """_make_efficientnet_backbone (dmidas/blocks.py:179-189) of tf_efficientnet_lite3: the reference's Sequential indices."""
    effnet = EfficientNetLite()
    pretrained = nn.Module()
    pretrained.layer1 = nn.Sequential(effnet.conv_stem, effnet.bn1, effnet.act1, *effnet.blocks[0:2])
    pretrained.layer2 = nn.Sequential(*effnet.blocks[2:3])
    pretrained.layer3 = nn.Sequential(*effnet.blocks[3:5])
    pretrained.layer4 = nn.Sequential(*effnet.blocks[5:9])
    return pretrained


# ---- the folded GPU route ------------------------------------------------------------------------------------------------------
def _bn_fold(conv, bn):
    """float32 (weight, bias) of conv -> BatchNorm in inference mode."""
    scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
    return conv.weight.float() * scale.view(-1, 1, 1, 1), bn.bias.float() - bn.running_mean.float() * scale


def _pw_operands(conv, bn, dtype, flat=True):
    w, b = _bn_fold(conv, bn)
    return {"w": (w.reshape(w.shape[0], -1) if flat else w).to(dtype).contiguous(), "b": b.to(dtype), "b32": b.contiguous()}


def _dw_operands(conv, bn, dtype):
    w, b = _bn_fold(conv, bn)
    k2 = w.shape[2] * w.shape[3]
    return {"taps": w.reshape(w.shape[0], k2).t().contiguous(), "b32": b.contiguous(), "w": w.to(dtype), "b": b.to(dtype)}


def _cached(holder, modules, dtype, build):
    """The folded operands of `modules`, cached on `holder` per weight version and dtype.  A captured hipGraph holds pointers to
    them: replacing an entry moves vm's cache epoch, which makes GraphedForward capture again."""
    key = (dtype,) + tuple((t.data_ptr(), t._version) for m in modules for t in (*m.parameters(), *m.buffers()))
    hit = getattr(holder, "_ds_fold", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = build()
    if not torch.is_grad_enabled():
        if hit is not None:
            vm.cache_evicted()
        holder._ds_fold = (key, value)
    return value


def _pointwise(x, w, b=None):
    """1x1 convolution of a channels_last activation as ONE library GEMM on its NHWC rows (no copy on either side)."""
    n, c, h, wd = x.shape
    y = F.linear(x.permute(0, 2, 3, 1).reshape(-1, c), w, b)
    return y.view(n, h, wd, -1).permute(0, 3, 1, 2)


def _dwconv(conv, x, dw, pre):
    """relu6(bn(conv(relu6(x + bias)))) with both BatchNorms folded: x is the PRE-activation of the convolution in front, `pre`
    its folded bias (the operands of _pw_operands), dw the depthwise convolution's (_dw_operands)."""
    k, s = conv.kernel_size[0], conv.stride[0]
    h, w = x.shape[-2:]
    if isinstance(conv, Conv2dSame):
        pt, pb, pl, pr = conv.pads(x)
    else:
        pt = pb = pl = pr = conv.padding[0]
    oh, ow = (h + pt + pb - k) // s + 1, (w + pl + pr - k) // s + 1
    if DWCONV_HIP and conv.padding_mode == 'zeros' and x.shape[1] % 8 == 0:
        from src import _native
        return _native.dwconv(x, dw["taps"], pre["b32"], dw["b32"], k, s, pt, pl, (oh, ow))
    a = (x + pre["b"].view(1, -1, 1, 1)).clamp_(0.0, 6.0)
    if conv.padding_mode == 'zeros' and (pt, pl) == (pb, pr):
        y = F.conv2d(a, dw["w"], dw["b"], s, (pt, pl), 1, conv.groups)
    else:                                      # SAME pads of the stride-2 convolutions; TILING_MODE's circular padding
        mode = 'constant' if conv.padding_mode == 'zeros' else conv.padding_mode
        y = F.conv2d(F.pad(a, (pl, pr, pt, pb), mode=mode), dw["w"], dw["b"], s, 0, 1, conv.groups)
    return y.clamp_(0.0, 6.0)


def _ir_fused(blk, x):
    P = _cached(blk, (blk,), x.dtype, lambda: {"pw": _pw_operands(blk.conv_pw, blk.bn1, x.dtype), "dw": _dw_operands(blk.conv_dw, blk.bn2, x.dtype),
                                               "pwl": _pw_operands(blk.conv_pwl, blk.bn3, x.dtype)})
    d = _dwconv(blk.conv_dw, _pointwise(x, P["pw"]["w"]), P["dw"], P["pw"])
    if not blk.has_residual:
        return _pointwise(d, P["pwl"]["w"], P["pwl"]["b"])
    from src import _native
    y = _pointwise(d, P["pwl"]["w"])
    if y.dtype == torch.float32:
        return _native.bias_act_f32(y, P["pwl"]["b32"], relu=False, res=x)
    return _native.bias_act(y, P["pwl"]["b"], relu=False, res1=x)


def _forward_fused(pretrained, x):
    x = x.contiguous(memory_format=torch.channels_last)
    l1 = pretrained.layer1
    conv_stem, stage0 = l1[0], l1[3]
    stem = _cached(conv_stem, (conv_stem, l1[1]), x.dtype, lambda: _pw_operands(conv_stem, l1[1], x.dtype, flat=False))
    pt, pb, pl, pr = conv_stem.pads(x)
    s = F.conv2d(F.pad(x, (pl, pr, pt, pb)).contiguous(memory_format=torch.channels_last), stem["w"], None, conv_stem.stride)
    s = s.contiguous(memory_format=torch.channels_last)
    # stage 0: one DepthwiseSeparableConv 32 -> 24 (no residual); the stem's bias + ReLU6 enter its depthwise convolution
    ds = stage0[0]
    P = _cached(ds, (ds,), x.dtype, lambda: {"dw": _dw_operands(ds.conv_dw, ds.bn1, x.dtype), "pw": _pw_operands(ds.conv_pw, ds.bn2, x.dtype)})
    h = _pointwise(_dwconv(ds.conv_dw, s, P["dw"], stem), P["pw"]["w"], P["pw"]["b"])
    for blk in l1[4]:
        h = _ir_fused(blk, h)
    taps = [h]
    for layer in (pretrained.layer2, pretrained.layer3, pretrained.layer4):
        for stage in layer:
            for blk in stage:
                h = _ir_fused(blk, h)
        taps.append(h)
    return taps


def forward_encoder(pretrained, x):
    """The outputs of pretrained.layer1 .. layer4 (midas_net_custom.py:87-90)."""
    if (not x.is_cuda or vm.STOCK[0]
            or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in pretrained.parameters())))):
        l1 = pretrained.layer1(x)
        l2 = pretrained.layer2(l1)
        l3 = pretrained.layer3(l2)
        return l1, l2, l3, pretrained.layer4(l3)
    return tuple(_forward_fused(pretrained, x))
