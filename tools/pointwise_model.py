"""float32 restatements, on the CPU, of four single-pass kernels in the kernels' own order of operations:

    bias_act              k_bias_act_nhwc           (csrc/ds_encoder_ops.hip)
    reassemble_readout    k_reassemble_readout      (csrc/ds_encoder_ops.hip)
    preprocess_bicubic    k_preprocess_bicubic      (csrc/ds_encoder_ops.hip, pre_cubic of csrc/ds_common.h)
    gconv3x3              k_gconv3x3_nhwc_f32       (csrc/ds_gconv.hip)

Each takes `mutant`: None is the faithful restatement; a name from MUTANTS changes ONE thing a kernel could get subtly wrong.
tests/test_pointwise_model_cpu.py runs the checkers of tests/pointwise_cases.py on both: the faithful restatement passes every case,
every mutant is rejected -- the evidence, without a GPU, that tests/test_gpu_pointwise_exact.py would notice such a kernel."""
import numpy as np
import torch

MUTANTS = {
    "bias_act": ("round_between_residuals", "relu_before_residuals", "relu_nan_to_zero"),
    "reassemble_readout": ("tanh_gelu", "no_storage_rounding", "cls0_for_every_image"),
    "preprocess_bicubic": ("cubic_a_minus_half", "no_half_pixel_offset", "clamp_to_n_minus_2", "unflipped_mean_std"),
    "gconv3x3": ("taps_transposed", "block_shifted_one_group", "edge_replication"),
}


def _known(kernel, mutant):
    assert mutant is None or mutant in MUTANTS[kernel], (kernel, mutant)


def _relu(f, nan_to_zero=False):
    """f < 0 ? 0 : f -- a NaN stays NaN; nan_to_zero: f > 0 ? f : 0."""
    zero = torch.zeros_like(f)
    return torch.where(f > 0, f, zero) if nan_to_zero else torch.where(f < 0, zero, f)


def bias_act(x, bias, res1, res2, relu, mutant=None):
    """x, res1, res2 [pixels, channels], bias [channels] of one half-precision type (res1 / res2 may be None).  Returns x's type."""
    _known("bias_act", mutant)
    dtype = x.dtype
    f = x.float() + bias.float()[None, :]
    if relu and mutant == "relu_before_residuals":
        f = _relu(f)
    if res1 is not None:
        f = f + res1.float()
    if res2 is not None:
        if mutant == "round_between_residuals":
            f = f.to(dtype).float()
        f = f + res2.float()
    if relu and mutant != "relu_before_residuals":
        f = _relu(f, nan_to_zero=mutant == "relu_nan_to_zero")
    return f.to(dtype)


def reassemble_readout(proj, cls, mutant=None):
    """proj [B, N, C], cls [B, C] of one half-precision type -> gelu(proj[:, 1:] + cls[:, None]) [B, N - 1, C]."""
    _known("reassemble_readout", mutant)
    dtype = proj.dtype
    c = cls[:1].expand_as(cls) if mutant == "cls0_for_every_image" else cls
    x = proj[:, 1:].float() + c.float()[:, None, :]
    if mutant != "no_storage_rounding":
        x = x.to(dtype).float()
    if mutant == "tanh_gelu":
        y = torch.nn.functional.gelu(x, approximate="tanh")
    else:
        y = 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))          # float32 tensors: the scalars become float32
    assert y.dtype == torch.float32
    return y.to(dtype)


def _cubic(t, a):
    f32 = np.float32
    x0, x3, x2 = t + f32(1.0), f32(2.0) - t, f32(1.0) - t
    return [((a * x0 - f32(5.0) * a) * x0 + f32(8.0) * a) * x0 - f32(4.0) * a,
            ((a + f32(2.0)) * t - (a + f32(3.0))) * t * t + f32(1.0),
            ((a + f32(2.0)) * x2 - (a + f32(3.0))) * x2 * x2 + f32(1.0),
            ((a * x3 - f32(5.0) * a) * x3 + f32(8.0) * a) * x3 - f32(4.0) * a]


def _axis(n_in, n_out, mutant):
    f32 = np.float32
    o = np.arange(n_out, dtype=np.float32)
    s = f32(n_in) / f32(n_out)
    f = s * o if mutant == "no_half_pixel_offset" else s * (o + f32(0.5)) - f32(0.5)
    f0 = np.floor(f)
    c = _cubic(f - f0, f32(-0.5) if mutant == "cubic_a_minus_half" else f32(-0.75))
    top = max(n_in - 2, 0) if mutant == "clamp_to_n_minus_2" else n_in - 1
    idx = [np.clip(f0.astype(np.int64) - 1 + k, 0, top) for k in range(4)]
    return idx, c


def preprocess_bicubic(img, size, mean, std, flip, dtype, mutant=None):
    """img uint8 [B, H, W, 3] (numpy), mean / std float32 [3] -> [B, 3, oh, ow] tensor of `dtype`: h += cx[kx] * (px / 255) over kx,
    acc += cy[ky] * h over ky, (acc[flip ? 2 - c : c] - mean[c]) * (1 / std[c]), every operation in float32."""
    _known("preprocess_bicubic", mutant)
    f32 = np.float32
    oh, ow = size
    iy, cy = _axis(img.shape[1], oh, mutant)
    ix, cx = _axis(img.shape[2], ow, mutant)
    px = img.astype(np.float32) / f32(255.0)
    acc = np.zeros((img.shape[0], oh, ow, 3), np.float32)
    for ky in range(4):
        h = np.zeros_like(acc)
        for kx in range(4):
            h = h + cx[kx][None, None, :, None] * px[:, iy[ky][:, None], ix[kx][None, :]]
        acc = acc + cy[ky][None, :, None, None] * h
    if flip:
        acc = acc[..., ::-1]
    m, istd = np.asarray(mean, np.float32), f32(1.0) / np.asarray(std, np.float32)
    if mutant == "unflipped_mean_std" and flip:
        m, istd = m[::-1], istd[::-1]
    o = (acc - m) * istd
    assert o.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(o.transpose(0, 3, 1, 2))).to(dtype)


def gconv3x3(x, w_gtio, bias, relu, cpg, mutant=None):
    """x float32 [B, H, W, C] (NHWC), w_gtio [C / cpg][9][cpg in][cpg out], bias [C] or None -> [B, H, W, C]: acc = bias, then one FMA
    per (tap, input channel) in that order (the product is exact in float64, the sum is rounded to float32), ReLU last."""
    _known("gconv3x3", mutant)
    x, w = x.double(), w_gtio.double()
    b, h, wd, c = x.shape
    g = c // cpg
    xp = x.permute(0, 3, 1, 2)
    pad = torch.nn.functional.pad(xp, (1, 1, 1, 1), mode="replicate") if mutant == "edge_replication" else torch.nn.functional.pad(xp, (1, 1, 1, 1))
    pad = pad.permute(0, 2, 3, 1).reshape(b, h + 2, wd + 2, g, cpg)
    if mutant == "block_shifted_one_group":
        pad = torch.roll(pad, -1, dims=3)
    acc = torch.zeros((b, h, wd, g, cpg), dtype=torch.float64)                       # float64 storage of float32 values
    if bias is not None:
        acc += bias.double().view(1, 1, 1, g, cpg)
    for tap in range(9):
        dy, dx = (tap % 3, tap // 3) if mutant == "taps_transposed" else (tap // 3, tap % 3)
        src = pad[:, dy:dy + h, dx:dx + wd]
        for ci in range(cpg):
            acc = torch.addcmul(acc, src[..., ci:ci + 1], w[None, None, None, :, tap, ci, :]).float().double()
    y = acc.float().reshape(b, h, wd, c)
    return _relu(y) if relu else y
