"""GPU tests of the forward's two ends (csrc/ds_forward_ends.hip).  Every new pass replaces a chain of passes and must leave the SAME
BITS, so every comparison is torch.equal against the chain it replaces:

    ds_preprocess_bicubic_rows          ds_preprocess_bicubic + the patch gather of vm.patch_embed_tokens, zero rows / columns around it
    ds_linear on those rows + ds_tokens_fixup     pad_tokens(cat(cls, patch_embed_tokens(x)))
    ds_upsample_bicubic_to_f32          F.interpolate(mode="bicubic", align_corners=False) on the half tensor, then .float()
    ds_im2col3x3_s2_nhwc                F.pad + NHWC copy + as_strided rows of vm.strided3x3_rows

Shapes are the smallest that reach every path of each kernel: non-integer scales, upsampling (replicated borders), a row pitch and a
base address that are no multiple of 4 bytes, a source region too large for LDS (the generic paths), more than one tile per axis,
partial tiles, and pixels beyond the patch grid."""
import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


def _image(b, h, w, seed, offset=0):
    """uint8 [b, h, w, 3] on the GPU whose first byte sits `offset` bytes past an aligned address."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randint(0, 256, (offset + b * h * w * 3,), generator=g, dtype=torch.uint8).cuda()
    return flat[offset:].view(b, h, w, 3)


def _gather_rows(x, p, n_pad, kpad):
    """[B, 3, H, W] network input -> the operand ds_preprocess_bicubic_rows must write (the gather of vm.patch_embed_tokens inside)."""
    b, c, h, w = x.shape
    gh, gw = h // p, w // p
    xv = x.permute(0, 2, 3, 1)[:, :gh * p, :gw * p].reshape(b, gh, p, gw, p, c).permute(0, 1, 3, 2, 4, 5)
    want = x.new_zeros((b, n_pad, kpad))
    want[:, 1:1 + gh * gw, :p * p * c] = xv.reshape(b, gh * gw, p * p * c)
    return want


# (input h x w, network h x w, patch, n_pad, byte offset of the image): the metric's exact 2:1; a non-integer scale with a row pitch
# of 210 bytes on an odd base address; upsampling (borders); p = 14 with kpad 640; the same with pixels beyond the patch grid;
# rows shrunk 9.4 : 1 (no LDS room: the generic path); three strips of patches per row with a partial last strip
PRE_CASES = [((64, 96), (32, 48), 16, 8, 0), ((45, 70), (32, 48), 16, 16, 3), ((20, 30), (32, 48), 16, 8, 1),
             ((61, 35), (28, 42), 14, 8, 0), ((61, 35), (30, 45), 14, 8, 0), ((300, 40), (32, 48), 16, 8, 2),
             ((50, 300), (16, 144), 16, 16, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("case", PRE_CASES)
def test_preprocess_rows_equals_preprocess_then_gather(gpu, case, flip, dtype):
    from src import _native
    (ih, iw), (oh, ow), p, n_pad, offset = case
    img = _image(2, ih, iw, seed=ih * 7 + iw, offset=offset)
    mean, std = (0.5, 0.5) if flip else ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    kpad = (3 * p * p + 127) // 128 * 128
    assert n_pad >= 1 + (oh // p) * (ow // p)
    x = _native.preprocess_bicubic(img, (oh, ow), mean, std, flip=flip, dtype=dtype)
    want = _gather_rows(x, p, n_pad, kpad)
    out = torch.full((2 * n_pad * kpad * 2,), 0x7f, dtype=torch.uint8, device="cuda").view(dtype).view(2, n_pad, kpad)
    got = _native.preprocess_bicubic_rows(img, (oh, ow), mean, std, p, n_pad, kpad, flip=flip, dtype=dtype, out=out)
    assert got is out and torch.equal(got, want)
    gg = (oh // p) * (ow // p)
    # the zeros are written by the kernel (the buffer held 0x7f bytes), and the patch rows are not all zero
    assert not got[:, 0].any() and not got[:, 1 + gg:].any() and not got[:, :, 3 * p * p:].any() and got[:, 1:1 + gg].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_buffer_equals_cat_and_pad(gpu, dtype):
    """Conv2d(3, 256, 16, 16) on a 12 x 12 grid, B = 2: 145 tokens in a stride of 192 -- 384 GEMM rows, one full panel and a partial one."""
    from src import _native
    from src import vit_mi355x as vm
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(3, 256, 16, 16).cuda().to(dtype)
    cls = (torch.randn(1, 1, 256) * 0.5).cuda().to(dtype)
    img = _image(2, 200, 210, seed=11)
    grid, n_valid, n_pad, kpad = vm.patch_rows_geometry(conv, (192, 192), 2)
    assert (grid, n_valid, n_pad, kpad) == ((12, 12), 145, 192, 768) and vm.patch_rows_ok(conv, dtype, (192, 192))
    with torch.no_grad():
        x = _native.preprocess_bicubic(img, (192, 192), 0.5, 0.5, flip=True, dtype=dtype)
        assert vm.patch_embed_hip_ok(conv, x)
        t = vm.patch_embed_tokens(conv, x)
        want = vm.pad_tokens(torch.cat((cls.expand(2, -1, -1), t), dim=1), n_pad)
        rows = _native.preprocess_bicubic_rows(img, (192, 192), 0.5, 0.5, 16, n_pad, kpad, flip=True, dtype=dtype)
        got = vm.patch_rows_tokens(conv, cls, rows, n_valid)
    assert got.shape == want.shape == (2, 192, 256) and torch.equal(got, want)
    assert torch.equal(got[:, 0], cls.view(1, 256).expand(2, -1)) and not got[:, n_valid:].any()


def _tail_inputs(shape, kind, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "signed":
        x = torch.randn(shape, generator=g) * 20
    elif kind == "constant":
        x = torch.full(shape, 3.3203125)
    else:                                   # magnitudes near 6e4: the cubic overshoot passes float16's largest finite value
        x = (torch.rand(shape, generator=g) * 1e4 + 5.5e4) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return x.cuda().to(dtype)


# the issue's shapes; then several tiles per axis with partial ones, downsampling (no LDS room: the generic path), equal sizes (a copy)
TAIL_CASES = [((2, 5, 7), (10, 14)), ((2, 5, 7), (11, 13)), ((1, 16, 16), (32, 32)), ((1, 40, 90), (70, 150)), ((1, 50, 60), (20, 25)),
              ((1, 6, 7), (6, 7))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["signed", "constant", "large"])
@pytest.mark.parametrize("shape,size", TAIL_CASES)
def test_depth_tail_equals_torch_bicubic_then_float(gpu, shape, size, kind, dtype):
    from src import _native
    x = _tail_inputs(shape, kind, dtype, seed=shape[1] * 31 + size[0])
    want = F.interpolate(x[:, None], size=size, mode="bicubic", align_corners=False)[:, 0].float()
    got = _native.upsample_bicubic_to_f32(x, size)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert not torch.isnan(want).any()
    if kind == "large" and dtype == torch.float16 and size != shape[1:]:
        assert torch.isinf(want).any(), "the case is meant to reach +-inf in the half rounding"
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("hw", [(6, 6), (5, 7)])
def test_im2col_equals_pad_and_strided_view(gpu, hw, circular, dtype):
    from src import vit_mi355x as vm
    g = torch.Generator().manual_seed(hw[1])
    x = torch.randn((2, 128) + hw, generator=g).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    want = vm.strided3x3_rows(x, circular, hip=False)
    got = vm.strided3x3_rows(x, circular, hip=True)
    ho, wo = (hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1
    assert got.shape == want.shape == (2 * ho * wo, 9 * 128) and torch.equal(got, want)


def test_infer_batch_takes_the_new_passes_and_keeps_every_bit(gpu):
    """dpt_beit_large_512 at batch 8, float16 (every GEMM and convolution in-tree, so a forward is reproducible bit for bit): infer_batch
    with the three switches on against the same call with all of them off, and the counters of the binding for the route it took."""
    from dmidas.dpt_depth import DPTDepthModel
    from src import _native
    from src import vit_mi355x as vm
    torch.manual_seed(3)
    m = DPTDepthModel(path=None, backbone="beitl16_512", non_negative=True).eval().cuda().half()
    img = _image(8, 96, 112, seed=23)
    names = ("ds_preprocess_bicubic_rows", "ds_tokens_fixup", "ds_upsample_bicubic_to_f32", "ds_im2col3x3_s2_nhwc", "ds_preprocess_bicubic")
    saved = vm.PATCH_ROWS, vm.DEPTH_TAIL, vm.IM2COL_HIP
    try:
        outs = []
        for on in (True, False):
            vm.PATCH_ROWS = vm.DEPTH_TAIL = vm.IM2COL_HIP = on
            before = dict(_native.CALLS)
            outs.append(m.infer_batch(img, net_size=512, resize_mode="minimal"))
            calls = {n: _native.CALLS[n] - before.get(n, 0) for n in names}
            if on:
                assert calls == {"ds_preprocess_bicubic_rows": 1, "ds_tokens_fixup": 1, "ds_upsample_bicubic_to_f32": 1,
                                 "ds_im2col3x3_s2_nhwc": 1, "ds_preprocess_bicubic": 0}, calls
            else:
                assert calls == {"ds_preprocess_bicubic_rows": 0, "ds_tokens_fixup": 0, "ds_upsample_bicubic_to_f32": 0,
                                 "ds_im2col3x3_s2_nhwc": 0, "ds_preprocess_bicubic": 1}, calls
    finally:
        vm.PATCH_ROWS, vm.DEPTH_TAIL, vm.IM2COL_HIP = saved
    assert outs[0].dtype == torch.float32 and outs[0].shape == (8, 96, 112) and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
