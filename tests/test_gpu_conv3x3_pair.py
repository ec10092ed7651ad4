"""GPU tests of ds_conv3x3_nhwc_pair (csrc/ds_linear.hip: k_linear256<.., VT 5>): two bias-free 3x3 convolutions with common
channels in one persistent walk over both tile lists.

Operands are exact integers: x, w in {-1, 0, 1}, C = 128 (the smallest the convolution kernels take: K = 9 C must be an even number
of 64-wide K-tiles), so |y| <= 9 * 128 = 1152 and every product, every partial sum in any order and the result are representable in
float16 (integers are exact to 2048).  Each output must equal the float64 convolution on the CPU bit for bit -- a dropped, duplicated
or misplaced tile, a tap taken across an image border or from the other segment's geometry is a whole-number difference -- and it must
be torch.equal to the route it replaces, one _native.conv3x3 call per convolution (where that entry point takes the shape: it needs
256 pixels).

Segment 0 is 4 x 16 x 16 (4 tiles); segment 1 is 4 x 8 x 8 (one full tile) or 3 x 8 x 8 (192 pixels: a partial tile whose last 64
rows read the zero line and go to the dummy row).  16 + 1 tiles on 8 workgroups make one workgroup walk from the last tile of
segment 0 into segment 1."""
import os

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu
ENV = ("DS_LIN_GRID", "DS_LIN_EARLY")
C, N = 128, 256


@pytest.fixture
def lin_env(gpu):
    from src import _native
    old = {k: os.environ.get(k) for k in ENV}
    try:
        yield _native
    finally:
        _native.linear_env(**old)


def _conv(seed):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(C, N, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-1, 2, (N, C, 3, 3), generator=g).float())
    return conv


def _image(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (shape[0], C, shape[1], shape[2]), generator=g).double()


def _run_and_check(nat, shape0, shape1, seed):
    conv0, conv1 = _conv(seed), _conv(seed + 1)
    x0, x1 = _image(shape0, seed + 2), _image(shape1, seed + 3)
    want = [F.conv2d(x, c.weight.double(), padding=1) for c, x in ((conv0, x0), (conv1, x1))]
    assert max(w.abs().max().item() for w in want) <= 2048
    c0, c1 = conv0.cuda().half(), conv1.cuda().half()
    d0, d1 = (x.half().cuda().contiguous(memory_format=torch.channels_last) for x in (x0, x1))
    assert nat.conv3x3_pair_supported(c0, d0, c1, d1)
    before = dict(nat.CALLS)
    got = nat.conv3x3_pair(c0, d0, c1, d1)
    torch.cuda.synchronize()
    assert nat.CALLS["ds_conv3x3_nhwc_pair"] == before.get("ds_conv3x3_nhwc_pair", 0) + 1
    assert nat.CALLS["ds_conv3x3_nhwc"] == before.get("ds_conv3x3_nhwc", 0) + 2
    for i, (g, w, c, d) in enumerate(zip(got, want, (c0, c1), (d0, d1))):
        worst = (g.double().cpu() - w).abs().max().item()
        print(f"ds_conv3x3_nhwc_pair segment {i} {tuple(d.shape)}: worst |got - exact| {worst}")
        assert g.shape == w.shape and g.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(g.cpu(), w.half()), f"segment {i} differs from the exact integer convolution"
        if nat.conv3x3_supported(c, d):
            assert torch.equal(g, nat.conv3x3(c, d)), f"segment {i} differs from the single-convolution launch"


@pytest.mark.parametrize("grid", ["8", None], ids=["grid8", "default_grid"])
@pytest.mark.parametrize("batch1", [4, 3], ids=["full_tile", "partial_tile"])
def test_four_tiles_and_one(lin_env, grid, batch1):
    lin_env.linear_env(DS_LIN_GRID=grid)
    _run_and_check(lin_env, (4, 16, 16), (batch1, 8, 8), seed=20 + batch1)


@pytest.mark.parametrize("early", ["1", "0"])
def test_workgroup_that_walks_from_segment_0_into_segment_1(lin_env, early):
    """16 + 1 tiles on 8 workgroups: the workgroup of the list's last range renders tile 15 (segment 0) and then tile 16 (segment 1,
    partial) -- in early mode set_tile(next) switches the geometry while the first tile's epilogue is still to run."""
    lin_env.linear_env(DS_LIN_GRID="8", DS_LIN_EARLY=early)
    _run_and_check(lin_env, (16, 16, 16), (3, 8, 8), seed=40)


def test_non_square_images_of_different_widths(lin_env):
    """The row step of a tap follows the segment: 2 x 12 x 20 (480 pixels, a shifted last panel) beside 5 x 6 x 10."""
    lin_env.linear_env(DS_LIN_GRID="8")
    _run_and_check(lin_env, (2, 12, 20), (5, 6, 10), seed=50)
