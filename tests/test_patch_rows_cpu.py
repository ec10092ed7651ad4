"""CPU check of the row layout of ds_preprocess_bicubic_rows (tools/patch_rows_model.py restates it in plain Python) against the torch
chain the kernel replaces: the patch gather of vm.patch_embed_tokens, the cls slot of torch.cat and the pad rows of vm.pad_tokens, on
random integers (every element distinct enough that a transposed or shifted index cannot pass)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import patch_rows_model as pm  # noqa: E402

from src import vit_mi355x as vm  # noqa: E402


def _torch_rows(x, p, n_pad, kpad):
    """x [B, H, W, 3] -> [B, n_pad, kpad] the way the tensor route builds the GEMM operand and the sequence around it."""
    b, h, w, c = x.shape
    gh, gw = h // p, w // p
    k = p * p * c
    xv = x[:, :gh * p, :gw * p].reshape(b, gh, p, gw, p, c).permute(0, 1, 3, 2, 4, 5)       # vm.patch_embed_tokens' gather
    rows = x.new_zeros((b * gh * gw, kpad))
    rows[:, :k] = xv.reshape(b * gh * gw, k)
    t = torch.cat((x.new_zeros((b, 1, kpad)), rows.view(b, gh * gw, kpad)), dim=1)          # the cls slot
    return vm.pad_tokens(t, n_pad)


# (patch, height, width, n_pad): p = 16 on a 2 x 3 grid (7 tokens) at every pad, p = 14 with kpad 640, an image with pixels beyond gh * p
CASES = [(16, 32, 48, 8), (16, 32, 48, 16), (16, 32, 48, 64), (14, 28, 42, 8), (14, 28, 42, 64), (16, 37, 53, 8), (14, 33, 44, 16)]


@pytest.mark.parametrize("p,h,w,n_pad", CASES)
def test_row_layout_equals_gather_cat_pad(p, h, w, n_pad):
    g = torch.Generator().manual_seed(p * 1000 + h + n_pad)
    x = torch.randint(1, 1 << 20, (2, h, w, 3), generator=g, dtype=torch.int64)
    gh, gw, n_valid, kpad = pm.geometry(h, w, p)
    assert n_valid <= n_pad and kpad % 128 == 0 and (kpad == 640 if p == 14 else kpad == 768)
    want = _torch_rows(x, p, n_pad, kpad)
    got = torch.tensor(pm.rows(x.tolist(), 2, h, w, p, n_pad, kpad), dtype=torch.int64)
    assert got.shape == want.shape == (2, n_pad, kpad)
    assert torch.equal(got, want)
    # the zero regions, stated directly
    assert not got[:, 0].any() and not got[:, n_valid:].any() and not got[:, :, 3 * p * p:].any()
    assert (got[:, 1:n_valid, :3 * p * p] > 0).all()


def test_geometry_matches_the_route():
    """The (grid, n_valid, n_pad, kpad) the route computes is the model's, and n_pad is what pad_len gives the batch."""
    import torch.nn as nn
    for p, h, w, batch in ((16, 512, 512, 32), (16, 32, 48, 2), (14, 28, 42, 4), (16, 192, 192, 2)):
        conv = nn.Conv2d(3, 256, p, p)
        grid, n_valid, n_pad, kpad = vm.patch_rows_geometry(conv, (h, w), batch)
        gh, gw, nv, kp = pm.geometry(h, w, p)
        assert (grid, n_valid, kpad) == ((gh, gw), nv, kp) and n_pad == vm.pad_len(n_valid, batch)
    assert vm.patch_rows_geometry(nn.Conv2d(3, 256, 16, 16), (512, 512), 32)[1:3] == (1025, 1032)
    assert vm.patch_rows_geometry(nn.Conv2d(3, 256, 16, 16), (192, 192), 2)[1:3] == (145, 192)
