"""GPU tests of the 16x16x32 accumulation chain of csrc/ds_linear.hip: the dense token GEMMs (k_linear256 and its ragged / thin
rounds) at the shapes of dpt_beit_large_512 at batch 32 against float32, bit-identity of the main rounds with both ragged kernels for
every dense epilogue, and the implicit-GEMM convolutions next to them."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu
ENV = ("DS_LIN_GRID", "DS_LIN_RAGGED", "DS_LIN_RAGGED_THIN", "DS_LIN_RAGGED_RING", "DS_LIN_RAGGED_PIPE")


@pytest.fixture
def lin_env():
    from src import _native
    old = {k: os.environ.get(k) for k in ENV}
    yield _native
    for k, v in old.items():
        _native.linear_env(**{k: v})


def _rand(g, *s, scale=1.0):
    return (torch.randn(s, generator=g) * scale).half().cuda()


@pytest.mark.parametrize("name,n,k", [("fc1", 4096, 1024), ("qk", 2048, 1024), ("proj", 1024, 1024), ("fc2", 1024, 4096)])
def test_token_gemms_at_benchmark_shapes_against_float32(gpu, lin_env, name, n, k):
    """M = 32 images x 1032 token rows: 129 row panels, the last one rendered by k_linear_thin.  Rows of every kind of tile (first,
    middle, the shifted last panel) against float32 on the same fp16 operands."""
    nat = lin_env
    m = 32 * 1032
    g = torch.Generator().manual_seed(n + k)
    x, w, b = _rand(g, m, k), _rand(g, n, k, scale=k ** -0.5), _rand(g, n)
    rows = torch.cat([torch.arange(0, 40), torch.randint(0, m, (200,), generator=g), torch.arange(m - 300, m)]).cuda()
    if name in ("proj", "fc2"):
        gam, res = _rand(g, n, scale=0.1), _rand(g, m, n)
        got = nat.linear_residual(x, w, b, gam, res)
        want = res[rows].float() + gam.float() * (x[rows].float() @ w.float().T + b.float())
    else:
        gelu = name == "fc1"
        got = nat.linear(x, w, b, gelu)
        want = x[rows].float() @ w.float().T + b.float()
        if gelu:
            want = F.gelu(want)
    err = (got[rows].float() - want).abs().max().item()
    assert err < 2e-2 * (1 + want.abs().max().item()) and err < 3e-2, (name, err)
    again = nat.linear_residual(x, w, b, gam, res) if name in ("proj", "fc2") else nat.linear(x, w, b, name == "fc1")
    assert torch.equal(again, got), "run-to-run difference"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_main_ragged_and_thin_rounds_are_one_chain_for_every_epilogue(gpu, lin_env, dtype):
    """The same output tile through the persistent kernel, the ragged kernel (3- and 6-slot ring, plain and pipelined loop) and the
    thin kernel: bit-identical for the plain, GELU, ReLU-free bias-less, LayerScale + residual and V^T epilogues."""
    nat = lin_env
    g = torch.Generator().manual_seed(16)
    mk = lambda *s: torch.randn(s, generator=g).to(dtype).cuda()  # noqa: E731
    m, n, k = 2100, 512, 384                      # grid 8: 9 x 2 tiles, the last row panel is the ragged round (thin-eligible)
    x, w, b = mk(m, k), mk(n, k) * k ** -0.5, mk(n)
    gam, res = mk(n), mk(m, n)
    hv, wv = mk(4, 320, 256), mk(512, 256) * 256 ** -0.5

    def run():
        return (nat.linear(x, w, b, False), nat.linear(x, w, b, True), nat.linear(x, w, None, False),
                nat.linear_residual(x, w, b, gam, res), nat.linear_residual(x, w, b, None, res), nat.linear_vt(wv, hv))
    nat.linear_env(DS_LIN_GRID="8", DS_LIN_RAGGED="0")
    walk = run()
    for ragged, thin, ring, pipe in (("1", "1", None, None), ("1", "0", "6", "1"), ("1", "0", "6", "0"), ("1", "0", "3", None)):
        nat.linear_env(DS_LIN_RAGGED=ragged, DS_LIN_RAGGED_THIN=thin, DS_LIN_RAGGED_RING=ring, DS_LIN_RAGGED_PIPE=pipe)
        for i, (a, c) in enumerate(zip(run(), walk)):
            assert torch.equal(a, c), ("ragged / thin round differs from the main rounds", i, thin, ring, pipe)
    want = x.double() @ w.double().T + b.double()
    assert (walk[0].double() - want).abs().max().item() < (1.5e-3 if dtype == torch.float16 else 1.2e-2) * (1 + want.abs().max().item())


@pytest.mark.parametrize("relu,nres,relu_in,cout", [(True, 0, False, 256), (False, 2, False, 256), (True, 1, False, 256),
                                                    (True, 0, True, 256), (False, 0, False, 128)])
def test_conv3x3_variants_against_float32(gpu, lin_env, relu, nres, relu_in, cout):
    """The convolution front end (CONV 1 / 2, NH = 1 for 128 output channels) beside the dense chain: against float32 and
    run-to-run identical."""
    nat = lin_env
    g = torch.Generator().manual_seed(cout + nres)
    conv = nn.Conv2d(256, cout, 3, padding=1).half().cuda()
    x = (torch.randn((2, 256, 45, 38), generator=g)).half().cuda().contiguous(memory_format=torch.channels_last)
    rs = [torch.randn((2, cout, 45, 38), generator=g).half().cuda().contiguous(memory_format=torch.channels_last) for _ in range(nres)]
    kw = dict(relu=relu, relu_in=relu_in)
    if nres >= 1:
        kw["res1"] = rs[0]
    if nres >= 2:
        kw["res2"] = rs[1]
    got = nat.conv3x3(conv, x, **kw)
    xi = F.relu(x.float()) if relu_in else x.float()
    want = F.conv2d(xi, conv.weight.float(), conv.bias.float(), padding=1)
    for r in rs:
        want = want + r.float()
    if relu:
        want = F.relu(want)
    err = (got.float() - want).abs().max().item()
    assert err < 2e-2 * (1 + want.abs().max().item()), err
    assert torch.equal(nat.conv3x3(conv, x, **kw), got)
