"""GPU tests of ds_linear_qkv (csrc/ds_linear.hip: k_linear256<.., VT 4> and ln_launch_qkv): the Q/K projection and V^T of an
encoder block in one persistent launch over both tile lists.

Operands are exact integers in ranges where every product, every partial sum in any order and the result are representable:
    float16:   x, w in [-2, 2], K = 256, bias in [-8, 8]:  |y| <= 4 * 256 + 8 = 1032  (integers are exact to 2048)
    bfloat16:  x, w in {-1, 0, 1}, K = 128, bias in [-8, 8]:  |y| <= 128 + 8 = 136    (integers are exact to 256)
so the result must equal the integer product computed in float64 on the CPU bit for bit -- a dropped, duplicated or misplaced
tile is a whole-number difference -- and it must be torch.equal to _native.linear + _native.linear_vt.  qk and vt are slices of
larger buffers filled with a sentinel no result can take, and the sentinel must survive on both sides of both slices.

Which launches a shape takes (T0 = Q/K tiles, T1 = V^T tiles, G workgroups; tests/test_linear_qkv_model.py):
    R = (T0 + T1) % G is handed to the V^T ragged kernel when T0 + T1 > G, 4 R <= G and R <= T1; else the main kernel walks all."""
import os

import pytest
import torch

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu
ENV = ("DS_LIN_GRID", "DS_LIN_EARLY", "DS_LIN_RAGGED", "DS_LIN_RAGGED_THIN", "DS_LIN_RAGGED_RING", "DS_LIN_RAGGED_PIPE")
SENTINEL = -1536.0          # exact in float16 and bfloat16, outside [-1032, 1032]
GUARD = 1024                # elements on either side of a slice (a multiple of 8: the slices stay 16-byte aligned)


@pytest.fixture
def lin_env(gpu):
    from src import _native
    old = {k: os.environ.get(k) for k in ENV}
    try:
        yield _native
    finally:
        _native.linear_env(**old)
        _native.kernel_timer_enable(torch.cuda.current_device(), False)


def _operands(dtype, batch, tokens, k, nqk, c, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-2, 3) if dtype == torch.float16 else (-1, 2)
    assert k * max(abs(lo), hi - 1) ** 2 + 8 <= (2048 if dtype == torch.float16 else 256)
    ri = lambda *s, a=lo, b=hi: torch.randint(a, b, s, generator=g).double()  # noqa: E731
    return ri(batch, tokens, k), ri(nqk, k), (ri(nqk, a=-8, b=9) if bias else None), ri(c, k)


def _reference(h, w_qk, b_qk, w_v):
    """float64 on the CPU: qk [B, Np, N], vt [B, C, Np]."""
    qk = h @ w_qk.T
    if b_qk is not None:
        qk = qk + b_qk
    return qk, torch.matmul(w_v, h.transpose(1, 2))


def _guarded(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _run_and_check(nat, dtype, batch, tokens, k, nqk, c, seed, bias=True, launches=None):
    h, w_qk, b_qk, w_v = _operands(dtype, batch, tokens, k, nqk, c, seed, bias)
    want_qk, want_vt = _reference(h, w_qk, b_qk, w_v)
    dev = lambda t: None if t is None else t.to(dtype).cuda()  # noqa: E731
    hd, wqd, bqd, wvd = dev(h), dev(w_qk), dev(b_qk), dev(w_v)
    buf_qk, qk = _guarded((batch, tokens, nqk), dtype)
    buf_vt, vt = _guarded((batch, c, tokens), dtype)
    device = torch.cuda.current_device()
    nat.kernel_timer_enable(device, True)
    before = dict(nat.CALLS)
    out = nat.linear_qkv(hd, wqd, bqd, wvd, out=(qk, vt))
    assert out[0] is qk and out[1] is vt and nat.CALLS["ds_linear_qkv"] == before.get("ds_linear_qkv", 0) + 1
    timed = {kind: nat.kernel_timer_read(device, kind)[0] for kind in ("linear", "linear+ragged", "linear_vt", "linear_vt+ragged")}
    nat.kernel_timer_enable(device, False)
    worst = max((qk.double().cpu() - want_qk).abs().max().item(), (vt.double().cpu() - want_vt).abs().max().item())
    print(f"ds_linear_qkv {dtype} B={batch} Np={tokens} K={k} N={nqk} C={c}: launches {timed}, worst |got - exact| {worst}")
    assert torch.equal(qk.cpu(), want_qk.to(dtype)), "qk differs from the exact integer product"
    assert torch.equal(vt.cpu(), want_vt.to(dtype)), "vt differs from the exact integer product"
    for name, buf in (("qk", buf_qk), ("vt", buf_vt)):
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f"{name}: a store outside the slice"
    assert torch.equal(nat.linear(hd, wqd, bqd), qk) and torch.equal(nat.linear_vt(wvd, hd), vt), "differs from the two-launch route"
    if launches is not None:
        assert (timed["linear"], timed["linear+ragged"]) == launches and timed["linear_vt"] == timed["linear_vt+ragged"] == 0, timed


@pytest.mark.parametrize("early", ["1", "0"])
def test_two_rounds_across_the_segment_boundary_plus_ragged_vt_tiles(lin_env, early):
    """(a) 12 + 6 tiles on 8 workgroups: two whole rounds that span the segment boundary (workgroups 0-5 render Q/K tiles, 6-7 V^T
    tiles) and 2 ragged V^T tiles; with the next tile's prologue issued before the epilogue and after it."""
    lin_env.linear_env(DS_LIN_GRID="8", DS_LIN_EARLY=early)
    _run_and_check(lin_env, torch.float16, 2, 768, 256, 512, 256, seed=1, launches=(1, 1))


@pytest.mark.parametrize("early", ["1", "0"])
def test_workgroup_that_walks_from_a_qk_tile_into_a_vt_tile(lin_env, early):
    """(a2) 9 + 9 tiles on 8 workgroups: an XCD takes a contiguous range of the list (2 tiles per workgroup), so in shape (a) the
    boundary at 12 falls between two workgroups; here workgroup 4 renders tile 8 (Q/K) and then tile 9 (V^T) -- in early mode
    set_tile(next) switches the segment while the Q/K tile's epilogue is still to run.  Plus 2 ragged V^T tiles."""
    lin_env.linear_env(DS_LIN_GRID="8", DS_LIN_EARLY=early)
    _run_and_check(lin_env, torch.float16, 1, 768, 256, 768, 768, seed=9, launches=(1, 1))


def test_partial_last_round_that_ends_inside_vt(lin_env):
    """(b) 10 + 5 = 15 tiles on 8 workgroups: 7 left over is more than a quarter of the grid -- no ragged round, the last round is
    partial and ends inside V^T."""
    lin_env.linear_env(DS_LIN_GRID="8")
    _run_and_check(lin_env, torch.float16, 2, 640, 256, 512, 256, seed=2, launches=(1, 0))


def test_more_leftover_tiles_than_vt_tiles_walks_everything(lin_env):
    """(c) 9 + 1 tiles on 8 workgroups at K = 128 (one K iteration): R = 2 > T1 = 1, so the persistent kernel walks the whole list."""
    lin_env.linear_env(DS_LIN_GRID="8")
    _run_and_check(lin_env, torch.float16, 1, 256, 128, 2304, 256, seed=3, launches=(1, 0))


def test_benchmark_tile_arithmetic_with_a_short_k(lin_env):
    """(d) the metric's 1032 + 516 tiles on the default grid (one workgroup per CU), K = 256: values and guards."""
    lin_env.linear_env(DS_LIN_GRID=None)
    _run_and_check(lin_env, torch.float16, 32, 1032, 256, 2048, 1024, seed=4)


def test_null_qk_bias(lin_env):
    """(e) b_qk = NULL: the null-bias decision is per tile (Q/K tiles now take it too)."""
    lin_env.linear_env(DS_LIN_GRID="8")
    _run_and_check(lin_env, torch.float16, 2, 768, 256, 512, 256, seed=5, bias=False, launches=(1, 1))


def test_bfloat16_instantiation(lin_env):
    """(f) shape (a) in bfloat16 (K = 128 keeps the integers exact)."""
    lin_env.linear_env(DS_LIN_GRID="8")
    _run_and_check(lin_env, torch.bfloat16, 2, 768, 128, 512, 256, seed=6, launches=(1, 1))


def test_beit_block_attend_o_takes_the_route_and_keeps_its_bits(lin_env, monkeypatch):
    """(g) EncoderBlock.attend_o of a BEiT-L block (dim 1024, batch 8, 1025 tokens at stride 1056): DS_LINEAR_QKV on against off is
    bit-equal, and the counters of the binding show which entry points ran."""
    from dmidas.backbones.beit import Block
    from src import vit_mi355x as vm
    nat = lin_env
    nat.linear_env(DS_LIN_GRID=None)
    torch.manual_seed(7)
    blk = Block(1024, 16, (32, 32)).eval()
    with torch.no_grad():
        blk.attn.q_bias.normal_(0, 0.5)
        blk.attn.v_bias.normal_(0, 0.5)
        blk.attn.relative_position_bias_table.normal_(0, 0.2)
    blk = blk.half().cuda()
    npad = vm.pad_len(1025, 8)
    assert npad == 1056
    h = torch.randn((8, npad, 1024), generator=torch.Generator().manual_seed(8)).half().cuda()
    names = ("ds_linear_qkv", "ds_linear", "ds_linear_vt", "ds_attention_fwd")

    def run(on):
        monkeypatch.setattr(vm, "LINEAR_QKV", on)
        before = dict(nat.CALLS)
        with torch.no_grad():
            o, b_v = blk.attend_o(h, 1025, (32, 32))
        torch.cuda.synchronize()
        return o, {n: nat.CALLS[n] - before.get(n, 0) for n in names}
    o1, calls1 = run(True)
    o0, calls0 = run(False)
    assert calls1 == {"ds_linear_qkv": 1, "ds_linear": 1, "ds_linear_vt": 1, "ds_attention_fwd": 1}, calls1
    assert calls0 == {"ds_linear_qkv": 0, "ds_linear": 1, "ds_linear_vt": 1, "ds_attention_fwd": 1}, calls0
    assert torch.equal(o1, o0), "the one-launch route changed the attention output"
    assert bool(torch.isfinite(o1[:, :1025].float()).all())
