"""GPU tests of ds_linear_rows4 (csrc/ds_linear.hip: k_linear_rows4): the cls vectors of up to four read-outs, row 0 of every image of
a padded tap times that read-out's W_cls, in one launch that reads the rows where they lie.

Operands are exact integers: x, w in {-1, 0, 1}, K = 128, bias in [-8, 8], so |y| <= 136 and every product, every partial sum in
any order and the result are representable in float16 and bfloat16 (integers are exact to 256 in bfloat16).  The result must equal
the integer product computed in float64 on the CPU bit for bit, and it must be torch.equal to the route it replaces,
_native.linear(tap[:, 0].contiguous(), w, b) per tap.  Every row of a tap other than row 0 of an image is NaN: one element read from
anywhere else makes an output NaN.  The outputs are a slice of a larger buffer filled with a sentinel no result can take; the
sentinel must survive on both sides (rows of the last 32-row block beyond the batch are not stored).

Batches 3, 32 and 40: a partial 32-row block, a full one, a full one followed by a partial one."""
import pytest
import torch

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -1536.0          # exact in float16 and bfloat16, outside [-136, 136]
GUARD = 1024                # elements on either side of the outputs (a multiple of 8: the slice stays 16-byte aligned)
NP, K, N = 16, 128, 256


def _problems(dtype, batch, count, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    ri = lambda *s, a=-1, b=2: torch.randint(a, b, s, generator=g).double()  # noqa: E731
    rows = [ri(batch, K) for _ in range(count)]
    ws = [ri(N, K) for _ in range(count)]
    bs = [ri(N, a=-8, b=9) if bias else None for _ in range(count)]
    taps = []
    for r in rows:
        t = torch.full((batch, NP, K), float("nan"), dtype=dtype)
        t[:, 0] = r.to(dtype)
        taps.append(t.cuda())
    return rows, ws, bs, taps


def _run_and_check(nat, dtype, batch, count, seed, bias=True):
    rows, ws, bs, taps = _problems(dtype, batch, count, seed, bias)
    dev = lambda t: None if t is None else t.to(dtype).cuda()  # noqa: E731
    wd, bd = [dev(w) for w in ws], [dev(b) for b in bs]
    buf = torch.full((count * batch * N + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    out = buf[GUARD:GUARD + count * batch * N].view(count, batch, N)
    before = dict(nat.CALLS)
    got = nat.linear_rows4(taps, wd, bd, out=out)
    torch.cuda.synchronize()
    assert nat.CALLS["ds_linear_rows4"] == before.get("ds_linear_rows4", 0) + 1
    assert nat.CALLS["ds_linear"] == before.get("ds_linear", 0) + count
    assert len(got) == count
    worst = 0.0
    for p in range(count):
        want = rows[p] @ ws[p].T
        if bs[p] is not None:
            want = want + bs[p]
        g = got[p].cpu()
        worst = max(worst, (g.double() - want).abs().nan_to_num(nan=float("inf")).max().item())
        assert torch.equal(g, want.to(dtype)), f"problem {p} differs from the exact integer product (worst so far {worst})"
        ref = nat.linear(taps[p][:, 0].contiguous(), wd[p], bd[p])
        assert torch.equal(got[p], ref), f"problem {p} differs from _native.linear on the gathered rows"
    print(f"ds_linear_rows4 {dtype} batch {batch} x {count} problems: worst |got - exact| {worst}")
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "a store outside the outputs"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("batch", [3, 32, 40])
def test_four_cls_vectors_exact_and_equal_to_the_padded_panel(gpu, dtype, batch):
    from src import _native
    _run_and_check(_native, dtype, batch, 4, seed=100 + batch)


def test_three_problems_and_null_biases(gpu):
    """count < 4 (the unused pointer sets are never touched) and bias = NULL."""
    from src import _native
    _run_and_check(_native, torch.float16, 40, 3, seed=7)
    _run_and_check(_native, torch.float16, 3, 1, seed=8, bias=False)


def test_launch_is_capturable_into_a_graph(gpu):
    """No allocation, table or synchronisation behind the binding's own output buffer: the launch replays from a captured graph
    on new tap contents."""
    from src import _native
    rows, ws, bs, taps = _problems(torch.float16, 40, 4, seed=11)
    wd, bd = [w.half().cuda() for w in ws], [b.half().cuda() for b in bs]
    out = torch.empty((4, 40, N), dtype=torch.float16, device="cuda")
    _native.linear_rows4(taps, wd, bd, out=out)                 # eager first: function attributes are set outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _native.linear_rows4(taps, wd, bd, out=out)
    rows2 = _problems(torch.float16, 40, 4, seed=12)[0]
    for t, r in zip(taps, rows2):
        t[:, 0] = r.half().cuda()
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for p in range(4):
        assert torch.equal(out[p].cpu(), (rows2[p] @ ws[p].T + bs[p]).half()), p
