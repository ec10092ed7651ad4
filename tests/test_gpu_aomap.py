"""Ambient-occlusion maps (include/depthstereo.h: ds_aomap_u16; src/aomap_generation.py; ops={'aomap': ...}) against the NumPy model,
tests/aomap_cases.py.  Every comparison is torch.equal / np.array_equal: the definition fixes the ray table (made on the host), the
exact horizon compare and every rounding, so there is nothing to tolerate.  Shapes: smaller than a tile (5 x 7), ragged in both
directions (9 x 33), several 64 x 32 tiles at the largest radius (40 x 70), a map narrower than the halo (17 x 16, and 4 x 6 at
R = 32), a radius whose diagonal rays are empty.  tests/test_aomap_cpu.py shows that these cases contain ties, clamped values and
empty rays."""
import numpy as np
import pytest

import aomap_cases as ac

pytestmark = pytest.mark.gpu


def _run(torch, d, params, invert=False, wrap=False):
    from src import _native
    u8, f64 = _native.aomap_u16(torch.from_numpy(np.array(d, order='C')).cuda(), *params, invert=invert, wrap=wrap, want_f64=True)
    return u8, f64


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


@pytest.mark.parametrize("shape,params", ac.KERNEL_CASES, ids=ac.KERNEL_IDS)
def test_kernel_equals_the_model_bit_for_bit(gpu, shape, params):
    torch = gpu
    from src import _native
    for name, d in ac.inputs(shape).items():
        for wrap in (False, True):
            for invert in ((False, True) if name in ac.INVERTED else (False,)):
                before = _native.CALLS["ds_aomap_u16"]
                u8, f64 = _run(torch, d, params, invert, wrap)
                assert _native.CALLS["ds_aomap_u16"] == before + 1
                assert u8.dtype == torch.uint8 and f64.dtype == torch.float64 and tuple(u8.shape) == shape == tuple(f64.shape) and u8.is_cuda
                want_u8, want_f64 = ac.want(shape, params, name, invert, wrap)
                got_u8, got_f64 = u8.cpu().numpy(), f64.cpu().numpy()
                assert np.array_equal(got_f64, want_f64), (name, wrap, invert, _mismatch(got_f64, want_f64))
                assert np.array_equal(got_u8, want_u8), (name, wrap, invert, _mismatch(got_u8, want_u8))
                alone = _native.aomap_u16(torch.from_numpy(d.copy()).cuda(), *params, invert=invert, wrap=wrap)        # out_f64 == NULL
                assert torch.equal(alone, u8), (name, wrap, invert)


def test_radius_32_on_a_4_by_6_map(gpu):
    torch = gpu
    params = (32, 16, 64.0, 1.0)
    for name, d in ac.depth_cases(4, 6, seed=46, n=1):
        for wrap in (False, True):
            u8, f64 = _run(torch, d, params, wrap=wrap)
            want_u8, want_f64 = ac.model(d, *params, wrap=wrap)
            assert np.array_equal(f64.cpu().numpy(), want_f64) and np.array_equal(u8.cpu().numpy(), want_u8), (name, wrap)


def test_misaligned_buffers_give_the_same_bits(gpu):
    """Depth at ptr % 8 == 2 and the uint8 output at an odd address."""
    torch = gpu
    from src import _native
    for shape, params in ac.KERNEL_CASES[:4]:
        n, h, w = shape
        d = ac.inputs(shape)["random"]
        dbuf = torch.zeros(n * h * w + 4, dtype=torch.uint16, device="cuda")
        dview = dbuf.view(-1)[1:1 + n * h * w]
        dview.copy_(torch.from_numpy(d.copy()).cuda().view(-1))
        dview = dview.view(n, h, w)
        obuf = torch.full((n * h * w + 8,), 77, dtype=torch.uint8, device="cuda")
        oview = obuf[1:1 + n * h * w].view(n, h, w)
        assert dview.data_ptr() % 8 == 2 and dview.is_contiguous() and oview.data_ptr() % 2 == 1 and oview.is_contiguous()
        for wrap in (False, True):
            obuf.fill_(77)
            got = _native.aomap_u16(dview, *params, wrap=wrap, out=oview)
            assert got.data_ptr() == oview.data_ptr()
            assert np.array_equal(got.cpu().numpy(), ac.want(shape, params, "random", False, wrap)[0]), (shape, wrap)
            assert int(obuf[0]) == 77 and bool((obuf[1 + n * h * w:] == 77).all())                    # nothing beside the view is written


def test_batch_invariance_and_independence(gpu):
    """Image 2 of a batch of 3 equals that image run alone; changing image 0 changes only output 0."""
    torch = gpu
    for (h, w), params in (((9, 33), (8, 8, 64.0, 1.0)), ((40, 70), (32, 16, 2000.0, 1.5)), ((17, 16), (16, 16, 32.0, 1.0))):
        for wrap in (False, True):
            d = ac.ramp_noise(h, w, seed=h, n=3)
            d[1] = ac.random_depth(h, w, seed=w)
            y3 = _run(torch, d, params, wrap=wrap)
            y1 = _run(torch, d[2:3].copy(), params, wrap=wrap)
            assert torch.equal(y3[0][2:3], y1[0]) and torch.equal(y3[1][2:3], y1[1]), (h, w, wrap)
            d2 = d.copy()
            d2[0] = ac.random_depth(h, w, seed=h + w + 1)
            z3 = _run(torch, d2, params, wrap=wrap)
            assert torch.equal(z3[0][1:], y3[0][1:]) and torch.equal(z3[1][1:], y3[1][1:]) and not torch.equal(z3[1][0], y3[1][0]), (h, w, wrap)


def test_table_cache_is_bounded(gpu):
    torch = gpu
    from src import _native
    d = ac.ramp_noise(8, 8, seed=1, n=1)
    first = _run(torch, d, (3, 8, 64.0, 1.0))[0]
    for r in range(4, 10):
        _run(torch, d, (r, 8, 64.0, 1.0))
    assert _native.cached_tables("aomap") == 4
    _run(torch, d, (9, 8, 999.0, 2.0))                                                 # relief and intensity are no part of the key
    assert _native.cached_tables("aomap") == 4
    assert torch.equal(_run(torch, d, (3, 8, 64.0, 1.0))[0], first)                    # evicted and rebuilt: same bits
    assert _native.cached_tables("aomap") == 4
    assert np.array_equal(first.cpu().numpy(), ac.model(d, 3, 8, 64.0)[0])


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    dev = torch.cuda.current_device()
    ctx = _native.ctx_for(dev)
    EINVAL = -1
    n, h, w, r, k = 1, 8, 12, 2, 8
    SENT = 93
    tabs = {(R, K): tuple(torch.from_numpy(t).cuda() for t in _native.aomap_offsets(R, K)) for R, K in ((2, 8), (1, 4), (32, 16), (2, 4), (2, 16))}
    x = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
    out = torch.full((n, h, w), SENT, dtype=torch.uint8, device="cuda")
    f64 = torch.full((n * h * w + 1,), -7.0, dtype=torch.float64, device="cuda")
    big = torch.full((16 * n * h * w,), SENT, dtype=torch.uint8, device="cuda")        # one block to carve overlapping buffers from
    count = n * h * w
    B = big.data_ptr()
    assert B % 8 == 0
    inf, nan = float("inf"), float("nan")

    def call(c=ctx, xp=x.data_ptr(), n=n, h=h, w=w, r=r, k=k, tp=-1, sp=-1, z=1e-3, cc=0.125, invert=0, wrap=0, op=out.data_ptr(),
             fp=f64.data_ptr()):
        taps, start = tabs.get((r, k), tabs[(2, 8)])                                   # (an illegal (r, k) gets some real table)
        return L.ds_aomap_u16(c, xp, n, h, w, r, k, taps.data_ptr() if tp == -1 else tp, start.data_ptr() if sp == -1 else sp, z, cc,
                              invert, wrap, op, fp, None)
    _native.kernel_timer_enable(dev, True)
    try:
        assert call(c=None) == EINVAL and call(xp=None) == EINVAL and call(tp=None) == EINVAL and call(sp=None) == EINVAL
        assert call(op=None) == EINVAL
        assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-3) == EINVAL and call(n=-1) == EINVAL
        assert call(r=0) == EINVAL and call(r=33) == EINVAL and call(r=-1) == EINVAL
        for bad_k in (0, 1, 2, 3, 5, 12, 32, -8):
            assert call(k=bad_k) == EINVAL, bad_k
        for bad in (0.0, -1.0, inf, -inf, nan):
            assert call(z=bad) == EINVAL and call(cc=bad) == EINVAL, bad
        # alignment: taps, dir_start 4 bytes; out_f64 8 bytes; depth 2 bytes
        taps28, start28 = tabs[(2, 8)]
        assert call(tp=taps28.data_ptr() + 2) == EINVAL and call(sp=start28.data_ptr() + 1) == EINVAL
        assert call(fp=f64.data_ptr() + 4) == EINVAL and call(xp=x.data_ptr() + 1) == EINVAL
        # an output overlapping depth: equal pointers, beginning in the other's last byte
        assert count % 2 == 0
        assert call(xp=B, op=B) == EINVAL and call(xp=B, op=B + 2 * count - 1) == EINVAL and call(xp=B + count - 2, op=B) == EINVAL
        assert call(xp=B, fp=B) == EINVAL and call(xp=B, fp=B + 2 * count - 8) == EINVAL and call(xp=B + 8 * count - 2, fp=B) == EINVAL
        assert call(op=B, fp=B) == EINVAL and call(op=B + 8 * count - 1, fp=B) == EINVAL              # and the outputs each other
        # the grid limit: n = 65536 one-pixel images (every buffer really that large): DS_EUNSUPPORTED, one fewer runs (below)
        xn = torch.zeros((65536, 1, 1), dtype=torch.int16, device="cuda")
        on = torch.full((65536, 1, 1), SENT, dtype=torch.uint8, device="cuda")
        many = dict(xp=xn.data_ptr(), op=on.data_ptr(), fp=None, h=1, w=1, wrap=1)
        assert call(n=65536, **many) == -2 and bool((on == SENT).all())
        torch.cuda.synchronize()
        launches, _ = _native.kernel_timer_read(dev, "aomap")
        assert launches == 0                                                                          # every one returned before the launch
        assert bool((out == SENT).all()) and bool((big == SENT).all()) and bool((f64 == -7.0).all())
        assert b"ds_aomap_u16" in L.ds_last_error()
        # and the legal neighbours of those cases run: the ends of every range, out_f64 == NULL, out_u8 at an odd address, adjacent but
        # disjoint blocks
        assert call(r=1, k=4) == 0 and call(r=32, k=16) == 0 and call(k=4) == 0 and call(k=16) == 0
        assert call(z=5e-324, cc=1.7976931348623157e308) == 0 and call(wrap=1, invert=1) == 0
        assert call(fp=None) == 0 and call(op=B + 1, fp=None) == 0
        assert call(xp=B + count + count % 2, op=B, fp=None) == 0                                    # depth begins where out_u8 ends
        assert call(xp=B, op=B + 2 * count, fp=B + 8 * count) == 0                                   # outputs behind depth, apart
        assert call(n=65535, **many) == 0
        torch.cuda.synchronize()
        assert bool((on[:65535] == 255).all()) and int(on[65535]) == SENT
        launches, ms = _native.kernel_timer_read(dev, "aomap")
        assert launches == 11 and ms > 0.0, (launches, ms)                                          # the timer brackets each launch
        assert _native.kernel_timer_read(dev, "normalmap")[0] == 0                                    # and it is a kind of its own
        assert bool((out == 255).all()) and bool((f64[:count] == 1.0).all()) and float(f64[count]) == -7.0   # flat depth: open sky, written
    finally:
        _native.kernel_timer_enable(dev, False)


def test_public_interface(gpu):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.aomap_generation as ag
    h, w = 12, 20
    d = ac.ramp_noise(h, w, seed=3)
    x = torch.from_numpy(d).cuda()[None]
    for kwargs in ({}, {'radius': 5, 'directions': 16, 'relief': 500.0, 'intensity': 1.25, 'invert': True, 'wrap': True}):
        params = (kwargs.get('radius', 16), kwargs.get('directions', 8), kwargs.get('relief', 32.0), kwargs.get('intensity', 1.0))
        want = ac.model(d, *params, invert=kwargs.get('invert', False), wrap=kwargs.get('wrap', False))[0]
        batch = ag.create_aomap_batch(x, **kwargs)
        assert batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (1, h, w)
        assert np.array_equal(batch[0].cpu().numpy(), want)
        for depth in (d, Image.fromarray(d)):
            got = ag.create_aomap(depth, **kwargs)
            assert isinstance(got, Image.Image) and got.mode == 'L' and got.size == (w, h)
            assert np.array_equal(np.asarray(got), batch[0].cpu().numpy())
    before = dict(_native.CALLS)
    for bad_depth in (d.astype(np.float32), d.astype(np.int32), d.astype(np.uint8), d.astype(np.int16), d.astype(np.float64),
                      Image.fromarray(d.astype(np.uint8)), d[None], d[:0]):
        with pytest.raises(_native.DepthStereoError):
            ag.create_aomap(bad_depth)
    for bad in ({'radius': 0}, {'radius': 33}, {'radius': True}, {'radius': 2.5}, {'directions': 6}, {'directions': True}, {'relief': 0.0},
                {'relief': float('nan')}, {'intensity': -1.0}, {'intensity': float('inf')}, {'relief': "x"}):
        with pytest.raises(_native.DepthStereoError):
            ag.create_aomap(d, **bad)
        with pytest.raises(_native.DepthStereoError):
            ag.create_aomap_batch(x, **bad)
    for bad_x in (x.to(torch.int32), x.view(torch.int16), x.to(torch.float32), x[0], x.cpu(), d):
        with pytest.raises(_native.DepthStereoError):
            ag.create_aomap_batch(bad_x)
    assert dict(_native.CALLS) == before


def test_funnel_aomap_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'aomap': P}) with caller-supplied I;16 depth maps (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.aomap_generation as ag
    from src import _native
    h, w = 24, 40
    P = (6, 8, 300.0)
    rng = np.random.default_rng(5)
    imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(2)]
    d16 = [ac.staircase(h, w), ac.ramp_noise(h, w, seed=40)]
    base = {'gen_stereo': True, 'gen_normalmap': True, 'gen_heatmap': True, 'stereo_modes': ['left-right']}
    plain_kinds = ['depth', 'left-right', 'normalmap', 'heatmap']

    def run(ops, opts=base, kinds=plain_kinds):
        got = list(core.core_generation_funnel(None, list(imgs), [Image.fromarray(d) for d in d16], None, dict(opts), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(2) for k in kinds], [(i, k) for i, k, _ in got]
        return {k: [r if isinstance(r, str) else np.asarray(r) for _, kk, r in got if kk == k] for k in kinds}

    def same(a, b):
        return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)

    def delta(before):
        return {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}

    run(None)                                                                 # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(None)
    plain_delta = delta(before)
    assert "ds_aomap_u16" not in plain_delta
    own = plain['depth']                                                      # the funnel's own uint16 depth output
    with_ao = plain_kinds + ['aomap']

    def expect(params, wrap=False):
        return dict(plain, aomap=[np.asarray(ag.create_aomap(d, *params, wrap=wrap)) for d in own])

    want = expect(P)
    assert all(np.array_equal(a, ac.model(d, *P)[0]) for a, d in zip(want['aomap'], own)) and not (want['aomap'][0] == 255).all()
    before = dict(_native.CALLS)
    got = run({'aomap': P}, kinds=with_ao)                                    # after 'heatmap', every other output as it was
    assert same(got, want)
    assert delta(before) == dict(plain_delta, ds_aomap_u16=1)                 # one group: one launch, nothing else changes
    # gone on the next call; absent, None and {} make the launches and the bytes of a plain call
    for ops in (None, {}, {'aomap': None}, {'aomap': None, 'aomap_wrap': True}):
        before = dict(_native.CALLS)
        assert same(run(ops), plain), ops
        assert delta(before) == plain_delta, ops
    assert same(run({'aomap': list(P) + [1.5]}, kinds=with_ao), expect(P + (1.5,)))
    wrapped = expect(P, wrap=True)
    assert not np.array_equal(wrapped['aomap'][0], want['aomap'][0])
    assert same(run({'aomap': P, 'aomap_wrap': True}, kinds=with_ao), wrapped)
    assert same(run({'aomap': P, 'aomap_wrap': False}, kinds=with_ao), want)
    assert same(run({'aomap': P, 'aomap_wrap': 'tiling'}, kinds=with_ao), want)                       # TILING_MODE is off
    tiled = run({'aomap': P, 'aomap_wrap': 'tiling'}, dict(base, tiling_mode=True), with_ao)          # custom maps: no network to tile
    assert same({'aomap': tiled['aomap']}, {'aomap': wrapped['aomap']})
    # alone, and in front of the mesh
    only = run({'aomap': P}, {'do_output_depth': False}, ['aomap'])
    assert same(only, {'aomap': want['aomap']})
    for name in ('aomap', 'aomap_wrap'):
        assert not hasattr(core.model_holder, name)                           # the options do not become holder settings
    for bad in ({'aomap': (0, 8, 32.0)}, {'aomap': (8, 5, 32.0)}, {'aomap': (8, 8)}, {'aomap': "8"}, {'aomap': (8, 8, 0.0)},
                {'aomap': (True, 8, 32.0)}, {'aomap': (8, 8, 32.0, float('inf'))}, {'aomap': P, 'aomap_wrap': 'yes'}):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(bad)
        assert dict(_native.CALLS) == before, bad                             # before any device work
    assert same(run(None), plain)


def test_funnel_aomap_reads_the_refined_map_and_precedes_the_mesh(gpu, tmp_path):
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.aomap_generation as ag
    h, w = 24, 40
    P, REFINE = (6, 8, 300.0), (5, 60.0, 2.0)
    rng = np.random.default_rng(6)
    img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    d = ac.staircase(h, w)
    got = list(core.core_generation_funnel(str(tmp_path), [img], [Image.fromarray(d)], None,
                                           {'gen_heatmap': True, 'gen_simple_mesh': True}, {'aomap': P, 'depth_refine': REFINE}))
    assert [k for _, k, _ in got] == ['depth', 'heatmap', 'aomap', 'simple_mesh']
    refined = np.asarray(got[0][2])
    plain = np.asarray(next(r for _, k, r in core.core_generation_funnel(None, [img], [Image.fromarray(d)], None, {}, None) if k == 'depth'))
    assert not np.array_equal(refined, plain)
    assert np.array_equal(np.asarray(got[2][2]), np.asarray(ag.create_aomap(refined, *P)))
    assert not np.array_equal(np.asarray(got[2][2]), np.asarray(ag.create_aomap(plain, *P)))
