"""Autostereograms from depth (include/depthstereo.h: ds_autostereogram_u8; src/autostereogram_generation.py;
ops={'autostereogram': ...}) against the NumPy model, tests/autostereogram_cases.py.  Every comparison is byte for byte: the
definition is all-integer and a component's representative is a maximum, so there is nothing to tolerate and nothing that depends on
the order of the LDS atomics.  Shapes: one column; width 20, which links nothing from period 32 on; widths below, across and above a
256-thread workgroup (67, 130, 257) at heights 1 and 5 in a batch of 3; one 96 x 300; 2 x 700, where period 512 links; 2 x 2100,
above the width at which the entry point launches 1024-thread workgroups; 1 x 16384, the widest row; and the 1 x 1500 chain whose
components have 137 members.
tests/test_autostereogram_cpu.py shows from the model that the cases contain hidden columns and components of several members."""
import numpy as np
import pytest

import autostereogram_cases as ac

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


def _variants():
    """(mode, seed, tile index) of one sweep: both seeds on the coloured dots, the black / white dots, every tile."""
    return [(0, ac.SEEDS[0], None), (0, ac.SEEDS[1], None), (1, ac.SEEDS[1], None)] + [(2, 0, k) for k in range(len(ac.TILES))]


def _sweep(torch, shape, names, params):
    from src import _native
    tiles = [_dev(torch, ac.tile_input(k)) for k in range(len(ac.TILES))]
    for name in names:
        depth = ac.depth_input(name, shape)
        depth_t = _dev(torch, depth)
        for P, m in params:
            for invert in (False, True):
                for mode, seed, k in _variants():
                    before = _native.CALLS["ds_autostereogram_u8"]
                    out = _native.autostereogram_u8(depth_t, P, m, mode, seed, tile=None if k is None else tiles[k], invert=invert)
                    assert _native.CALLS["ds_autostereogram_u8"] == before + 1
                    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == shape + (3,)
                    want = ac.want(name, shape, P, m, invert, mode, seed, None if k is None else ac.tile_input(k))
                    got = out.cpu().numpy()
                    assert np.array_equal(got, want), (name, P, m, invert, mode, seed, k, _mismatch(got, want))


@pytest.mark.parametrize("shape", ac.SMALL_SHAPES, ids=["%dx%dx%d" % s for s in ac.SMALL_SHAPES])
def test_kernel_equals_the_model_byte_for_byte(gpu, shape):
    _sweep(gpu, shape, tuple(ac.DEPTHS), ac.SMALL_PARAMS)


@pytest.mark.parametrize("case", range(len(ac.LARGE_CASES)), ids=["%dx%dx%d" % c[0] for c in ac.LARGE_CASES])
def test_kernel_equals_the_model_on_the_larger_shapes(gpu, case):
    shape, params, names = ac.LARGE_CASES[case]
    if case == 0:
        # so that the comparison cannot pass vacuously: hidden columns, components of several members, links at all
        P, m = params[0]
        rect, noise = (ac.census(ac.depth_input(name, shape)[0], P, m) for name in ("rect", "noise"))
        assert rect['hidden'] >= 1 and rect['largest'] >= 3 and noise['hidden'] >= 1 and noise['links'] >= 1, (rect, noise)
    _sweep(gpu, shape, names, params)


def test_the_long_chain_converges_to_the_model(gpu):
    """1 x 1500 flat near at P = 16, m = 128: separation 11, components of 137 members -- the convergence loop runs its longest here."""
    shape, P, m = ac.CHAIN
    rep = ac.want_rep("full", shape, P, m, False)
    assert int(np.bincount(rep[0, 0]).max()) == 137
    _sweep(gpu, shape, ("full",), [(P, m)])
    # the same chain as the inverted far plane, and a chain that a near block cuts in two
    _sweep(gpu, shape, ("zeros", "rect"), [(P, m)])


def _raw(torch, depth_t, P, m, mode, seed, tile_t, invert, out_ptr):
    from src import _native
    n, h, w = depth_t.shape
    return _native.lib().ds_autostereogram_u8(_native.ctx_for(torch.cuda.current_device()), depth_t.data_ptr(), n, h, w, P, m, mode, seed,
                                              None if tile_t is None else tile_t.data_ptr(), 0 if tile_t is None else tile_t.shape[0],
                                              0 if tile_t is None else tile_t.shape[1], invert, out_ptr, None)


def test_out_at_an_odd_byte_address(gpu):
    """out at ptr % 2 == 1, depth at ptr % 8 == 2, the tile at an odd address; nothing beside the output view is written."""
    torch = gpu
    for shape, P, m in (((3, 5, 67), 16, 128), ((3, 1, 257), 96, 85)):
        n, h, w = shape
        count = n * h * w
        depth = ac.depth_input("noise", shape)
        dbuf = torch.zeros(count + 4, dtype=torch.uint16, device="cuda")
        dview = dbuf[1:1 + count]
        dview.copy_(_dev(torch, depth).view(-1))
        dview = dview.view(n, h, w)
        tile = ac.tile_input(1)
        tbuf = torch.zeros(tile.size + 8, dtype=torch.uint8, device="cuda")
        tview = tbuf[3:3 + tile.size]
        tview.copy_(_dev(torch, tile).view(-1))
        tview = tview.view(tile.shape)
        for mode, tile_t in ((0, None), (2, tview)):
            obuf = torch.full((3 * count + 16,), 77, dtype=torch.uint8, device="cuda")
            oview = obuf[5:5 + 3 * count]
            assert oview.data_ptr() % 2 == 1 and dview.data_ptr() % 8 == 2 and tview.data_ptr() % 2 == 1
            assert _raw(torch, dview, P, m, mode, 3, tile_t, 0, oview.data_ptr()) == 0
            want = ac.want("noise", shape, P, m, False, mode, 3, tile if mode == 2 else None)
            assert np.array_equal(oview.view(n, h, w, 3).cpu().numpy(), want), (shape, mode)
            assert bool((obuf[:5] == 77).all()) and bool((obuf[5 + 3 * count:] == 77).all())


def test_batch_independence_and_repeatability(gpu):
    """Image 2 of a batch of 3 equals that image alone; changing image 0 changes output 0 only; two runs are equal."""
    torch = gpu
    from src import _native
    for shape, P, m in (((3, 5, 130), 16, 128), ((3, 5, 257), 96, 85)):
        depth = np.array(ac.depth_input("noise", shape))
        depth[1] = ac.depth_input("rect", shape)[1]
        tile = ac.tile_input(2)
        for mode in ac.MODES:
            y3 = _native.autostereogram_u8(_dev(torch, depth), P, m, mode, 11, tile=tile)
            y1 = _native.autostereogram_u8(_dev(torch, depth[2:3]), P, m, mode, 11, tile=tile)
            assert torch.equal(y3[2:3], y1), (shape, mode)
            assert torch.equal(_native.autostereogram_u8(_dev(torch, depth), P, m, mode, 11, tile=tile), y3), (shape, mode)
            depth2 = depth.copy()
            depth2[0] = ac.depth_input("ramp", shape)[0]
            z3 = _native.autostereogram_u8(_dev(torch, depth2), P, m, mode, 11, tile=tile)
            assert torch.equal(z3[1:], y3[1:]) and not torch.equal(z3[0], y3[0]), (shape, mode)
            into = torch.full(shape + (3,), 9, dtype=torch.uint8, device="cuda")
            assert _native.autostereogram_u8(_dev(torch, depth), P, m, mode, 11, tile=tile, out=into) is into and torch.equal(into, y3)
        # another seed gives other dots; the seed does not enter a pattern
        a, b = (_native.autostereogram_u8(_dev(torch, depth), P, m, 0, s) for s in (11, 12))
        assert not torch.equal(a, b)
        a, b = (_native.autostereogram_u8(_dev(torch, depth), P, m, 2, s, tile=tile) for s in (11, 12))
        assert torch.equal(a, b)


def test_rounds_entry_point_gives_the_same_bytes_and_counts_rounds(gpu):
    torch = gpu
    from src import _native
    L, ctx = _native.lib(), _native.ctx_for(torch.cuda.current_device())
    shape, P, m = ac.CHAIN
    for name, shp in (("full", shape), ("noise", (3, 5, 257)), ("zeros", (3, 1, 1))):
        n, h, w = shp
        depth_t = _dev(torch, ac.depth_input(name, shp))
        out = torch.empty(shp + (3,), dtype=torch.uint8, device="cuda")
        rounds = torch.full((n * h + 1,), 777, dtype=torch.int16, device="cuda")
        assert L.ds_autostereogram_rounds_u8(ctx, depth_t.data_ptr(), n, h, w, P, m, 0, 5, None, 0, 0, 0, out.data_ptr(), rounds.data_ptr(), None) == 0
        assert np.array_equal(out.cpu().numpy(), ac.want(name, shp, P, m, False, 0, 5))
        r = rounds.cpu().numpy()
        assert r[-1] == 777 and (r[:-1] >= 1).all() and (r[:-1] <= 64).all(), r
        links = ac.census(ac.depth_input(name, shp)[0], P, m)['links']
        assert (r[:-1] >= 2).all() if name == "full" else links > 0 or (r[:-1] == 1).all()     # no link: one idle round
    assert L.ds_autostereogram_rounds_u8(ctx, depth_t.data_ptr(), n, h, w, P, m, 0, 5, None, 0, 0, 0, out.data_ptr(), None, None) == EINVAL
    assert b"ds_autostereogram_rounds_u8" in L.ds_last_error()


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    ctx = _native.ctx_for(torch.cuda.current_device())
    SENT = 93
    n, h, w = 2, 4, 24
    count = n * h * w
    dep = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
    til = torch.full((2, 5, 3), 50, dtype=torch.uint8, device="cuda")
    out = torch.full((n, h, w, 3), SENT, dtype=torch.uint8, device="cuda")
    big = torch.full((16 * count,), SENT, dtype=torch.uint8, device="cuda")   # one block to carve overlapping buffers from
    B = big.data_ptr()
    assert B % 2 == 0

    def call(c=ctx, dp=dep.data_ptr(), n=n, h=h, w=w, P=16, m=85, mode=2, seed=1, tp=til.data_ptr(), ph=2, pw=5, invert=0, op=out.data_ptr()):
        return L.ds_autostereogram_u8(c, dp, n, h, w, P, m, mode, seed, tp, ph, pw, invert, op, None)
    assert call(c=None) == EINVAL and call(dp=None) == EINVAL and call(op=None) == EINVAL and call(tp=None) == EINVAL
    assert b"ds_autostereogram_u8" in L.ds_last_error()
    assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-3) == EINVAL and call(n=-1) == EINVAL
    assert call(P=15) == EINVAL and call(P=513) == EINVAL and call(P=0) == EINVAL and call(P=-96) == EINVAL
    assert call(m=0) == EINVAL and call(m=129) == EINVAL and call(m=-1) == EINVAL
    assert call(mode=-1) == EINVAL and call(mode=3) == EINVAL
    assert call(ph=0) == EINVAL and call(pw=0) == EINVAL and call(ph=4097) == EINVAL and call(pw=4097) == EINVAL and call(pw=-5) == EINVAL
    assert call(dp=dep.data_ptr() + 1) == EINVAL
    # the order of the checks: a bad parameter beside a size above the limit is EINVAL, the size alone EUNSUPPORTED
    assert call(w=16385, P=15) == EINVAL and call(w=16385) == EUNSUPPORTED and call(h=16385) == EUNSUPPORTED and call(n=65536, h=1, w=1) == EUNSUPPORTED
    assert b"ds_autostereogram_u8" in L.ds_last_error()
    # a size above the limit beside an overlap is EUNSUPPORTED: the overlap test comes last
    assert call(w=16385, dp=B, op=B) == EUNSUPPORTED
    # out (3 count bytes) against depth (2 count bytes) and the tile (30 bytes): equal pointers, and beginning in the other's last byte
    assert call(dp=B, op=B) == EINVAL and call(dp=B, op=B + 2 * count - 1) == EINVAL
    assert call(dp=B + 3 * count - 2, op=B) == EINVAL
    assert call(tp=B, op=B) == EINVAL and call(tp=B, op=B + 29) == EINVAL and call(tp=B + 3 * count - 1, op=B) == EINVAL
    torch.cuda.synchronize()
    big.fill_(SENT)
    out.fill_(SENT)
    torch.cuda.synchronize()
    for bad in (dict(c=None), dict(n=0), dict(P=15), dict(m=129), dict(mode=3), dict(ph=0), dict(dp=dep.data_ptr() + 1), dict(w=16385),
                dict(dp=B, op=B), dict(tp=B, op=B + 29)):
        assert call(**bad) in (EINVAL, EUNSUPPORTED)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((big == SENT).all())            # no refusal launched anything
    # and the legal neighbours run: the ends of every range, a tile that is not looked at, adjacent but disjoint blocks
    assert call(P=16) == 0 and call(P=512) == 0 and call(m=1) == 0 and call(m=128) == 0 and call(invert=1) == 0
    assert call(mode=0, tp=None, ph=0, pw=0) == 0 and call(mode=1, tp=None, ph=-7, pw=99999) == 0 and call(mode=0, tp=out.data_ptr()) == 0
    o_at = B + 1
    d_at = o_at + 3 * count + 1
    t_at = d_at + 2 * count
    assert d_at % 2 == 0 and t_at + 30 <= B + big.numel()
    big[t_at - B:t_at - B + 30] = 50                                          # a tile of one colour: every pixel becomes 50
    assert call(op=o_at, dp=d_at, tp=t_at) == 0
    torch.cuda.synchronize()
    assert int(big[0]) == SENT and bool((big[1:1 + 3 * count] == 50).all()) and bool((big[1 + 3 * count:t_at - B] == SENT).all())
    assert bool((big[t_at - B:t_at - B + 30] == 50).all()) and bool((big[t_at - B + 30:] == SENT).all())
    assert not bool((out == SENT).any())                                      # the calls above wrote all of it


def test_public_interface(gpu):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.autostereogram_generation as ag
    h, w = 12, 150
    d = ac.depth_input("rect", (1, h, w))[0]
    x = _dev(torch, d)[None]
    tile = ac.tile_input(1)
    for kwargs in ({}, {'period': 40, 'depth_factor': 0.5, 'pattern': 'mono', 'seed': 77, 'invert': True},
                   {'period': 33, 'depth_factor': 0.1, 'pattern': tile}, {'period': 64, 'pattern': Image.fromarray(tile), 'seed': 5}):
        P, mu = kwargs.get('period', 96), kwargs.get('depth_factor', 1 / 3)
        pattern = kwargs.get('pattern', 'dots')
        mode = {'dots': 0, 'mono': 1}[pattern] if isinstance(pattern, str) else 2
        want = ac.model(d, P, int(np.rint(256 * mu)), mode, kwargs.get('seed', 0), tile if mode == 2 else None, kwargs.get('invert', False))
        batch = ag.create_autostereogram_batch(x, **kwargs)
        assert batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (1, h, w, 3)
        assert np.array_equal(batch[0].cpu().numpy(), want)
        for depth in (d, Image.fromarray(d)):
            got = ag.create_autostereogram(depth, **kwargs)
            assert isinstance(got, Image.Image) and got.mode == 'RGB' and got.size == (w, h)
            assert np.array_equal(np.asarray(got), want)
    assert len({np.asarray(ag.create_autostereogram(d, seed=s)).tobytes() for s in range(4)}) == 4
    before = dict(_native.CALLS)
    for bad_depth in (d.astype(np.float32), d.astype(np.int32), d.astype(np.uint8), Image.fromarray(d.astype(np.uint8)), d[None], d[:0]):
        with pytest.raises(_native.DepthStereoError):
            ag.create_autostereogram(bad_depth)
    for bad in ({'period': 15}, {'period': 513}, {'period': True}, {'period': 96.5}, {'depth_factor': 0.0}, {'depth_factor': 0.51},
                {'depth_factor': float('nan')}, {'depth_factor': '0.3'}, {'pattern': 'stripes'}, {'pattern': None},
                {'pattern': np.zeros((2, 2, 3), np.float32)}, {'pattern': np.zeros((0, 2, 3), np.uint8)}, {'seed': -1}, {'seed': 2**32},
                {'seed': True}, {'seed': 1.5}):
        with pytest.raises(_native.DepthStereoError):
            ag.create_autostereogram(d, **bad)
        with pytest.raises(_native.DepthStereoError):
            ag.create_autostereogram_batch(x, **bad)
    for bad_x in (x.to(torch.int32), x.view(torch.int16), x.to(torch.float32), x[0], x.cpu(), d, x[:0]):
        with pytest.raises(_native.DepthStereoError):
            ag.create_autostereogram_batch(bad_x)
    for bad in (dict(period=15), dict(m=0), dict(m=129), dict(mode=3), dict(mode=2), dict(mode=2, tile=torch.zeros((2, 2, 4), dtype=torch.uint8, device="cuda")),
                dict(mode=2, tile=np.zeros((2, 2, 3), np.float32)), dict(mode=2, tile=torch.zeros((2, 2, 3), dtype=torch.uint8)), dict(seed=-1),
                dict(seed=True), dict(out=torch.empty((1, h, w, 4), dtype=torch.uint8, device="cuda")),
                dict(out=torch.empty((1, h, w, 3), dtype=torch.int8, device="cuda"))):
        args = dict(dict(period=96, m=85, mode=0, seed=0), **bad)
        with pytest.raises(_native.DepthStereoError):
            _native.autostereogram_u8(x, args.pop('period'), args.pop('m'), args.pop('mode'), args.pop('seed'), **args)
    assert dict(_native.CALLS) == before


def test_funnel_autostereogram_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'autostereogram': A}) with caller-supplied I;16 depth maps (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.autostereogram_generation as ag
    from src import _native
    h, w = 24, 120
    tile = ac.tile_input(1)
    A = (32, 0.4, 'mono', 9)
    PX = ('circle', 3, 20.0, 8.0, 0.1, ('point', 0.25, 0.5), 6)
    rng = np.random.default_rng(5)
    imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(2)]
    d16 = [np.array(ac.depth_input("rect", (1, h, w))[0]), np.array(ac.depth_input("ramp", (1, h, w))[0])]
    base = {'gen_stereo': True, 'gen_normalmap': True, 'gen_heatmap': True, 'stereo_modes': ['left-right']}
    plain_kinds = ['depth', 'left-right', 'normalmap', 'heatmap']

    def run(ops, opts=base, kinds=plain_kinds):
        got = list(core.core_generation_funnel(None, list(imgs), [Image.fromarray(d) for d in d16], None, dict(opts), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(2) for k in kinds], [(i, k) for i, k, _ in got]
        for _, k, r in got:
            if k == 'autostereogram':
                assert isinstance(r, Image.Image) and r.mode == 'RGB' and r.size == (w, h)
        return {k: [r if isinstance(r, str) else np.stack([np.asarray(f) for f in r]) if isinstance(r, list) else np.asarray(r)
                    for _, kk, r in got if kk == k] for k in kinds}

    def same(a, b):
        return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)

    def delta(before):
        return {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}

    run(None)                                                                 # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(None)
    plain_delta = delta(before)
    assert "ds_autostereogram_u8" not in plain_delta
    own = plain['depth']                                                      # the funnel's own uint16 depth output

    def expect(params):
        pattern = params[2] if len(params) > 2 else 'dots'
        mode = {'dots': 0, 'mono': 1}[pattern] if isinstance(pattern, str) else 2
        model = [ac.model(d, params[0], int(np.rint(256 * params[1])), mode, params[3] if len(params) > 3 else 0, tile if mode == 2 else None)
                 for d in own]
        return dict(plain, autostereogram=model)

    want = expect(A)
    assert all(np.array_equal(m, np.asarray(ag.create_autostereogram(d, *A))) for m, d in zip(want['autostereogram'], own))
    before = dict(_native.CALLS)
    got = run({'autostereogram': A}, kinds=plain_kinds + ['autostereogram'])  # after 'heatmap', every other output as it was
    assert same(got, want)
    assert delta(before) == dict(plain_delta, ds_autostereogram_u8=1)         # one group: one call, nothing else changes
    # gone on the next call; absent, None and {} make the launches and the bytes of a plain call
    for ops in (None, {}, {'autostereogram': None}):
        before = dict(_native.CALLS)
        assert same(run(ops), plain), ops
        assert delta(before) == plain_delta, ops
    assert same(run({'autostereogram': list(A[:2])}, kinds=plain_kinds + ['autostereogram']), expect(A[:2]))          # pattern and seed default
    assert same(run({'autostereogram': (48, 0.25, tile)}, kinds=plain_kinds + ['autostereogram']), expect((48, 0.25, tile)))
    # after 'parallax' when both are asked for
    both = run({'autostereogram': A, 'parallax': PX}, kinds=plain_kinds + ['parallax', 'autostereogram'])
    assert same({k: both[k] for k in want}, want)
    # alone
    only = run({'autostereogram': A}, {'do_output_depth': False}, ['autostereogram'])
    assert same(only, {'autostereogram': want['autostereogram']})
    assert not hasattr(core.model_holder, 'autostereogram')                   # the option does not become a holder setting
    for bad in ({'autostereogram': (15, 0.3)}, {'autostereogram': (96, 0.6)}, {'autostereogram': (96,)}, {'autostereogram': "dots"},
                {'autostereogram': (True, 0.3)}, {'autostereogram': (96, float('nan'))}, {'autostereogram': (96, 0.3, 'stripes')},
                {'autostereogram': (96, 0.3, 'dots', -1)}, {'autostereogram': (96, 0.3, np.zeros((2, 2, 3), np.float32))}, {'autostereogram': {}}):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(bad)
        assert dict(_native.CALLS) == before, bad                             # before any device work
    assert same(run(None), plain)


def test_funnel_autostereogram_reads_the_refined_map_and_precedes_the_mesh(gpu, tmp_path):
    torch = gpu
    from PIL import Image
    import src.core as core
    h, w = 24, 120
    A, REFINE, PX = (32, 0.4, 'dots', 3), (5, 60.0, 2.0), ('line', 2, 30.0, 10.0, 0.1, 30000, 8)
    rng = np.random.default_rng(6)
    img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    d = np.array(ac.depth_input("rect", (1, h, w))[0])
    got = list(core.core_generation_funnel(str(tmp_path), [img], [Image.fromarray(d)], None, {'gen_heatmap': True, 'gen_simple_mesh': True},
                                           {'autostereogram': A, 'parallax': PX, 'depth_refine': REFINE}))
    assert [k for _, k, _ in got] == ['depth', 'heatmap', 'parallax', 'autostereogram', 'simple_mesh']
    refined = np.asarray(got[0][2])
    plain = np.asarray(next(r for _, k, r in core.core_generation_funnel(None, [img], [Image.fromarray(d)], None, {}, None) if k == 'depth'))
    assert not np.array_equal(refined, plain)
    picture = np.asarray(got[3][2])
    assert np.array_equal(picture, ac.model(refined, 32, 102, 0, 3))
    assert not np.array_equal(picture, ac.model(plain, 32, 102, 0, 3))
