"""Depth refinement (include/depthstereo.h: ds_joint_bilateral_u16; src/depth_refine.py; ops={'depth_refine': ...}) against its float64
NumPy model, tests/depth_refine_cases.py.  Every comparison is torch.equal / np.array_equal: the definition fixes the tables (made on
the host), the tap order and every rounding, so there is nothing to tolerate.  Shapes: smaller than a tile (5 x 7), ragged in both
directions (9 x 33), several 64 x 32 tiles (40 x 70), the largest radius against the smallest legal size (R = 15, 17 x 16), a window
wider than the image (4 x 6 under wrap).  tests/test_depth_refine_cpu.py shows what the definition is good for."""
import functools

import numpy as np
import pytest

import depth_refine_cases as rc

pytestmark = pytest.mark.gpu

# (n, h, w), (d, sigma_color, sigma_space)
KERNEL_CASES = [((1, 5, 7), (3, 3.0, 1.0)), ((2, 9, 33), (9, 300.0, 2.5)), ((1, 40, 70), (15, 40.0, 5.0)), ((3, 17, 16), (31, 25.0, 9.0)),
                ((2, 9, 33), (9, 0.05, 2.5))]
KERNEL_IDS = ["%dx%dx%d-d%d-sc%g" % (s + (p[0], p[1])) for s, p in KERNEL_CASES]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """{name: depth} and {name: guide} of one shape (seeded: the same arrays for every test that asks)."""
    n, h, w = shape
    return dict(rc.depth_cases(h, w, seed=100 * h + w, n=n)), dict(rc.guide_cases(h, w, seed=7 * h + w, n=n))


@functools.lru_cache(maxsize=None)
def _want(shape, params, dname, gname, wrap):
    """The model's answer, computed once per (inputs, parameters, border rule)."""
    depths, guides = _inputs(shape)
    out = rc.model(depths[dname], guides[gname], params, wrap)
    out.setflags(write=False)
    return out


def _filter(torch, d, g, params, wrap=False):
    from src import _native
    return _native.joint_bilateral_u16(torch.from_numpy(np.ascontiguousarray(d)).cuda(), torch.from_numpy(np.ascontiguousarray(g)).cuda(),
                                       *params, wrap=wrap)


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


@pytest.mark.parametrize("shape,params", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_equals_the_model_bit_for_bit(gpu, shape, params):
    torch = gpu
    from src import _native
    depths, guides = _inputs(shape)
    for dname, d in depths.items():
        for gname, g in guides.items():
            g4 = rc.with_fourth_byte(g, seed=shape[1] + shape[2])
            for wrap in (False, True):
                before = _native.CALLS["ds_joint_bilateral_u16"]
                got3 = _filter(torch, d, g, params, wrap)
                assert _native.CALLS["ds_joint_bilateral_u16"] == before + 1
                assert got3.dtype == torch.uint16 and tuple(got3.shape) == shape and got3.is_cuda
                got4 = _filter(torch, d, g4, params, wrap)
                assert torch.equal(got3, got4), (dname, gname, wrap, "c == 3 against c == 4")
                want = _want(shape, params, dname, gname, wrap)
                assert np.array_equal(got3.cpu().numpy(), want), (dname, gname, wrap, _mismatch(got3.cpu().numpy(), want))


def test_window_wider_than_the_image_under_wrap(gpu):
    torch = gpu
    from src import _native
    params = (31, 25.0, 9.0)
    for (dname, d), (gname, g) in zip(rc.depth_cases(4, 6, seed=46, n=1), rc.guide_cases(4, 6, seed=47, n=1)):
        got = _filter(torch, d, g, params, wrap=True).cpu().numpy()
        assert np.array_equal(got, rc.model(d, g, params, wrap=True)), (dname, gname)
        before = _native.CALLS["ds_joint_bilateral_u16"]
        with pytest.raises(_native.DepthStereoError):
            _filter(torch, d, g, params, wrap=False)
        assert _native.CALLS["ds_joint_bilateral_u16"] == before


def test_iterations_are_model_passes(gpu):
    torch = gpu
    from src import _native
    shape, params = (2, 9, 33), (9, 300.0, 2.5)
    depths, guides = _inputs(shape)
    for dname, gname in (("random", "regions"), ("ramp", "noise"), ("staircase", "regions")):
        for wrap in (False, True):
            want = depths[dname]
            for _ in range(3):
                want = rc.model(want, guides[gname], params, wrap)
            before = _native.CALLS["ds_joint_bilateral_u16"]
            got = _filter(torch, depths[dname], guides[gname], params + (3,), wrap)
            assert _native.CALLS["ds_joint_bilateral_u16"] == before + 3                     # one launch per pass
            assert np.array_equal(got.cpu().numpy(), want), (dname, gname, wrap)
            assert np.array_equal(rc.model(depths[dname], guides[gname], params + (3,), wrap), want)
            two = _filter(torch, depths[dname], guides[gname], params + (2,), wrap)            # an even count ends in the other buffer
            assert np.array_equal(two.cpu().numpy(), rc.model(depths[dname], guides[gname], params + (2,), wrap)), (dname, gname, wrap)


def test_misaligned_inputs_give_the_same_bits(gpu):
    """Depth at ptr % 8 == 2 and the guide at an odd byte address, c == 3 and c == 4."""
    torch = gpu
    from src import _native
    for shape, params in KERNEL_CASES[:4]:
        n, h, w = shape
        depths, guides = _inputs(shape)
        d = depths["random"]
        dbuf = torch.zeros(n * h * w + 4, dtype=torch.uint16, device="cuda")
        dview = dbuf.view(-1)[1:1 + n * h * w]
        dview.copy_(torch.from_numpy(d).cuda().view(-1))
        dview = dview.view(n, h, w)
        assert dview.data_ptr() % 8 == 2 and dview.is_contiguous()
        for gname in ("noise", "regions"):
            for g in (guides[gname], rc.with_fourth_byte(guides[gname], seed=h)):
                c = g.shape[-1]
                gbuf = torch.zeros(n * h * w * c + 8, dtype=torch.uint8, device="cuda")
                gview = gbuf[1:1 + n * h * w * c]
                gview.copy_(torch.from_numpy(g).cuda().view(-1))
                gview = gview.view(n, h, w, c)
                assert gview.data_ptr() % 2 == 1 and gview.is_contiguous()
                for wrap in (False, True):
                    got = _native.joint_bilateral_u16(dview, gview, *params, wrap=wrap)
                    assert torch.equal(got, _filter(torch, d, g, params, wrap)), (shape, gname, c, wrap)
                    assert np.array_equal(got.cpu().numpy(), _want(shape, params, "random", gname, wrap)), (shape, gname, c, wrap)


def test_batch_invariance_and_independence(gpu):
    """Image 2 of a batch of 3 equals that image run alone; changing image 0 (its depth or its guide) changes only output 0."""
    torch = gpu
    for (h, w), params in (((9, 33), (9, 300.0, 2.5)), ((40, 70), (15, 40.0, 5.0)), ((17, 16), (31, 25.0, 9.0))):
        for wrap in (False, True):
            d = rc.ramp_noise(h, w, seed=h, n=3)
            d[1] = rc.random_depth(h, w, seed=w)
            g = rc.regions_guide(h, w, seed=h + 1, n=3)
            g[2] = rc.noise_guide(h, w, seed=w + 1)
            y3 = _filter(torch, d, g, params, wrap)
            y1 = _filter(torch, d[2:3].copy(), g[2:3].copy(), params, wrap)
            assert torch.equal(y3[2:3], y1), (h, w, wrap)
            d2 = d.copy()
            d2[0] = rc.random_depth(h, w, seed=h + w + 1)
            z3 = _filter(torch, d2, g, params, wrap)
            assert torch.equal(z3[1:], y3[1:]) and not torch.equal(z3[0], y3[0]), (h, w, wrap)
            g2 = g.copy()
            g2[0] = rc.noise_guide(h, w, seed=h + w + 2)
            z3 = _filter(torch, d, g2, params, wrap)
            assert torch.equal(z3[1:], y3[1:]) and not torch.equal(z3[0], y3[0]), (h, w, wrap)


def test_table_cache_is_bounded(gpu):
    torch = gpu
    from src import _native
    d, g = rc.ramp_noise(8, 8, seed=1, n=1), rc.regions_guide(8, 8, seed=2, n=1)
    first = _filter(torch, d, g, (3, 10.0, 1.0))
    for k in range(6):
        _filter(torch, d, g, (3, 11.0 + k, 1.0))
    assert _native.cached_tables("depth_refine") == 4
    assert torch.equal(_filter(torch, d, g, (3, 10.0, 1.0)), first)                    # evicted and rebuilt: same bits
    assert _native.cached_tables("depth_refine") == 4
    assert np.array_equal(first.cpu().numpy(), rc.model(d, g, (3, 10.0, 1.0)))


def test_families_share_one_cache_but_no_table(gpu):
    """The tables of the pre-filter, of depth refinement and of the temporal filter live in ONE cache.  The same (3, 10.0, 1.0) names a
    65536-entry wr, a 766-entry wc and a 4-entry wt: each family must get its own, and a family that overflows its bound of 4 must
    evict only its own."""
    torch = gpu
    import normalmap_bilateral_cases as bc
    import video_stabilize_cases as sc
    from src import _native
    P = (3, 10.0, 1.0)
    d, g = rc.ramp_noise(8, 8, seed=1, n=1), rc.regions_guide(8, 8, seed=2, n=1)
    x = torch.from_numpy(d).cuda()
    want_plain, want_joint, (want_wt, want_wc) = bc.model(d, P), rc.model(d, g, P), sc.tables(*P)

    def stabilize_tables():
        wt, wc = _native.stabilize_tables_on(x.device, *P)
        assert wt.is_cuda and wc.is_cuda and tuple(wt.shape) == (4,) and tuple(wc.shape) == (766,)
        assert np.array_equal(wt.cpu().numpy(), want_wt) and np.array_equal(wc.cpu().numpy(), want_wc)

    assert np.array_equal(_native.bilateral_u16(x, *P).cpu().numpy(), want_plain)
    stabilize_tables()
    assert np.array_equal(_filter(torch, d, g, P).cpu().numpy(), want_joint)
    stabilize_tables()
    assert np.array_equal(_native.bilateral_u16(x, *P).cpu().numpy(), want_plain)
    families = ("bilateral", "depth_refine", "stabilize")
    for family in families:
        before = {f: _native.cached_tables(f) for f in families}
        assert all(1 <= c <= 4 for c in before.values()), before
        for k in range(5):                                                             # five further sets: past the bound whatever it held
            if family == "bilateral":
                _native.bilateral_u16(x, 3, 21.0 + k, 1.0)
            elif family == "depth_refine":
                _filter(torch, d, g, (3, 21.0 + k, 1.0))
            else:
                _native.stabilize_tables_on(x.device, 3, 21.0 + k, 1.0)
        after = {f: _native.cached_tables(f) for f in families}
        assert after == dict(before, **{family: 4}), (family, before, after)
    # the three tables of P were evicted by their own families only, and come back with the same bits
    assert np.array_equal(_native.bilateral_u16(x, *P).cpu().numpy(), want_plain)
    assert np.array_equal(_filter(torch, d, g, P).cpu().numpy(), want_joint)
    stabilize_tables()


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    dev = torch.cuda.current_device()
    ctx = _native.ctx_for(dev)
    EINVAL = -1
    n, h, w, r = 1, 8, 12, 2
    SENT = -21555                                                                      # (int16 views of the uint16 planes: torch fills those)
    ws_np, wc_np = _native.depth_refine_tables(2 * r + 1, 40.0, 2.0)
    ws, wc = torch.from_numpy(ws_np).cuda(), torch.from_numpy(wc_np).cuda()
    ws3, ws15, ws17 = (torch.from_numpy(_native.depth_refine_tables(d, 40.0, 2.0)[0]).cuda() for d in (3, 15, 17))
    x = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
    gd = torch.zeros((n * h * w * 4 + 1,), dtype=torch.uint8, device="cuda")          # room for c == 4 at an odd address
    out = torch.full((n, h, w), SENT, dtype=torch.int16, device="cuda")
    big = torch.full((2 * n * h * w,), SENT, dtype=torch.int16, device="cuda")         # one block to carve overlapping depth / out from
    nd = 2 * n * h * w                                                                 # bytes of depth and of out; big has 2 * nd
    B = big.data_ptr()
    assert B % 8 == 0 and gd.data_ptr() % 2 == 0

    def call(c=ctx, xp=x.data_ptr(), gp=gd.data_ptr(), gc=3, n=n, h=h, w=w, r=r, wsp=ws.data_ptr(), wcp=wc.data_ptr(), wrap=0,
             op=out.data_ptr()):
        return L.ds_joint_bilateral_u16(c, xp, gp, gc, n, h, w, r, wsp, wcp, wrap, op, None)
    _native.kernel_timer_enable(dev, True)
    try:
        assert call(c=None) == EINVAL and call(xp=None) == EINVAL and call(gp=None) == EINVAL and call(wsp=None) == EINVAL
        assert call(wcp=None) == EINVAL and call(op=None) == EINVAL
        assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-3) == EINVAL and call(n=-1) == EINVAL
        assert call(gc=0) == EINVAL and call(gc=1) == EINVAL and call(gc=2) == EINVAL and call(gc=5) == EINVAL and call(gc=-3) == EINVAL
        assert call(r=0) == EINVAL and call(r=16) == EINVAL and call(r=-1) == EINVAL
        assert call(r=8) == EINVAL and call(r=9) == EINVAL and call(h=2, r=2) == EINVAL               # radius >= min(h, w), no wrap
        # out overlapping depth: equal pointers, out beginning in the last 2 bytes of depth, depth beginning in the last 2 bytes of out
        assert call(xp=B, op=B) == EINVAL
        assert call(xp=B, op=B + nd - 2) == EINVAL
        assert call(xp=B + nd - 2, op=B) == EINVAL
        # alignment: ws, wc 8 bytes; depth, out 2 bytes
        assert call(wsp=ws.data_ptr() + 4) == EINVAL and call(wcp=wc.data_ptr() + 4) == EINVAL and call(wcp=wc.data_ptr() + 2) == EINVAL
        assert call(xp=x.data_ptr() + 1) == EINVAL and call(op=out.data_ptr() + 1) == EINVAL
        # the grid limit: n = 65536 one-pixel images (every buffer really that large): DS_EUNSUPPORTED, one fewer runs (below)
        xn = torch.zeros((65536, 1, 1), dtype=torch.int16, device="cuda")
        gn = torch.zeros((65536, 1, 1, 3), dtype=torch.uint8, device="cuda")
        on = torch.full((65536, 1, 1), SENT, dtype=torch.int16, device="cuda")
        many = dict(xp=xn.data_ptr(), gp=gn.data_ptr(), op=on.data_ptr(), h=1, w=1, wrap=1)
        assert call(n=65536, **many) == -2 and bool((on == SENT).all())
        torch.cuda.synchronize()
        launches, _ = _native.kernel_timer_read(dev, "depth_refine")
        assert launches == 0                                                                          # every one returned before the launch
        assert bool((out == SENT).all()) and bool((big == SENT).all())
        assert b"ds_joint_bilateral_u16" in L.ds_last_error()
        # and the legal neighbours of those cases run: r = 1, r = 7 = min - 1, r = 8 under wrap, c == 4, a guide at an odd address,
        # adjacent but disjoint blocks
        assert call(r=1, wsp=ws3.data_ptr()) == 0
        assert call(r=7, wsp=ws15.data_ptr()) == 0 and call(r=8, wsp=ws17.data_ptr(), wrap=1) == 0
        assert call(gc=4) == 0 and call(gp=gd.data_ptr() + 1) == 0 and call(gp=gd.data_ptr() + 1, gc=4) == 0
        assert call(xp=B + nd, op=B) == 0                                                             # depth begins where out ends
        assert call(xp=B, op=B + nd) == 0                                                             # out begins where depth ends
        assert call(n=65535, **many) == 0
        torch.cuda.synchronize()
        assert bool((on[:65535] == 0).all()) and int(on[65535]) == SENT
        launches, ms = _native.kernel_timer_read(dev, "depth_refine")
        assert launches == 9 and ms > 0.0, (launches, ms)                                          # the timer brackets each launch
        assert _native.kernel_timer_read(dev, "normalmap")[0] == 0                                    # and it is a kind of its own
        assert bool((out == 0).all())                                                                 # flat zero depth stays flat: written
    finally:
        _native.kernel_timer_enable(dev, False)


def test_public_interface_checks_before_any_launch(gpu):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.depth_refine as dr
    h, w = 12, 20
    P = (5, 40.0, 2.0)
    d, g = rc.ramp_noise(h, w, seed=3), rc.regions_guide(h, w, seed=4)
    want = rc.model(d, g, P)
    for image in (g, Image.fromarray(g), rc.with_fourth_byte(g, 5), Image.fromarray(rc.with_fourth_byte(g, 5))):
        for depth in (d, Image.fromarray(d)):
            got = dr.refine_depthmap(image, depth, P)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(dr.refine_depthmap(g, d, list(P) + [2], wrap=True), rc.model(d, g, P + (2,), wrap=True))
    gray = Image.fromarray(g[:, :, 0])
    assert gray.mode == "L"
    assert np.array_equal(dr.refine_depthmap(gray, d, P), rc.model(d, np.asarray(gray.convert("RGB")), P))
    y = dr.refine_depthmap_batch(torch.from_numpy(d).cuda()[None], torch.from_numpy(g).cuda()[None], P)
    assert y.is_cuda and y.dtype == torch.uint16 and np.array_equal(y[0].cpu().numpy(), want)
    before = dict(_native.CALLS)
    for bad_depth in (d.astype(np.float32), d.astype(np.int32), d.astype(np.uint8), Image.fromarray(d.astype(np.uint8)), d[None]):
        with pytest.raises(_native.DepthStereoError):
            dr.refine_depthmap(g, bad_depth, P)
    for bad_image in (g[:, :-1], g[:-1], g.astype(np.float32), Image.fromarray(g).resize((w + 1, h))):
        with pytest.raises(_native.DepthStereoError):
            dr.refine_depthmap(bad_image, d, P)
    for bad in ((4, 1, 1), (5, 0.0, 1.0), (33, 1.0, 1.0), (5, 1.0), (5, 1, 1, 0), (5, 1, 1, 9), (True, 1, 1), "5"):
        with pytest.raises(_native.DepthStereoError):
            dr.refine_depthmap(g, d, bad)
        with pytest.raises(_native.DepthStereoError):
            dr.refine_depthmap_batch(torch.from_numpy(d).cuda()[None], torch.from_numpy(g).cuda()[None], bad)
    with pytest.raises(_native.DepthStereoError):
        dr.refine_depthmap(g, d, (31, 25.0, 9.0))                                      # 15 >= min(h, w) without wrap
    x, gg = torch.from_numpy(d).cuda()[None], torch.from_numpy(g).cuda()[None]
    for bd, bg in ((x.to(torch.int32), gg), (x, gg.to(torch.int16)), (x, gg[:, :, :, :2]), (x, gg[:, :-1]), (x[0], gg), (x, gg.cpu()),
                   (x.cpu(), gg)):
        with pytest.raises(_native.DepthStereoError):
            dr.refine_depthmap_batch(bd, bg, P)
    assert dict(_native.CALLS) == before


def test_funnel_depth_refine_is_an_option_of_the_call(gpu, oracle):
    """core_generation_funnel(..., ops={'depth_refine': P}) with caller-supplied I;16 depth maps (no network involved), stereo and
    normal map on: every consumer of the uint16 depth map sees the refined one."""
    torch = gpu
    from PIL import Image
    import src.core as core
    from src import _native
    h, w = 24, 40
    P = (5, 60.0, 2.0)
    rgb = [rc.regions_guide(h, w, seed=12), (rc.noise_guide(h, w, seed=13) // 16 + 100).astype(np.uint8)]
    imgs = [Image.fromarray(a) for a in rgb]
    d16 = [rc.staircase(h, w, cliff_at=w // 2 + 2), rc.ramp_noise(h, w, seed=40)]          # a cliff 2 columns off image 0's colour edge
    base = {'gen_stereo': True, 'gen_normalmap': True, 'stereo_modes': ['left-right']}
    kinds = ['depth', 'left-right', 'normalmap']

    def run(ops, images=imgs, opts=base, kinds=kinds):
        got = list(core.core_generation_funnel(None, list(images), [Image.fromarray(d) for d in d16], None, dict(opts), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(2) for k in kinds], [(i, k) for i, k, _ in got]
        return {k: [np.asarray(r) for _, kk, r in got if kk == k] for k in kinds}

    def same(a, b):
        return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)

    def expect(params, wrap=False, bilateral=None, rgbs=rgb):
        refined = [rc.model(d, g, params, wrap) for d, g in zip(own, rgbs)]
        nm_in = refined
        if bilateral is not None:
            import normalmap_bilateral_cases as bc
            nm_in = [bc.model(d, bilateral) for d in refined]
        return {'depth': refined,
                'left-right': [oracle.create_stereoimages_arrays(g, d, 2.5, 0.0, ['left-right'], 0.0, 1.0, 'polylines_sharp')[0]
                               for g, d in zip(rgbs, refined)],
                'normalmap': [oracle.create_normalmap_array(d) for d in nm_in]}

    run(None)                                                                 # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(None)
    plain_delta = {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}
    assert "ds_joint_bilateral_u16" not in plain_delta
    own = plain['depth']                                                      # the funnel's own uint16 depth (renormalised)
    assert len(own) == 2 and all(d.dtype == np.uint16 and d.shape == (h, w) for d in own)
    want = expect(P)
    assert not any(np.array_equal(a, b) for a, b in zip(want['depth'], plain['depth']))
    assert not any(np.array_equal(want[k][0], plain[k][0]) for k in kinds)                             # at the cliff every output changes
    before = _native.CALLS["ds_joint_bilateral_u16"]
    assert same(run({'depth_refine': P}), want)
    assert _native.CALLS["ds_joint_bilateral_u16"] == before + 1             # one group, one pass: one launch
    # gone on the next call; absent, None and {} make the launches and the bytes of a plain call
    for ops in (None, {}, {'depth_refine': None}, {'depth_refine': None, 'depth_refine_wrap': True}):
        before = dict(_native.CALLS)
        assert same(run(ops), plain), ops
        assert {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)} == plain_delta, ops
    assert same(run({'depth_refine': list(P)}), want)
    before = _native.CALLS["ds_joint_bilateral_u16"]
    assert same(run({'depth_refine': P + (3,)}), expect(P + (3,)))
    assert _native.CALLS["ds_joint_bilateral_u16"] == before + 3
    wrapped = expect(P, wrap=True)
    assert not np.array_equal(wrapped['depth'][0], want['depth'][0])
    assert same(run({'depth_refine': P, 'depth_refine_wrap': True}), wrapped)
    assert same(run({'depth_refine': P, 'depth_refine_wrap': False}), want)
    assert same(run({'depth_refine': P, 'depth_refine_wrap': 'tiling'}), want)                        # TILING_MODE is off
    B = (5, 300.0, 2.0)
    assert same(run({'depth_refine': P, 'normalmap_bilateral': B}), expect(P, bilateral=B))
    for name in ('depth_refine', 'depth_refine_wrap'):
        assert not hasattr(core.model_holder, name)                           # the options do not become holder settings
    for bad in ({'depth_refine': (4, 1, 1)}, {'depth_refine': (5, 1.0)}, {'depth_refine': "5"}, {'depth_refine': (5, 1, 1, 0)},
                {'depth_refine': (5, 1, 1, 9)}, {'depth_refine': (True, 1, 1)}, {'depth_refine': P, 'depth_refine_wrap': 'yes'}):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(bad)
        assert dict(_native.CALLS) == before, bad                             # before any device work
    assert same(run(None), plain)
    # an L-mode image plus a custom map, without stereo: the guide is the image's RGB conversion
    gray = [Image.fromarray(a[:, :, 1]) for a in rgb]
    assert gray[0].mode == "L"
    nost = {'gen_normalmap': True}
    kn = ['depth', 'normalmap']
    plain_gray = run(None, gray, nost, kn)
    assert same(plain_gray, {k: plain[k] for k in kn})                        # (the custom maps do not depend on the image)
    gray_rgb = [np.asarray(im.convert("RGB")) for im in gray]
    want_gray = expect(P, rgbs=gray_rgb)
    assert same(run({'depth_refine': P}, gray, nost, kn), {k: want_gray[k] for k in kn})
    # and an RGB image without stereo: nothing uploaded the image yet
    assert same(run({'depth_refine': P}, imgs, nost, kn), {k: want[k] for k in kn})


def test_funnel_network_branch_refines_what_the_consumers_read(gpu, oracle):
    """The network branch (a registered predictor stands in for the network): the guide is the RGB tensor the branch uploaded anyway
    (no stereo) or the stereo step's image tensor; the raw prediction of DO_OUTPUT_DEPTH_PREDICTION stays the network's."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import util
    from src import _native
    h, w = 48, 72
    P = (7, 40.0, 2.5, 2)
    img = rc.regions_guide(h, w, seed=31, noise=6)
    pred = util.smooth_depth(h, w, 6)
    core.model_holder.register_predictor(4, lambda pil, nw, nh, dev: torch.from_numpy(pred).to(dev))
    d16 = oracle.convert_to_i16(oracle.depth_normalize01(pred, False))
    refined = rc.model(d16, img, P)
    assert not np.array_equal(refined, d16)
    for image, guide in ((Image.fromarray(img), img), (Image.fromarray(img).convert("L"), None)):
        if guide is None:
            guide = np.asarray(image.convert("RGB"))
        want = rc.model(d16, guide, P)
        for opts in ({'gen_normalmap': True}, {'gen_normalmap': True, 'do_output_depth_prediction': True}):
            got = list(core.core_generation_funnel(None, [image], None, None, dict(opts, model_type=4), {'depth_refine': P}))
            res = {k: r for _, k, r in got}
            assert np.array_equal(np.asarray(res['depth']), want)
            assert np.array_equal(np.asarray(res['normalmap']), oracle.create_normalmap_array(want))
            if 'do_output_depth_prediction' in opts:
                assert np.array_equal(np.asarray(res['depth_prediction']), pred)              # untouched
    before = dict(_native.CALLS)
    got = list(core.core_generation_funnel(None, [Image.fromarray(img)], None, None,
                                           {'model_type': 4, 'gen_stereo': True, 'stereo_modes': ['left-right'], 'gen_heatmap': True},
                                           {'depth_refine': P}))
    assert [k for _, k, _ in got] == ['depth', 'left-right', 'heatmap']
    assert _native.CALLS["ds_joint_bilateral_u16"] == before.get("ds_joint_bilateral_u16", 0) + 2
    assert np.array_equal(np.asarray(got[0][2]), refined)
    assert np.array_equal(np.asarray(got[1][2]),
                          oracle.create_stereoimages_arrays(img, refined, 2.5, 0.0, ['left-right'], 0.0, 1.0, 'polylines_sharp')[0])
    plain = list(core.core_generation_funnel(None, [Image.fromarray(img)], None, None, {'model_type': 4, 'gen_heatmap': True}))
    from src import heatmap
    want_heat = heatmap.colorize_batch(torch.from_numpy(refined).cuda()[None])[0].cpu().numpy()
    assert np.array_equal(np.asarray(got[2][2]), want_heat) and not np.array_equal(np.asarray(plain[-1][2]), want_heat)
