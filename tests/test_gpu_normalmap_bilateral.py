"""The bilateral pre-filter of the normal map (include/depthstereo.h: ds_bilateral_u16; create_normalmap(..., bilateral=(d,
sigma_color, sigma_space)); ops={'normalmap_bilateral': ...}) against its float64 NumPy model, tests/normalmap_bilateral_cases.py.
Every comparison is torch.equal / np.array_equal: the definition fixes the tables (made on the host), the tap order and every
rounding, so there is nothing to tolerate.  Shapes: smaller than a tile (5 x 7), ragged in both directions (9 x 33), several 64 x 32
tiles (40 x 70), the largest radius against the smallest legal size (R = 15, 17 x 16), a window wider than the image (4 x 6 under
wrap).  tests/test_normalmap_bilateral_cpu.py shows what the definition is good for."""
import numpy as np
import pytest

import normalmap_bilateral_cases as bc

pytestmark = pytest.mark.gpu

# (n, h, w), (d, sigma_color, sigma_space)
KERNEL_CASES = [((1, 5, 7), (3, 3.0, 1.0)), ((2, 9, 33), (9, 300.0, 2.5)), ((1, 40, 70), (15, 20000.0, 5.0)), ((3, 17, 16), (31, 50.0, 9.0))]
KERNEL_IDS = ["%dx%dx%d-d%d" % (s + (p[0],)) for s, p in KERNEL_CASES]


def _filter(torch, d, params, wrap=False):
    from src import _native
    return _native.bilateral_u16(torch.from_numpy(np.ascontiguousarray(d)).cuda(), *params, wrap=wrap)


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


@pytest.mark.parametrize("shape,params", KERNEL_CASES, ids=KERNEL_IDS)
def test_kernel_equals_the_model_bit_for_bit(gpu, shape, params):
    torch = gpu
    from src import _native
    n, h, w = shape
    for name, d in bc.cases(h, w, seed=100 * h + w, n=n):
        for wrap in (False, True):
            before = _native.CALLS["ds_bilateral_u16"]
            got = _filter(torch, d, params, wrap)
            assert _native.CALLS["ds_bilateral_u16"] == before + 1
            assert got.dtype == torch.float64 and tuple(got.shape) == shape and got.is_cuda
            want = bc.model(d, params, wrap)
            assert np.array_equal(got.cpu().numpy(), want), (name, wrap, _mismatch(got.cpu().numpy(), want))


def test_window_wider_than_the_image_under_wrap(gpu):
    torch = gpu
    from src import _native
    params = (31, 50.0, 9.0)
    for name, d in bc.cases(4, 6, seed=46, n=1):
        got = _filter(torch, d, params, wrap=True).cpu().numpy()
        assert np.array_equal(got, bc.model(d, params, wrap=True)), name
        with pytest.raises(_native.DepthStereoError):
            _filter(torch, d, params, wrap=False)


def test_misaligned_input_gives_the_same_bits(gpu):
    torch = gpu
    from src import _native
    for (n, h, w), params in KERNEL_CASES:
        d = bc.random_depth(h, w, seed=7 * h + w, n=n)
        buf = torch.zeros(n * h * w + 4, dtype=torch.uint16, device="cuda")
        view = buf.view(-1)[1:1 + n * h * w]
        view.copy_(torch.from_numpy(d).cuda().view(-1))
        view = view.view(n, h, w)
        assert view.data_ptr() % 8 == 2 and view.is_contiguous()
        for wrap in (False, True):
            got = _native.bilateral_u16(view, *params, wrap=wrap)
            assert torch.equal(got, _filter(torch, d, params, wrap)), (h, w, wrap)
            assert np.array_equal(got.cpu().numpy(), bc.model(d, params, wrap)), (h, w, wrap)


def test_batch_invariance_and_independence(gpu):
    """Image 2 of a batch of 3 equals that image run alone; changing image 0 leaves the other images' outputs untouched."""
    torch = gpu
    for (h, w), params in (((9, 33), (9, 300.0, 2.5)), ((40, 70), (15, 20000.0, 5.0)), ((17, 16), (31, 50.0, 9.0))):
        for wrap in (False, True):
            d = bc.ramp_noise(h, w, seed=h, n=3)
            d[1] = bc.random_depth(h, w, seed=w)
            y3 = _filter(torch, d, params, wrap)
            y1 = _filter(torch, d[2:3].copy(), params, wrap)
            assert torch.equal(y3[2:3], y1), (h, w, wrap)
            d2 = d.copy()
            d2[0] = bc.random_depth(h, w, seed=h + w + 1)
            z3 = _filter(torch, d2, params, wrap)
            assert torch.equal(z3[1:], y3[1:]) and not torch.equal(z3[0], y3[0]), (h, w, wrap)


CHAIN_PARAMS = (5, 300.0, 2.0)


@pytest.mark.parametrize("opt", [(None, 3, None), (3, 5, 3), (None, None, None)], ids=["sobel3", "blur3-sobel5-blur3", "gradient"])
def test_whole_chain_equals_the_oracle_on_the_filtered_map(gpu, oracle, opt):
    torch = gpu
    import src.normalmap_generation as nm
    import normalmap_wrap_cases as wc
    n, h, w = 2, 24, 40
    r = CHAIN_PARAMS[0] // 2
    maps = [bc.ramp_noise(h, w, seed=5), bc.staircase(h, w)]
    for d in maps:
        for inv in (False, True):
            got = np.asarray(nm.create_normalmap(d, opt[0], opt[1], opt[2], inv, False, bilateral=CHAIN_PARAMS))
            want = oracle.create_normalmap_array(bc.model(d, CHAIN_PARAMS), opt[0], opt[1], opt[2], inv)
            assert got.shape == (h, w, 3) and got.dtype == np.uint8
            assert np.array_equal(got, want), (opt, inv, "reflect")
            # wrap: the same call on the np.pad(mode='wrap')-padded map, cropped; pad = R + the summed radii of the other passes
            pad = r + wc.radius(opt[0] or 0, opt[1] or 0, opt[2] or 0)
            got = np.asarray(nm.create_normalmap(d, opt[0], opt[1], opt[2], inv, True, bilateral=CHAIN_PARAMS))
            big = np.pad(d, pad, mode='wrap')
            want = oracle.create_normalmap_array(bc.model(big, CHAIN_PARAMS), opt[0], opt[1], opt[2], inv)[pad:pad + h, pad:pad + w]
            assert np.array_equal(got, want), (opt, inv, "wrap")
    # the batch entry point: both maps at once = each alone
    x = torch.from_numpy(np.stack(maps)).cuda()
    y = nm.create_normalmap_batch(x, opt[0], opt[1], opt[2], False, bilateral=CHAIN_PARAMS).cpu().numpy()
    for j in range(n):
        assert np.array_equal(y[j], np.asarray(nm.create_normalmap(maps[j], opt[0], opt[1], opt[2], False, bilateral=CHAIN_PARAMS))), j


def test_defaults_keep_todays_bytes_and_entry_points(gpu, oracle):
    torch = gpu
    import src.normalmap_generation as nm
    from src import _native
    d = bc.ramp_noise(24, 40, seed=9)
    x = torch.from_numpy(d).cuda().unsqueeze(0)
    for opt, name in (((None, 3, None), "ds_normalmap"), ((5, 3, 5), "ds_normalmap"), ((None, None, None), "ds_normalmap")):
        for wrap in (False, True):
            before = dict(_native.CALLS)
            a = nm.create_normalmap_batch(x, *opt, False, wrap)
            b = nm.create_normalmap_batch(x, *opt, False, wrap, bilateral=None)
            c = nm.create_normalmap_batch(x, *opt, False, wrap=wrap, bilateral=None)
            delta = {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}
            assert delta == {name + ("_wrap" if wrap else ""): 3}, delta                 # the parent's entry point and nothing else
            assert torch.equal(a, b) and torch.equal(a, c)
            if not wrap:
                assert np.array_equal(a[0].cpu().numpy(), oracle.create_normalmap_array(d, *opt, False)), opt
                assert np.array_equal(np.asarray(nm.create_normalmap(d, *opt, False)), a[0].cpu().numpy()), opt
    for dt, name in ((np.float64, "ds_normalmap_f64"), (np.float32, "ds_normalmap_gradient_f32")):
        xf = torch.from_numpy(d.astype(dt)).cuda().unsqueeze(0)
        before = dict(_native.CALLS)
        a = nm.create_normalmap_batch(xf, None, None, None, False)
        b = nm.create_normalmap_batch(xf, None, None, None, False, bilateral=None)
        delta = {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}
        assert delta == {name: 2} and torch.equal(a, b), delta
    # with the filter: ds_bilateral_u16 once, then the float64 entry point
    for wrap in (False, True):
        before = dict(_native.CALLS)
        f = nm.create_normalmap_batch(x, None, 3, None, False, wrap, bilateral=(5, 300.0, 2.0))
        delta = {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}
        assert delta == {"ds_bilateral_u16": 1, "ds_normalmap_f64" + ("_wrap" if wrap else ""): 1}, delta
        assert not torch.equal(f, nm.create_normalmap_batch(x, None, 3, None, False, wrap))
    # uint16 only, bad tuples
    for dt in (np.float64, np.float32, np.int32):
        with pytest.raises(_native.DepthStereoError, match="uint16"):
            nm.create_normalmap(d.astype(dt), None, 3, None, False, bilateral=(5, 300.0, 2.0))
        with pytest.raises(_native.DepthStereoError, match="uint16"):
            nm.create_normalmap_batch(torch.from_numpy(d.astype(dt)).cuda().unsqueeze(0), None, 3, None, False, bilateral=(5, 300.0, 2.0))
    for bad in ((4, 1, 1), (5, 0.0, 1.0), (33, 1.0, 1.0), (5, 1.0)):
        with pytest.raises(_native.DepthStereoError):
            nm.create_normalmap(d, None, 3, None, False, bilateral=bad)
        if len(bad) == 3:
            with pytest.raises(_native.DepthStereoError):
                _native.bilateral_u16(x, *bad)
    with pytest.raises(_native.DepthStereoError):
        _native.bilateral_u16(x.to(torch.int32), 5, 300.0, 2.0)


def test_table_cache_is_bounded(gpu):
    torch = gpu
    from src import _native
    d = bc.ramp_noise(8, 8, seed=1, n=1)
    first = _filter(torch, d, (3, 10.0, 1.0))
    for k in range(6):
        _filter(torch, d, (3, 11.0 + k, 1.0))
    assert _native.cached_tables("bilateral") == 4
    assert torch.equal(_filter(torch, d, (3, 10.0, 1.0)), first)                       # evicted and rebuilt: same bits
    assert _native.cached_tables("bilateral") == 4


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    dev = torch.cuda.current_device()
    ctx = _native.ctx_for(dev)
    EINVAL = -1
    n, h, w, r = 1, 8, 12, 2
    ws_np, wr_np = _native.bilateral_tables(2 * r + 1, 300.0, 2.0)
    ws, wr = torch.from_numpy(ws_np).cuda(), torch.from_numpy(wr_np).cuda()
    ws3, ws15, ws17 = (torch.from_numpy(_native.bilateral_tables(d, 300.0, 2.0)[0]).cuda() for d in (3, 15, 17))
    x = torch.zeros((n, h, w), dtype=torch.uint16, device="cuda")
    out = torch.full((n, h, w), -1.0, dtype=torch.float64, device="cuda")
    big = torch.full((2 * n * h * w,), -1.0, dtype=torch.float64, device="cuda")       # one block to carve overlapping depth / out from
    nd, no = 2 * n * h * w, 8 * n * h * w                                              # bytes of depth and of out; big has 2 * no
    B = big.data_ptr()
    assert B % 8 == 0 and nd % 8 == 0

    def call(c=ctx, xp=x.data_ptr(), n=n, h=h, w=w, r=r, wsp=ws.data_ptr(), wrp=wr.data_ptr(), wrap=0, op=out.data_ptr()):
        return L.ds_bilateral_u16(c, xp, n, h, w, r, wsp, wrp, wrap, op, None)
    _native.kernel_timer_enable(dev, True)
    try:
        assert call(c=None) == EINVAL and call(xp=None) == EINVAL and call(wsp=None) == EINVAL and call(wrp=None) == EINVAL
        assert call(op=None) == EINVAL
        assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-3) == EINVAL and call(n=-1) == EINVAL
        assert call(r=0) == EINVAL and call(r=16) == EINVAL and call(r=-1) == EINVAL
        assert call(r=8) == EINVAL and call(r=9) == EINVAL and call(h=2, r=2) == EINVAL               # radius >= min(h, w), no wrap
        # out overlapping depth: out inside the depth block, depth inside the out block, equal pointers
        assert call(xp=B, op=B) == EINVAL
        assert call(xp=B, op=B + nd - 8) == EINVAL                       # out begins in the last 8 bytes of depth
        assert call(xp=B + no - 2, op=B) == EINVAL                       # depth begins in the last 2 bytes of out
        assert call(xp=B + 64, op=B) == EINVAL                           # depth inside out
        # alignment: out, ws, wr 8 bytes
        assert call(op=B + 4) == EINVAL and call(wsp=ws.data_ptr() + 4) == EINVAL and call(wrp=wr.data_ptr() + 2) == EINVAL
        assert call(xp=x.data_ptr() + 1) == EINVAL                                                    # depth: 2 bytes
        torch.cuda.synchronize()
        launches, _ = _native.kernel_timer_read(dev, "normalmap")
        assert launches == 0                                                                          # every one returned before the launch
        assert bool((out == -1.0).all()) and bool((big == -1.0).all())
        assert b"ds_bilateral_u16" in L.ds_last_error()
        # and the legal neighbours of those cases run: r = 7 = min - 1, r = 8 under wrap, adjacent but disjoint blocks
        assert call(r=1, wsp=ws3.data_ptr()) == 0
        assert call(r=7, wsp=ws15.data_ptr()) == 0 and call(r=8, wsp=ws17.data_ptr(), wrap=1) == 0
        assert call(xp=B + no, op=B) == 0                                                             # depth begins where out ends
        assert call(xp=B, op=B + nd) == 0                                                             # out begins where depth ends
        torch.cuda.synchronize()
        launches, ms = _native.kernel_timer_read(dev, "normalmap")
        assert launches == 5 and ms > 0.0, (launches, ms)                                             # the timer brackets each launch
    finally:
        _native.kernel_timer_enable(dev, False)


def test_funnel_normalmap_bilateral_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'normalmap_bilateral': P}) with caller-supplied I;16 depth maps (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.normalmap_generation as nm
    from src import _native
    P = (5, 300.0, 2.0)
    rng = np.random.default_rng(12)
    imgs = [Image.fromarray(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)) for _ in range(2)]
    d16 = [bc.ramp_noise(24, 40, seed=40), bc.staircase(24, 40)]
    base = {'gen_normalmap': True}
    depth_out = []

    def run(ops):
        got = list(core.core_generation_funnel(None, list(imgs), [Image.fromarray(d) for d in d16], None, dict(base), ops))
        assert [(i, k) for i, k, _ in got] == [(0, 'depth'), (0, 'normalmap'), (1, 'depth'), (1, 'normalmap')], [(i, k) for i, k, _ in got]
        depth_out[:] = [np.asarray(r) for _, k, r in got if k == 'depth']           # the funnel's own uint16 depth (renormalised)
        return [np.asarray(r) for _, k, r in got if k == 'normalmap']

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    plain = run(None)
    assert len(depth_out) == 2 and all(d.dtype == np.uint16 and d.shape == (24, 40) for d in depth_out)
    unfiltered = [np.asarray(nm.create_normalmap(d)) for d in depth_out]
    filtered = [np.asarray(nm.create_normalmap(d, bilateral=P)) for d in depth_out]
    assert same(plain, unfiltered) and not any(np.array_equal(a, b) for a, b in zip(filtered, unfiltered))
    before = _native.CALLS["ds_bilateral_u16"]
    assert same(run({'normalmap_bilateral': P}), filtered)
    assert _native.CALLS["ds_bilateral_u16"] > before
    before = _native.CALLS["ds_bilateral_u16"]
    assert same(run(None), unfiltered)                                        # gone on the next call
    assert same(run({}), unfiltered) and same(run({'normalmap_bilateral': None}), unfiltered)
    assert _native.CALLS["ds_bilateral_u16"] == before
    assert same(run({'normalmap_bilateral': list(P)}), filtered)
    wrapped = [np.asarray(nm.create_normalmap(d, wrap=True, bilateral=P)) for d in depth_out]
    assert same(run({'normalmap_bilateral': P, 'normalmap_wrap': True}), wrapped)
    assert not hasattr(core.model_holder, 'normalmap_bilateral')              # the option does not become a holder setting
    for bad in ((4, 1, 1), (5, 1.0), "5"):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run({'normalmap_bilateral': bad})
        assert dict(_native.CALLS) == before                                  # before any device work
    assert same(run(None), unfiltered)
