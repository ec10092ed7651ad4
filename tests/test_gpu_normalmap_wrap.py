"""The wrap-around border mode of the normal-map kernels (`wrap=True`; include/depthstereo.h: ds_normalmap_wrap and its four
siblings) against its definition, bit for bit:

    normalmap_wrap(d) = normalmap(np.pad(d, R, mode='wrap'))[R:R+h, R:R+w]        (tests/normalmap_wrap_cases.py)

with `normalmap` (a) the project's own non-wrap entry point on the GPU, which the existing tests pin to the reference, for every
entry point and kernel path, and (b) the CPU oracle, an independent value, for uint16 and float64.  The shapes are the smallest at
which an index can go wrong: 2 x 2 (smallest legal map), 2 x 4 (one four-pixel group that is its own left and right neighbour),
5 x 7 (kernel radius above the image size with 7 / 7 / 7), 8 x 8, 37 x 52 (odd height), 33 x 260 (two blocks of four-pixel groups
per row), 64 x 64.  tests/test_normalmap_wrap_cpu.py pins the definition itself."""
import ctypes

import numpy as np
import pytest

import normalmap_wrap_cases as wc

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (2, 4), (5, 7), (8, 8), (37, 52), (33, 260), (64, 64)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


def _batch(torch, d):
    return torch.from_numpy(np.ascontiguousarray(d)).cuda().unsqueeze(0)


def _gpu_plain(torch):
    """The project's non-wrap function in the oracle's calling convention (depth array -> h x w x 3 array), dtype kept as given."""
    import src.normalmap_generation as nm

    def fn(d, pre, sob, post, inv):
        return nm.create_normalmap_batch(_batch(torch, d), pre, sob, post, inv)[0].cpu().numpy()
    return fn


def _gpu_wrap(torch, d, opt, inv=False):
    import src.normalmap_generation as nm
    return nm.create_normalmap_batch(_batch(torch, d), opt[0], opt[1], opt[2], inv, wrap=True)[0].cpu().numpy()


# (dtype, options): every entry point and every kernel path
PATHS = ([(np.uint16, (0, 3, 0)), (np.uint16, (0, 0, 0))]                       # fused4 (w % 4 == 0) or the scalar fused kernel
         + [(np.uint16, o) for o in wc.SEPARABLE] + [(np.float64, o) for o in wc.OPTIONS]      # separable float64 passes
         + [(np.float32, (0, 0, 0)), (np.float32, (3, 0, 3)), (np.float32, (5, 0, 0)), (np.float32, (0, 0, 7))]
         + [(np.float16, (0, 0, 0))])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_wrap_equals_the_non_wrap_entry_point_on_the_wrap_padded_input(gpu, shape):
    torch = gpu
    from src import _native
    h, w = shape
    plain = _gpu_plain(torch)
    for dtype, opt in PATHS:
        d = wc.depth(h, w, dtype, seed=h * 1000 + w)
        for inv in (False, True):
            before = dict(_native.CALLS)
            got = _gpu_wrap(torch, d, opt, inv)
            new = {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}
            assert len(new) == 1 and list(new)[0].endswith("_wrap"), new
            want = wc.wrap_by_definition(plain, d, *opt, invert=inv)
            assert np.array_equal(got, want), (np.dtype(dtype).name, opt, inv, np.argwhere((got != want).any(axis=2))[:8].tolist())


def test_wrap_scalar_fused_kernel_on_a_misaligned_slice(gpu):
    """w % 4 == 0 but the depth pointer is not 8-byte aligned: the launcher must take the one-pixel-per-lane kernel, in wrap mode too."""
    torch = gpu
    import src.normalmap_generation as nm
    plain = _gpu_plain(torch)
    for h, w in ((2, 4), (8, 8), (33, 260)):
        d = wc.depth(h, w, np.uint16, seed=h + w)
        host = np.zeros(h * w + 4, np.uint16)
        host[1:1 + h * w] = d.ravel()
        view = torch.from_numpy(host).cuda()[1:1 + h * w].view(1, h, w)
        assert view.data_ptr() % 8 == 2 and view.is_contiguous()
        for sob in (3, 0):
            got = nm.create_normalmap_batch(view, None, sob, None, False, wrap=True)[0].cpu().numpy()
            assert np.array_equal(got, wc.wrap_by_definition(plain, d, 0, sob, 0)), (h, w, sob)
            assert np.array_equal(got, _gpu_wrap(torch, d, (0, sob, 0))), (h, w, sob)           # = the aligned (fused4) launch


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_wrap_equals_the_oracle_on_the_wrap_padded_input(gpu, oracle, shape):
    torch = gpu
    h, w = shape
    for dtype in (np.uint16, np.float64):
        d = wc.depth(h, w, dtype, seed=h * 1000 + w + 7)
        for opt in wc.OPTIONS:
            for inv in (False, True):
                got = _gpu_wrap(torch, d, opt, inv)
                want = wc.wrap_by_definition(oracle.create_normalmap_array, d, *opt, invert=inv)
                assert np.array_equal(got, want), (np.dtype(dtype).name, opt, inv, np.argwhere((got != want).any(axis=2))[:8].tolist())


def test_wrap_commutes_with_roll_per_image_of_a_batch(gpu):
    torch = gpu
    import src.normalmap_generation as nm
    shifts = [(3, 50), (0, 1), (36, 17)]
    for dtype, opt in PATHS:
        for h, w in ((37, 52), (5, 8)):
            d = [wc.depth(h, w, dtype, seed=31 * j + h) for j in range(3)]
            sh = [(a % h, b % w) for a, b in shifts]
            x = torch.from_numpy(np.stack(d)).cuda()
            xr = torch.from_numpy(np.stack([np.roll(d[j], sh[j], axis=(0, 1)) for j in range(3)])).cuda()
            y = nm.create_normalmap_batch(x, *opt, False, wrap=True).cpu().numpy()
            yr = nm.create_normalmap_batch(xr, *opt, False, wrap=True).cpu().numpy()
            for j in range(3):
                assert np.array_equal(yr[j], np.roll(y[j], sh[j], axis=(0, 1))), (np.dtype(dtype).name, opt, h, w, j)


def test_wrap_images_of_a_batch_are_independent(gpu):
    """Image 1 of a batch of 3 equals the same image alone: the sample before row 0 / behind the last row of an image is a sample
    of the SAME image, not of its neighbour in memory."""
    torch = gpu
    import src.normalmap_generation as nm
    for dtype, opt in PATHS:
        for h, w in ((2, 4), (5, 7), (33, 260)):
            d = np.stack([wc.depth(h, w, dtype, seed=5 * j + w) for j in range(3)])
            y3 = nm.create_normalmap_batch(torch.from_numpy(d).cuda(), *opt, False, wrap=True)
            y1 = nm.create_normalmap_batch(torch.from_numpy(d[1:2].copy()).cuda(), *opt, False, wrap=True)
            assert torch.equal(y3[1:2], y1), (np.dtype(dtype).name, opt, h, w)


@pytest.mark.parametrize("shape", [(6, 8), (6, 7)], ids=["fused4", "scalar"])
def test_wrap_border_sentinel(gpu, oracle, shape):
    """A constant map with ONE distinct value in the last column: with wrap, column 0's zx sees it (and column w - 2's; nothing
    else in that row does); with the reference's borders column 0 is flat."""
    torch = gpu
    h, w = shape
    d = np.full((h, w), 20000, np.uint16)
    d[3, w - 1] = 20000 + 5 * 256
    flat = np.array([128, 128, 255], np.uint8)                       # the normal of a constant map: (0, 0, 1)
    for sob in (3, 0):
        got = _gpu_wrap(torch, d, (0, sob, 0))
        assert np.array_equal(got, wc.wrap_by_definition(oracle.create_normalmap_array, d, 0, sob, 0)), sob
        assert got[3, 0, 0] != 128, (sob, got[3, 0])                 # zx != 0 at column 0 of the sentinel's row
        ref = _gpu_plain(torch)(d, None, sob or None, None, False)
        assert np.array_equal(ref[3, 0], flat) and not np.array_equal(got[3, 0], ref[3, 0]), (sob, ref[3, 0])
        assert np.array_equal(got[0, :], np.broadcast_to(flat, (w, 3))), sob                     # two rows away: untouched
        assert np.array_equal(got[3, 1:w - 2], np.broadcast_to(flat, (w - 3, 3))), sob           # same row, away from the sentinel


def test_wrap_defaults_keep_todays_bytes_and_entry_points(gpu, oracle):
    torch = gpu
    import src.normalmap_generation as nm
    from src import _native
    old = ["ds_normalmap", "ds_normalmap_f64", "ds_normalmap_gradient_f32", "ds_normalmap_gradient_f16", "ds_normalmap_gradient_blur_f32"]
    cases = [(np.uint16, (0, 3, 0), "ds_normalmap"), (np.uint16, (5, 3, 5), "ds_normalmap"), (np.float64, (0, 3, 0), "ds_normalmap_f64"),
             (np.float32, (0, 0, 0), "ds_normalmap_gradient_f32"), (np.float32, (3, 0, 3), "ds_normalmap_gradient_blur_f32"),
             (np.float16, (0, 0, 0), "ds_normalmap_gradient_f16")]
    for dtype, opt, name in cases:
        d = wc.depth(24, 36, dtype, seed=9)
        x = _batch(torch, d)
        before = dict(_native.CALLS)
        a = nm.create_normalmap_batch(x, *opt, False)
        b = nm.create_normalmap_batch(x, *opt, False, wrap=False)
        c = _native.normalmap(x, opt[0], opt[1], opt[2], False)
        delta = {k: _native.CALLS[k] - before.get(k, 0) for k in old + [n + "_wrap" for n in old]}
        assert delta == dict({k: 0 for k in delta}, **{name: 3}), delta
        assert torch.equal(a, b) and torch.equal(a, c)
        if dtype != np.float16:
            assert np.array_equal(a[0].cpu().numpy(), wc.plain(oracle.create_normalmap_array, d, *opt)), (name, opt)
        before = dict(_native.CALLS)
        nm.create_normalmap_batch(x, *opt, False, wrap=True)
        delta = {k: _native.CALLS[k] - before.get(k, 0) for k in old + [n + "_wrap" for n in old]}
        assert delta == dict({k: 0 for k in delta}, **{name + "_wrap": 1}), delta
    # the PIL-level function: the reference's positional signature with the new keyword last
    d16 = wc.depth(24, 36, np.uint16, seed=10)
    assert np.array_equal(np.asarray(nm.create_normalmap(d16, 5, 3, None, True)), oracle.create_normalmap_array(d16, 5, 3, None, True))
    assert np.array_equal(np.asarray(nm.create_normalmap(d16, 5, 3, None, True, wrap=True)),
                          wc.wrap_by_definition(oracle.create_normalmap_array, d16, 5, 3, 0, invert=True))
    # dtype rules as without wrap: float32 with Sobel is promoted (the value of the float64 route), float16 cannot be blurred
    d32 = wc.depth(24, 36, np.float32, seed=11)
    assert np.array_equal(np.asarray(nm.create_normalmap(d32, None, 3, None, False, wrap=True)),
                          wc.wrap_by_definition(oracle.create_normalmap_array, d32, 0, 3, 0))
    with pytest.raises(_native.DepthStereoError):
        nm.create_normalmap(d32.astype(np.float16), 3, None, None, False, wrap=True)


def test_wrap_entry_points_check_their_arguments_like_their_twins(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    ctx = _native.ctx_for(torch.cuda.current_device())
    out = torch.empty((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    EINVAL, EUNSUPPORTED = -1, -2
    for sfx in ("", "_wrap"):
        for name, dt in (("ds_normalmap", torch.uint16), ("ds_normalmap_f64", torch.float64)):
            x = torch.zeros((1, 8, 8), dtype=dt, device="cuda")
            fn = getattr(L, name + sfx)

            def call(xp=x.data_ptr(), op=out.data_ptr(), n=1, h=8, w=8, pre=0, sob=3, post=0):
                return fn(ctx, xp, n, h, w, pre, sob, post, 0, op, None)
            assert call() == 0 and call(pre=5, sob=5, post=63) == 0 and call(sob=0) == 0, name + sfx
            assert call(xp=None) == EINVAL and call(op=None) == EINVAL, name + sfx
            assert fn(None, x.data_ptr(), 1, 8, 8, 0, 3, 0, 0, out.data_ptr(), None) == EINVAL, name + sfx
            assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-1) == EINVAL, name + sfx
            assert call(pre=4) == EINVAL and call(post=2) == EINVAL and call(sob=4) == EINVAL, name + sfx       # even sizes
            assert call(pre=65) == EUNSUPPORTED and call(post=65) == EUNSUPPORTED and call(sob=63) == EUNSUPPORTED, name + sfx
            assert call(n=65536) == EUNSUPPORTED, name + sfx
            assert call(sob=0, w=1) == EINVAL and call(sob=0, h=1) == EINVAL, name + sfx                        # np.gradient on 1 sample
            assert call(sob=3, w=1, h=1) == 0, name + sfx
        for name, dt in (("ds_normalmap_gradient_f32", torch.float32), ("ds_normalmap_gradient_f16", torch.float16)):
            x = torch.zeros((1, 8, 8), dtype=dt, device="cuda")
            fn = getattr(L, name + sfx)

            def call(xp=x.data_ptr(), op=out.data_ptr(), n=1, h=8, w=8):
                return fn(ctx, xp, n, h, w, 0, op, None)
            assert call() == 0, name + sfx
            assert call(xp=None) == EINVAL and call(op=None) == EINVAL and call(n=0) == EINVAL and call(n=65536) == EINVAL, name + sfx
            assert call(w=1) == EINVAL and call(h=1) == EINVAL, name + sfx
            assert fn(None, x.data_ptr(), 1, 8, 8, 0, out.data_ptr(), None) == EINVAL, name + sfx
        x = torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda")
        fn = getattr(L, "ds_normalmap_gradient_blur_f32" + sfx)

        def call(xp=x.data_ptr(), op=out.data_ptr(), n=1, h=8, w=8, pre=3, post=3):
            return fn(ctx, xp, n, h, w, pre, post, 0, op, None)
        assert call() == 0 and call(pre=0, post=0) == 0 and call(pre=63, post=0) == 0, sfx
        assert call(xp=None) == EINVAL and call(op=None) == EINVAL and call(n=0) == EINVAL, sfx
        assert call(w=1) == EINVAL and call(h=1) == EINVAL and call(pre=4) == EINVAL and call(post=6) == EINVAL, sfx
        assert call(pre=65) == EUNSUPPORTED and call(post=65) == EUNSUPPORTED, sfx
        assert fn(None, x.data_ptr(), 1, 8, 8, 3, 3, 0, out.data_ptr(), None) == EINVAL, sfx
    torch.cuda.synchronize()


def test_wrap_kernel_timer_brackets_the_fused_launch_like_its_twin(gpu):
    torch = gpu
    import src.normalmap_generation as nm
    from src import _native
    dev = torch.cuda.current_device()
    x = _batch(torch, wc.depth(16, 32, np.uint16, seed=3))
    for wrap in (False, True):
        _native.kernel_timer_enable(dev, True)
        try:
            nm.create_normalmap_batch(x, None, 3, None, False, wrap=wrap)
            nm.create_normalmap_batch(x, None, None, None, False, wrap=wrap)
            n, ms = _native.kernel_timer_read(dev, "normalmap")
        finally:
            _native.kernel_timer_enable(dev, False)
        assert n == 2 and ms > 0.0, (wrap, n, ms)


def test_funnel_normalmap_wrap_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'normalmap_wrap': V}) with caller-supplied I;16 depth maps (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.normalmap_generation as nm
    rng = np.random.default_rng(12)
    imgs = [Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)) for _ in range(2)]
    d16 = [wc.depth(48, 64, np.uint16, seed=40 + j) for j in range(2)]
    base = {'gen_normalmap': True, 'normalmap_pre_blur': True, 'normalmap_pre_blur_kernel': 5}
    depth_out = []

    def run(inp, ops):
        got = list(core.core_generation_funnel(None, list(imgs), [Image.fromarray(d) for d in d16], None, dict(inp), ops))
        assert [(i, k) for i, k, _ in got] == [(0, 'depth'), (0, 'normalmap'), (1, 'depth'), (1, 'normalmap')], [(i, k) for i, k, _ in got]
        depth_out[:] = [np.asarray(r) for _, k, r in got if k == 'depth']           # the funnel's own uint16 depth (renormalised)
        return [np.asarray(r) for _, k, r in got if k == 'normalmap']

    def want(wrap):
        return [np.asarray(nm.create_normalmap(d, 5, 3, None, False, wrap=wrap)) for d in depth_out]
    run(base, None)
    assert len(depth_out) == 2 and all(d.dtype == np.uint16 and d.shape == (48, 64) for d in depth_out)
    wrapped, reflected = want(True), want(False)
    assert not any(np.array_equal(a, b) for a, b in zip(wrapped, reflected))

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    assert same(run(base, None), reflected)
    assert same(run(base, {'normalmap_wrap': True}), wrapped)
    assert same(run(base, None), reflected)                                   # a call without ops after a call with it
    assert same(run(base, {}), reflected)
    assert same(run(base, {'normalmap_wrap': False}), reflected)
    assert same(run(dict(base, tiling_mode=True), {'normalmap_wrap': 'tiling'}), wrapped)
    assert same(run(dict(base, tiling_mode=False), {'normalmap_wrap': 'tiling'}), reflected)
    assert same(run(base, {'normalmap_wrap': 'tiling'}), reflected)           # TILING_MODE defaults to off
    assert same(run(dict(base, tiling_mode=True), None), reflected)           # tiling alone changes nothing
    assert not hasattr(core.model_holder, 'normalmap_wrap')                   # the option does not become a holder setting
