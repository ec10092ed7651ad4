"""The 3D-photo depth preparation on the GPU (include/depthstereo.h: ds_sparse_bilateral_f32; inpaint/bilateral_filtering.py): the
drop-in module against what the REFERENCE returned (tests/golden/sparse_bilateral_cases.npz), the kernel against the NumPy model of
tests/sparse_bilateral_cases.py pass by pass.  Every comparison is on bit patterns: a pass selects one of its window's depths, so there
is nothing to tolerate.  Shapes: the smallest legal one (3 x 3), smaller than a 64 x 8 tile, ragged in both tile directions (33 x 70: ten
tiles), 40 x 70; every window 1..15."""
import functools

import numpy as np
import pytest

import sparse_bilateral_cases as sc

pytestmark = pytest.mark.gpu

T = sc.THRESHOLD


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _mismatch(got, want):
    return np.argwhere(_bits(got) != _bits(want))[:6].tolist()


@functools.lru_cache(maxsize=None)
def _golden():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_bilateral_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _batch():
    """Three different 33 x 70 maps: steps plus noise, white noise, and steps with a block of zero depths (holes)."""
    holes = sc.steps_noise(33, 70, 21).copy()
    holes[10:14, 30:41] = 0.0
    holes[0, 5] = holes[32, 69] = holes[16, 0] = 0.0
    maps = np.stack([sc.steps_noise(33, 70, 20), sc.white_noise(33, 70, 22), holes])
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _model_pass(window, second):
    """The model's (out, jump) for every map of _batch(): the first pass (v0 is v), or -- second -- a pass on the result of a window-7
    pass with the original as v0."""
    outs, jumps = [], []
    for v0 in _batch():
        v = sc.filter_pass(v0, v0, 7, T)[0] if second else v0
        o, j = sc.filter_pass(v, v0, window, T)
        outs.append(o)
        jumps.append(j)
    outs, jumps = np.stack(outs), np.stack(jumps)
    outs.setflags(write=False)
    jumps.setflags(write=False)
    return outs, jumps


def _pass(torch, v, v0, window, t=T):
    from src import _native
    vt = torch.from_numpy(np.array(v)).cuda()                                # (a copy: the shared inputs are read-only)
    v0t = vt if v0 is None else torch.from_numpy(np.array(v0)).cuda()
    out, jump = _native.sparse_bilateral_pass_f32(vt, v0t, window, t)
    assert out.dtype == torch.float32 and jump.dtype == torch.uint8 and out.shape == vt.shape == jump.shape
    return out.cpu().numpy(), jump.cpu().numpy()


def test_drop_in_module_returns_the_reference_arrays(gpu):
    from inpaint.bilateral_filtering import sparse_bilateral_filtering
    from src import _native
    golden = _golden()
    for name, (depth, image, config, num_iter) in sc.cases().items():
        before = dict(_native.CALLS)
        images, depths = sparse_bilateral_filtering(depth.copy(), image.copy(), dict(config), num_iter=num_iter)
        delta = {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}
        want = {"ds_sparse_bilateral_jump_f32": 1}
        if num_iter > 1:
            want["ds_sparse_bilateral_f32"] = num_iter - 1                    # the last pass's filter is never launched
        assert delta == want, (name, delta)
        assert isinstance(images, list) and isinstance(depths, list) and len(images) == len(depths) == num_iter
        for i in range(num_iter):
            gd, gi = golden[f"{name}__depth{i}"], golden[f"{name}__image{i}"]
            assert isinstance(depths[i], np.ndarray) and depths[i].dtype == np.float32 and depths[i].shape == gd.shape
            assert np.array_equal(depths[i], gd) and np.array_equal(_bits(depths[i]), _bits(gd)), (name, i, _mismatch(depths[i], gd))
            assert images[i].dtype == np.uint8 and np.array_equal(images[i], gi), (name, i)
        assert depths[0] is not depth and not np.shares_memory(depths[0], depth)
    # one pass only: no filter launch at all, the image is still blackened
    depth, image, config, _ = sc.cases()["33x70_steps"]
    before = _native.CALLS["ds_sparse_bilateral_f32"]
    images, depths = sparse_bilateral_filtering(depth, image, config, num_iter=1)
    assert _native.CALLS["ds_sparse_bilateral_f32"] == before
    assert np.array_equal(images[0], golden["33x70_steps__image0"]) and np.array_equal(_bits(depths[0]), _bits(depth))
    # the arguments the reference ignores on this branch are ignored
    images2, depths2 = sparse_bilateral_filtering(depth, image, config, HR=True, gsHR=False, edge_id=3, num_iter=2, num_gs_iter=4, spdb=True)
    assert all(np.array_equal(_bits(a), _bits(golden[f"33x70_steps__depth{i}"])) for i, a in enumerate(depths2))
    assert all(np.array_equal(a, golden[f"33x70_steps__image{i}"]) for i, a in enumerate(images2))


@pytest.mark.parametrize("window", [1, 3, 5, 7, 9, 11, 13, 15])
def test_kernel_equals_the_model_pass_by_pass(gpu, window):
    """A batch of three different maps, every window; as a first pass (v0 is v) and as a later pass (v0 the original map)."""
    torch = gpu
    maps = _batch()
    want, want_j = _model_pass(window, False)
    got, got_j = _pass(torch, maps, None, window)
    assert np.array_equal(got_j, want_j.astype(np.uint8)), np.argwhere(got_j != want_j)[:6].tolist()
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)
    assert window == 1 or not np.array_equal(_bits(got), _bits(maps))
    first = _model_pass(7, False)[0]
    want, want_j = _model_pass(window, True)
    got, got_j = _pass(torch, first, maps, window)
    assert np.array_equal(got_j, want_j.astype(np.uint8))
    assert np.array_equal(_bits(got), _bits(want)), _mismatch(got, want)


def test_native_driver_lists_inputs_and_jump_maps(gpu):
    torch = gpu
    from src import _native
    for name in ("40x70_wide", "12x17_ties_zeros", "3x3", "10x13_scalar"):
        depth, image, config, num_iter = sc.cases()[name]
        windows = sc.windows_of(config, num_iter)
        _, want = sc.model(depth, image, windows, T)
        x = torch.from_numpy(depth.copy()).cuda()[None]
        before = dict(_native.CALLS)
        maps, jumps = _native.sparse_bilateral_f32(x, windows, T)
        assert _native.CALLS["ds_sparse_bilateral_f32"] == before.get("ds_sparse_bilateral_f32", 0) + num_iter - 1
        assert _native.CALLS["ds_sparse_bilateral_jump_f32"] == before.get("ds_sparse_bilateral_jump_f32", 0) + 1
        assert len(maps) == len(jumps) == num_iter and maps[0] is x
        for i in range(num_iter):
            assert maps[i].is_cuda and jumps[i].is_cuda and jumps[i].dtype == torch.uint8
            assert np.array_equal(_bits(maps[i][0].cpu().numpy()), _bits(want[i])), (name, i)
            assert np.array_equal(jumps[i][0].cpu().numpy(), sc.jump_map(want[i], T).astype(np.uint8)), (name, i)
    assert _native.cached_tables("sparse_bilateral") == 1                     # one rank table per device, whatever the windows


def test_jump_map_alone_and_ieee_specials(gpu):
    """The jump entry point on maps holding 0 (disparity inf), inf (disparity 0) and NaN: the model's IEEE rules, not the filter's
    precondition, apply to J."""
    torch = gpu
    from src import _native
    rng = np.random.default_rng(9)
    v = sc.steps_noise(37, 131, 30).copy()
    at = rng.integers(0, v.size, 60)
    v.ravel()[at[:30]] = 0.0
    v.ravel()[at[30:45]] = np.inf
    v.ravel()[at[45:]] = np.nan
    v[5, 5] = v[5, 6] = 0.0                                                  # inf - inf between them
    for t in (T, 0.0, 1e30):
        want = sc.jump_map(v, t).astype(np.uint8)
        got = _native.sparse_bilateral_jump_f32(torch.from_numpy(v).cuda()[None], t)[0].cpu().numpy()
        assert np.array_equal(got, want), (t, np.argwhere(got != want)[:6].tolist())
        assert np.array_equal(_pass(torch, v[None], None, 5, t)[1][0], want), t         # the filter's second output is the same map


def test_v0_as_the_same_buffer_and_as_another(gpu):
    torch = gpu
    maps = _batch()
    same = _pass(torch, maps, None, 7)
    other = _pass(torch, maps, maps.copy(), 7)
    assert np.array_equal(_bits(same[0]), _bits(other[0])) and np.array_equal(same[1], other[1])
    # V0 decides D, not V: holes of the original that an earlier pass has filled in still mask their taps
    v0 = maps[2]
    v = sc.filter_pass(v0, v0, 7, T)[0]
    assert (v[10:14, 30:41] != 0).any() and (v0[10:14, 30:41] == 0).all()
    with_v0 = _pass(torch, v[None], v0[None], 5)[0][0]
    without = _pass(torch, v[None], None, 5)[0][0]
    assert np.array_equal(_bits(with_v0), _bits(sc.filter_pass(v, v0, 5, T)[0]))
    assert np.array_equal(_bits(without), _bits(sc.filter_pass(v, v, 5, T)[0]))
    assert not np.array_equal(_bits(with_v0), _bits(without))


def test_batch_invariance_and_independence(gpu):
    """Image 2 of a batch of 3 equals that image run alone; changing image 0 changes only output 0."""
    torch = gpu
    maps = _batch()
    for window in (5, 15):
        y3, j3 = _pass(torch, maps, None, window)
        y1, j1 = _pass(torch, maps[2:3], None, window)
        assert np.array_equal(_bits(y3[2:3]), _bits(y1)) and np.array_equal(j3[2:3], j1), window
        changed = maps.copy()
        changed[0] = sc.white_noise(33, 70, 99)
        z3, k3 = _pass(torch, changed, None, window)
        assert np.array_equal(_bits(z3[1:]), _bits(y3[1:])) and np.array_equal(k3[1:], j3[1:]), window
        assert not np.array_equal(_bits(z3[0]), _bits(y3[0])) and not np.array_equal(k3[0], j3[0]), window


def test_refusals_launch_nothing(gpu):
    torch = gpu
    from inpaint.bilateral_filtering import sparse_bilateral_filtering
    from src import _native
    E = _native.DepthStereoError
    depth, image, config, num_iter = sc.cases()["9x11_noise"]
    x = torch.from_numpy(depth.copy()).cuda()[None]
    sparse_bilateral_filtering(depth, image, config, num_iter=num_iter)      # (whatever a first call does once is done)
    dev = torch.cuda.current_device()
    before = dict(_native.CALLS)
    _native.kernel_timer_enable(dev, True)
    try:
        with pytest.raises(NotImplementedError):
            sparse_bilateral_filtering(depth, image, config, num_iter=num_iter, mask=np.ones_like(depth))
        for bad in (dict(config, filter_size=[5, 3, 8]), dict(config, filter_size=17), dict(config, filter_size=[5, 3])):
            with pytest.raises(E):
                sparse_bilateral_filtering(depth, image, bad, num_iter=num_iter)
        hole = depth.copy()
        hole[2, 2] = -0.5
        for bad_depth in (hole, depth.astype(np.float64), depth[:2]):
            with pytest.raises(E):
                sparse_bilateral_filtering(bad_depth, image, config, num_iter=num_iter)
        with pytest.raises(E):
            sparse_bilateral_filtering(depth, image[:, :-1], config, num_iter=num_iter)
        for windows in ([5, 4], [], [17], [True], "5"):
            with pytest.raises(E):
                _native.sparse_bilateral_f32(x, windows, T)
        for bad_x in (x[0], x.double(), x.cpu(), x[:, :, ::2], x[:, :2], depth):
            with pytest.raises(E):
                _native.sparse_bilateral_f32(bad_x, [5, 3], T)
            with pytest.raises(E):
                _native.sparse_bilateral_jump_f32(bad_x, T)
            with pytest.raises(E):
                _native.sparse_bilateral_pass_f32(bad_x, bad_x, 5, T)
        with pytest.raises(E):
            _native.sparse_bilateral_pass_f32(x, x[:, :-1].contiguous(), 5, T)
        with pytest.raises(E):
            _native.sparse_bilateral_pass_f32(x, x, 6, T)
        torch.cuda.synchronize()
        assert dict(_native.CALLS) == before
        assert _native.kernel_timer_read(dev, "sparse_bilateral")[0] == 0
    finally:
        _native.kernel_timer_enable(dev, False)


def test_entry_points_check_their_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    dev = torch.cuda.current_device()
    ctx = _native.ctx_for(dev)
    EINVAL, EUNSUPPORTED = -1, -2
    n, h, w = 1, 8, 12
    SENT = 7.25
    count = n * h * w
    rank = torch.from_numpy(_native.sparse_bilateral_rank_table()).cuda()
    rank_off = torch.zeros(228, dtype=torch.int32, device="cuda")             # room for a table at a 2-byte offset
    x = torch.full((n, h, w), 2.0, dtype=torch.float32, device="cuda")
    x0 = torch.full((n, h, w), 2.0, dtype=torch.float32, device="cuda")
    out = torch.full((n, h, w), SENT, dtype=torch.float32, device="cuda")
    jump = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    big = torch.full((3 * count + 2,), SENT, dtype=torch.float32, device="cuda")       # one block to carve overlapping maps from
    nb = 4 * count                                                            # bytes of a map
    B = big.data_ptr()
    assert B % 4 == 0

    def call(c=ctx, vp=x.data_ptr(), v0p=x0.data_ptr(), n=n, h=h, w=w, s=5, t=0.04, rp=rank.data_ptr(), op=out.data_ptr(),
             jp=jump.data_ptr()):
        return L.ds_sparse_bilateral_f32(c, vp, v0p, n, h, w, s, t, rp, op, jp, None)

    def call_jump(c=ctx, vp=x.data_ptr(), n=n, h=h, w=w, t=0.04, jp=jump.data_ptr()):
        return L.ds_sparse_bilateral_jump_f32(c, vp, n, h, w, t, jp, None)
    _native.kernel_timer_enable(dev, True)
    try:
        for name in ("c", "vp", "v0p", "rp", "op", "jp"):
            assert call(**{name: None}) == EINVAL, name
        for name in ("c", "vp", "jp"):
            assert call_jump(**{name: None}) == EINVAL, name
        for shape in (dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(h=-4), dict(h=2), dict(w=2), dict(h=1, w=1)):
            assert call(**shape) == EINVAL and call_jump(**shape) == EINVAL, shape
        for s in (0, 2, 4, 14, 16, 17, 31, -1, -3):
            assert call(s=s) == EINVAL, s
        # out overlapping v or v0: equal pointers, out beginning in the last 4 bytes of the map, the map beginning in the last 4 of out
        for other in ("vp", "v0p"):
            assert call(op=B, **{other: B}) == EINVAL and call(op=B + nb - 4, **{other: B}) == EINVAL, other
            assert call(op=B, **{other: B + nb - 4}) == EINVAL, other
        # jump overlapping v, v0 or out (jump has count bytes)
        assert call(vp=B, jp=B + nb - 1) == EINVAL and call(v0p=B, jp=B) == EINVAL and call(op=B, jp=B + 8) == EINVAL
        assert call(vp=B + count, jp=B + 1) == EINVAL
        assert call_jump(vp=B, jp=B + nb - 1) == EINVAL and call_jump(vp=B + count, jp=B + 1) == EINVAL
        # alignment: the maps and rank 4 bytes; jump any
        assert call(vp=x.data_ptr() + 2) == EINVAL and call(v0p=x0.data_ptr() + 1) == EINVAL and call(op=out.data_ptr() + 2) == EINVAL
        assert call(rp=rank_off.data_ptr() + 2) == EINVAL and call_jump(vp=x.data_ptr() + 2) == EINVAL
        # the grid limit: n = 65536 smallest maps (every buffer really that large): DS_EUNSUPPORTED, one fewer runs (below)
        xn = torch.full((65536, 3, 3), 2.0, dtype=torch.float32, device="cuda")
        on = torch.full((65536, 3, 3), SENT, dtype=torch.float32, device="cuda")
        jn = torch.full((65536, 3, 3), 9, dtype=torch.uint8, device="cuda")
        many = dict(vp=xn.data_ptr(), v0p=xn.data_ptr(), op=on.data_ptr(), jp=jn.data_ptr(), h=3, w=3)
        many_jump = dict(vp=xn.data_ptr(), jp=jn.data_ptr(), h=3, w=3)
        assert call(n=65536, **many) == EUNSUPPORTED and call_jump(n=65536, **many_jump) == EUNSUPPORTED
        assert b"ds_sparse_bilateral_jump_f32" in L.ds_last_error()
        torch.cuda.synchronize()
        assert _native.kernel_timer_read(dev, "sparse_bilateral")[0] == 0     # every one returned before the launch
        assert bool((out == SENT).all()) and bool((big == SENT).all()) and bool((on == SENT).all())
        assert bool((jump == 9).all()) and bool((jn == 9).all())
        # and the legal neighbours of those cases run: v0 the same buffer as v, the extreme windows, adjacent but disjoint blocks, a
        # jump map at an odd address right behind out, n = 65535
        assert call(v0p=x.data_ptr()) == 0 and call(s=1) == 0 and call(s=15) == 0 and call(h=3, w=3) == 0
        assert call(vp=B, v0p=B, op=B + nb, jp=B + 2 * nb + 1) == 0
        assert call(vp=B + nb, v0p=B + 2 * nb, op=B) == 0
        assert call(n=65535, **many) == 0
        torch.cuda.synchronize()
        assert bool((on[:65535] == 2.0).all()) and bool((on[65535] == SENT).all())
        assert bool((jn[:65535] == 0).all()) and bool((jn[65535] == 9).all())
        assert call_jump() == 0 and call_jump(n=65535, **many_jump) == 0
        torch.cuda.synchronize()
        launches, ms = _native.kernel_timer_read(dev, "sparse_bilateral")
        assert launches == 9 and ms > 0.0, (launches, ms)                    # the timer brackets each launch, of both entry points
        assert _native.kernel_timer_read(dev, "depth_refine")[0] == 0         # and it is a kind of its own
        assert bool((out == 2.0).all()) and bool((jump == 0).all())           # a flat map stays flat and has no jump: written
    finally:
        _native.kernel_timer_enable(dev, False)
