"""Eight paths and the speckle filter inside the matcher (include/depthstereo.h: ds_stereo_match_ex_u8; src/stereo_matching.py;
ops={'stereo_paths': ..., 'stereo_speckle': ...}) against the NumPy model, tests/stereo_match_ex_cases.py.  Every comparison is exact on
all three outputs -- disparity, valid, depth.  Shapes: those of tests/test_gpu_stereo_match.py -- (1,1,1), (3,1,67) and (1,5,1), where
every diagonal has length 1; (1,7,20), w < D; (2,9,130) and (1,33,257), h < w --, (1,67,5), h > w, and 96 x 300.
tests/test_stereo_match_ex_cpu.py shows from the model that the eight-path cases differ from their four-path planes and that every
filtered case has a component removed and one kept."""
import numpy as np
import pytest

import stereo_match_cases as sc
import stereo_match_ex_cases as ex

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
NAMES = ("disparity", "valid", "depth")


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _host(t):
    return t.cpu().numpy()


def _same(got, want, what):
    for name, g, wv in zip(NAMES, got, want):
        g = _host(g)
        assert g.dtype == wv.dtype and g.shape == wv.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, wv), (what, name, int((g != wv).sum()), np.argwhere(g != wv)[:6].tolist())


def _run(torch, name, shape, c, params, e, **kwargs):
    from src import _native
    l, r = sc.pair(name, shape, c)
    before = dict(_native.CALLS)
    got = _native.stereo_match_ex_u8(_dev(torch, l), _dev(torch, r), *params, *e, want_valid=True, **kwargs)
    assert _native.CALLS["ds_stereo_match_ex_u8"] == before.get("ds_stereo_match_ex_u8", 0) + 1
    assert _native.CALLS["ds_stereo_match_u8"] == before.get("ds_stereo_match_u8", 0)
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.uint8 and got[2].dtype == torch.uint16
    assert all(t.is_cuda and tuple(t.shape) == tuple(shape) for t in got)
    return got


@pytest.mark.parametrize("shape", ex.EX_SHAPES, ids=["%dx%dx%d" % s for s in ex.EX_SHAPES])
def test_kernels_equal_the_model_exactly(gpu, shape):
    for row, e in ex.EX_PARAMS:
        params, c = row[:6], row[6]
        for name in sc.INPUTS:
            _same(_run(gpu, name, shape, c, params, e), ex.want(name, shape, c, params, e), (name, shape, row, e))


@pytest.mark.parametrize("case", range(len(ex.SPECKLE_CASES)), ids=["%s-%dx%dx%d-%dpaths" % ((c[0],) + c[1] + (c[3],)) for c in ex.SPECKLE_CASES])
def test_speckle_sizes_on_both_sides_of_the_components_present(gpu, case):
    name, shape, params, paths, rng, sizes = ex.SPECKLE_CASES[case]
    _same(_run(gpu, name, shape, 3, params, (paths, 0, rng)), ex.want(name, shape, 3, params, (paths, 0, rng)), (name, paths, "off"))
    for size in sizes:
        _same(_run(gpu, name, shape, 3, params, (paths, size, rng)), ex.want(name, shape, 3, params, (paths, size, rng)), (name, paths, size))


def test_kernels_equal_the_model_on_a_larger_shape(gpu):
    name, shape, params = ex.LARGE_EX
    for inp in sc.INPUTS:
        for e in ((8, 0, 0), ex.PRESET):
            _same(_run(gpu, inp, shape, 3, params, e), ex.want(inp, shape, 3, params, e), (inp, shape, e))


@pytest.mark.parametrize("D", [32, 64, 128])
def test_four_paths_without_filter_are_ds_stereo_match_u8_bit_for_bit(gpu, D):
    from src import _native
    params = (D, -7, 4, 48, 5, 1)
    for name, shape in (("planes", (2, 9, 130)), ("stripes", (1, 33, 257)), ("noise", (3, 5, 67))):
        l, r = (_dev(gpu, v) for v in sc.pair(name, shape))
        old = _native.stereo_match_u8(l, r, *params, want_valid=True)
        for e in ((4, 0, 0), (4, 0, 16)):
            new = _run(gpu, name, shape, 3, params, e)
            assert all(np.array_equal(_host(a), _host(b)) for a, b in zip(old, new)), (name, shape, e)
        _same(old, sc.want(name, shape, 3, params), (name, shape))
    assert _native.stereo_match_ex_workspace_bytes(33, 257, D, 4, 0) == _native.stereo_match_workspace_bytes(33, 257, D)
    assert _native.stereo_match_ex_workspace_bytes(33, 257, D, 8, 0) == _native.stereo_match_workspace_bytes(33, 257, D)


def test_the_result_does_not_depend_on_the_group(gpu):
    shape, params, e = (3, 9, 130), (64, -7, 4, 48, 5, 1), (8, 3, 1)
    l, r = (np.array(v) for v in sc.pair("planes", shape))
    l[1], r[1] = (v[1] for v in sc.pair("stripes", shape))
    from src import _native
    lt, rt = _dev(gpu, l), _dev(gpu, r)
    want = ex.model_ex(l, r, *params, *e)
    assert not np.array_equal(want[1], ex.model_ex(l, r, *params, 8, 0, 0)[1])
    outs = {g: _native.stereo_match_ex_u8(lt, rt, *params, *e, want_valid=True, group=g) for g in (1, 2, 3, None)}
    for g, got in outs.items():
        _same(got, want, ("group", g))
    alone = _native.stereo_match_ex_u8(lt[2:3], rt[2:3], *params, *e, want_valid=True)
    assert all(np.array_equal(_host(a), _host(b)[2:3]) for a, b in zip(alone, outs[3]))
    for bad in (0, 4, -1, True, 1.5, "1"):
        with pytest.raises(_native.DepthStereoError):
            _native.stereo_match_ex_u8(lt, rt, *params, *e, group=bad)


class _Buffers:
    """left, right, the workspace and the three outputs carved from guarded blocks, for calls of the raw entry point."""
    GUARD, SENT = 512, 0xA5

    def __init__(self, torch, shape, c, D, e, group, name="planes"):
        from src import _native
        self.torch, self.shape, self.c, self.D, self.e, self.group = torch, shape, c, D, e, group
        n, h, w = shape
        self.count = n * h * w
        self.l, self.r = sc.pair(name, shape, c)
        self.per_image = _native.stereo_match_ex_workspace_bytes(h, w, D, e[0], e[1])
        base = _native.stereo_match_workspace_bytes(h, w, D)
        assert self.per_image % 256 == 0 and self.per_image >= base + (12 * h * w if e[1] else 0)
        G = self.GUARD
        self.size = {"left": self.count * c, "right": self.count * c, "ws": self.per_image * group, "disparity": 2 * self.count,
                     "valid": self.count, "depth": 2 * self.count}
        self.blocks = {k: torch.full((size + 2 * G,), self.SENT, dtype=torch.uint8, device="cuda") for k, size in self.size.items()}
        for k, a in (("left", self.l), ("right", self.r)):
            self.view(k).copy_(_dev(torch, a).view(-1))
        assert self.ptr("ws") % 256 == 0 and self.ptr("disparity") % 2 == 0 and self.ptr("depth") % 2 == 0

    def view(self, k):
        return self.blocks[k][self.GUARD:self.GUARD + self.size[k]]

    def ptr(self, k):
        return self.blocks[k].data_ptr() + self.GUARD

    def call(self, params, want_valid=True, want_depth=True, stages=None, **over):
        from src import _native
        n, h, w = self.shape
        a = dict(ctx=_native.ctx_for(self.torch.cuda.current_device()), left=self.ptr("left"), right=self.ptr("right"), n=n, h=h, w=w, c=self.c,
                 D=params[0], d0=params[1], P1=params[2], P2=params[3], u=params[4], lr=params[5], paths=self.e[0], speckle_size=self.e[1],
                 speckle_range=self.e[2], ws=self.ptr("ws"), group=self.group, disparity=self.ptr("disparity"),
                 valid=self.ptr("valid") if want_valid else None, depth=self.ptr("depth") if want_depth else None)
        a.update(over)
        args = (a["ctx"], a["left"], a["right"], a["n"], a["h"], a["w"], a["c"], a["D"], a["d0"], a["P1"], a["P2"], a["u"], a["lr"], a["paths"],
                a["speckle_size"], a["speckle_range"], a["ws"], a["group"], a["disparity"], a["valid"], a["depth"])
        if stages is not None:
            return _native.lib().ds_stereo_match_ex_stages_u8(*args, stages, None)
        return _native.lib().ds_stereo_match_ex_u8(*args, None)

    def outputs(self):
        self.torch.cuda.synchronize()
        n, h, w = self.shape
        return (self.view("disparity").view(self.torch.int16).view(n, h, w), self.view("valid").clone().view(n, h, w),
                self.view("depth").view(self.torch.uint16).view(n, h, w))

    def guards_untouched(self, also=()):
        self.torch.cuda.synchronize()
        G = self.GUARD
        for k, b in self.blocks.items():
            if not (bool((b[:G] == self.SENT).all()) and bool((b[G + self.size[k]:] == self.SENT).all())):
                return False
            if k in also and not bool((b[G:G + self.size[k]] == self.SENT).all()):
                return False
        return True


@pytest.mark.parametrize("D,shape,group", [(32, (3, 5, 67), 2), (64, (2, 9, 130), 2), (128, (3, 5, 67), 3)])
def test_workspace_content_does_not_matter_and_nothing_else_is_written(gpu, D, shape, group):
    torch = gpu
    params, e = (D, -7, 4, 48, 5, 1), (8, 2, 1)
    want = ex.want("stripes", shape, 3, params, e)
    assert not np.array_equal(want[1], ex.want("stripes", shape, 3, params, (8, 0, 0))[1])                # the filter has work to do
    b = _Buffers(torch, shape, 3, D, e, group, name="stripes")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    for fill in (0xFF, "random", 0x00):
        if fill == "random":                                                  # random bytes: links and counters anywhere in 32 bits
            b.view("ws").copy_(torch.randint(0, 256, (b.size["ws"],), dtype=torch.uint8, device="cuda", generator=gen))
        else:
            b.view("ws").fill_(fill)
        for k in NAMES:
            b.view(k).fill_(0x3C)
        assert b.call(params) == 0
        _same(b.outputs(), want, ("workspace", fill))
        assert b.guards_untouched()                                           # behind workspace_bytes * group and around every output


def test_optional_outputs_leave_the_others_unchanged(gpu):
    shape, params, e = (2, 9, 130), (64, 0, 4, 48, 5, 1), (8, 2, 1)
    want = ex.want("stripes", shape, 3, params, e)
    b = _Buffers(gpu, shape, 3, 64, e, 1, name="stripes")
    for valid, depth in ((False, True), (True, False), (False, False)):
        for k in NAMES:
            b.view(k).fill_(b.SENT)
        assert b.call(params, want_valid=valid, want_depth=depth) == 0
        got = b.outputs()
        assert np.array_equal(_host(got[0]), want[0])
        assert np.array_equal(_host(got[1]), want[1]) if valid else bool((b.view("valid") == b.SENT).all())
        assert np.array_equal(_host(got[2]), want[2]) if depth else bool((b.view("depth") == b.SENT).all())
        assert b.guards_untouched()
    from src import _native
    l, r = (_dev(gpu, v) for v in sc.pair("stripes", shape))
    d, v, z = _native.stereo_match_ex_u8(l, r, *params, *e, want_valid=False, want_depth=False)
    assert v is None and z is None and np.array_equal(_host(d), want[0])


def test_stages_add_up_to_the_call(gpu):
    """ds_stereo_match_ex_stages_u8, the timing tool's entry point: the launches one after the other give the call's result."""
    shape, params, e = (2, 9, 130), (64, 0, 4, 48, 5, 1), (8, 2, 1)
    want = ex.want("stripes", shape, 3, params, e)
    b = _Buffers(gpu, shape, 3, 64, e, 2, name="stripes")
    for bit in (1, 2, 4, 64, 8, 128, 16, 32):
        assert b.call(params, stages=bit) == 0
    _same(b.outputs(), want, "stages")
    for bad in (0, 256, -1):
        assert b.call(params, stages=bad) == EINVAL
    assert b.guards_untouched()


def test_entry_point_refuses_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    shape, params, e = (2, 4, 24), (32, 0, 4, 48, 5, 1), (8, 3, 1)
    n, h, w = shape
    b = _Buffers(torch, shape, 3, 32, e, 2)
    count, ws_bytes = b.count, b.per_image * 2
    big = torch.full((4 * ws_bytes,), b.SENT, dtype=torch.uint8, device="cuda")    # one block to carve overlapping buffers from
    B = big.data_ptr()
    assert B % 256 == 0

    def refused(code, **over):
        rc = b.call(params, **over)
        assert rc == code, (over, rc)
        assert b"ds_stereo_match_ex_u8" in L.ds_last_error(), over
        return True

    cases = []
    cases += [(EINVAL, dict(ctx=None)), (EINVAL, dict(left=None)), (EINVAL, dict(right=None)), (EINVAL, dict(ws=None)), (EINVAL, dict(disparity=None))]
    cases += [(EINVAL, dict(n=0)), (EINVAL, dict(h=0)), (EINVAL, dict(w=0)), (EINVAL, dict(n=-1)), (EINVAL, dict(w=-3))]
    cases += [(EINVAL, dict(c=2)), (EINVAL, dict(D=48)), (EINVAL, dict(d0=128)), (EINVAL, dict(P1=0)), (EINVAL, dict(P2=256)), (EINVAL, dict(u=51)),
              (EINVAL, dict(lr=4))]
    # the new parameters
    cases += [(EINVAL, dict(paths=0)), (EINVAL, dict(paths=2)), (EINVAL, dict(paths=5)), (EINVAL, dict(paths=16)), (EINVAL, dict(paths=-8)),
              (EINVAL, dict(speckle_size=-1)), (EINVAL, dict(speckle_size=65536)), (EINVAL, dict(speckle_range=-1)), (EINVAL, dict(speckle_range=17)),
              (EINVAL, dict(speckle_size=0, speckle_range=17))]
    cases += [(EINVAL, dict(group=0)), (EINVAL, dict(group=3)), (EINVAL, dict(ws=b.ptr("ws") + 128)), (EINVAL, dict(disparity=b.ptr("disparity") + 1)),
              (EINVAL, dict(depth=b.ptr("depth") + 1))]
    # the order of the checks: a bad parameter beside a size above the limit is EINVAL, the size alone EUNSUPPORTED
    cases += [(EINVAL, dict(w=16385, paths=6)), (EUNSUPPORTED, dict(w=16385)), (EUNSUPPORTED, dict(h=16385)), (EUNSUPPORTED, dict(n=65536, group=1)),
              (EUNSUPPORTED, dict(h=16384, w=16384)),
              (EUNSUPPORTED, dict(h=16384, w=1600)),                          # 1.8 GiB without the filter's planes, 2.1 GiB with them
              (EUNSUPPORTED, dict(w=16385, left=B, disparity=B))]             # the overlap test comes last
    cases += [(EINVAL, dict(left=B, disparity=B)), (EINVAL, dict(left=B, valid=B)), (EINVAL, dict(right=B, depth=B)), (EINVAL, dict(left=B + ws_bytes - 1, ws=B)),
              (EINVAL, dict(disparity=B, depth=B)), (EINVAL, dict(disparity=B, valid=B + 2 * count - 1)), (EINVAL, dict(ws=B, disparity=B + ws_bytes - 2)),
              (EINVAL, dict(ws=B, valid=B)), (EINVAL, dict(ws=B, depth=B + 256))]
    torch.cuda.synchronize()
    for code, over in cases:
        assert refused(code, **over)
    assert b.guards_untouched(also=("ws",) + NAMES) and bool((big == b.SENT).all())   # poisoned stays poisoned: no refusal launched anything
    # (h, w) = (16384, 1600) at D = 32: inside 2 GiB without the filter, above it with
    assert 0 < _native.stereo_match_ex_workspace_bytes(16384, 1600, 32, 8, 0) <= 1 << 31 < _native.stereo_match_ex_workspace_bytes(16384, 1600, 32, 8, 1)
    # the workspace size of what is refused is 0
    W = _native.stereo_match_ex_workspace_bytes
    assert W(0, 5, 32, 8, 0) == 0 and W(5, 16385, 32, 8, 0) == 0 and W(5, 5, 48, 8, 0) == 0 and W(5, 5, 32, 6, 0) == 0 and W(5, 5, 32, 8, -1) == 0
    assert W(5, 5, 32, 8, 65536) == 0 and W(5, 5, 32, 8, 65535) > W(5, 5, 32, 8, 0) > 0
    # and the legal neighbours run: the ends of every new range, adjacent but disjoint blocks
    for over in (dict(paths=4), dict(speckle_size=1), dict(speckle_size=65535), dict(speckle_range=0), dict(speckle_range=16), dict(group=1),
                 dict(valid=None, depth=None)):
        assert b.call(params, **over) == 0, over
    d_at = B + ws_bytes
    assert b.call(params, ws=B, disparity=d_at, depth=d_at + 2 * count, valid=d_at + 4 * count) == 0
    torch.cuda.synchronize()
    got = (big[ws_bytes:ws_bytes + 2 * count].view(torch.int16).view(n, h, w), big[ws_bytes + 4 * count:ws_bytes + 5 * count].clone().view(n, h, w),
           big[ws_bytes + 2 * count:ws_bytes + 4 * count].view(torch.uint16).view(n, h, w))
    _same(got, ex.want("planes", shape, 3, params, e), "adjacent blocks")
    assert bool((big[ws_bytes + 5 * count:] == b.SENT).all())
    assert b.guards_untouched()


def test_public_interface(gpu):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.stereo_matching as sm
    name, shape, params = ex.PLANES_EX
    l, r = sc.pair(name, shape)
    kwargs = dict(max_disparity=32, min_disparity=-4)
    for extra, e in ((dict(paths=8), (8, 0, 0)), (dict(paths=8, speckle=(2, 1)), (8, 2, 1)), (dict(speckle=(764, 1)), (4, 764, 1)),
                     (dict(paths=8, speckle=ex.PRESET[1:]), ex.PRESET)):
        want = ex.want(name, shape, 3, params, e)
        before = dict(_native.CALLS)
        for left, right in ((l[0], r[0]), (Image.fromarray(l[0]), Image.fromarray(r[0]))):
            depth, disparity, mask = sm.depth_from_stereo(left, right, return_disparity=True, **kwargs, **extra)
            assert isinstance(depth, Image.Image) and depth.mode == 'I;16' and np.array_equal(np.asarray(depth), want[2][0])
            assert disparity.dtype == np.float32 and np.array_equal(disparity * 16, want[0][0].astype(np.float32))
            assert mask.dtype == bool and np.array_equal(mask, want[1][0] == 1)
        batch = sm.depth_from_stereo_batch(_dev(torch, l), _dev(torch, r), **kwargs, **extra)
        assert batch.is_cuda and batch.dtype == torch.uint16 and np.array_equal(_host(batch), want[2])
        assert _native.CALLS["ds_stereo_match_ex_u8"] == before.get("ds_stereo_match_ex_u8", 0) + 3
        assert _native.CALLS["ds_stereo_match_u8"] == before.get("ds_stereo_match_u8", 0)
    # the defaults, spelled out or not, stay with ds_stereo_match_u8
    before = dict(_native.CALLS)
    for extra in ({}, dict(paths=4), dict(speckle=None), dict(paths=4, speckle=(0, 1))):
        assert np.array_equal(np.asarray(sm.depth_from_stereo(l[0], r[0], **kwargs, **extra)), sc.want(name, shape, 3, params)[2][0])
    assert _native.CALLS["ds_stereo_match_u8"] == before.get("ds_stereo_match_u8", 0) + 4
    assert _native.CALLS["ds_stereo_match_ex_u8"] == before.get("ds_stereo_match_ex_u8", 0)
    # filter_speckles on the matcher's own disparity reproduces the mask of the filtered call
    _, disparity, mask = sm.depth_from_stereo(l[0], r[0], return_disparity=True, paths=8, **kwargs)
    d16 = np.rint(disparity * 16).astype(np.int16)
    sizes_want = ex.speckle_sizes(d16, mask, 16)
    kept, sizes = sm.filter_speckles(d16, mask, 4, 16, return_sizes=True)
    assert kept.dtype == bool and np.array_equal(kept, sizes_want > 4) and sizes.dtype == np.int32 and np.array_equal(sizes, sizes_want)
    assert np.array_equal(sm.filter_speckles(d16, mask.astype(np.uint8), 718, 16), sizes_want > 718)
    before = dict(_native.CALLS)
    lt, rt = _dev(torch, l), _dev(torch, r)
    for bad in ({'paths': 6}, {'paths': True}, {'paths': '8'}, {'speckle': 64}, {'speckle': (64,)}, {'speckle': (64, 17)}, {'speckle': (65536, 1)},
                {'speckle': (64, float('nan'))}, {'speckle': (True, 1)}, {'paths': 8, 'speckle': (-1, 1)}):
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo(l[0], r[0], **bad)
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo_batch(lt, rt, **bad)
    for bad in ((d16, mask, 0, 16), (d16, mask, 65536, 16), (d16, mask, 4, -1), (d16, mask, 4, 65536), (d16, mask, True, 16), (d16, mask, 4, 1.5),
                (d16.astype(np.int32), mask, 4, 16), (d16, mask[:, :-1], 4, 16), (d16[0], mask[0], 4, 16), (d16, mask.astype(np.int16), 4, 16)):
        with pytest.raises(_native.DepthStereoError):
            sm.filter_speckles(*bad)
    assert dict(_native.CALLS) == before


def test_funnel_options_need_stereo_input_and_add_nothing_when_absent(gpu):
    """ops={'stereo_input': ..., 'stereo_paths': 8, 'stereo_speckle': (size, range)}: the call with the maps of
    depth_from_stereo(paths=8, speckle=...); without 'stereo_input', or malformed, a ValueError before any device work; absent, the
    launches of the call without them."""
    from PIL import Image
    import src.core as core
    import src.stereo_matching as sm
    from src import _native
    shape = (2, 64, 96)
    l, r = sc.pair("planes", shape)
    sbs = [Image.fromarray(np.concatenate([l[k], r[k]], axis=1)) for k in range(2)]
    lefts = [Image.fromarray(l[k]) for k in range(2)]
    S = ('left-right', 32)
    base = {'gen_stereo': True, 'gen_normalmap': True, 'stereo_modes': ['left-right']}
    kinds = ['depth', 'left-right', 'normalmap']

    def run(images, depthmaps, ops):
        got = list(core.core_generation_funnel(None, list(images), depthmaps, None, dict(base), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(len(images)) for k in kinds]
        return {k: [np.asarray(res) for _, kk, res in got if kk == k] for k in kinds}

    def same(a, b):
        return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)

    def delta(before):
        return {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}

    e = (8, 3, 1)
    maps = [sm.depth_from_stereo(l[k], r[k], 32, paths=8, speckle=(3, 1)) for k in range(2)]
    want = ex.want("planes", shape, 3, (32, 0, 4, 48, 5, 1), e)
    assert all(np.array_equal(np.asarray(m), want[2][k]) for k, m in enumerate(maps))
    assert not np.array_equal(want[2], sc.want("planes", shape, 3, (32, 0, 4, 48, 5, 1))[2])
    run(lefts, list(maps), None)                                              # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(lefts, list(maps), None)
    plain_delta = delta(before)
    assert "ds_stereo_match_u8" not in plain_delta and "ds_stereo_match_ex_u8" not in plain_delta
    # the options: the plain call's launches plus one extended match per pair, and no ds_stereo_match_u8
    before = dict(_native.CALLS)
    assert same(run(sbs, None, {'stereo_input': S, 'stereo_paths': 8, 'stereo_speckle': (3, 1)}), plain)
    assert delta(before) == dict(plain_delta, ds_stereo_match_ex_u8=2)
    # absent or None beside stereo_input: the launches the call made before, ds_stereo_match_u8's
    before = dict(_native.CALLS)
    old = run(sbs, None, {'stereo_input': S})
    old_delta = delta(before)
    assert old_delta == dict(plain_delta, ds_stereo_match_u8=2) and not same(old, plain)
    for ops in ({'stereo_input': S, 'stereo_paths': None, 'stereo_speckle': None}, {'stereo_input': S, 'stereo_paths': 4}):
        before = dict(_native.CALLS)
        assert same(run(sbs, None, ops), old), ops
        assert delta(before) == old_delta, ops
    # absent, and None, without stereo_input: the plain call
    before = dict(_native.CALLS)
    assert same(run(lefts, list(maps), {'stereo_paths': None, 'stereo_speckle': None}), plain)
    assert delta(before) == plain_delta
    assert not hasattr(core.model_holder, 'stereo_paths') and not hasattr(core.model_holder, 'stereo_speckle')
    # without stereo_input, or malformed: a ValueError before any device work
    for images, depthmaps, bad in ((lefts, list(maps), {'stereo_paths': 8}), (lefts, list(maps), {'stereo_speckle': (64, 1)}),
                                   (lefts, list(maps), {'stereo_paths': 4}), (lefts, list(maps), {'stereo_input': None, 'stereo_paths': 8}),
                                   (sbs, None, {'stereo_input': S, 'stereo_paths': 6}), (sbs, None, {'stereo_input': S, 'stereo_paths': True}),
                                   (sbs, None, {'stereo_input': S, 'stereo_paths': '8'}), (sbs, None, {'stereo_input': S, 'stereo_speckle': 64}),
                                   (sbs, None, {'stereo_input': S, 'stereo_speckle': (64,)}), (sbs, None, {'stereo_input': S, 'stereo_speckle': (64, 17)}),
                                   (sbs, None, {'stereo_input': S, 'stereo_speckle': (65536, 1)}),
                                   (sbs, None, {'stereo_input': S, 'stereo_speckle': (64, float('nan'))}),
                                   (sbs, None, {'stereo_input': S, 'stereo_paths': 8, 'stereo_speckle': 'on'})):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(images, depthmaps, bad)
        assert dict(_native.CALLS) == before, bad
    assert same(run(lefts, list(maps), None), plain)
