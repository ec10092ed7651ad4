"""Depth from stereo pairs (include/depthstereo.h: ds_stereo_match_u8; src/stereo_matching.py; ops={'stereo_input': ...}) against the
NumPy model, tests/stereo_match_cases.py.  Every comparison is exact on all three outputs -- disparity, valid, depth: the definition is
all-integer and every step is a min, a sum or a compare, so there is nothing to tolerate and nothing that depends on the schedule.
Shapes: one pixel; 7 x 20, where w < D and most disparities leave the row; heights 1 and 5 at width 67 in a batch of 3; 9 x 130 and
33 x 257, below, across and above the 4 (at D = 32: 8) rows or columns a workgroup of the path kernels owns and the 256 columns a
pass of the winner kernel covers; 5 x 1, where only the vertical paths move; 96 x 300 at D = 64 and 2 x 40 x 700 at D = 128, d0 = -16.
tests/test_stereo_match_cpu.py shows from the model that the cases contain pixels failing each check, filled pixels, pixels the
median changes and sub-pixel parts."""
import numpy as np
import pytest

import stereo_match_cases as sc

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


def _run(torch, name, shape, c, params, **kwargs):
    from src import _native
    l, r = sc.pair(name, shape, c)
    before = _native.CALLS["ds_stereo_match_u8"]
    got = _native.stereo_match_u8(_dev(torch, l), _dev(torch, r), *params, want_valid=True, **kwargs)
    assert _native.CALLS["ds_stereo_match_u8"] == before + 1
    assert got[0].dtype == torch.int16 and got[1].dtype == torch.uint8 and got[2].dtype == torch.uint16
    assert all(t.is_cuda and tuple(t.shape) == tuple(shape) for t in got)
    return got


@pytest.mark.parametrize("shape", sc.SMALL_SHAPES, ids=["%dx%dx%d" % s for s in sc.SMALL_SHAPES])
def test_kernels_equal_the_model_exactly(gpu, shape):
    for row in sc.SMALL_PARAMS:
        params, c = row[:6], row[6]
        for name in sc.INPUTS:
            _same(_run(gpu, name, shape, c, params), sc.want(name, shape, c, params), (name, shape, row))


@pytest.mark.parametrize("case", range(len(sc.LARGE_CASES)), ids=["%dx%dx%d" % c[0] for c in sc.LARGE_CASES])
def test_kernels_equal_the_model_on_the_larger_shapes(gpu, case):
    shape, params, c = sc.LARGE_CASES[case]
    for name in sc.INPUTS:
        _same(_run(gpu, name, shape, c, params), sc.want(name, shape, c, params), (name, shape, params))


def test_the_result_does_not_depend_on_the_group(gpu):
    shape, params = (3, 9, 130), (64, -7, 4, 48, 5, 1)
    l, r = (np.array(v) for v in sc.pair("planes", shape))
    l[1], r[1] = (v[1] for v in sc.pair("noise", shape))
    from src import _native
    lt, rt = _dev(gpu, l), _dev(gpu, r)
    want = sc.model(l, r, *params)
    outs = {g: _native.stereo_match_u8(lt, rt, *params, want_valid=True, group=g) for g in (1, 2, 3, None)}
    for g, got in outs.items():
        _same(got, want, ("group", g))
    alone = _native.stereo_match_u8(lt[2:3], rt[2:3], *params, want_valid=True)
    assert all(np.array_equal(_host(a), _host(b)[2:3]) for a, b in zip(alone, outs[3]))
    for bad in (0, 4, -1, True, 1.5, "1"):
        with pytest.raises(_native.DepthStereoError):
            _native.stereo_match_u8(lt, rt, *params, group=bad)


class _Buffers:
    """left, right, the workspace and the three outputs carved from guarded blocks, for calls of the raw entry point."""
    GUARD, SENT = 512, 0xA5

    def __init__(self, torch, shape, c, D, group, name="planes", odd=False):
        from src import _native
        self.torch, self.shape, self.c, self.D, self.group = torch, shape, c, D, group
        n, h, w = shape
        self.count = n * h * w
        self.l, self.r = sc.pair(name, shape, c)
        shift = 1 if odd else 0                                               # odd: left, right and valid at odd byte addresses
        self.per_image = _native.stereo_match_workspace_bytes(h, w, D)
        assert self.per_image % 256 == 0 and self.per_image >= 2 * h * w * D + 8 * h * w + 2 * h * w + 8
        G = self.GUARD
        self.blocks = {k: torch.full((size + 2 * G,), self.SENT, dtype=torch.uint8, device="cuda")
                       for k, size in (("left", self.count * c + 2), ("right", self.count * c + 2), ("ws", self.per_image * group),
                                       ("disparity", 2 * self.count), ("valid", self.count + 2), ("depth", 2 * self.count))}
        self.at = {k: G + (shift if k in ("left", "right", "valid") else 0) for k in self.blocks}
        self.size = {"left": self.count * c, "right": self.count * c, "ws": self.per_image * group, "disparity": 2 * self.count,
                     "valid": self.count, "depth": 2 * self.count}
        for k, a in (("left", self.l), ("right", self.r)):
            self.view(k).copy_(_dev(torch, a).view(-1))
        assert self.ptr("ws") % 256 == 0 and self.ptr("disparity") % 2 == 0 and self.ptr("depth") % 2 == 0
        if odd:
            assert self.ptr("left") % 2 == 1 and self.ptr("right") % 2 == 1 and self.ptr("valid") % 2 == 1

    def view(self, k):
        return self.blocks[k][self.at[k]:self.at[k] + self.size[k]]

    def ptr(self, k):
        return self.blocks[k].data_ptr() + self.at[k]

    def call(self, params, want_valid=True, want_depth=True, **over):
        from src import _native
        n, h, w = self.shape
        a = dict(ctx=_native.ctx_for(self.torch.cuda.current_device()), left=self.ptr("left"), right=self.ptr("right"), n=n, h=h, w=w, c=self.c,
                 D=params[0], d0=params[1], P1=params[2], P2=params[3], u=params[4], lr=params[5], ws=self.ptr("ws"), group=self.group,
                 disparity=self.ptr("disparity"), valid=self.ptr("valid") if want_valid else None, depth=self.ptr("depth") if want_depth else None)
        a.update(over)
        return _native.lib().ds_stereo_match_u8(a["ctx"], a["left"], a["right"], a["n"], a["h"], a["w"], a["c"], a["D"], a["d0"], a["P1"],
                                                a["P2"], a["u"], a["lr"], a["ws"], a["group"], a["disparity"], a["valid"], a["depth"], None)

    def outputs(self):
        self.torch.cuda.synchronize()
        n, h, w = self.shape
        return (self.view("disparity").view(self.torch.int16).view(n, h, w), self.view("valid").clone().view(n, h, w),
                self.view("depth").view(self.torch.uint16).view(n, h, w))

    def guards_untouched(self, also=()):
        self.torch.cuda.synchronize()
        for k, b in self.blocks.items():
            lo, hi = self.at[k], self.at[k] + self.size[k]
            if not (bool((b[:lo] == self.SENT).all()) and bool((b[hi:] == self.SENT).all())):
                return False
            if k in also and not bool((b[lo:hi] == self.SENT).all()):
                return False
        return True


@pytest.mark.parametrize("D,shape,group", [(32, (3, 5, 67), 2), (64, (2, 9, 130), 2), (128, (3, 5, 67), 3)])
def test_workspace_content_does_not_matter_and_nothing_else_is_written(gpu, D, shape, group):
    params = (D, -7, 4, 48, 5, 1)
    want = sc.want("planes", shape, 3, params)
    b = _Buffers(gpu, shape, 3, D, group)
    for fill in (0xFF, 0x00, 0x7F):
        b.view("ws").fill_(fill)
        for k in NAMES:
            b.view(k).fill_(0x3C)
        assert b.call(params) == 0
        _same(b.outputs(), want, ("workspace", fill))
        assert b.guards_untouched()                                           # behind workspace_bytes * group and around every output


def test_optional_outputs_leave_the_others_unchanged(gpu):
    shape, params = (2, 9, 130), (64, 0, 4, 48, 5, 1)
    want = sc.want("planes", shape, 3, params)
    b = _Buffers(gpu, shape, 3, 64, 1)
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
    l, r = (_dev(gpu, v) for v in sc.pair("planes", shape))
    d, v, z = _native.stereo_match_u8(l, r, *params, want_valid=False, want_depth=False)
    assert v is None and z is None and np.array_equal(_host(d), want[0])


@pytest.mark.parametrize("c", [1, 3, 4])
def test_inputs_and_valid_at_odd_byte_addresses(gpu, c):
    shape, params = (3, 5, 67), (32, 5, 4, 48, 5, 1)
    b = _Buffers(gpu, shape, c, 32, 3, name="ramp", odd=True)
    assert b.call(params) == 0
    _same(b.outputs(), sc.want("ramp", shape, c, params), ("odd", c))
    assert b.guards_untouched()


def test_entry_point_refuses_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    shape, params = (2, 4, 24), (32, 0, 4, 48, 5, 1)
    n, h, w = shape
    b = _Buffers(torch, shape, 3, 32, 2)
    count, ws_bytes = b.count, b.per_image * 2
    big = torch.full((4 * ws_bytes,), b.SENT, dtype=torch.uint8, device="cuda")    # one block to carve overlapping buffers from
    B = big.data_ptr()
    assert B % 256 == 0

    def refused(code, **over):
        rc = b.call(params, **over)
        assert rc == code, (over, rc)
        assert b"ds_stereo_match_u8" in L.ds_last_error(), over
        return True

    cases = []
    # null pointers other than valid / depth
    cases += [(EINVAL, dict(ctx=None)), (EINVAL, dict(left=None)), (EINVAL, dict(right=None)), (EINVAL, dict(ws=None)), (EINVAL, dict(disparity=None))]
    # shape
    cases += [(EINVAL, dict(n=0)), (EINVAL, dict(h=0)), (EINVAL, dict(w=0)), (EINVAL, dict(n=-1)), (EINVAL, dict(w=-3))]
    # parameters
    cases += [(EINVAL, dict(c=0)), (EINVAL, dict(c=2)), (EINVAL, dict(c=5)), (EINVAL, dict(D=0)), (EINVAL, dict(D=16)), (EINVAL, dict(D=48)),
              (EINVAL, dict(D=256)), (EINVAL, dict(d0=-129)), (EINVAL, dict(d0=128)), (EINVAL, dict(P1=0)), (EINVAL, dict(P1=65)),
              (EINVAL, dict(P2=3)), (EINVAL, dict(P2=256)), (EINVAL, dict(u=-1)), (EINVAL, dict(u=51)), (EINVAL, dict(lr=-2)), (EINVAL, dict(lr=4))]
    # group, alignment
    cases += [(EINVAL, dict(group=0)), (EINVAL, dict(group=3)), (EINVAL, dict(group=-1)), (EINVAL, dict(ws=b.ptr("ws") + 128)),
              (EINVAL, dict(ws=b.ptr("ws") + 1)), (EINVAL, dict(disparity=b.ptr("disparity") + 1)), (EINVAL, dict(depth=b.ptr("depth") + 1))]
    # the order of the checks: a bad parameter beside a size above the limit is EINVAL, the size alone EUNSUPPORTED
    cases += [(EINVAL, dict(w=16385, u=51)), (EUNSUPPORTED, dict(w=16385)), (EUNSUPPORTED, dict(h=16385)), (EUNSUPPORTED, dict(n=65536, group=1)),
              (EUNSUPPORTED, dict(h=16384, w=16384)),                         # one image's workspace: 16 GiB of S alone
              (EUNSUPPORTED, dict(h=16384, w=2048)),                          # 2 GiB of S and the planes on top
              (EUNSUPPORTED, dict(w=16385, left=B, disparity=B))]             # the overlap test comes last
    # overlaps: an output or the workspace on an input; outputs on each other; beginning in the other's last byte
    cases += [(EINVAL, dict(left=B, disparity=B)), (EINVAL, dict(right=B, disparity=B + 3 * count - 2)), (EINVAL, dict(left=B + 2 * count - 2, disparity=B)),
              (EINVAL, dict(left=B, valid=B)), (EINVAL, dict(right=B, depth=B)), (EINVAL, dict(left=B + ws_bytes - 1, ws=B)), (EINVAL, dict(right=B, ws=B)),
              (EINVAL, dict(disparity=B, depth=B)), (EINVAL, dict(disparity=B, valid=B + 2 * count - 1)), (EINVAL, dict(depth=B, valid=B + 1)),
              (EINVAL, dict(ws=B, disparity=B + ws_bytes - 2)), (EINVAL, dict(ws=B, valid=B)), (EINVAL, dict(ws=B, depth=B + 256))]
    torch.cuda.synchronize()
    for code, over in cases:
        assert refused(code, **over)
    assert b.guards_untouched(also=("ws",) + NAMES) and bool((big == b.SENT).all())   # poisoned stays poisoned: no refusal launched anything
    # the workspace size of a refused shape is 0
    assert _native.stereo_match_workspace_bytes(0, 5, 32) == 0 and _native.stereo_match_workspace_bytes(5, 16385, 32) == 0
    assert _native.stereo_match_workspace_bytes(5, 5, 48) == 0
    # and the legal neighbours run: the ends of every range, adjacent but disjoint blocks
    for over in (dict(d0=-128), dict(d0=127), dict(P1=1, P2=1), dict(P1=64, P2=255), dict(P1=64, P2=64), dict(u=0), dict(u=50), dict(lr=-1),
                 dict(lr=3), dict(group=1), dict(valid=None, depth=None)):
        assert b.call(params, **over) == 0, over
    d_at = B + ws_bytes
    assert b.call(params, ws=B, disparity=d_at, depth=d_at + 2 * count, valid=d_at + 4 * count) == 0
    torch.cuda.synchronize()
    got = (big[ws_bytes:ws_bytes + 2 * count].view(torch.int16).view(n, h, w), big[ws_bytes + 4 * count:ws_bytes + 5 * count].clone().view(n, h, w),
           big[ws_bytes + 2 * count:ws_bytes + 4 * count].view(torch.uint16).view(n, h, w))
    _same(got, sc.want("planes", shape, 3, params), "adjacent blocks")
    assert bool((big[ws_bytes + 5 * count:] == b.SENT).all())
    assert b.guards_untouched()


def test_public_interface(gpu):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.stereo_matching as sm
    shape = (1, 24, 90)
    l, r = sc.pair("planes", shape)
    for kwargs, params in (({}, (64, 0, 4, 48, 5, 1)),
                           (dict(max_disparity=32, min_disparity=-4, p1=2, p2=30, uniqueness=10, lr_check=2), (32, -4, 2, 30, 10, 2)),
                           (dict(max_disparity=128, lr_check=-1, uniqueness=0), (128, 0, 4, 48, 0, -1))):
        want = sc.model(l, r, *params)
        for left, right in ((l[0], r[0]), (Image.fromarray(l[0]), Image.fromarray(r[0]))):
            depth = sm.depth_from_stereo(left, right, **kwargs)
            assert isinstance(depth, Image.Image) and depth.mode == 'I;16' and depth.size == (90, 24)
            assert np.array_equal(np.asarray(depth), want[2][0])
            depth2, disparity, mask = sm.depth_from_stereo(left, right, return_disparity=True, **kwargs)
            assert np.array_equal(np.asarray(depth2), want[2][0])
            assert disparity.dtype == np.float32 and np.array_equal(disparity * 16, want[0][0].astype(np.float32))
            assert mask.dtype == bool and np.array_equal(mask, want[1][0] == 1)
        batch = sm.depth_from_stereo_batch(_dev(torch, l), _dev(torch, r), **kwargs)
        assert batch.is_cuda and batch.dtype == torch.uint16 and tuple(batch.shape) == shape
        assert np.array_equal(_host(batch), _host(_native.stereo_match_u8(_dev(torch, l), _dev(torch, r), *params)[2]))
        assert np.array_equal(_host(batch), want[2])
    # grey input: a PIL 'L' image and a 2-D array are c = 1
    lg, rg = sc.pair("planes", shape, 1)
    want = sc.model(lg, rg, 32, 0, 4, 48, 5, 1)
    for left, right in ((lg[0, :, :, 0], rg[0, :, :, 0]), (Image.fromarray(lg[0, :, :, 0]), Image.fromarray(rg[0, :, :, 0])), (lg[0], rg[0])):
        assert np.array_equal(np.asarray(sm.depth_from_stereo(left, right, max_disparity=32)), want[2][0])
    before = dict(_native.CALLS)
    lt, rt = _dev(torch, l), _dev(torch, r)
    for bad in ({'max_disparity': 48}, {'min_disparity': -129}, {'p1': 0}, {'p2': 3}, {'uniqueness': 51}, {'lr_check': 4}, {'p1': True}):
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo(l[0], r[0], **bad)
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo_batch(lt, rt, **bad)
    for bad_l, bad_r in ((lt, rt[:, :, :80]), (lt.to(torch.int32), rt), (lt[0], rt[0]), (lt.cpu(), rt.cpu()), (l, r), (lt[..., :2], rt[..., :2]), (lt[:0], rt[:0])):
        with pytest.raises(_native.DepthStereoError):
            sm.depth_from_stereo_batch(bad_l, bad_r)
    assert dict(_native.CALLS) == before


def test_funnel_stereo_input_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'stereo_input': ...}): the pair is split, the left view's depth map computed, and the call goes
    on as the one with the left halves and inputdepthmaps=[depth_from_stereo(...)] (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.stereo_matching as sm
    from src import _native
    shape = (2, 64, 96)
    l, r = sc.pair("planes", shape)
    sbs = [Image.fromarray(np.concatenate([l[k], r[k]], axis=1)) for k in range(2)]
    tb_swapped = [Image.fromarray(np.concatenate([r[k], l[k]], axis=0)) for k in range(2)]
    lefts = [Image.fromarray(l[k]) for k in range(2)]
    S = ('left-right', 32)
    base = {'gen_stereo': True, 'gen_normalmap': True, 'stereo_modes': ['left-right']}
    kinds = ['depth', 'left-right', 'normalmap']

    def run(images, depthmaps, ops, opts=base, kinds=kinds):
        got = list(core.core_generation_funnel(None, list(images), depthmaps, None, dict(opts), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(len(images)) for k in kinds], [(i, k) for i, k, _ in got]
        return {k: [np.asarray(res) for _, kk, res in got if kk == k] for k in kinds}

    def same(a, b):
        return set(a) == set(b) and all(len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)

    def delta(before):
        return {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}

    maps = [sm.depth_from_stereo(l[k], r[k], 32) for k in range(2)]
    assert all(np.array_equal(np.asarray(m), sc.want("planes", shape, 3, (32, 0, 4, 48, 5, 1))[2][k]) for k, m in enumerate(maps))
    run(lefts, list(maps), None)                                              # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(lefts, list(maps), None)
    plain_delta = delta(before)
    assert "ds_stereo_match_u8" not in plain_delta
    # absent, None and {} make the launches and the bytes of a plain call
    for ops in ({}, {'stereo_input': None}):
        before = dict(_native.CALLS)
        assert same(run(lefts, list(maps), ops), plain), ops
        assert delta(before) == plain_delta, ops
    # the option: the same results from the pairs alone, and the plain call's launches plus one match per pair
    for depthmaps in (None, [], [None, None]):
        before = dict(_native.CALLS)
        got = run(sbs, depthmaps, {'stereo_input': S})
        assert same(got, plain)
        assert delta(before) == dict(plain_delta, ds_stereo_match_u8=2)
    assert same(run(tb_swapped, None, {'stereo_input': ('bottom-top', 32, 0, 4, 48, 5, 1)}), plain)
    assert [im.size for im in sbs] == [(192, 64)] * 2                         # the caller's list and images are left alone
    # other parameters give another map; depth_refine applies to it
    other = run(sbs, None, {'stereo_input': ('left-right', 32, 0, 4, 48, 0, -1)})
    assert not same(other, plain)
    refined = run(sbs, None, {'stereo_input': S, 'depth_refine': (5, 60.0, 2.0)})
    assert same(refined, run(lefts, list(maps), {'depth_refine': (5, 60.0, 2.0)})) and not same(refined, plain)
    assert not hasattr(core.model_holder, 'stereo_input')                     # the option does not become a holder setting
    for bad in ({'stereo_input': 'left-right'}, {'stereo_input': ('sbs', 32)}, {'stereo_input': ('left-right', 48)}, {'stereo_input': ()},
                {'stereo_input': ('left-right', 32, 0, 4)}, {'stereo_input': ('left-right', True)}, {'stereo_input': (32,)},
                {'stereo_input': ('left-right', 32, 0, 4, 48, float('nan'))}, {'stereo_input': {}}):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(sbs, None, bad)
        assert dict(_native.CALLS) == before, bad                             # before any device work
    # together with inputdepthmaps, and on an odd width
    for images, depthmaps in ((sbs, list(maps)), (sbs, [maps[0], None]), ([im.crop((0, 0, 191, 64)) for im in sbs], None)):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(images, depthmaps, {'stereo_input': S})
        assert dict(_native.CALLS) == before
    assert same(run(lefts, list(maps), None), plain)
