"""The speckle filter alone (include/depthstereo.h: ds_speckle_filter_i16) against the flood fill of tests/stereo_match_ex_cases.py, on
valid_out and size_out, exactly: membership and counts are properties of the graph.  The patterns are topologies a matcher never
produces: one component of the whole image; a checkerboard (all singletons: diagonal contact is no link); a serpentine, a spiral and a
comb (long thin components whose links the merge must follow a long way); value ramps in steps of t (one component) and t + 1 (all
singletons); -32768 beside 32767; a random mask with random values; and borders that would link if rows or images ran on.  Shapes: one
pixel, one row, one column, a batch of 3, and 40 x 300, whose components span dozens of the 256-pixel workgroups in both directions.
tests/test_stereo_match_ex_cpu.py shows that the patterns are what their names say."""
import numpy as np
import pytest

import stereo_match_ex_cases as ex

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
T = ex.PATTERN_T


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _check(torch, disp, valid, size, t, sizes_want, what, **kwargs):
    from src import _native
    before = _native.CALLS["ds_speckle_filter_i16"]
    out, sizes = _native.speckle_filter_i16(_dev(torch, disp), _dev(torch, valid), size, t, want_sizes=True, **kwargs)
    assert _native.CALLS["ds_speckle_filter_i16"] == before + 1
    assert out.dtype == torch.uint8 and sizes.dtype == torch.int32 and tuple(out.shape) == tuple(sizes.shape) == disp.shape
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy().view(np.uint32)
    assert np.array_equal(sizes, sizes_want), (what, int((sizes != sizes_want).sum()), np.argwhere(sizes != sizes_want)[:6].tolist())
    assert np.array_equal(out, (sizes_want > size).astype(np.uint8)), (what, size)


@pytest.mark.parametrize("shape", ex.SPECKLE_SHAPES, ids=["%dx%dx%d" % s for s in ex.SPECKLE_SHAPES])
def test_patterns_equal_the_flood_fill(gpu, shape):
    for name in ex.PATTERNS:
        disp, valid = ex.pattern(name, shape)
        want = ex.pattern_sizes(name, shape)
        present = sorted(set(int(v) for v in np.unique(want) if v > 0))
        # sizes on both sides of what is present: below the smallest, on a count, on a count minus 1, at the top of the range
        sizes = {1, 65535, max(present[0] - 1, 1), min(present[0], 65535), min(max(present[-1] - 1, 1), 65535), min(present[-1], 65535)}
        for size in sorted(sizes):
            _check(gpu, disp, valid, size, T, want, (name, shape, size))


def test_t_is_compared_in_int32_at_both_ends_of_its_range(gpu):
    shape = (2, 9, 130)
    disp, valid = ex.pattern("extremes", shape)
    for t in (0, 65534, 65535):
        want = np.stack([ex.speckle_sizes(d, v, t) for d, v in zip(disp, valid)]).astype(np.uint32)
        _check(gpu, disp, valid, 3, t, want, ("extremes", t))
    assert (want == 9 * 130).all()                                           # at t = 65535 everything links
    disp, valid = ex.pattern("random", shape)
    for t in (0, 1, 2 * T, 4 * T):
        want = np.stack([ex.speckle_sizes(d, v, t) for d, v in zip(disp, valid)]).astype(np.uint32)
        _check(gpu, disp, valid, 5, t, want, ("random", t))


def test_images_of_a_batch_stay_apart_whatever_the_group(gpu):
    from src import _native
    shape = (3, 5, 67)
    disp, valid = (np.array(v) for v in ex.pattern("borders", shape))
    disp[1], valid[1] = (v[1] for v in ex.pattern("random", shape))
    want = np.stack([ex.speckle_sizes(d, v, T) for d, v in zip(disp, valid)]).astype(np.uint32)
    for g in (1, 2, 3, None):
        _check(gpu, disp, valid, 4, T, want, ("group", g), group=g)
    dt, vt = _dev(gpu, disp), _dev(gpu, valid)
    alone = _native.speckle_filter_i16(dt[2:3], vt[2:3], 4, T, want_sizes=True)
    assert np.array_equal(alone[1].cpu().numpy().view(np.uint32), want[2:3])
    out, none = _native.speckle_filter_i16(dt, vt, 4, T)
    assert none is None and np.array_equal(out.cpu().numpy(), (want > 4).astype(np.uint8))
    for bad in (0, 4, -1, True, 1.5, "1"):
        with pytest.raises(_native.DepthStereoError):
            _native.speckle_filter_i16(dt, vt, 4, T, group=bad)
    before = dict(_native.CALLS)
    for args in ((dt, vt, 0, T), (dt, vt, 65536, T), (dt, vt, 4, -1), (dt, vt, 4, 65536), (dt, vt, True, T), (dt, vt, 4, float('nan')), (dt, vt, "4", T),
                 (dt.int(), vt, 4, T), (dt, vt.int(), 4, T), (dt[0], vt[0], 4, T), (dt, vt[:, :, :60], 4, T), (dt.cpu(), vt.cpu(), 4, T), (dt[:0], vt[:0], 4, T)):
        with pytest.raises(_native.DepthStereoError):
            _native.speckle_filter_i16(*args)
    assert dict(_native.CALLS) == before


class _Buffers:
    """disp, valid, the workspace and the two outputs carved from guarded blocks, for calls of the raw entry point."""
    GUARD, SENT = 512, 0xA5

    def __init__(self, torch, shape, group, name="random", odd=False):
        from src import _native
        self.torch, self.shape, self.group = torch, shape, group
        n, h, w = shape
        self.count = n * h * w
        self.disp, self.valid = ex.pattern(name, shape)
        self.per_image = _native.speckle_filter_workspace_bytes(h, w)
        assert self.per_image % 256 == 0 and self.per_image >= 8 * h * w
        G = self.GUARD
        self.size = {"disp": 2 * self.count, "valid": self.count, "ws": self.per_image * group, "valid_out": self.count, "size_out": 4 * self.count}
        self.blocks = {k: torch.full((size + 2 * G + 2,), self.SENT, dtype=torch.uint8, device="cuda") for k, size in self.size.items()}
        self.at = {k: G + (1 if odd and k in ("valid", "valid_out") else 0) for k in self.size}
        self.view("disp").copy_(_dev(torch, self.disp).view(-1).view(torch.uint8))
        self.view("valid").copy_(_dev(torch, self.valid).view(-1))
        assert self.ptr("ws") % 256 == 0 and self.ptr("disp") % 2 == 0 and self.ptr("size_out") % 4 == 0

    def view(self, k):
        return self.blocks[k][self.at[k]:self.at[k] + self.size[k]]

    def ptr(self, k):
        return self.blocks[k].data_ptr() + self.at[k]

    def call(self, size, t, want_sizes=True, **over):
        from src import _native
        n, h, w = self.shape
        a = dict(ctx=_native.ctx_for(self.torch.cuda.current_device()), disp=self.ptr("disp"), valid=self.ptr("valid"), n=n, h=h, w=w, size=size, t=t,
                 ws=self.ptr("ws"), group=self.group, valid_out=self.ptr("valid_out"), size_out=self.ptr("size_out") if want_sizes else None)
        a.update(over)
        return _native.lib().ds_speckle_filter_i16(a["ctx"], a["disp"], a["valid"], a["n"], a["h"], a["w"], a["size"], a["t"], a["ws"], a["group"],
                                                   a["valid_out"], a["size_out"], None)

    def outputs(self):
        self.torch.cuda.synchronize()
        n, h, w = self.shape
        return (self.view("valid_out").clone().view(n, h, w).cpu().numpy(),
                self.view("size_out").clone().view(self.torch.int32).view(n, h, w).cpu().numpy().view(np.uint32))

    def guards_untouched(self, also=()):
        self.torch.cuda.synchronize()
        for k, b in self.blocks.items():
            lo, hi = self.at[k], self.at[k] + self.size[k]
            if not (bool((b[:lo] == self.SENT).all()) and bool((b[hi:] == self.SENT).all())):
                return False
            if k in also and not bool((b[lo:hi] == self.SENT).all()):
                return False
        return True


@pytest.mark.parametrize("shape,group,odd", [((3, 5, 67), 2, False), ((2, 9, 130), 1, True), ((1, 33, 257), 1, False)])
def test_workspace_content_does_not_matter_and_nothing_else_is_written(gpu, shape, group, odd):
    torch = gpu
    want = ex.pattern_sizes("random", shape)
    b = _Buffers(torch, shape, group, odd=odd)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    for fill in (0xFF, "random", 0x00):                                       # 0xFF: every link -1 and every counter 2^32 - 1
        if fill == "random":
            b.view("ws").copy_(torch.randint(0, 256, (b.size["ws"],), dtype=torch.uint8, device="cuda", generator=gen))
        else:
            b.view("ws").fill_(fill)
        b.view("valid_out").fill_(0x3C)
        b.view("size_out").fill_(0x3C)
        assert b.call(3, T) == 0
        out, sizes = b.outputs()
        assert np.array_equal(sizes, want) and np.array_equal(out, (want > 3).astype(np.uint8)), fill
        assert b.guards_untouched()
    # size_out may be NULL: valid_out the same, size_out left alone
    b.view("valid_out").fill_(0x3C)
    b.view("size_out").fill_(b.SENT)
    assert b.call(3, T, want_sizes=False) == 0
    assert np.array_equal(b.outputs()[0], (want > 3).astype(np.uint8)) and b.guards_untouched(also=("size_out",))


def test_entry_point_refuses_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    shape = (2, 4, 24)
    n, h, w = shape
    b = _Buffers(torch, shape, 2)
    count, ws_bytes = b.count, b.per_image * 2
    big = torch.full((8 * ws_bytes,), b.SENT, dtype=torch.uint8, device="cuda")
    B = big.data_ptr()
    assert B % 256 == 0

    def refused(code, size=3, t=T, **over):
        rc = b.call(size, t, **over)
        assert rc == code, (over, size, t, rc)
        assert b"ds_speckle_filter_i16" in L.ds_last_error(), over
        return True

    cases = [(EINVAL, dict(ctx=None)), (EINVAL, dict(disp=None)), (EINVAL, dict(valid=None)), (EINVAL, dict(ws=None)), (EINVAL, dict(valid_out=None)),
             (EINVAL, dict(n=0)), (EINVAL, dict(h=0)), (EINVAL, dict(w=0)), (EINVAL, dict(n=-1)), (EINVAL, dict(w=-3)),
             (EINVAL, dict(size=0)), (EINVAL, dict(size=-1)), (EINVAL, dict(size=65536)), (EINVAL, dict(t=-1)), (EINVAL, dict(t=65536)),
             (EINVAL, dict(group=0)), (EINVAL, dict(group=3)), (EINVAL, dict(group=-1)),
             (EINVAL, dict(ws=b.ptr("ws") + 128)), (EINVAL, dict(disp=b.ptr("disp") + 1)), (EINVAL, dict(size_out=b.ptr("size_out") + 2)),
             # the order of the checks
             (EINVAL, dict(w=16385, size=0)), (EUNSUPPORTED, dict(w=16385)), (EUNSUPPORTED, dict(h=16385)), (EUNSUPPORTED, dict(n=65536, group=1)),
             (EUNSUPPORTED, dict(w=16385, disp=B, valid_out=B)),              # the overlap test comes last
             # overlaps; valid_out may not alias valid
             (EINVAL, dict(valid_out=b.ptr("valid"))), (EINVAL, dict(disp=B, valid_out=B + 2 * count - 1)), (EINVAL, dict(valid=B, size_out=B)),
             (EINVAL, dict(disp=B, ws=B)), (EINVAL, dict(valid=B + ws_bytes - 1, ws=B)), (EINVAL, dict(ws=B, valid_out=B + ws_bytes - 1)),
             (EINVAL, dict(ws=B, size_out=B + 256)), (EINVAL, dict(valid_out=B + 4, size_out=B))]
    cases = [(code, dict(over)) for code, over in cases]
    torch.cuda.synchronize()
    for code, over in cases:
        size, t = over.pop("size", 3), over.pop("t", T)
        assert refused(code, size=size, t=t, **over)
    assert b.guards_untouched(also=("ws", "valid_out", "size_out")) and bool((big == b.SENT).all())
    W = _native.speckle_filter_workspace_bytes
    assert W(0, 5) == 0 and W(5, 0) == 0 and W(5, 16385) == 0 and W(16385, 5) == 0 and W(1, 1) == 512 and W(16384, 16384) == (1 << 31)
    # (the largest legal image, 16384 x 16384 = 2^28 pixels, takes exactly 2 GiB: the side limit is the one that binds)
    # the legal neighbours run: the ends of every range, adjacent but disjoint blocks
    want = ex.pattern_sizes("random", shape)
    for size, t in ((1, 0), (65535, 65535), (3, T)):
        assert b.call(size, t) == 0
    d_at = B + ws_bytes
    assert b.call(3, T, ws=B, valid_out=d_at, size_out=d_at + 4 * ((count + 3) // 4)) == 0
    torch.cuda.synchronize()
    s_at = ws_bytes + 4 * ((count + 3) // 4)
    assert np.array_equal(big[ws_bytes:ws_bytes + count].cpu().numpy().reshape(shape), (want > 3).astype(np.uint8))
    assert np.array_equal(big[s_at:s_at + 4 * count].clone().view(torch.int32).cpu().numpy().view(np.uint32).reshape(shape), want)
    assert bool((big[s_at + 4 * count:] == b.SENT).all()) and b.guards_untouched()
