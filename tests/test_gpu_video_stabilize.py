"""Video mode's temporal depth filter on the device (include/depthstereo.h: ds_temporal_joint_bilateral_u16; csrc/ds_video.hip) and
its public interface (src/video_mode.py: stabilize_depth, gen_frames_sharded(stabilize=)).  The kernel is compared with the float64
NumPy model of the definition (tests/video_stabilize_cases.py) by integer equality of the uint16 results: nothing here has a
tolerance, the definition fixes every rounding."""
import numpy as np
import pytest

import video_stabilize_cases as sc

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
# (m, h, w, c).  (6, 4, 257, 3): odd row bytes, a frame crosses a 256-thread workgroup; (12, 24, 40, 3): the flicker clip's size, more
# than one workgroup per frame and (12 outputs at under 1024 workgroups) more than one chunk of the time axis.
SHAPES = [(7, 5, 13, 3), (9, 3, 67, 4), (5, 1, 1, 3), (6, 4, 257, 3), (12, 24, 40, 3)]


def _ranges(m):
    """(first, count, lo, hi): the full clip; an interior run with lo > 0 and hi < m - 1; count == 1; lo == hi == first."""
    return [(0, m, 0, m - 1), (2, m - 4, 1, m - 2), (m // 2, 1, 0, m - 1), (m // 2, 1, m // 2, m // 2), (1, 2, 1, m - 1)]


def _inputs(m, h, w, c, seed):
    return [("noise", sc.noise_clip(m, h, w, c, seed)), ("static", sc.static_clip(m, h, w, c, seed + 1))]


def _run(torch, nat, frames_dev, depth_dev, params, first, count, lo, hi, out=None):
    wt, wc = nat.stabilize_tables_on(depth_dev.device, *params)
    return nat.temporal_joint_bilateral_u16(depth_dev, frames_dev, params[0], wt, wc, first, count, lo, hi, out=out)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_equals_the_model_bit_for_bit(gpu, shape):
    torch = gpu
    from src import _native as nat
    m, h, w, c = shape
    for name, (frames, depth) in _inputs(m, h, w, c, seed=100 * h + w):
        fd, dd = torch.from_numpy(frames).cuda(), torch.from_numpy(depth).cuda()
        # the guide at an odd byte offset: a slice of a larger uint8 buffer
        buf = torch.zeros(frames.size + 32, dtype=torch.uint8, device="cuda")
        off = 1 + (-buf.data_ptr()) % 16
        odd = buf[off:off + frames.size]
        odd.copy_(fd.reshape(-1))
        odd = odd.view(frames.shape)
        assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
        for radius in (1, 2, 3, 4):
            params = (radius, 30.0 if name == "noise" else 6.0, 0.6 * radius + 0.4)
            for first, count, lo, hi in _ranges(m):
                want = sc.model_range(depth, frames, params, first, count, lo, hi)
                before = nat.CALLS["ds_temporal_joint_bilateral_u16"]
                got = _run(torch, nat, fd, dd, params, first, count, lo, hi)
                assert nat.CALLS["ds_temporal_joint_bilateral_u16"] == before + 1
                assert got.is_cuda and got.dtype == torch.uint16 and tuple(got.shape) == (count, h, w)
                g = got.cpu().numpy()
                assert np.array_equal(g, want), (name, params, first, count, lo, hi, np.argwhere(g != want)[:6].tolist())
                if lo == hi:
                    assert np.array_equal(g, depth[first:first + 1])                  # a scene of one frame: the output is the input
                g = _run(torch, nat, odd, dd, params, first, count, lo, hi).cpu().numpy()
                assert np.array_equal(g, want), ("odd guide address", name, params, first, count, lo, hi)
        if name == "static" and m > 2:
            assert not np.array_equal(sc.model_range(depth, frames, (1, 6.0, 1.0), 0, m, 0, m - 1), depth)


def test_extreme_values_and_weights_that_underflow(gpu):
    torch = gpu
    from src import _native as nat
    frames, depth = sc.extreme_clip()
    m = depth.shape[0]
    fd, dd = torch.from_numpy(frames).cuda(), torch.from_numpy(depth).cuda()
    for params in ((1, 300.0, 1.0), (4, 1000.0, 50.0), (2, 0.5, 1.0)):
        want = sc.model_range(depth, frames, params, 0, m, 0, m - 1)
        assert np.array_equal(_run(torch, nat, fd, dd, params, 0, m, 0, m - 1).cpu().numpy(), want), params


def test_a_frame_alone_has_the_bits_of_the_full_run_and_frames_outside_lo_hi_are_not_read(gpu):
    torch = gpu
    from src import _native as nat
    m, h, w = 12, 24, 40
    frames, depth = sc.static_clip(m, h, w, 3, seed=9)
    fd, dd = torch.from_numpy(frames).cuda(), torch.from_numpy(depth).cuda()
    for radius in (1, 4):
        params = (radius, 8.0, 2.0)
        full = _run(torch, nat, fd, dd, params, 0, m, 0, m - 1)
        for i in range(m):                                                        # count = 1: another first, another chunking of time
            assert torch.equal(_run(torch, nat, fd, dd, params, i, 1, 0, m - 1)[0].view(torch.int16), full[i].view(torch.int16)), (radius, i)
        part = _run(torch, nat, fd, dd, params, 3, 5, 0, m - 1)
        assert torch.equal(part.view(torch.int16), full[3:8].view(torch.int16))
        # frames outside [lo, hi] filled with garbage change no output
        lo, hi = 2, 8
        clean = _run(torch, nat, fd, dd, params, lo, hi - lo + 1, lo, hi)
        gf, gd = sc.noise_clip(m, h, w, 3, seed=77)
        gf[lo:hi + 1], gd[lo:hi + 1] = frames[lo:hi + 1], depth[lo:hi + 1]
        dirty = _run(torch, nat, torch.from_numpy(gf).cuda(), torch.from_numpy(gd).cuda(), params, lo, hi - lo + 1, lo, hi)
        assert torch.equal(clean.view(torch.int16), dirty.view(torch.int16)), radius
        assert np.array_equal(clean.cpu().numpy(), sc.model_range(depth, frames, params, lo, hi - lo + 1, lo, hi))


def test_out_slice_is_written_and_nothing_beside_it(gpu):
    torch = gpu
    from src import _native as nat
    m, h, w = 6, 3, 67
    frames, depth = sc.noise_clip(m, h, w, 4, seed=4)
    fd, dd = torch.from_numpy(frames).cuda(), torch.from_numpy(depth).cuda()
    big = torch.full((m + 2, h, w), 12345, dtype=torch.int16, device="cuda").view(torch.uint16)
    params = (2, 50.0, 1.0)
    ret = _run(torch, nat, fd, dd, params, 1, 4, 0, 5, out=big[1:5])
    assert ret.data_ptr() == big[1:5].data_ptr()
    assert np.array_equal(big[1:5].cpu().numpy(), sc.model_range(depth, frames, params, 1, 4, 0, 5))
    assert bool((big[0].view(torch.int16) == 12345).all()) and bool((big[5:].view(torch.int16) == 12345).all()), "the kernel wrote outside out"


def test_entry_point_rejects_bad_arguments_before_any_launch(gpu):
    torch = gpu
    from src import _native as nat
    L, ctx = nat.lib(), nat.ctx_for(torch.cuda.current_device())
    m, h, w, SENT = 6, 4, 5, 1234
    depth = torch.zeros((m, h, w), dtype=torch.int16, device="cuda")
    guide = torch.zeros((m, h, w, 4), dtype=torch.uint8, device="cuda")
    out = torch.full((m, h, w), SENT, dtype=torch.int16, device="cuda")
    wt, wc = nat.stabilize_tables_on(depth.device, 4, 10.0, 2.0)
    nd = 2 * m * h * w
    big = torch.full((2 * m * h * w,), SENT, dtype=torch.int16, device="cuda")     # one block to carve overlapping depth / out from
    B = big.data_ptr()
    st = nat._stream(depth)

    def call(c=ctx, dp=depth.data_ptr(), gp=guide.data_ptr(), gc=3, m_=m, h_=h, w_=w, r=2, wtp=wt.data_ptr(), wcp=wc.data_ptr(), first=1,
             count=3, lo=0, hi=5, op=out.data_ptr()):
        return L.ds_temporal_joint_bilateral_u16(c, dp, gp, gc, m_, h_, w_, r, wtp, wcp, first, count, lo, hi, op, st)
    bad = [dict(c=None), dict(dp=None), dict(gp=None), dict(wtp=None), dict(wcp=None), dict(op=None),
           dict(m_=0), dict(m_=-1), dict(h_=0), dict(w_=0), dict(w_=-3), dict(count=0), dict(count=-1),
           dict(gc=0), dict(gc=1), dict(gc=2), dict(gc=5), dict(r=0), dict(r=5), dict(r=-1),
           dict(lo=-1), dict(lo=2), dict(hi=2), dict(hi=6), dict(first=4, count=3), dict(first=-1, lo=-1), dict(hi=m, m_=m),
           dict(wtp=wt.data_ptr() + 4), dict(wcp=wc.data_ptr() + 4), dict(wcp=wc.data_ptr() + 2),
           dict(dp=depth.data_ptr() + 1), dict(op=out.data_ptr() + 1),
           # out overlapping depth: equal pointers, out beginning in the last 2 bytes of depth, depth beginning in the last 2 bytes of
           # out (count = 3 frames of out)
           dict(dp=B, op=B), dict(dp=B, op=B + nd - 2), dict(dp=B + 3 * 2 * h * w - 2, op=B)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert b"ds_temporal_joint_bilateral_u16" in L.ds_last_error(), kw
    assert call(m_=1, h_=65536, w_=65536, first=0, count=1, lo=0, hi=0) == EUNSUPPORTED                  # h * w = 2^32
    assert b"ds_temporal_joint_bilateral_u16" in L.ds_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((big == SENT).all()), "a rejected call wrote to out"
    # the legal neighbours run: every radius, c == 4, a guide at an odd address, adjacent but disjoint blocks
    for r in (1, 2, 3, 4):
        assert call(r=r) == 0
    assert call(gc=4) == 0 and call(gp=guide.data_ptr() + 1) == 0
    assert call(dp=B + 3 * 2 * h * w, op=B) == 0                                                          # depth begins where out ends
    assert call(dp=B, op=B + nd) == 0                                                                     # out begins where depth ends
    torch.cuda.synchronize()
    assert bool((out[:3] == 0).all()) and bool((out[3:] == SENT).all())
    # the binding's own checks
    f8 = torch.zeros((m, h, w, 3), dtype=torch.uint8, device="cuda")
    d16 = depth.view(torch.uint16)
    wt2, wc2 = nat.stabilize_tables_on(depth.device, 2, 10.0, 2.0)
    before = nat.CALLS["ds_temporal_joint_bilateral_u16"]
    for args in ((depth, f8, 2, wt2, wc2, 0, m, 0, m - 1), (d16, f8.float(), 2, wt2, wc2, 0, m, 0, m - 1), (d16, f8[:, :, :, :2], 2, wt2, wc2, 0, m, 0, m - 1),
                 (d16, f8[:5], 2, wt2, wc2, 0, m, 0, m - 1), (d16, f8, 2, wt, wc2, 0, m, 0, m - 1), (d16, f8, 2, wt2, wc2[:700], 0, m, 0, m - 1),
                 (d16, f8, 2, wt2.cpu(), wc2, 0, m, 0, m - 1), (d16.cpu(), f8, 2, wt2, wc2, 0, m, 0, m - 1)):
        with pytest.raises(nat.DepthStereoError):
            nat.temporal_joint_bilateral_u16(*args)
    with pytest.raises(nat.DepthStereoError):
        nat.temporal_joint_bilateral_u16(d16, f8, 2, wt2, wc2, 0, m, 0, m - 1, out=torch.empty((m, h, w), dtype=torch.int16, device="cuda"))
    assert nat.CALLS["ds_temporal_joint_bilateral_u16"] == before
    with pytest.raises(nat.DepthStereoError):
        nat.temporal_joint_bilateral_u16(d16, f8, 2, wt2, wc2, 0, m, 0, m)                                 # the library refuses: hi == m


def test_stabilize_depth_on_the_device_equals_its_host_route_one_launch_per_scene(gpu):
    torch = gpu
    from src import _native as nat, video_mode as vm
    frames, depth, bar = sc.flicker_clip()
    fd, dd = torch.from_numpy(frames).cuda(), torch.from_numpy(depth).cuda()
    for params, cuts in (((2, 10.0, 1.5), None), ((4, 10.0, 2.0), [5]), ((1, 10.0, 1.0), [1, 5, 11]), ((3, 12.0, 2.5), [])):
        before = nat.CALLS["ds_temporal_joint_bilateral_u16"]
        got = vm.stabilize_depth(fd, dd, params, cuts=cuts)
        assert nat.CALLS["ds_temporal_joint_bilateral_u16"] == before + len(cuts or []) + 1, (params, cuts)       # one launch per scene
        assert got.is_cuda and got.dtype == torch.uint16 and tuple(got.shape) == depth.shape
        host = vm.stabilize_depth(frames, depth, params, cuts=cuts)
        assert nat.CALLS["ds_temporal_joint_bilateral_u16"] == before + len(cuts or []) + 1, "the host route launched the kernel"
        assert np.array_equal(got.cpu().numpy(), host), (params, cuts)
        assert np.array_equal(host, sc.model(depth, frames, params, cuts=cuts))
    # scenes do not mix: with a cut at 5, frames 0..4 are the filter of the clip truncated to five frames
    cut = vm.stabilize_depth(fd, dd, (4, 10.0, 2.0), cuts=[5])
    assert torch.equal(cut[:5].view(torch.int16), vm.stabilize_depth(fd[:5], dd[:5], (4, 10.0, 2.0)).view(torch.int16))
    assert torch.equal(cut[5:].view(torch.int16), vm.stabilize_depth(fd[5:], dd[5:], (4, 10.0, 2.0)).view(torch.int16))
    assert not torch.equal(cut.view(torch.int16), vm.stabilize_depth(fd, dd, (4, 10.0, 2.0)).view(torch.int16))
    # the torch route on the device (the other side of tools/video_stabilize_ab.py) has the kernel's bits too
    wt, wc = nat.stabilize_tables_on(dd.device, 2, 10.0, 1.5)
    assert np.array_equal(vm._stabilize_torch(dd, fd, 2, wt, wc, 0, 12, 0, 11).cpu().numpy(), sc.model(depth, frames, (2, 10.0, 1.5)))
    # refused before any launch
    before = nat.CALLS["ds_temporal_joint_bilateral_u16"]
    for args, kw in (((fd, dd, (0, 10.0, 1.5)), {}), ((fd, dd.view(torch.int16), (2, 10.0, 1.5)), {}), ((fd[:5], dd, (2, 10.0, 1.5)), {}),
                     ((fd[..., :2], dd, (2, 10.0, 1.5)), {}), ((fd, dd.cpu(), (2, 10.0, 1.5)), {}), ((fd, dd, (2, 10.0, 1.5)), dict(cuts=[12]))):
        with pytest.raises((nat.DepthStereoError, ValueError)):
            vm.stabilize_depth(*args, **kw)
    assert nat.CALLS["ds_temporal_joint_bilateral_u16"] == before


def test_gen_frames_sharded_filters_between_quantisation_and_stereo(gpu):
    """A 7-frame 16 x 24 clip of two static scenes with colour noise through the two-pass pipeline with a stub network: with
    stabilize= the 'depth' output is stabilize_depth of the 'depth' the same call gives without it, the stereo pair is the warp of
    that filtered map, and without it no call of the new entry point is made."""
    torch = gpu
    from src import _native as nat, video_mode as vm
    from src.stereoimage_generation import create_stereoimages_batch
    a, _ = sc.static_clip(3, 16, 24, 3, seed=1)
    b, _ = sc.static_clip(4, 16, 24, 3, seed=2)
    frames = torch.from_numpy(np.concatenate([a, b]))
    params, cuts = (2, 10.0, 1.5), [3]

    def predict(x):
        assert x.is_cuda and x.dtype == torch.uint8
        return x[..., 0].float() * 0.5 + x[..., 1].float() * 0.25 + x[..., 2].float()

    inp = {'stereo_modes': ['left-right']}
    c0 = dict(nat.CALLS)
    plain = vm.gen_frames_sharded(frames, predict, inp, 'none', batch=4, cuts=cuts)
    c1 = dict(nat.CALLS)
    stab = vm.gen_frames_sharded(frames, predict, inp, 'none', batch=4, cuts=cuts, stabilize=params)
    c2 = dict(nat.CALLS)
    used_plain = {k for k in c1 if c1[k] != c0.get(k, 0)}
    used_stab = {k for k in c2 if c2[k] != c1.get(k, 0)}
    assert "ds_temporal_joint_bilateral_u16" not in used_plain                                    # None adds no launch
    assert used_stab - used_plain == {"ds_temporal_joint_bilateral_u16"}
    assert c2["ds_temporal_joint_bilateral_u16"] - c1.get("ds_temporal_joint_bilateral_u16", 0) == 2       # one per scene
    assert set(stab.keys()) == set(plain.keys()) == {'depth', 'left-right', 'cuts'}
    want = vm.stabilize_depth(frames.cuda(), plain['depth'], params, cuts=cuts)
    assert stab['depth'].dtype == torch.uint16 and torch.equal(stab['depth'].view(torch.int16), want.view(torch.int16))
    assert not torch.equal(want.view(torch.int16), plain['depth'].view(torch.int16))
    assert np.array_equal(want.cpu().numpy(), sc.model(plain['depth'].cpu().numpy(), frames.numpy(), params, cuts=cuts))
    sbs = create_stereoimages_batch(frames.cuda(), want, 2.5, 0.0, ['left-right'], 0.0, 1.0, 'polylines_sharp')[0]
    assert torch.equal(stab['left-right'], sbs) and not torch.equal(plain['left-right'], sbs)
