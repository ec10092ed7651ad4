"""Parallax frames from depth (include/depthstereo.h: ds_parallax_u8; src/parallax_generation.py; ops={'parallax': ...}) against the
NumPy model, tests/parallax_cases.py.  Every comparison is torch.equal / np.array_equal: the definition is all-integer and the depth
test is a maximum, so there is nothing to tolerate and nothing that depends on the order of the atomics.  Shapes: smaller than a
block of threads (5 x 7), ragged in both directions with a focus per image (19 x 37), scans longer than a block over several blocks
(40 x 70, G = 64), narrower than a wave (33 x 16); six poses each: the identity, an extreme of every component, mixed signs.
tests/test_parallax_cpu.py shows that every case contains collided targets, two-wide footprints, dropped splats, holes won by each of
the four directions and fallback pixels."""
import numpy as np
import pytest

import parallax_cases as pc

pytestmark = pytest.mark.gpu

POSES = np.asarray(pc.POSES, np.int32)


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _run(torch, image, depth, poses, focus, G, invert=False, want_mask=True, out=None):
    from src import _native
    return _native.parallax_u8(_dev(torch, image), _dev(torch, depth), poses, focus, G, invert=invert, want_mask=want_mask, out=out)


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


def _raw(torch, image_t, depth_t, focus_t, poses_t, G, keys_t, out_t, mask_t=None, invert=0):
    """The C entry point on the caller's buffers (the binding allocates keys itself)."""
    from src import _native
    n, h, w = depth_t.shape
    return _native.lib().ds_parallax_u8(_native.ctx_for(torch.cuda.current_device()), image_t.data_ptr(), depth_t.data_ptr(), focus_t.data_ptr(),
                                        n, h, w, poses_t.data_ptr(), poses_t.shape[0], G, invert, keys_t.data_ptr(), out_t.data_ptr(),
                                        None if mask_t is None else mask_t.data_ptr(), None)


@pytest.mark.parametrize("case", range(len(pc.KERNEL_CASES)), ids=pc.KERNEL_IDS)
def test_kernels_equal_the_model_bit_for_bit(gpu, case):
    torch = gpu
    from src import _native
    shape, G, focus = pc.KERNEL_CASES[case]
    image, depths = pc.inputs(shape)
    F = len(POSES)
    for name in pc.DEPTHS:
        depth = depths[name]
        for invert in (False, True):
            before = _native.CALLS["ds_parallax_u8"]
            out, mask = _run(torch, image, depth, POSES, pc.focus_list(depth, focus), G, invert)
            assert _native.CALLS["ds_parallax_u8"] == before + 1
            assert out.dtype == torch.uint8 and mask.dtype == torch.uint8 and out.is_cuda and mask.is_cuda
            assert tuple(out.shape) == (shape[0], F) + shape[1:] + (3,) and tuple(mask.shape) == (shape[0], F) + shape[1:]
            want_out, want_mask = pc.want(case, name, invert)
            got_out, got_mask = out.cpu().numpy(), mask.cpu().numpy()
            assert np.array_equal(got_mask, want_mask), (name, invert, _mismatch(got_mask, want_mask))
            assert np.array_equal(got_out, want_out), (name, invert, _mismatch(got_out, want_out))
            alone = _run(torch, image, depth, POSES, pc.focus_list(depth, focus), G, invert, want_mask=False)         # out_mask == NULL
            assert torch.equal(alone, out), (name, invert)


def test_buffers_at_odd_addresses_give_the_same_bits(gpu):
    """image and out at odd byte addresses, depth at ptr % 8 == 2, keys at ptr % 16 == 8; nothing beside the output view is written."""
    torch = gpu
    for case in range(len(pc.KERNEL_CASES)):
        shape, G, focus = pc.KERNEL_CASES[case]
        n, h, w = shape
        image, depths = pc.inputs(shape)
        depth = depths["noise"]
        count, F = n * h * w, len(POSES)
        ibuf = torch.zeros(3 * count + 8, dtype=torch.uint8, device="cuda")
        iview = ibuf[1:1 + 3 * count]
        iview.copy_(_dev(torch, image).view(-1))
        iview = iview.view(n, h, w, 3)
        dbuf = torch.zeros(count + 4, dtype=torch.uint16, device="cuda")
        dview = dbuf[1:1 + count]
        dview.copy_(_dev(torch, depth).view(-1))
        dview = dview.view(n, h, w)
        kbuf = torch.zeros(F * count + 2, dtype=torch.int64, device="cuda")
        kview = kbuf[1:1 + F * count]
        obuf = torch.full((3 * F * count + 8,), 77, dtype=torch.uint8, device="cuda")
        oview = obuf[3:3 + 3 * F * count].view(n, F, h, w, 3)
        mbuf = torch.full((F * count + 8,), 78, dtype=torch.uint8, device="cuda")
        mview = mbuf[5:5 + F * count].view(n, F, h, w)
        assert iview.data_ptr() % 2 == 1 and dview.data_ptr() % 8 == 2 and oview.data_ptr() % 2 == 1 and kview.data_ptr() % 16 == 8
        focus_t = _dev(torch, np.asarray(pc.focus_list(depth, focus), np.uint16))
        assert _raw(torch, iview, dview, focus_t, _dev(torch, POSES), G, kview, oview, mview) == 0
        want_out, want_mask = pc.want(case, "noise", False)
        assert np.array_equal(oview.cpu().numpy(), want_out) and np.array_equal(mview.cpu().numpy(), want_mask), shape
        assert bool((obuf[:3] == 77).all()) and bool((obuf[3 + 3 * F * count:] == 77).all())
        assert bool((mbuf[:5] == 78).all()) and bool((mbuf[5 + F * count:] == 78).all())
        assert int(kbuf[0]) == 0 and int(kbuf[-1]) == 0


def test_batch_and_view_independence(gpu, monkeypatch):
    """Image 2 of 3 equals that image alone; view k of F equals a call with that pose alone; changing image 0 changes output 0 only;
    a workspace limit that forces the views into several calls gives the same bits."""
    torch = gpu
    from src import _native
    for (h, w), G in (((19, 37), 4), ((33, 16), 8)):
        image = pc.random_image(h, w, h, n=3)
        depth = pc.noise(h, w, w, n=3)
        depth[1] = pc.cliff(h, w, 5)
        focus = [int(depth[0, 0, 0]), int(depth[1].max()), int(depth[2, h // 2, w // 3])]
        y3 = _run(torch, image, depth, POSES, focus, G)
        y1 = _run(torch, image[2:3], depth[2:3], POSES, focus[2:3], G)
        assert torch.equal(y3[0][2:3], y1[0]) and torch.equal(y3[1][2:3], y1[1]), (h, w)
        for k in range(len(POSES)):
            v = _run(torch, image, depth, POSES[k:k + 1], focus, G)
            assert torch.equal(v[0][:, 0], y3[0][:, k]) and torch.equal(v[1][:, 0], y3[1][:, k]), (h, w, k)
        image2, depth2 = image.copy(), depth.copy()
        image2[0] = pc.random_image(h, w, h + 1)
        depth2[0] = pc.noise(h, w, w + 1)
        z3 = _run(torch, image2, depth2, POSES, focus, G)
        assert torch.equal(z3[0][1:], y3[0][1:]) and torch.equal(z3[1][1:], y3[1][1:]) and not torch.equal(z3[0][0], y3[0][0]), (h, w)
        f_t = _dev(torch, np.asarray(focus, np.uint16))                       # the focus values as a device tensor: the same launch
        t3 = _run(torch, image, depth, POSES, f_t, G)
        assert torch.equal(t3[0], y3[0]) and torch.equal(t3[1], y3[1])
        # the view split: room for two views of the batch of 3 (the calls write temporaries), for four views of one image (in place)
        for imgs, deps, foc, whole, per_call in ((image, depth, focus, y3, 2), (image[2:3], depth[2:3], focus[2:3], y1, 4)):
            monkeypatch.setattr(_native, "PARALLAX_WS_BYTES", 8 * len(imgs) * h * w * per_call + 7)
            before = _native.CALLS["ds_parallax_u8"]
            split = _run(torch, imgs, deps, POSES, foc, G)
            assert _native.CALLS["ds_parallax_u8"] == before + -(-len(POSES) // per_call) > before + 1
            assert torch.equal(split[0], whole[0]) and torch.equal(split[1], whole[1]), (h, w, per_call)
            monkeypatch.undo()
        monkeypatch.setattr(_native, "PARALLAX_WS_BYTES", 1)                  # less than one view: one view per call
        before = _native.CALLS["ds_parallax_u8"]
        assert torch.equal(_run(torch, image, depth, POSES, focus, G, want_mask=False), y3[0])
        assert _native.CALLS["ds_parallax_u8"] == before + len(POSES)
        monkeypatch.undo()


def test_a_workspace_full_of_garbage_gives_the_same_bits(gpu):
    """The entry point clears keys itself."""
    torch = gpu
    for case in (1, 3):
        shape, G, focus = pc.KERNEL_CASES[case]
        n, h, w = shape
        image, depths = pc.inputs(shape)
        depth = depths["cliff"]
        F = len(POSES)
        args = (_dev(torch, image), _dev(torch, depth), _dev(torch, np.asarray(pc.focus_list(depth, focus), np.uint16)), _dev(torch, POSES), G)
        want_out, want_mask = pc.want(case, "cliff", False)
        for garbage in (-1, 0x7fffffffffffffff, 0x0001000000000003):
            keys = torch.full((n * F * h * w,), garbage, dtype=torch.int64, device="cuda")
            out = torch.empty((n, F, h, w, 3), dtype=torch.uint8, device="cuda")
            mask = torch.empty((n, F, h, w), dtype=torch.uint8, device="cuda")
            assert _raw(torch, *args, keys, out, mask) == 0
            assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(mask.cpu().numpy(), want_mask), (shape, garbage)


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    ctx = _native.ctx_for(torch.cuda.current_device())
    EINVAL, EUNSUPPORTED, SENT = -1, -2, 93
    n, h, w, F = 1, 8, 12, 2
    count = n * h * w
    targets = count * F
    img = torch.full((n, h, w, 3), 50, dtype=torch.uint8, device="cuda")
    dep = torch.zeros((n, h, w), dtype=torch.int16, device="cuda")
    foc = torch.zeros((4,), dtype=torch.int16, device="cuda")
    pos = torch.tensor([[0, 0, 0], [1024, -1024, 1024], [0, 0, 0]], dtype=torch.int32, device="cuda")
    keys = torch.full((targets + 2,), SENT, dtype=torch.int64, device="cuda")
    out = torch.full((n, F, h, w, 3), SENT, dtype=torch.uint8, device="cuda")
    msk = torch.full((n, F, h, w), SENT, dtype=torch.uint8, device="cuda")
    big = torch.full((64 * count,), SENT, dtype=torch.uint8, device="cuda")   # one block to carve overlapping buffers from
    B = big.data_ptr()
    assert B % 8 == 0 and count % 8 == 0

    def call(c=ctx, ip=img.data_ptr(), dp=dep.data_ptr(), fp=foc.data_ptr(), n=n, h=h, w=w, pp=pos.data_ptr(), F=F, fill=4, invert=0,
             kp=keys.data_ptr(), op=out.data_ptr(), mp=msk.data_ptr()):
        return L.ds_parallax_u8(c, ip, dp, fp, n, h, w, pp, F, fill, invert, kp, op, mp, None)
    assert call(c=None) == EINVAL and call(ip=None) == EINVAL and call(dp=None) == EINVAL and call(fp=None) == EINVAL
    assert call(pp=None) == EINVAL and call(kp=None) == EINVAL and call(op=None) == EINVAL
    assert call(n=0) == EINVAL and call(h=0) == EINVAL and call(w=-3) == EINVAL and call(n=-1) == EINVAL and call(F=0) == EINVAL and call(F=-2) == EINVAL
    assert call(fill=0) == EINVAL and call(fill=65) == EINVAL and call(fill=-1) == EINVAL
    # alignment: keys 8 bytes, poses 4, depth and focus 2
    assert call(kp=keys.data_ptr() + 4) == EINVAL and call(kp=keys.data_ptr() + 1) == EINVAL
    assert call(pp=pos.data_ptr() + 2) == EINVAL and call(pp=pos.data_ptr() + 1) == EINVAL
    assert call(fp=foc.data_ptr() + 1) == EINVAL and call(dp=dep.data_ptr() + 1) == EINVAL
    # out (3 targets bytes) against every input: equal pointers, and beginning in the other's last byte
    assert call(ip=B, op=B) == EINVAL and call(ip=B, op=B + 3 * count - 1) == EINVAL and call(ip=B + 3 * targets - 1, op=B) == EINVAL
    assert call(dp=B, op=B) == EINVAL and call(dp=B, op=B + 2 * count - 1) == EINVAL and call(dp=B + 3 * targets - 2, op=B) == EINVAL
    assert call(fp=B, op=B) == EINVAL and call(fp=B + 2, op=B + 3) == EINVAL and call(fp=B + 3 * targets - 2, op=B) == EINVAL
    assert call(pp=B, op=B) == EINVAL and call(pp=B, op=B + 12 * F - 1) == EINVAL and call(pp=B + 3 * targets - 4, op=B) == EINVAL
    # keys (8 targets bytes) against every input
    assert call(ip=B, kp=B) == EINVAL and call(ip=B + 8 * targets - 1, kp=B) == EINVAL and call(ip=B, kp=B + 3 * count - 8) == EINVAL
    assert call(dp=B, kp=B) == EINVAL and call(dp=B + 8 * targets - 2, kp=B) == EINVAL and call(dp=B, kp=B + 2 * count - 8) == EINVAL
    assert call(fp=B, kp=B) == EINVAL and call(fp=B + 8 * targets - 2, kp=B) == EINVAL
    assert call(pp=B, kp=B) == EINVAL and call(pp=B, kp=B + 8 * F) == EINVAL and call(pp=B + 8 * targets - 4, kp=B) == EINVAL
    # out_mask (targets bytes) against every input
    assert call(ip=B, mp=B) == EINVAL and call(ip=B, mp=B + 3 * count - 1) == EINVAL and call(ip=B + targets - 1, mp=B) == EINVAL
    assert call(dp=B, mp=B) == EINVAL and call(dp=B + targets - 2, mp=B) == EINVAL
    assert call(fp=B, mp=B + 1) == EINVAL and call(pp=B, mp=B + 12 * F - 1) == EINVAL
    # the three among themselves
    assert call(op=B, kp=B) == EINVAL and call(op=B, kp=B + 3 * targets - 8) == EINVAL and call(op=B + 8 * targets - 1, kp=B) == EINVAL
    assert call(op=B, mp=B) == EINVAL and call(op=B, mp=B + 3 * targets - 1) == EINVAL and call(op=B + targets - 1, mp=B) == EINVAL
    assert call(kp=B, mp=B) == EINVAL and call(kp=B, mp=B + 8 * targets - 1) == EINVAL and call(kp=B + targets - 8, mp=B) == EINVAL
    # the size limits: n * F = 65536 one-pixel images (every buffer really that large), a side of 16385
    imn = torch.full((65536, 1, 1, 3), 9, dtype=torch.uint8, device="cuda")
    den = torch.zeros((65536, 1, 1), dtype=torch.int16, device="cuda")
    fon = torch.zeros((65536,), dtype=torch.int16, device="cuda")
    kn = torch.full((65536,), SENT, dtype=torch.int64, device="cuda")
    on = torch.full((65536, 1, 1, 3), SENT, dtype=torch.uint8, device="cuda")
    many = dict(ip=imn.data_ptr(), dp=den.data_ptr(), fp=fon.data_ptr(), kp=kn.data_ptr(), op=on.data_ptr(), mp=None, h=1, w=1)
    assert call(n=65536, F=1, **many) == EUNSUPPORTED and call(n=32768, F=2, **many) == EUNSUPPORTED
    assert b"ds_parallax_u8" in L.ds_last_error()
    assert call(h=1, w=16385) == EUNSUPPORTED and call(h=16385, w=1) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert b"ds_parallax_u8" in L.ds_last_error()
    assert bool((out == SENT).all()) and bool((msk == SENT).all()) and bool((big == SENT).all()) and bool((on == SENT).all())
    assert bool((keys == SENT).all()) and bool((kn == SENT).all())
    # and the legal neighbours of those cases run: the ends of every range, out_mask == NULL, outputs at odd addresses, adjacent but
    # disjoint blocks
    assert call(fill=1) == 0 and call(fill=64) == 0 and call(invert=1) == 0 and call(F=1) == 0 and call(mp=None) == 0
    # out at an odd address, then out_mask, keys, image (odd), depth, focus and poses, each beginning where the one before ends
    # (rounded up to its alignment).  The inputs are the block's own bytes: depth == focus everywhere, so every mask byte becomes 0
    o_at, m_at, k_at = B + 1, B + 1 + 3 * targets, B + 8 + 4 * targets
    i_at = k_at + 8 * targets + 1
    d_at = i_at + 3 * count + 1
    f_at, p_at = d_at + 2 * count, d_at + 2 * count + 2
    assert m_at + targets <= k_at and k_at % 8 == 0 and i_at % 2 == 1 and d_at % 2 == 0 and p_at % 4 == 0 and p_at + 12 * F <= B + big.numel()
    assert call(op=o_at, mp=m_at, kp=k_at, ip=i_at, dp=d_at, fp=f_at, pp=p_at) == 0
    assert call(n=65535, F=1, **many) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((big[m_at - B:m_at - B + targets] == 0).all()) and bool((big[:m_at - B] == SENT).all()) and bool((big[i_at - B:] == SENT).all())
    assert bool((on[:65535] == 9).all()) and bool((on[65535] == SENT).all())
    assert bool((kn[:65535] == 1 << 32).all()) and int(kn[65535]) == keys[-1].item() == keys[-2].item()      # (z + 1) << 32 | 0; the words behind are untouched
    assert bool((out == 50).all()) and bool((msk == 0).all())                # flat depth at the focus: the image, mask 0, written
    assert bool((keys[:targets] >> 32 == 1).all())


def test_public_interface(gpu, tmp_path):
    torch = gpu
    from PIL import Image
    from src import _native
    import src.parallax_generation as pg
    h, w = 12, 20
    image = pc.random_image(h, w, 3)
    d = pc.cliff(h, w, 4)
    x, im = _dev(torch, d)[None], _dev(torch, image)[None]
    for kwargs in ({}, {'path': 'line', 'frames': 5, 'shift': (20.0, -3.0), 'zoom': -0.1, 'focus': 20000, 'fill': 3, 'invert': True},
                   {'path': 'circle', 'frames': 1, 'focus': ('point', 0.9, 0.1)}, {'path': [[3.0, 1.0, 0.0], [-64.0, 64.0, 0.25]], 'fill': 64}):
        path = kwargs.get('path', 'circle')
        shift = kwargs.get('shift', (12.0, 6.0))
        poses = _native.parallax_poses(path, kwargs.get('frames', 24) if isinstance(path, str) else None, shift[0], shift[1], kwargs.get('zoom', 0.04))
        want = pc.model(image, d, kwargs.get('focus', ('point', 0.5, 0.5)), poses.tolist(), kwargs.get('fill', 32), kwargs.get('invert', False))[0]
        batch = pg.create_parallax_batch(im, x, poses, kwargs.get('focus', ('point', 0.5, 0.5)), fill=kwargs.get('fill', 32), invert=kwargs.get('invert', False))
        assert batch.is_cuda and batch.dtype == torch.uint8 and tuple(batch.shape) == (1, len(poses), h, w, 3)
        assert np.array_equal(batch[0].cpu().numpy(), want)
        for pixels in (image, Image.fromarray(image)):
            for depth in (d, Image.fromarray(d)):
                got = pg.create_parallax_frames(pixels, depth, **kwargs)
                assert isinstance(got, list) and len(got) == len(poses)
                assert all(isinstance(f, Image.Image) and f.mode == 'RGB' and f.size == (w, h) for f in got)
                assert np.array_equal(np.stack([np.asarray(f) for f in got]), want)
    frames = pg.create_parallax_frames(image, d)
    assert len({np.asarray(f).tobytes() for f in frames}) > 12                # the camera moves
    name = pg.save_animation(frames, str(tmp_path / "clip.gif"))
    with Image.open(name) as clip:
        assert clip.n_frames == len(frames) == 24 and clip.size == (w, h)
    # every focus form of the binding: one integer (above 32767), a list, a device tensor, a point
    im2, x2 = torch.cat([im, im]), torch.cat([x, x])
    poses = _native.parallax_poses('line', 3, 30.0, 10.0, 0.1)
    two = pg.create_parallax_batch(im2, x2, poses, [2000, 62000], 6)
    for i, f in enumerate((2000, 62000)):
        assert np.array_equal(two[i].cpu().numpy(), pc.model(image, d, f, poses.tolist(), 6)[0])
    assert torch.equal(pg.create_parallax_batch(im2, x2, poses, _dev(torch, np.array([2000, 62000], np.uint16)), 6), two)
    assert torch.equal(pg.create_parallax_batch(im2, x2, poses, 62000, 6)[0], two[1])
    point = pg.create_parallax_batch(im2, x2, poses, ('point', 0.0, 1.0), 6)
    assert np.array_equal(point[1].cpu().numpy(), pc.model(image, d, int(d[h - 1, 0]), poses.tolist(), 6)[0])
    before = dict(_native.CALLS)
    for bad_depth in (d.astype(np.float32), d.astype(np.int32), d.astype(np.uint8), d.astype(np.int16), d.astype(np.float64),
                      Image.fromarray(d.astype(np.uint8)), d[None], d[:0], d[:, :-1], d[:-1]):
        with pytest.raises(_native.DepthStereoError):
            pg.create_parallax_frames(image, bad_depth)
    for bad_image in (image.astype(np.float32), image[..., :2], image[None]):
        with pytest.raises(_native.DepthStereoError):
            pg.create_parallax_frames(bad_image, d)
    for bad in ({'path': 'spiral'}, {'path': None}, {'path': [[65.0, 0, 0]]}, {'path': np.zeros((3, 2))}, {'frames': 0}, {'frames': 257}, {'frames': True},
                {'frames': 2.5}, {'shift': (65.0, 0.0)}, {'shift': 5.0}, {'shift': (1.0, float('nan'))}, {'shift': ('1', 0)}, {'zoom': 0.3},
                {'zoom': float('nan')}, {'zoom': '0'}, {'focus': -1}, {'focus': 65536}, {'focus': ('point', 2.0, 0.5)}, {'focus': 'near'},
                {'fill': 0}, {'fill': 65}, {'fill': True}, {'fill': 2.5}):
        with pytest.raises(_native.DepthStereoError):
            pg.create_parallax_frames(image, d, **bad)
    for bad in ({'fill': 0}, {'fill': 65}, {'fill': True}, {'focus': -1}, {'focus': 65536}, {'focus': ('point', 2.0, 0.5)}, {'focus': 'near'},
                {'focus': [1, 2]}, {'focus': [1.5]}, {'focus': torch.zeros(1, dtype=torch.uint8, device="cuda")},
                {'focus': torch.zeros(2, dtype=torch.int16, device="cuda").view(torch.uint16)},
                {'poses': [[1025, 0, 0]]}, {'poses': [[0, 0, -1025]]}, {'poses': np.zeros((0, 3), np.int32)}, {'poses': np.zeros((2, 2), np.int32)},
                {'poses': np.zeros((2, 3), np.float32)}, {'poses': np.zeros(3, np.int32)}, {'poses': None}, {'poses': 'circle'},
                {'poses': torch.zeros((2, 3), dtype=torch.int32, device="cuda")}):
        args = dict(dict(poses=poses, focus=2000, fill=6), **bad)
        with pytest.raises(_native.DepthStereoError):
            pg.create_parallax_batch(im, x, args['poses'], args['focus'], fill=args['fill'])
    for bad_x in (x.to(torch.int32), x.view(torch.int16), x.to(torch.float32), x[0], x.cpu(), d, x[:, :-1]):
        with pytest.raises(_native.DepthStereoError):
            pg.create_parallax_batch(im, bad_x, poses, 2000)
    for bad_im in (im.to(torch.float32), im[..., :2], im[0], im.cpu(), image):
        with pytest.raises(_native.DepthStereoError):
            pg.create_parallax_batch(bad_im, x, poses, 2000)
    with pytest.raises(_native.DepthStereoError):
        _native.parallax_u8(im, x, poses, 2000, 6, out=torch.empty((1, 3, h, w, 4), dtype=torch.uint8, device="cuda"))
    assert dict(_native.CALLS) == before


def test_funnel_parallax_is_an_option_of_the_call(gpu):
    """core_generation_funnel(..., ops={'parallax': P}) with caller-supplied I;16 depth maps (no network involved)."""
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.parallax_generation as pg
    from src import _native
    h, w = 24, 40
    P = ('circle', 5, 20.0, 8.0, 0.1, ('point', 0.25, 0.5), 6)
    LB = (6, 30.0, ('point', 0.25, 0.5), 200)
    rng = np.random.default_rng(5)
    imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(2)]
    d16 = [pc.cliff(h, w, 1), pc.ramp(h, w, 40)]
    base = {'gen_stereo': True, 'gen_normalmap': True, 'gen_heatmap': True, 'stereo_modes': ['left-right']}
    plain_kinds = ['depth', 'left-right', 'normalmap', 'heatmap']

    def run(ops, opts=base, kinds=plain_kinds, images=imgs):
        got = list(core.core_generation_funnel(None, list(images), [Image.fromarray(d) for d in d16], None, dict(opts), ops))
        assert [(i, k) for i, k, _ in got] == [(i, k) for i in range(2) for k in kinds], [(i, k) for i, k, _ in got]
        for _, k, r in got:
            if k == 'parallax':
                assert isinstance(r, list) and all(isinstance(f, Image.Image) and f.mode == 'RGB' and f.size == (w, h) for f in r)
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
    assert "ds_parallax_u8" not in plain_delta
    own = plain['depth']                                                      # the funnel's own uint16 depth output

    def expect(params, images=imgs):
        kw = dict(path=params[0], frames=params[1], shift=params[2:4], zoom=params[4])
        if len(params) > 5:
            kw['focus'] = params[5]
        if len(params) > 6:
            kw['fill'] = params[6]
        return dict(plain, parallax=[np.stack([np.asarray(f) for f in pg.create_parallax_frames(im, d, **kw)]) for im, d in zip(images, own)])

    want = expect(P)
    poses = _native.parallax_poses(*P[:5]).tolist()
    for got, im, d in zip(want['parallax'], imgs, own):
        assert got.shape == (5, h, w, 3) and np.array_equal(got, pc.model(np.asarray(im), d, P[5], poses, P[6])[0])
        assert not np.array_equal(got[0], np.asarray(im))
    before = dict(_native.CALLS)
    got = run({'parallax': P}, kinds=plain_kinds + ['parallax'])              # after 'heatmap', every other output as it was
    assert same(got, want)
    assert delta(before) == dict(plain_delta, ds_parallax_u8=1)               # one group: one call, nothing else changes
    # gone on the next call; absent, None and {} make the launches and the bytes of a plain call
    for ops in (None, {}, {'parallax': None}):
        before = dict(_native.CALLS)
        assert same(run(ops), plain), ops
        assert delta(before) == plain_delta, ops
    assert same(run({'parallax': list(P[:5])}, kinds=plain_kinds + ['parallax']), expect(P[:5]))         # focus and fill default
    assert same(run({'parallax': P[:6]}, kinds=plain_kinds + ['parallax']), expect(P[:6]))
    # after 'lensblur' when both are asked for
    both = run({'parallax': P, 'lensblur': LB}, kinds=plain_kinds + ['lensblur', 'parallax'])
    assert same({k: both[k] for k in want}, want)
    # alone (the pixels are uploaded for it), and from images that are not RGB (taken as their convert("RGB"))
    only = run({'parallax': P}, {'do_output_depth': False}, ['parallax'])
    assert same(only, {'parallax': want['parallax']})
    rgba = [im.convert('RGBA') for im in imgs]
    assert same(run({'parallax': P}, {'do_output_depth': False}, ['parallax'], images=rgba), {'parallax': want['parallax']})
    assert not hasattr(core.model_holder, 'parallax')                         # the option does not become a holder setting
    for bad in ({'parallax': ('spiral', 5, 1, 1, 0)}, {'parallax': ('circle', 0, 1, 1, 0)}, {'parallax': ('circle', 5, 65.0, 1, 0)},
                {'parallax': ('circle', 5, 1, 1)}, {'parallax': "circle"}, {'parallax': ('circle', 5, 1, 1, 0.3)}, {'parallax': ('circle', True, 1, 1, 0)},
                {'parallax': ('circle', 5, 1, 1, 0, -1)}, {'parallax': ('circle', 5, 1, 1, 0, ('point', 2.0, 0.5))}, {'parallax': ('circle', 5, 1, 1, 0, 0, 65)},
                {'parallax': ('circle', 5, float('nan'), 1, 0)}, {'parallax': {}}):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run(bad)
        assert dict(_native.CALLS) == before, bad                             # before any device work
    assert same(run(None), plain)


def test_funnel_parallax_reads_the_refined_map_and_precedes_the_mesh(gpu, tmp_path):
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.parallax_generation as pg
    h, w = 24, 40
    P, REFINE, LB = ('line', 3, 30.0, 10.0, 0.1, 30000, 8), (5, 60.0, 2.0), (6, 30.0, 9000, 100)
    kw = dict(path='line', frames=3, shift=(30.0, 10.0), zoom=0.1, focus=30000, fill=8)
    rng = np.random.default_rng(6)
    img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    d = pc.cliff(h, w, 2)
    got = list(core.core_generation_funnel(str(tmp_path), [img], [Image.fromarray(d)], None, {'gen_heatmap': True, 'gen_simple_mesh': True},
                                           {'parallax': P, 'lensblur': LB, 'depth_refine': REFINE}))
    assert [k for _, k, _ in got] == ['depth', 'heatmap', 'lensblur', 'parallax', 'simple_mesh']
    refined = np.asarray(got[0][2])
    plain = np.asarray(next(r for _, k, r in core.core_generation_funnel(None, [img], [Image.fromarray(d)], None, {}, None) if k == 'depth'))
    assert not np.array_equal(refined, plain)
    frames = np.stack([np.asarray(f) for f in got[3][2]])
    assert np.array_equal(frames, np.stack([np.asarray(f) for f in pg.create_parallax_frames(img, refined, **kw)]))
    assert not np.array_equal(frames, np.stack([np.asarray(f) for f in pg.create_parallax_frames(img, plain, **kw)]))
