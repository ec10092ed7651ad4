"""Mesh videos (include/depthstereo.h: ds_mesh_render_u8; src/mesh_render.py; ops={'mesh_video': ...}) against the NumPy model,
tests/mesh_render_cases.py.  Every comparison is np.array_equal / torch.equal: behind the vertex stage the definition is all-integer,
the vertex stage is a handful of separately rounded float64 operations, and the depth test is a maximum, so there is nothing to
tolerate and nothing that depends on the order of the atomics, on small_cap or on the grouping of the frames.
tests/test_mesh_render_cpu.py shows what each case contains."""
import numpy as np
import pytest

import mesh_render_cases as mc

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _run(torch, name, **over):
    from src import _native
    c = dict(mc.case(name), **over)
    return _native.mesh_render_u8(_dev(torch, c['verts']), _dev(torch, c['colors']), _dev(torch, c['faces']), c['cameras'], c['H'], c['W'], c['s'],
                                  c['near'], c['background'], small_cap=c.get('small_cap'), group=c.get('group'), want_hits=True)


def _mismatch(got, want):
    return np.argwhere(got != want)[:6].tolist()


def _same(got, name):
    out, hits, _ = mc.want(name)
    g_out, g_hits = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(g_hits, hits), (name, _mismatch(g_hits, hits))
    assert np.array_equal(g_out, out), (name, _mismatch(g_out, out))


def _raw(torch, c, ws, out, hits=None, small_cap=16, group=None, verts=None, colors=None, faces=None, cams=None):
    """The C entry point on the caller's buffers (the binding allocates the workspace itself)."""
    from src import _native
    F = len(c['cameras'])
    bg = c['background']
    return _native.lib().ds_mesh_render_u8(_native.ctx_for(torch.cuda.current_device()), verts.data_ptr(), colors.data_ptr(), faces.data_ptr(),
                                           len(c['verts']), len(c['faces']), cams.data_ptr(), F, c['H'], c['W'], c['s'], c['near'], bg[0], bg[1], bg[2],
                                           small_cap, ws.data_ptr(), F if group is None else group, out.data_ptr(),
                                           None if hits is None else hits.data_ptr(), None)


@pytest.mark.parametrize("name", mc.CASES)
def test_kernels_equal_the_model_bit_for_bit(gpu, name):
    torch = gpu
    from src import _native
    before = _native.CALLS["ds_mesh_render_u8"]
    got = _run(torch, name)
    assert _native.CALLS["ds_mesh_render_u8"] == before + 1
    c = mc.case(name)
    F = len(c['cameras'])
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.uint8 and got[0].is_cuda and got[1].is_cuda
    assert tuple(got[0].shape) == (F, c['H'], c['W'], 3) and tuple(got[1].shape) == (F, c['H'], c['W'])
    _same(got, name)


def test_small_cap_and_the_large_path_give_the_same_bits(gpu):
    """'caps' holds boxes of 1, 2, 4, 5, 16, 17, 64 and 65 samples: exactly small_cap and small_cap + 1 for the caps 1, 4, 16 and 64;
    small_cap = 0 sends every face to the listed-faces kernel."""
    torch = gpu
    from src import _native
    assert _native.MESH_RENDER_SMALL_CAP in (0, 4, 16, 64)
    for name in ('caps', 'grid13x37-s3', 'golden-occluded', 'malformed-faces', 'two-large-faces'):
        for cap in (0, 1, 4, 16, _native.MESH_RENDER_SMALL_CAP, 64):
            _same(_run(torch, name, small_cap=cap), name)


def test_buffers_at_odd_addresses_give_the_same_bits(gpu):
    """colors, out and out_hits at odd byte addresses, verts and cameras at ptr % 16 == 8, faces at ptr % 8 == 4; nothing beside the
    output views is written."""
    torch = gpu
    from src import _native
    for name in ('grid13x37-s2', 'malformed-faces'):
        c = mc.case(name)
        N, M, F, H, W = len(c['verts']), len(c['faces']), len(c['cameras']), c['H'], c['W']
        vbuf = torch.zeros(3 * N + 2, dtype=torch.float64, device="cuda")
        verts = vbuf[1:1 + 3 * N]
        verts.copy_(_dev(torch, c['verts']).view(-1))
        cbuf = torch.zeros(3 * N + 8, dtype=torch.uint8, device="cuda")
        colors = cbuf[1:1 + 3 * N]
        colors.copy_(_dev(torch, c['colors']).view(-1))
        fbuf = torch.zeros(3 * M + 2, dtype=torch.int32, device="cuda")
        faces = fbuf[1:1 + 3 * M]
        faces.copy_(_dev(torch, c['faces']).view(-1))
        kbuf = torch.zeros(6 * F + 2, dtype=torch.float64, device="cuda")
        cams = kbuf[1:1 + 6 * F]
        cams.copy_(_dev(torch, c['cameras']).view(-1))
        obuf = torch.full((3 * F * H * W + 8,), 77, dtype=torch.uint8, device="cuda")
        out = obuf[3:3 + 3 * F * H * W]
        hbuf = torch.full((F * H * W + 8,), 78, dtype=torch.uint8, device="cuda")
        hits = hbuf[5:5 + F * H * W]
        assert verts.data_ptr() % 16 == 8 and colors.data_ptr() % 2 == 1 and faces.data_ptr() % 8 == 4 and cams.data_ptr() % 16 == 8
        assert out.data_ptr() % 2 == 1 and hits.data_ptr() % 2 == 1
        ws = torch.empty((F * _native.mesh_render_workspace_bytes(N, M, H, W, c['s']),), dtype=torch.uint8, device="cuda")
        assert _raw(torch, c, ws, out, hits, verts=verts, colors=colors, faces=faces, cams=cams) == 0
        _same((out.view(F, H, W, 3), hits.view(F, H, W)), name)
        assert bool((obuf[:3] == 77).all()) and bool((obuf[3 + 3 * F * H * W:] == 77).all())
        assert bool((hbuf[:5] == 78).all()) and bool((hbuf[5 + F * H * W:] == 78).all())


def test_a_poisoned_workspace_gives_the_same_bits(gpu):
    """The memset and the vertex launch write everything a later launch reads: a workspace full of 0xFF, and one of random bytes."""
    torch = gpu
    from src import _native
    for name, group in (('golden-5-frames', 2), ('grid13x37-s2', 2), ('caps', 1), ('near-and-far', 3)):
        c = mc.case(name)
        N, M, F, H, W = len(c['verts']), len(c['faces']), len(c['cameras']), c['H'], c['W']
        args = dict(verts=_dev(torch, c['verts']), colors=_dev(torch, c['colors']), faces=_dev(torch, c['faces']), cams=_dev(torch, c['cameras']))
        nbytes = group * _native.mesh_render_workspace_bytes(N, M, H, W, c['s'])
        noise = torch.from_numpy(np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)).cuda()
        for ws in (torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda"), noise):
            for cap in (0, 16):
                out = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
                hits = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
                assert _raw(torch, c, ws, out, hits, small_cap=cap, group=group, **args) == 0
                _same((out, hits), name)


def test_frames_and_groups_are_independent(gpu):
    """F = 5 with group = 2 (three rounds, the last one short), every other group, a frame alone, and out_hits == NULL."""
    torch = gpu
    from src import _native
    name = 'golden-5-frames'
    c = mc.case(name)
    whole = _run(torch, name)
    for group in (1, 2, 3, 4, 5):
        got = _run(torch, name, group=group)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]), group
    _same(_run(torch, name, group=2), name)
    for k in range(5):
        one = _run(torch, name, cameras=c['cameras'][k:k + 1])
        assert torch.equal(one[0][0], whole[0][k]) and torch.equal(one[1][0], whole[1][k]), k
    alone = _native.mesh_render_u8(_dev(torch, c['verts']), _dev(torch, c['colors']), _dev(torch, c['faces']), c['cameras'], c['H'], c['W'], c['s'],
                                   c['near'], c['background'])
    assert torch.equal(alone, whole[0])
    share = _native.mesh_render_workspace_bytes(len(c['verts']), len(c['faces']), c['H'], c['W'], c['s'])
    assert share > 0 and share % 256 == 0


def test_renumbering_the_vertices_changes_nothing(gpu):
    torch = gpu
    for name in ('golden-occluded', 'grid13x37-s3', 'ties'):
        c = mc.case(name)
        n = len(c['verts'])
        perm = np.random.default_rng(n).permutation(n)                           # the new index of old vertex i
        inv = np.argsort(perm)
        _same(_run(torch, name, verts=c['verts'][inv], colors=c['colors'][inv], faces=perm[c['faces']].astype(np.int32)), name)


def test_entry_point_checks_its_arguments_without_a_launch(gpu):
    torch = gpu
    from src import _native
    L = _native.lib()
    ctx = _native.ctx_for(torch.cuda.current_device())
    EINVAL, EUNSUPPORTED, SENT = -1, -2, 93
    c = mc.case('ties')
    N, M, F, H, W, s = len(c['verts']), len(c['faces']), 2, c['H'], c['W'], 1
    verts, colors, faces = _dev(torch, c['verts']), _dev(torch, c['colors']), _dev(torch, c['faces'])
    cams = _dev(torch, np.repeat(c['cameras'], 3, axis=0))
    share = _native.mesh_render_workspace_bytes(N, M, H, W, s)
    ws = torch.full((F * share + 256,), SENT, dtype=torch.uint8, device="cuda")
    out = torch.full((F, H, W, 3), SENT, dtype=torch.uint8, device="cuda")
    hits = torch.full((F, H, W), SENT, dtype=torch.uint8, device="cuda")
    big = torch.full((4 * F * share,), SENT, dtype=torch.uint8, device="cuda")    # one block to carve overlapping buffers from
    B = big.data_ptr()
    assert B % 256 == 0 and ws.data_ptr() % 256 == 0
    px = H * W

    def call(c_=ctx, vp=verts.data_ptr(), cp=colors.data_ptr(), fp=faces.data_ptr(), N=N, M=M, kp=cams.data_ptr(), F=F, H=H, W=W, s=s, near=0.05,
             bg=(1, 2, 3), cap=16, wp=ws.data_ptr(), group=F, op=out.data_ptr(), hp=hits.data_ptr()):
        return L.ds_mesh_render_u8(c_, vp, cp, fp, N, M, kp, F, H, W, s, near, bg[0], bg[1], bg[2], cap, wp, group, op, hp, None)
    assert call(c_=None) == EINVAL and call(vp=None) == EINVAL and call(cp=None) == EINVAL and call(fp=None) == EINVAL and call(kp=None) == EINVAL
    assert call(wp=None) == EINVAL and call(op=None) == EINVAL
    assert call(N=0) == EINVAL and call(N=-1) == EINVAL and call(M=-1) == EINVAL and call(F=0) == EINVAL and call(H=0) == EINVAL and call(W=-3) == EINVAL
    assert call(s=0) == EINVAL and call(s=5) == EINVAL
    assert call(near=0.0) == EINVAL and call(near=-1.0) == EINVAL and call(near=float('nan')) == EINVAL and call(near=float('inf')) == EINVAL
    assert call(bg=(256, 0, 0)) == EINVAL and call(bg=(0, -1, 0)) == EINVAL and call(bg=(0, 0, 1000)) == EINVAL
    assert call(cap=-1) == EINVAL and call(cap=65) == EINVAL
    assert call(group=0) == EINVAL and call(group=F + 1) == EINVAL
    # alignment: workspace 256 bytes, verts and cameras 8, faces 4
    assert call(wp=ws.data_ptr() + 128) == EINVAL and call(wp=ws.data_ptr() + 8) == EINVAL
    assert call(vp=verts.data_ptr() + 4) == EINVAL and call(kp=cams.data_ptr() + 4) == EINVAL and call(fp=faces.data_ptr() + 2) == EINVAL
    assert b"ds_mesh_render_u8" in L.ds_last_error()
    # out (3 F px bytes), out_hits (F px) and the workspace (group shares) against every input and each other: equal pointers, and
    # beginning in the other's last byte
    for kw, nbytes in ((dict(vp=B), 24 * N), (dict(cp=B), 3 * N), (dict(fp=B), 12 * M), (dict(kp=B), 48 * F)):
        assert call(op=B, **kw) == EINVAL and call(op=B + nbytes - 1, **kw) == EINVAL and call(hp=B, **kw) == EINVAL, kw
        assert call(hp=B + nbytes - 1, **kw) == EINVAL and call(wp=B, **kw) == EINVAL, kw
    assert call(vp=B + F * share - 8, wp=B) == EINVAL and call(cp=B + F * share - 1, wp=B) == EINVAL and call(fp=B + F * share - 4, wp=B) == EINVAL
    assert call(vp=B + 3 * F * px - 8, op=B) == EINVAL and call(cp=B + F * px - 1, hp=B) == EINVAL
    assert call(op=B, hp=B) == EINVAL and call(op=B, hp=B + 3 * F * px - 1) == EINVAL and call(op=B + F * px - 1, hp=B) == EINVAL
    assert call(op=B, wp=B) == EINVAL and call(op=B + F * share - 1, wp=B) == EINVAL and call(hp=B + F * share - 1, wp=B) == EINVAL
    assert call(wp=B + 256, op=B + 255) == EINVAL
    # the size limits
    assert call(H=16385, W=1) == EUNSUPPORTED and call(H=1, W=16385) == EUNSUPPORTED and call(H=8193, W=1, s=2) == EUNSUPPORTED
    assert call(H=4097, W=4, s=4) == EUNSUPPORTED
    assert call(N=2**31) == EUNSUPPORTED and call(M=2**31) == EUNSUPPORTED and call(F=65536, group=1) == EUNSUPPORTED
    assert call(H=16384, W=16384, group=1) == EUNSUPPORTED                        # a share above 2 GiB
    assert b"ds_mesh_render_u8" in L.ds_last_error()
    assert _native.mesh_render_workspace_bytes(N, M, 16384, 16384, 1) == 0 and _native.mesh_render_workspace_bytes(N, M, 16385, 1, 1) == 0
    assert _native.mesh_render_workspace_bytes(0, M, H, W, 1) == 0 and _native.mesh_render_workspace_bytes(N, M, H, W, 5) == 0
    assert L.ds_mesh_render_stages_u8(ctx, verts.data_ptr(), colors.data_ptr(), faces.data_ptr(), N, M, cams.data_ptr(), F, H, W, s, 0.05, 0, 0, 0, 16,
                                      ws.data_ptr(), F, out.data_ptr(), None, 0, None) == EINVAL
    assert L.ds_mesh_render_stages_u8(ctx, verts.data_ptr(), colors.data_ptr(), faces.data_ptr(), N, M, cams.data_ptr(), F, H, W, s, 0.05, 0, 0, 0, 16,
                                      ws.data_ptr(), F, out.data_ptr(), None, 32, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((hits == SENT).all()) and bool((big == SENT).all()) and bool((ws == SENT).all())
    # and the legal neighbours run: the ends of every range, out_hits == NULL, M = 0 with faces == NULL, adjacent but disjoint blocks
    ws4 = torch.empty((_native.mesh_render_workspace_bytes(N, M, H, W, 4),), dtype=torch.uint8, device="cuda")
    assert call(cap=0) == 0 and call(cap=64) == 0 and call(group=1) == 0 and call(s=4, wp=ws4.data_ptr(), group=1) == 0 and call(hp=None) == 0
    assert call(M=0, fp=None) == 0
    torch.cuda.synchronize()
    assert bool((out == torch.tensor([1, 2, 3], dtype=torch.uint8, device="cuda")).all()) and bool((hits == 0).all())
    o_at = B + F * share + 1
    h_at = o_at + 3 * F * px
    assert call(wp=B, op=o_at, hp=h_at) == 0 and call() == 0
    torch.cuda.synchronize()
    want = np.repeat(mc.model(c['verts'], c['colors'], c['faces'], c['cameras'], H, W, 1, 0.05, (1, 2, 3))[0], 2, axis=0)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(big[o_at - B:o_at - B + 3 * F * px].view(F, H, W, 3).cpu().numpy(), want)
    assert bool((big[h_at - B + F * px:] == SENT).all()) and bool((ws[F * share:] == SENT).all())


def test_public_interface(gpu, tmp_path):
    torch = gpu
    from PIL import Image
    import src.core as core
    import src.mesh_render as mr
    from src import _native
    from src import mesh_generation as mg
    depth = mc.golden_depth()
    image = mc.random_image(24, 24, 2)
    f, cx, cy = mc.intrinsics(24, 24)
    # render_mesh: arrays or tensors in, [F,H,W,3] on the device out
    c = mc.case('golden-occluded')
    for conv in (lambda a: a, lambda a: _dev(torch, a), lambda a: torch.from_numpy(np.array(a))):
        got = mr.render_mesh(conv(c['verts']), conv(c['faces'].astype(np.int64)), conv(c['colors']), c['cameras'], (24, 24), background=c['background'])
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), mc.want('golden-occluded')[0])
    c = mc.case('grid13x37-s3')
    got = mr.render_mesh(c['verts'], c['faces'], c['colors'], c['cameras'].tolist(), (31, 40), ssaa=3, near=0.05, background=c['background'])
    assert np.array_equal(got.cpu().numpy(), mc.want('grid13x37-s3')[0])
    # render_mesh_frames: the identity, every option against the model
    still = mr.render_mesh_frames(image, depth, frames=3, shift=(0, 0, 0))
    assert len(still) == 3 and all(isinstance(fr, Image.Image) and fr.mode == 'RGB' and np.array_equal(np.asarray(fr), image) for fr in still)
    for kw in (dict(), dict(traj='circle', frames=5, shift=(0.3, 0.2, -0.4), dolly=True, ssaa=2, keep_edges=False, background=(5, 6, 7)),
               dict(traj='straight-line', frames=4, shift=(-0.2, 0.1, 0.5), size=(31, 40), border=(0.1, 0.0, 0.26, 0.2), ssaa=3)):
        H, W = kw.get('size', (24, 24))
        verts, colors, faces = mc.grid_mesh(image, depth, kw.get('keep_edges', True))
        track = mc.path_closed_form(kw.get('traj', 'double-straight-line'), kw.get('frames', 24), *kw.get('shift', (0.15, 0.0, 0.3)))
        track = mr.camera_path(kw.get('traj', 'double-straight-line'), kw.get('frames', 24), *kw.get('shift', (0.15, 0.0, 0.3)))
        cams = mc.cameras_for(track, *mc.intrinsics(24, 24, H, W), dolly_depth=float(depth[12, 12]) if kw.get('dolly') else None)
        want = mc.model(verts, colors, faces, cams, H, W, kw.get('ssaa', 1), 0.05, kw.get('background', (0, 0, 0)))[0]
        want = mr.crop_border(want, kw.get('border', (0, 0, 0, 0)))
        for pixels in (image, Image.fromarray(image)):
            for dep in (depth, torch.from_numpy(depth), torch.from_numpy(depth).cuda()):
                got = mr.render_mesh_frames(pixels, dep, **kw)
                assert np.array_equal(np.stack([np.asarray(fr) for fr in got]), want), kw
    assert want.shape == (4, 31 - 3 - 8, 40 - 8, 3)
    assert len({np.asarray(fr).tobytes() for fr in mr.render_mesh_frames(image, depth)}) > 12           # the camera moves
    # run_makevideo on an OBJ the funnel wrote
    res = list(core.core_generation_funnel(str(tmp_path), [Image.fromarray(image)], [mc_raw_depth()], None,
                                           {'gen_simple_mesh': True, 'do_output_depth': False}))
    assert [k for _, k, _ in res] == ['simple_mesh']
    obj = res[0][2]
    for fmt, traj, dolly, ssaa, border in (('gif', 1, False, 1, "0, 0, 0, 0"), ('webp', 2, True, 2, "0.1, 0, 0.1, 0.2"), ('png', 0, False, 1, "0,0,0,0")):
        fn, fn2, text = mr.run_makevideo(obj, 5, 10, traj, "0.2, -0.1, 0.3", border, dolly, fmt, ssaa, outpath=str(tmp_path))
        assert fn == fn2 and text == '' and fn.endswith('_' + mr.TRAJS[traj] + '.' + fmt) and str(tmp_path) in fn
        verts, colors, faces = mr.read_obj(obj)
        cams = mc.cameras_for(mr.camera_path(mr.TRAJS[traj], 5, 0.2, -0.1, 0.3), f, cx, cy, dolly_depth=float(verts[12 * 24 + 12, 2]) if dolly else None)
        want = mr.crop_border(mc.model(verts, colors, faces, cams, 24, 24, ssaa)[0], [float(b) for b in border.split(',')])
        with Image.open(fn) as clip:
            assert clip.n_frames == 5 and clip.size == (want.shape[2], want.shape[1])
            if fmt == 'png':                                                      # lossless and unpaletted: the frames themselves
                for k in range(5):
                    clip.seek(k)
                    assert np.array_equal(np.asarray(clip.convert('RGB')), want[k]), k
    again = mr.run_makevideo(obj, 5, 10, 1, "0.2, -0.1, 0.3", "0, 0, 0, 0", False, 'gif', 1, outpath=str(tmp_path))[0]
    assert again.endswith('-0001_double-straight-line.gif')
    assert mr.run_makevideo(obj, 2, 10, 1, "0,0,0", "0,0,0,0", False, 'gif', 1, outpath=str(tmp_path), basename='clip')[0].endswith('clip_double-straight-line.gif')
    # refusals of the binding and the public functions, before any launch
    before = dict(_native.CALLS)
    c = mc.case('ties')
    v, co, fa = _dev(torch, c['verts']), _dev(torch, c['colors']), _dev(torch, c['faces'])
    ok = dict(verts=v, colors=co, faces=fa, cameras=c['cameras'], H=16, W=32)
    for bad in (dict(verts=v.float()), dict(verts=v.cpu()), dict(verts=c['verts']), dict(verts=v[:, :2]), dict(verts=v[:-1]), dict(colors=co.int()),
                dict(faces=fa.long()), dict(faces=fa[:, :2]), dict(faces=fa.cpu()), dict(cameras=None), dict(cameras='circle'), dict(cameras=_dev(torch, c['cameras'])),
                dict(cameras=np.zeros((0, 6))), dict(cameras=np.zeros((2, 5))), dict(cameras=[[0, 0, float('nan'), 1, 0, 0]]),
                dict(cameras=[[0, 0, 0, float('inf'), 0, 0]]), dict(H=0), dict(W=16385), dict(H=True), dict(H=2.5), dict(s=0), dict(s=5), dict(s='1'),
                dict(near=0), dict(near=float('nan')), dict(near='x'), dict(background=(0, 0)), dict(background=(0, 0, 256)), dict(background=(0, 0, 1.5)),
                dict(background=5), dict(small_cap=65), dict(small_cap=-1), dict(small_cap=True), dict(group=0), dict(group=2), dict(group=1.5),
                dict(H=16384, W=16384)):
        with pytest.raises(_native.DepthStereoError):
            _native.mesh_render_u8(**dict(ok, **bad))
    for bad in (dict(traj='spiral'), dict(frames=0), dict(frames=True), dict(shift=(1, 2)), dict(shift='1,2,3'), dict(shift=(0, 0, float('nan'))),
                dict(dolly=1), dict(ssaa=5), dict(ssaa=1.5), dict(keep_edges='yes'), dict(border=(0, 0, 0)), dict(border=(1.0, 0, 0, 0)),
                dict(border=(-0.1, 0, 0, 0)), dict(size=(0, 5)), dict(size=24), dict(size=(24.5, 24))):
        with pytest.raises(_native.DepthStereoError):
            mr.render_mesh_frames(image, depth, **bad)
    for bad_image, bad_depth in ((image[:-1], depth), (image.astype(np.float32), depth), (image, depth.astype(np.int32)), (image, depth[None]),
                                 (image, depth[:0])):
        with pytest.raises(_native.DepthStereoError):
            mr.render_mesh_frames(bad_image, bad_depth)
    for bad in (dict(verts=c['verts'][:, :2]), dict(faces=c['faces'].astype(np.float64)), dict(colors=c['colors'].astype(np.int32)),
                dict(faces=np.array([[0, 1, 2**31]])), dict(size=5)):
        with pytest.raises(_native.DepthStereoError):
            mr.render_mesh(**dict(dict(verts=c['verts'], faces=c['faces'], colors=c['colors'], cameras=c['cameras'], size=(16, 32)), **bad))
    assert dict(_native.CALLS) == before


def mc_raw_depth():
    """The custom depth map test_funnel_simple_mesh hands to the funnel (mesh_depth turns it into mc.golden_depth())."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_cases.npz'))
    return z['c__depth'].astype(np.float64) / 4.0


def test_funnel_mesh_video_is_an_option_of_the_call(gpu, tmp_path):
    """core_generation_funnel(..., ops={'mesh_video': P}) with a caller-supplied depth map (no network involved): the frames are the
    model's of the mesh GEN_SIMPLE_MESH writes, after 'autostereogram' and before 'simple_mesh'; absent, the call is today's."""
    torch = gpu
    from PIL import Image
    import src.core as core
    from src import _native
    image = mc.random_image(24, 24, 2)
    img = Image.fromarray(image)
    base = {'gen_heatmap': True, 'gen_simple_mesh': True}
    P = ('circle', 4, 0.3, 0.2, -0.4, True, 2, False)

    def run(ops, opts=base):
        return list(core.core_generation_funnel(str(tmp_path), [img], [mc_raw_depth()], None, dict(opts), ops))

    def delta(before):
        return {k: v - before.get(k, 0) for k, v in _native.CALLS.items() if v != before.get(k, 0)}

    run(None)                                                                     # (whatever a first call does once is done)
    before = dict(_native.CALLS)
    plain = run(None)
    plain_delta = delta(before)
    assert [k for _, k, _ in plain] == ['depth', 'heatmap', 'simple_mesh'] and "ds_mesh_render_u8" not in plain_delta
    before = dict(_native.CALLS)
    got = run({'mesh_video': P, 'autostereogram': (64, 0.3), 'parallax': ('circle', 3, 4.0, 2.0, 0.02)})
    assert [k for _, k, _ in got] == ['depth', 'heatmap', 'parallax', 'autostereogram', 'mesh_video', 'simple_mesh']
    d = delta(before)
    assert d.pop('ds_mesh_render_u8') == 1 and d.pop('ds_parallax_u8') == 1 and d.pop('ds_autostereogram_u8') == 1 and d == plain_delta
    frames = got[4][2]
    assert isinstance(frames, list) and len(frames) == 4 and all(isinstance(fr, Image.Image) and fr.mode == 'RGB' and fr.size == (24, 24) for fr in frames)
    from src import mesh_generation as mg
    from src import mesh_render as mr
    depth_t = mg.mesh_depth(torch.from_numpy(mc_raw_depth()).cuda(), -1, False, True)        # the mesh as GEN_SIMPLE_MESH builds it
    depth = depth_t.cpu().numpy()
    assert np.allclose(depth, mc.golden_depth(), rtol=0, atol=1e-12)

    def mesh(keep_edges):
        v, f, c = mg.create_mesh_arrays(torch.from_numpy(image).cuda(), depth_t, keep_edges=keep_edges)
        return v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy().astype(np.int32)
    verts, colors, faces = mesh(False)
    cams = mc.cameras_for(mr.camera_path(*P[:5]), *mc.intrinsics(24, 24), dolly_depth=float(depth[12, 12]))
    assert np.array_equal(np.stack([np.asarray(fr) for fr in frames]), mc.model(verts, colors, faces, cams, 24, 24, 2)[0])
    assert np.array_equal(np.asarray(got[0][2]), np.asarray(plain[0][2])) and np.array_equal(np.asarray(got[1][2]), np.asarray(plain[1][2]))
    # alone, with the defaults (stretched mesh, one sample, no dolly), and without the simple mesh
    only = run({'mesh_video': P[:5]}, {'do_output_depth': False})
    assert [k for _, k, _ in only] == ['mesh_video']
    verts, colors, faces = mesh(True)
    cams = mc.cameras_for(mr.camera_path(*P[:5]), *mc.intrinsics(24, 24))
    assert np.array_equal(np.stack([np.asarray(fr) for fr in only[0][2]]), mc.model(verts, colors, faces, cams, 24, 24, 1)[0])
    # gone on the next call; absent, None and {} make the launches of a plain call
    for ops in (None, {}, {'mesh_video': None}):
        before = dict(_native.CALLS)
        assert [k for _, k, _ in run(ops)] == ['depth', 'heatmap', 'simple_mesh'], ops
        assert delta(before) == plain_delta, ops
    assert not hasattr(core.model_holder, 'mesh_video')                           # the option does not become a holder setting
    for bad in ('circle', ('circle', 4, 0.3, 0.2), ('spiral', 4, 0, 0, 0), ('circle', 0, 0, 0, 0), ('circle', True, 0, 0, 0), ('circle', 4, float('nan'), 0, 0),
                ('circle', 4, 0, 0, 0, 1), ('circle', 4, 0, 0, 0, True, 5), ('circle', 4, 0, 0, 0, True, 1, 'no'), {}, ('circle', 4, 0, 0, 0, True, 1, True, 1)):
        before = dict(_native.CALLS)
        with pytest.raises(ValueError):
            run({'mesh_video': bad})
        assert dict(_native.CALLS) == before, bad                                 # before any device work
