"""The mesh renderer without a GPU: the identities of the definition (include/depthstereo.h, ds_mesh_render_u8) on the NumPy model
tests/mesh_render_cases.py, what the cases contain, camera_path against the closed forms (and scipy's interp1d where it imports),
run_makevideo's string parsing and errors, and the grid width recovered from an OBJ of each keep_edges setting."""
import numpy as np
import pytest

import mesh_render_cases as mc

IDENTITY_SHAPES = ((24, 24), (13, 37), (2, 2), (40, 9))


@pytest.mark.parametrize("shape", IDENTITY_SHAPES, ids=["%dx%d" % s for s in IDENTITY_SHAPES])
def test_pose_zero_returns_the_image(shape):
    """The mesh's own intrinsics, pose 0, keep_edges: every vertex lands on its sample.  s = 1: the image, one hit everywhere.  s > 1 (the
    definition was corrected here: Gouraud shading mixes the neighbours into the samples around a vertex, and the samples outside
    the first and last row and column see nothing): the hit counts of the closed form, every channel within the 3 x 3 neighbourhood's
    range, and an image of one colour comes back on a background of that colour."""
    h, w = shape
    image, depth = mc.random_image(h, w, h), mc.random_depth(h, w, w)
    verts, colors, faces = mc.grid_mesh(image, depth)
    cam = [(0.0, 0.0, 0.0) + mc.intrinsics(h, w)]
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    pad = np.pad(image.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode='edge')
    near = np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    flat = np.full_like(image, 77)
    for s in (1, 2, 3, 4):
        X, Y, iz, live = mc.project(verts, cam[0], s, 0.05)
        assert live.all() and np.array_equal(X, (16 * s * u + 8 * (s - 1)).ravel()) and np.array_equal(Y, (16 * s * v + 8 * (s - 1)).ravel())
        out, hits = mc.model(verts, colors, faces, cam, h, w, s)
        assert np.array_equal(hits[0], mc.identity_hits(h, w, s)), s
        if s == 1:
            assert np.array_equal(out[0], image) and (hits == 1).all()
        assert (out[0] >= np.minimum(near.min(0), 0)).all() and (out[0] <= near.max(0)).all(), s        # the background is (0, 0, 0)
        inner = (slice(1, h - 1), slice(1, w - 1))
        assert (out[0][inner] >= near.min(0)[inner]).all(), s                     # inside, every sample is hit: no background mixed in
        one, _ = mc.model(verts, flat.reshape(-1, 3), faces, cam, h, w, s, background=(77, 77, 77))
        assert np.array_equal(one[0], flat), s


def test_renumbering_the_vertices_changes_nothing():
    for name in ('golden-occluded', 'grid13x37-s3', 'ties', 'malformed-faces'):
        c = mc.case(name)
        n = len(c['verts'])
        perm = np.random.default_rng(n).permutation(n)                           # new index of old vertex i
        inv = np.argsort(perm)
        faces = c['faces'].astype(np.int64)
        valid = (faces >= 0) & (faces < n)
        remapped = np.where(valid, perm[np.where(valid, faces, 0)], np.where(faces < 0, faces, faces))    # bad indices stay bad
        got = mc.model(c['verts'][inv], c['colors'][inv], remapped.astype(np.int64), c['cameras'], c['H'], c['W'], c['s'], c['near'], c['background'])
        assert np.array_equal(got[0], mc.want(name)[0]) and np.array_equal(got[1], mc.want(name)[1]), name


def test_frames_are_independent():
    c = mc.case('golden-5-frames')
    out, hits, _ = mc.want('golden-5-frames')
    for k in (0, 3):
        one = mc.model(c['verts'], c['colors'], c['faces'], c['cameras'][k:k + 1], c['H'], c['W'], c['s'], c['near'], c['background'])
        assert np.array_equal(one[0][0], out[k]) and np.array_equal(one[1][0], hits[k])
    assert len({o.tobytes() for o in out}) == 5


def test_the_cases_contain_what_they_are_for():
    for name in ('grid1x5', 'grid5x1'):
        out, hits, _ = mc.want(name)
        assert len(mc.case(name)['faces']) == 0 and (hits == 0).all() and (out == np.array(mc.case(name)['background'], np.uint8)).all()
    out, hits, census = mc.want('grid2x2')
    assert census['kept'] == 2 and (hits == 1).all() and np.array_equal(out[0], mc.random_image(2, 2, 3))
    # dead vertices of both kinds
    c = mc.case('near-and-far')
    X, Y, iz, live = mc.project(c['verts'], c['cameras'][0], c['s'], c['near'])
    behind = c['verts'][:, 2] - 3.0 < c['near']
    assert 0.2 < behind.mean() < 0.8 and not live[behind].any() and live[~behind].any()
    X, Y, iz, live = mc.project(c['verts'], c['cameras'][1], c['s'], c['near'])
    in_front = c['verts'][:, 2] - 0.93 >= c['near']
    assert (in_front & ~live).any() and live.any()                               # beyond +-16384, and some that stay
    assert all(0 < mc.want('near-and-far')[1][k].mean() for k in (0, 2))
    # the large path and the viewport clip; the dropped face
    assert max(mc.want('two-large-faces')[2]['boxes']) == 64 * 48 and (mc.want('two-large-faces')[1] == 1).all()
    out, hits, census = mc.want('extent-over-2048')
    assert census['kept'] == 1 and 0 < hits.mean() < 2
    # ties: the lower face index wins (face 0 is drawn with the colours of vertices 3..5)
    c = mc.case('ties')
    out, hits, _ = mc.want('ties')
    lone = mc.model(c['verts'], c['colors'], c['faces'][:1], c['cameras'], c['H'], c['W'])[0]
    other = mc.model(c['verts'], c['colors'], c['faces'][1:2], c['cameras'], c['H'], c['W'])[0]
    assert np.array_equal(out[0][:, :16], lone[0][:, :16]) and not np.array_equal(lone, other)
    assert (hits[0][2:15, 16:29] == 1).all()                                     # the quad, its diagonal included, closed on all sides
    c = mc.case('malformed-faces')
    assert mc.want('malformed-faces')[2]['kept'] == 4                            # [0,1,2], both orientations of 5-6-7, [3,1,2]
    assert sorted(mc.want('caps')[2]['boxes']) == list(mc.CAP_BOXES)
    for name in ('golden-stretched', 'golden-occluded'):
        out, hits, _ = mc.want(name)
        assert out.shape == (18, 24, 24, 3) and len({o.tobytes() for o in out}) == 13      # pose 0 comes four times, the end of both lines twice each
    assert mc.want('golden-stretched')[1].mean() > mc.want('golden-occluded')[1].mean()


def test_camera_path_equals_the_closed_forms():
    from src import mesh_render as mr
    eps = np.finfo(np.float64).eps
    try:
        from scipy.interpolate import interp1d
    except ImportError:
        interp1d = None
    for x, y, z in ((0.3, -0.2, 0.5), (-0.015, 0.0, -0.05), (0.0, 0.0, 0.0), (100.0, 1e-3, -7.0)):
        v = np.array([x, y, z])
        tol = 8 * eps * np.abs(v)                                                 # a few ulps of the shift: the forms are sums of three products
        for frames in (1, 2, 3, 7, 24, 240):
            for traj in ('straight-line', 'double-straight-line'):
                got = mr.camera_path(traj, frames, x, y, z)
                assert got.shape == (frames, 3) and got.dtype == np.float64
                assert (np.abs(got - mc.path_closed_form(traj, frames, x, y, z)) <= tol).all(), (traj, frames)
                if interp1d is not None:
                    corners = np.array([[0, 0, 0], [(0 + x) * 0.5, (0 + y) * 0.5, (0 + z) * 0.5], [x, y, z]] if traj == 'straight-line'
                                       else [[-x, -y, -z], [0, 0, 0], [x, y, z]])
                    ref = interp1d(np.linspace(0, 1, 3), corners, axis=0, kind='quadratic')(np.linspace(0, 1, frames))
                    assert (np.abs(got - ref) <= tol).all(), (traj, frames)
            got = mr.camera_path('circle', frames, x, y, z)
            b = np.arange(-2.0, 2.0, 4. / frames)
            want = np.stack([np.cos(b * np.pi) * 1 * x, np.sin(b * np.pi) * 1 * y, np.cos(b * np.pi / 2.) * 1 * z], axis=1)
            assert np.array_equal(got, want) and len(got) == frames
    for bad in (('spiral', 5, 0, 0, 0), ('circle', 0, 0, 0, 0), ('circle', True, 0, 0, 0), ('circle', 2.5, 0, 0, 0), ('circle', 5, float('nan'), 0, 0),
                ('circle', 5, '1', 0, 0), (0, 5, 0, 0, 0), ('circle', 1025, 0, 0, 0)):
        with pytest.raises(ValueError):
            mr.camera_path(*bad)


def test_mesh_render_params():
    from src import _native
    P = _native.mesh_render_params
    assert P(('circle', 5, 1, 2, 3)) == ('circle', 5, 1.0, 2.0, 3.0, False, 1, True)
    assert P(['straight-line', np.int64(1), 0.5, -1, 0, True]) == ('straight-line', 1, 0.5, -1.0, 0.0, True, 1, True)
    assert P(('double-straight-line', 1024, 0, 0, 0, False, 4, False)) == ('double-straight-line', 1024, 0.0, 0.0, 0.0, False, 4, False)
    for bad in ("circle", None, 5, {}, ('circle', 5, 1, 2), ('circle', 5, 1, 2, 3, True, 1, True, 0), ('Circle', 5, 1, 2, 3), (2, 5, 1, 2, 3),
                ('circle', 0, 1, 2, 3), ('circle', 1025, 1, 2, 3), ('circle', True, 1, 2, 3), ('circle', '5', 1, 2, 3), ('circle', 2.5, 1, 2, 3),
                ('circle', 5, float('inf'), 2, 3), ('circle', 5, 1, float('nan'), 3), ('circle', 5, 1, 2, '3'), ('circle', 5, 1, 2, True),
                ('circle', 5, 1, 2, 3, 1), ('circle', 5, 1, 2, 3, 'yes'), ('circle', 5, 1, 2, 3, True, 0), ('circle', 5, 1, 2, 3, True, 5),
                ('circle', 5, 1, 2, 3, True, True), ('circle', 5, 1, 2, 3, True, 1.5), ('circle', 5, 1, 2, 3, True, 1, 0)):
        with pytest.raises(ValueError):
            P(bad)


def test_run_makevideo_parses_like_the_reference(tmp_path):
    from src import mesh_render as mr
    from src import mesh_generation as mg
    v, c, f = mc.grid_mesh(mc.random_image(4, 5, 1), mc.random_depth(4, 5, 2))
    obj = mg.write_obj(str(tmp_path / 'm.obj'), v, f, c)
    args = dict(fn_mesh=obj, vid_numframes=3, vid_fps=10, vid_traj=1, vid_shift="0.1, 0, 0.2", vid_border="0, 0, 0, 0", dolly=False,
                vid_format='gif', vid_ssaa=1)
    for bad, text in ((dict(fn_mesh=''), "Could not open mesh."), (dict(fn_mesh=str(tmp_path / 'absent.obj')), "Could not open mesh."),
                      (dict(vid_shift="0.1, 0"), "Translate requires 3 elements."), (dict(vid_shift="1,2,3,4"), "Translate requires 3 elements."),
                      (dict(vid_border="0, 0, 0"), "Crop Border requires 4 elements.")):
        with pytest.raises(Exception) as e:
            mr.run_makevideo(**dict(args, **bad))
        assert str(e.value) == text
    for bad in (dict(vid_shift="a, 0, 0"), dict(vid_border="0, x, 0, 0"), dict(vid_numframes='many'), dict(vid_ssaa='x'), dict(vid_numframes=0),
                dict(vid_ssaa=5), dict(vid_traj=3), dict(vid_traj='spiral')):
        with pytest.raises(ValueError):
            mr.run_makevideo(**dict(args, **bad))
    for fmt in ('mp4', 'mkv'):
        with pytest.raises(NotImplementedError, match="no video encoder is part of this build"):
            mr.run_makevideo(**dict(args, vid_format=fmt))
    frames = np.arange(2 * 10 * 20 * 3, dtype=np.uint8).reshape(2, 10, 20, 3)
    assert mr.crop_border(frames, [0, 0, 0, 0]) is frames
    assert np.array_equal(mr.crop_border(frames, [0.1, 0.26, 0.35, 0.0]), frames[:, 1:10 - 3, 5:20])        # int(10 * .35) = 3, int(20 * .26) = 5
    with pytest.raises(ValueError):
        mr.crop_border(frames, [0.5, 0, 0.5, 0])


def test_the_grid_width_comes_back_from_an_obj(tmp_path):
    from src import mesh_render as mr
    from src import mesh_generation as mg
    depth = mc.golden_depth()
    image = mc.random_image(24, 24, 2)
    for keep_edges in (True, False):
        v, c, f = mc.grid_mesh(image, depth, keep_edges)
        assert keep_edges == (len(f) == 2 * 23 * 23)
        v2, c2, f2 = mr.read_obj(mg.write_obj(str(tmp_path / ('k%d.obj' % keep_edges)), v, f, c))
        assert np.array_equal(f2, f) and f2.dtype == np.int32 and np.array_equal(c2, c) and c2.dtype == np.uint8
        assert v2.dtype == np.float64 and np.abs(v2 - v).max() <= 0.5e-8
        assert mr.obj_grid_width(len(v2), f2) == 24
    # a mesh whose first kept triangle is of the second kind (br, tr, bl): the first quad's tl vertex is masked out
    h, w = 5, 7
    v, c, f = mc.grid_mesh(mc.random_image(h, w, 3), mc.random_depth(h, w, 4))
    second = f[~(f == 0).any(axis=1)]
    assert second[0].tolist() == [w + 1, 1, w] and mr.obj_grid_width(h * w, second) == w
    for wide in ((3, 11), (11, 3)):
        v, c, f = mc.grid_mesh(mc.random_image(*wide, 3), mc.random_depth(*wide, 4))
        assert mr.obj_grid_width(len(v), f) == wide[1]
    with pytest.raises(ValueError):
        mr.obj_grid_width(5, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError):
        mr.obj_grid_width(35, np.array([[0, 4, 1]], np.int32))                   # 35 % 4 != 0
    with pytest.raises(ValueError):
        mr.obj_grid_width(35, np.array([[3, 3, 1]], np.int32))
