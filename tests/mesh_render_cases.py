"""Shared by tests/test_mesh_render_cpu.py and tests/test_gpu_mesh_render.py: the NumPy MODEL of the mesh renderer (include/depthstereo.h:
the comment of ds_mesh_render_u8 is the definition) and the seeded cases.

The model is written from the definition alone: the vertex stage in float64 NumPy (every operation rounds on its own), the faces in
int64, batched by the size of their bounding boxes (one np.maximum.at per batch), the resolve as one gather over all samples.  It shares
no code with the product and no structure with the kernels (a thread per face, a list of large faces, a wave per listed face, atomics)."""
import functools
import os

import numpy as np

EXTENT_MAX = 2048 * 16
COORD_MAX = 16384.0
U32 = 0xFFFFFFFF


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def project(verts, cam, s, near):
    """(X, Y int64 [N], iz int64 [N], live bool [N]) of the vertices under one camera row (tx, ty, tz, f, cx, cy)."""
    verts = np.asarray(verts, np.float64)
    cam = np.asarray(cam, np.float64)
    n = len(verts)
    if not np.isfinite(cam).all():
        return np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    tx, ty, tz, f, cx, cy = cam
    with np.errstate(all='ignore'):
        xc, yc, zc = verts[:, 0] - tx, verts[:, 1] - ty, verts[:, 2] - tz
        live = zc >= near
        sx = cx - (f * xc) / zc
        sy = cy - (f * yc) / zc
        sx = sx * float(s) + (s - 1) * 0.5
        sy = sy * float(s) + (s - 1) * 0.5
        live &= np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= COORD_MAX) & (np.abs(sy) <= COORD_MAX)
        sx, sy = np.where(live, sx, 0.0), np.where(live, sy, 0.0)
        q = np.floor((near / np.where(live, zc, 1.0)) * 2147483648.0)
    X, Y = np.rint(16.0 * sx).astype(np.int64), np.rint(16.0 * sy).astype(np.int64)
    iz = np.maximum(1, q.astype(np.int64))
    assert (iz[live] <= 2**31).all()
    return X, Y, iz, live


def _weights(Xa, Ya, Xb, Yb, Xc, Yc, A, PX, PY):
    """w0, w1, w2 and the flipped A (> 0) at the sample points, all int64 and broadcast."""
    w0 = (Xb - PX) * (Yc - PY) - (Yb - PY) * (Xc - PX)
    w1 = (Xc - PX) * (Ya - PY) - (Yc - PY) * (Xa - PX)
    sign = np.where(A < 0, -1, 1)
    w0, w1, A = w0 * sign, w1 * sign, A * sign
    return w0, w1, A - w0 - w1, A


def raster(X, Y, iz, live, faces, Hs, Ws, census=None):
    """keys uint64 [Hs, Ws] of one frame."""
    keys = np.zeros(Hs * Ws, np.uint64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(X)
    t = np.arange(len(faces), dtype=np.int64)
    ok = ((faces >= 0) & (faces < n)).all(axis=1)
    fc = np.where(ok[:, None], faces, 0)
    ok &= live[fc].all(axis=1)
    Xf, Yf = X[fc], Y[fc]                                                          # [M, 3]
    A = (Xf[:, 1] - Xf[:, 0]) * (Yf[:, 2] - Yf[:, 0]) - (Yf[:, 1] - Yf[:, 0]) * (Xf[:, 2] - Xf[:, 0])
    ok &= A != 0
    ok &= (Xf.max(1) - Xf.min(1) <= EXTENT_MAX) & (Yf.max(1) - Yf.min(1) <= EXTENT_MAX)
    x0, x1 = np.maximum(-((-Xf.min(1)) // 16), 0), np.minimum(Xf.max(1) // 16, Ws - 1)     # ceil and floor of the sixteenths
    y0, y1 = np.maximum(-((-Yf.min(1)) // 16), 0), np.minimum(Yf.max(1) // 16, Hs - 1)
    ok &= (x1 >= x0) & (y1 >= y0)
    if census is not None:
        census['kept'] = census.get('kept', 0) + int(ok.sum())
        census['boxes'] = census.get('boxes', []) + ((x1 - x0 + 1) * (y1 - y0 + 1))[ok].tolist()
    sel = np.flatnonzero(ok)
    nx, ny = (x1 - x0 + 1)[sel], (y1 - y0 + 1)[sel]
    side = np.maximum(nx, ny)
    done = np.zeros(len(sel), bool)
    for B in (2, 4, 8, 16, 64, None):                                               # None: what is left, face by face
        if B is None:
            batches = [np.array([i]) for i in np.flatnonzero(~done)]
        else:
            pick = np.flatnonzero(~done & (side <= B))
            done[pick] = True
            step = max(1, (1 << 18) // (B * B))
            batches = [pick[i:i + step] for i in range(0, len(pick), step)]
        for b in batches:
            if len(b) == 0:
                continue
            f = sel[b]
            bw, bh = int(nx[b].max()), int(ny[b].max())
            oy, ox = np.mgrid[0:bh, 0:bw].astype(np.int64)
            px, py = x0[f][:, None, None] + ox, y0[f][:, None, None] + oy
            inside = (ox < nx[b][:, None, None]) & (oy < ny[b][:, None, None])
            g = lambda a, i: a[f, i][:, None, None]
            w0, w1, w2, Ap = _weights(g(Xf, 0), g(Yf, 0), g(Xf, 1), g(Yf, 1), g(Xf, 2), g(Yf, 2), A[f][:, None, None], 16 * px, 16 * py)
            cover = inside & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
            izf = iz[fc[f]]
            num = w0 * izf[:, 0][:, None, None] + w1 * izf[:, 1][:, None, None] + w2 * izf[:, 2][:, None, None]
            assert (np.abs(np.where(inside, w0, 0)) <= 2**31).all() and (Ap <= 2**30).all() and (num[cover] <= 2**61).all()
            izp = np.where(cover, num, 0) // Ap
            assert (izp[cover] >= 1).all() and (izp[cover] <= 2**31).all()
            key = (izp.astype(np.uint64) << np.uint64(32)) | (U32 - t[f]).astype(np.uint64)[:, None, None]
            np.maximum.at(keys, (py * Ws + px)[cover], key[cover])
    return keys.reshape(Hs, Ws)


def resolve(keys, X, Y, faces, colors, H, W, s, background):
    """(out uint8 [H, W, 3], hits uint8 [H, W]) of one frame from its keys."""
    Hs, Ws = keys.shape
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    colors = np.asarray(colors).astype(np.int64)
    hit = keys != 0
    samples = np.empty((Hs, Ws, 3), np.int64)
    samples[:] = np.asarray(background, np.int64)
    if hit.any():
        py, px = np.nonzero(hit)
        t = U32 - (keys[hit] & np.uint64(U32)).astype(np.int64)
        a, b, c = faces[t, 0], faces[t, 1], faces[t, 2]
        A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
        w0, w1, w2, A = _weights(X[a], Y[a], X[b], Y[b], X[c], Y[c], A, 16 * px, 16 * py)
        assert (w0 >= 0).all() and (w1 >= 0).all() and (w2 >= 0).all() and (A > 0).all()
        samples[hit] = (w0[:, None] * colors[a] + w1[:, None] * colors[b] + w2[:, None] * colors[c] + (A // 2)[:, None]) // A[:, None]
    total = samples.reshape(H, s, W, s, 3).sum(axis=(1, 3))
    out = (total + (s * s) // 2) // (s * s)
    return out.astype(np.uint8), hit.reshape(H, s, W, s).sum(axis=(1, 3)).astype(np.uint8)


def model(verts, colors, faces, cameras, H, W, s=1, near=0.05, background=(0, 0, 0), census=None):
    """(out uint8 [F, H, W, 3], hits uint8 [F, H, W])."""
    cameras = np.asarray(cameras, np.float64).reshape(-1, 6)
    outs, hits = [], []
    for cam in cameras:
        X, Y, iz, live = project(verts, cam, s, near)
        keys = raster(X, Y, iz, live, faces, s * H, s * W, census)
        o, h = resolve(keys, X, Y, faces, colors, H, W, s, background)
        outs.append(o)
        hits.append(h)
    return np.stack(outs), np.stack(hits)


def identity_hits(h, w, s):
    """out_hits of the pose-0 identity (include/depthstereo.h): n(u, w) n(v, h), n = s inside and (s + 1) // 2 (the vertex's own sample
    and what lies on the mesh's side of it) on a first or last index."""
    def n(m):
        v = np.full(m, s)
        v[0] = v[-1] = (s + 1) // 2 if s % 2 else s // 2
        return v
    return (n(h)[:, None] * n(w)[None, :]).astype(np.uint8)


# ---- camera paths: the closed forms of the reference's path_planning (inpaint/utils.py:29) -------------------------------------------------
def path_closed_form(traj, frames, x, y, z):
    """float64 [F, 3].  The two line kinds are the parabola through three collinear, evenly spaced knots: a straight line."""
    v = np.array([x, y, z], np.float64)
    if traj == 'circle':
        b = np.arange(-2.0, 2.0, 4.0 / frames)
        return np.stack([np.cos(b * np.pi) * x, np.sin(b * np.pi) * y, np.cos(b * np.pi / 2.0) * z], axis=1)
    t = np.linspace(0, 1, frames)[:, None]
    return v * t if traj == 'straight-line' else v * (2.0 * t - 1.0)


TRAJS = ('straight-line', 'double-straight-line', 'circle')


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def grid_mesh(image, depth, keep_edges=True):
    """The simple mesh of an image [h, w, 3] uint8 and a float64 depth [h, w], through the package's own create_mesh_arrays on the CPU:
    (verts float64 [N, 3], colors uint8 [N, 3], faces int32 [M, 3])."""
    import torch
    from src import mesh_generation as mg
    v, f, c = mg.create_mesh_arrays(torch.from_numpy(np.ascontiguousarray(image)), torch.from_numpy(np.ascontiguousarray(depth, np.float64)),
                                    keep_edges=keep_edges)
    return v.numpy().copy(), np.ascontiguousarray(c.numpy()), f.numpy().astype(np.int32).reshape(-1, 3)


def intrinsics(h, w, H=None, W=None):
    """(f, cx, cy) of the mesh's own 55-degree camera, scaled to an H x W output."""
    from src import mesh_generation as mg
    K = mg.get_intrinsics(h, w)
    H, W = h if H is None else H, w if W is None else W
    return float(K[0, 0]) * W / w, float(K[0, 2]) * W / w, float(K[1, 2]) * H / h


def cameras_for(track, f, cx, cy, dolly_depth=None):
    """[F, 6] from translations [F, 3]; dolly_depth D: f_k = f (D - tz_k) / D."""
    track = np.asarray(track, np.float64).reshape(-1, 3)
    fk = np.full(len(track), f) if dolly_depth is None else f * (dolly_depth - track[:, 2]) / dolly_depth
    return np.concatenate([track, fk[:, None], np.full((len(track), 1), cx), np.full((len(track), 1), cy)], axis=1)


def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def random_depth(h, w, seed):
    return np.random.default_rng(seed).uniform(1.0, 5.0, (h, w))


def golden_depth():
    """The 24 x 24 depth of tests/golden/mesh_cases.npz as test_funnel_simple_mesh feeds it to the mesh: c__depth / 4 through mesh_depth."""
    import torch
    from src import mesh_generation as mg
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_cases.npz'))
    return mg.mesh_depth(torch.from_numpy(z['c__depth'].astype(np.float64) / 4.0), -1, False, True).numpy()


def screen_mesh(points, faces, colors_seed):
    """A general mesh from screen positions: points [(sx, sy, z)] seen by the camera (0, 0, 0, 1, 0, 0) land on (sx, sy) exactly when
    sx z is exact in float64 (small integers and powers of two here)."""
    p = np.asarray(points, np.float64)
    verts = np.stack([-p[:, 0] * p[:, 2], -p[:, 1] * p[:, 2], p[:, 2]], axis=1)
    colors = np.random.default_rng(colors_seed).integers(0, 256, (len(p), 3), dtype=np.uint8)
    return verts, colors, np.asarray(faces, np.int32).reshape(-1, 3)


UNIT_CAMERA = [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0]]
CAP_BOXES = (1, 2, 4, 5, 16, 17, 64, 65)                 # the sample counts of the boxes of the 'caps' case, in face order


def _golden_case(keep_edges, frames=3):
    depth = golden_depth()
    verts, colors, faces = grid_mesh(random_image(24, 24, 2), depth, keep_edges)
    f, cx, cy = intrinsics(24, 24)
    D = float(depth[12, 12])
    cams = [cameras_for(path_closed_form(traj, frames, 0.35, -0.2, 0.4), f, cx, cy, D if dolly else None) for traj in TRAJS for dolly in (False, True)]
    return dict(verts=verts, colors=colors, faces=faces, cameras=np.concatenate(cams), H=24, W=24, s=1, background=(9, 200, 31))


def _caps_case():
    pts, faces = [], []
    for x, y, dx, dy in ((5, 5, .5, .5), (7, 7, 1.5, .5), (10, 10, 1.5, 1.5), (14, 14, 4.5, .5), (20, 20, 3.5, 3.5), (1, 30, 16.5, .5),
                         (30, 1, 7.5, 7.5), (0, 40, 64.5, .5)):
        faces.append([len(pts), len(pts) + 1, len(pts) + 2])
        pts += [(x, y, 2.0), (x + dx, y, 4.0), (x, y + dy, 2.0)]
    verts, colors, faces = screen_mesh(pts, faces, 17)
    return dict(verts=verts, colors=colors, faces=faces, cameras=UNIT_CAMERA, H=44, W=70, s=1, background=(1, 2, 3))


def _case(name):
    if name == 'grid2x2':
        verts, colors, faces = grid_mesh(random_image(2, 2, 3), random_depth(2, 2, 4))
        return dict(verts=verts, colors=colors, faces=faces, cameras=[(0.0, 0.0, 0.0) + intrinsics(2, 2)], H=2, W=2, s=1)
    if name in ('grid1x5', 'grid5x1'):
        h, w = (1, 5) if name == 'grid1x5' else (5, 1)
        verts, colors, faces = grid_mesh(random_image(h, w, 5), random_depth(h, w, 6))
        assert len(faces) == 0
        return dict(verts=verts, colors=colors, faces=faces, cameras=[(0.0, 0.0, 0.0) + intrinsics(h, w)], H=h, W=w, s=2, background=(7, 8, 9))
    if name in ('golden-stretched', 'golden-occluded'):
        return _golden_case(name == 'golden-stretched')
    if name == 'golden-5-frames':
        c = _golden_case(True)
        return dict(c, cameras=c['cameras'][[0, 4, 8, 13, 17]])
    if name.startswith('grid13x37-s'):
        s = int(name[-1])
        verts, colors, faces = grid_mesh(random_image(13, 37, 7), random_depth(13, 37, 8))
        f, cx, cy = intrinsics(13, 37, 31, 40)
        return dict(verts=verts, colors=colors, faces=faces, cameras=cameras_for([(0, 0, 0), (0.4, -0.3, 0.5)], f, cx, cy), H=31, W=40, s=s,
                    background=(255, 0, 128))
    if name == 'near-and-far':
        # tz = 3: about half of the depths (1..5) lie behind the near plane; tz = 0.93 with near = 0.05: the nearest vertices get a zc of a few
        # hundredths and leave the +-16384 range
        verts, colors, faces = grid_mesh(random_image(13, 37, 9), random_depth(13, 37, 10))
        f, cx, cy = intrinsics(13, 37)
        return dict(verts=verts, colors=colors, faces=faces, cameras=cameras_for([(0, 0, 3.0), (90.0, 40.0, 0.93), (0.1, 0, 0.5)], f, cx, cy),
                    H=13, W=37, s=2, near=0.05)
    if name == 'two-large-faces':
        verts, colors, faces = screen_mesh([(-500, -300, 2.0), (700, -300, 4.0), (-500, 600, 1.0), (700, 600, 8.0)], [[0, 2, 1], [3, 1, 2]], 11)
        return dict(verts=verts, colors=colors, faces=faces, cameras=UNIT_CAMERA, H=48, W=64, s=1)
    if name == 'extent-over-2048':
        verts, colors, faces = screen_mesh([(-1100, 0, 1.0), (1100, 10, 1.0), (0, 40, 1.0), (2, 2, 4.0), (30, 4, 4.0), (5, 20, 4.0)],
                                           [[0, 1, 2], [3, 4, 5]], 12)
        return dict(verts=verts, colors=colors, faces=faces, cameras=UNIT_CAMERA, H=24, W=32, s=2, background=(50, 60, 70))
    if name == 'ties':
        # faces 0 and 1: the same triangle twice, other colours; faces 2 and 3: one depth, the shared diagonal runs through sample points
        tri = [(2, 2, 2.0), (14, 3, 2.0), (4, 13, 2.0)]
        quad = [(16, 2, 4.0), (28, 2, 4.0), (16, 14, 4.0), (28, 14, 4.0)]
        verts, colors, faces = screen_mesh(tri + tri + quad, [[3, 4, 5], [0, 1, 2], [6, 8, 7], [9, 7, 8]], 13)
        return dict(verts=verts, colors=colors, faces=faces, cameras=UNIT_CAMERA, H=16, W=32, s=1)
    if name == 'malformed-faces':
        pts = [(2, 2, 2.0), (12, 2, 2.0), (2, 12, 2.0), (12, 12, 3.0), (7, 7, 2.0), (20, 3, 1.0), (30, 5, 1.0), (22, 14, 1.0)]
        faces = [[0, 4, 3], [0, 0, 1], [1, 2, 2], [0, 1, 2], [5, 7, 6], [5, 6, 7], [-1, 1, 2], [0, 8, 2], [3, 1, 2], [0, 1, 2**31 - 1],
                 [-2**31, 5, 6]]
        verts, colors, faces = screen_mesh(pts, faces, 14)
        return dict(verts=verts, colors=colors, faces=faces, cameras=UNIT_CAMERA, H=16, W=32, s=3)
    if name == 'caps':
        return _caps_case()
    raise KeyError(name)


CASES = ('grid2x2', 'grid1x5', 'grid5x1', 'golden-stretched', 'golden-occluded', 'golden-5-frames', 'grid13x37-s1', 'grid13x37-s2',
         'grid13x37-s3', 'grid13x37-s4', 'near-and-far', 'two-large-faces', 'extent-over-2048', 'ties', 'malformed-faces', 'caps')


@functools.lru_cache(maxsize=None)
def case(name):
    """The arguments of one case as a dict (verts, colors, faces, cameras, H, W, s, near, background); arrays read-only, computed once."""
    c = dict(dict(near=0.05, background=(0, 0, 0)), **_case(name))
    c['cameras'] = np.asarray(c['cameras'], np.float64).reshape(-1, 6)
    c['faces'] = np.ascontiguousarray(c['faces'], np.int32).reshape(-1, 3)
    for k in ('verts', 'colors', 'faces', 'cameras'):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(name):
    """The model's (out, hits, census) of a case, computed once; read-only."""
    census = {}
    out, hits = model(census=census, **case(name))
    out.setflags(write=False)
    hits.setflags(write=False)
    return out, hits, census
