"""Mesh videos: the simple mesh rendered along camera paths, on four HIP kernels.

The reference's "generate video from mesh" tab (run_makevideo -> run_3dphoto_videos -> output_3d_photo, src/core.py:513-667) renders a
clip of a mesh along a 'straight-line', 'double-straight-line' or 'circle' trajectory through vispy / OpenGL, with a dolly zoom, a crop
border and supersampling.  This is the same for the SIMPLE mesh this package builds (src/mesh_generation.py: the occluded or the
stretched one) or any other coloured triangle mesh -- NOT for the inpainted mesh, which is not built here (GEN_INPAINTED_MESH raises).
A triangle rasteriser with a visibility buffer: perspective, any camera translation in front of the near plane, no cracks on stretched
surfaces.  The definition (vertex stage, coverage, depth key, Gouraud resolve) is in include/depthstereo.h, ds_mesh_render_u8;
tests/mesh_render_cases.py is its NumPy model, which the kernels reproduce bit for bit.  Colour is interpolated in screen space (not
perspective-correct); faces that reach behind the near plane are dropped, not clipped; nothing fills the holes behind culled faces.

A camera is (tx, ty, tz, f, cx, cy): a translation in the MESH's units (the simple mesh's depths run from 1 to about 5), the focal
length and principal point in output pixels.  camera_path is the reference's path_planning; the default shift (0.15, 0.0, 0.3) is a
starting point, not a measured optimum.

In the funnel: core_generation_funnel(..., ops={'mesh_video': (traj, frames, shift_x, shift_y, shift_z[, dolly[, ssaa[, keep_edges]]])}).
"""
import os
from pathlib import Path

import numpy as np
from PIL import Image

from . import _native
from . import mesh_generation as mg

TRAJS = _native.MESH_RENDER_TRAJS


def camera_path(traj, frames, x, y, z):
    """The reference's path_planning (inpaint/utils.py:29): float64 [F,3] camera translations.  'straight-line': the parabola through
    (0, 0, 0), (x, y, z) / 2 and (x, y, z) at t = 0, 1/2, 1; 'double-straight-line': through -(x, y, z), 0 and (x, y, z) -- what
    interp1d(kind='quadratic') gives for three knots, in Lagrange form (the knots are collinear and evenly spaced, so both are straight
    lines); t = linspace(0, 1, frames).  'circle': (cos(b pi) x, sin(b pi) y, cos(b pi / 2) z) over b = arange(-2, 2, 4 / frames).
    Raises ValueError."""
    traj, frames, x, y, z = _native.mesh_render_params((traj, frames, x, y, z))[:5]
    if traj == 'circle':
        b = np.arange(-2.0, 2.0, 4.0 / frames)
        return np.stack([np.cos(b * np.pi) * 1 * x, np.sin(b * np.pi) * 1 * y, np.cos(b * np.pi / 2.) * 1 * z], axis=1)
    v = np.array([x, y, z], np.float64)
    p0, p1, p2 = (0.0 * v, 0.5 * v, v) if traj == 'straight-line' else (-v, 0.0 * v, v)
    t = np.linspace(0, 1, frames)[:, None]
    return p0 * (2.0 * (t - 0.5) * (t - 1.0)) + p1 * (-4.0 * t * (t - 1.0)) + p2 * (2.0 * t * (t - 0.5))


def cameras_from_path(track, f, cx, cy, dolly_depth=None):
    """[F,6] camera rows from translations [F,3].  dolly_depth D (the reference's meanLoc): the plane at depth D keeps its width, so
    f_k = f (D - tz_k) / D."""
    track = np.asarray(track, np.float64).reshape(-1, 3)
    fk = np.full(len(track), float(f)) if dolly_depth is None else float(f) * (float(dolly_depth) - track[:, 2]) / float(dolly_depth)
    return np.concatenate([track, fk[:, None], np.full((len(track), 1), float(cx)), np.full((len(track), 1), float(cy))], axis=1)


def _on_device(torch, a, dtype, name):
    """a [*,3] (array or tensor; verts any numbers, faces integers that fit int32, colors uint8) as a contiguous cuda tensor of dtype."""
    try:
        t = a if torch.is_tensor(a) else torch.from_numpy(np.array(a, order='C'))
        kind_ok = (t.dtype == torch.uint8 if name == 'colors' else
                   not t.dtype.is_floating_point and t.dtype != torch.bool if name == 'faces' else t.dtype != torch.bool)
        if t.dim() != 2 or t.shape[1] != 3 or not kind_ok:
            raise TypeError
        if name == 'faces' and t.numel() and not (-2**31 <= int(t.min()) and int(t.max()) < 2**31):
            raise TypeError
    except (TypeError, ValueError, RuntimeError):
        raise _native.DepthStereoError("render_mesh: %s must be [*,3] (verts numbers, faces integers that fit int32, colors uint8), got %s %s"
                                       % (name, getattr(a, 'dtype', type(a)), tuple(getattr(a, 'shape', ())))) from None
    dev = t.device if t.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return t.to(device=dev, dtype=dtype).contiguous()


def render_mesh(verts, faces, colors, cameras, size, ssaa=1, near=0.05, background=(0, 0, 0)):
    """Any coloured triangle mesh through F cameras -> uint8 [F,H,W,3] on the device.  verts [N,3] (taken as float64), faces [M,3]
    integers, colors [N,3] uint8: arrays or tensors; cameras: a host array [F,6] of (tx, ty, tz, f, cx, cy); size = (H, W).  A bad
    argument raises DepthStereoError before any launch."""
    torch = _native.require_gpu()
    try:
        H, W = size
    except (TypeError, ValueError):
        raise _native.DepthStereoError("render_mesh: size must be (H, W), got %r" % (size,)) from None
    return _native.mesh_render_u8(_on_device(torch, verts, torch.float64, 'verts'), _on_device(torch, colors, torch.uint8, 'colors'),
                                  _on_device(torch, faces, torch.int32, 'faces'), cameras, H, W, ssaa, near, background)


def crop_border(frames, border):
    """The reference's crop (inpaint/mesh.py:2505-2511) of finished frames [F,H,W,3]: border = four fractions (top, left, bottom,
    right), each cut int(H b) or int(W b) pixels wide; nothing happens unless one of them is > 0."""
    b = [float(v) for v in border]
    if len(b) != 4:
        raise ValueError("border must hold four fractions (top, left, bottom, right), got %r" % (border,))
    if not any(v > 0.0 for v in b):
        return frames
    H_c, W_c = frames.shape[1:3]
    o_t, o_l, o_b, o_r = int(H_c * b[0]), int(W_c * b[1]), int(H_c * b[2]), int(W_c * b[3])
    cut = frames[:, o_t:H_c - o_b, o_l:W_c - o_r]
    if cut.shape[1] == 0 or cut.shape[2] == 0:
        raise ValueError("border %r leaves nothing of a %d x %d frame" % (border, H_c, W_c))
    return cut


def _grid_cameras(h, w, H, W, track, dolly_depth):
    K = mg.get_intrinsics(h, w)                                                   # 55 degrees, central principal point
    return cameras_from_path(track, float(K[0, 0]) * W / w, float(K[0, 2]) * W / w, float(K[1, 2]) * H / h, dolly_depth)


def _size(size, h, w, who):
    if size is None:
        return h, w
    try:
        H, W = size
        (H, okh), (W, okw) = _native._as_int(H), _native._as_int(W)
        if not (okh and okw and H >= 1 and W >= 1):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise _native.DepthStereoError("%s: size must be (H, W), two integers >= 1, got %r" % (who, size)) from None
    return H, W


def render_mesh_frames(image, depth, traj='double-straight-line', frames=24, shift=(0.15, 0.0, 0.3), dolly=False, ssaa=1,
                       border=(0, 0, 0, 0), keep_edges=True, size=None, background=(0, 0, 0)):
    """A clip of the simple mesh of `image` (PIL or uint8 array, taken as its convert("RGB")) and `depth` (a float array or tensor [h,w]
    in the mesh's units, as mesh_generation.mesh_depth gives them), as a list of PIL RGB images.  The mesh is create_mesh_arrays',
    unchanged (keep_edges=False: the occluded one); the camera has get_intrinsics' 55 degrees, scaled when size = (H, W) differs from
    the depth map's.  shift = (x, y, z) in the mesh's units; dolly: the plane at depth[h // 2, w // 2] keeps its width; border: the
    reference's four crop fractions (crop_border).  With shift 0, ssaa 1 and keep_edges the frames are the image."""
    who = 'render_mesh_frames'
    try:
        if isinstance(shift, (str, bytes)):
            raise TypeError
        x, y, z = shift
        traj, nframes, x, y, z, dolly, ssaa, keep_edges = _native.mesh_render_params((traj, frames, x, y, z, dolly, ssaa, keep_edges))
        border = [float(v) for v in border]
        if len(border) != 4 or not all(0.0 <= v < 1.0 for v in border):
            raise ValueError("border must hold four fractions in [0, 1), got %r" % (border,))
    except (TypeError, ValueError) as e:
        raise _native.DepthStereoError('%s: %s' % (who, e or 'shift must be (x, y, z)')) from None
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    depth_t = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(np.asarray(depth)))
    if depth_t.dim() != 2 or depth_t.numel() == 0 or not depth_t.dtype.is_floating_point:
        raise _native.DepthStereoError('%s: depth must be a non-empty float array [h,w], got %s %s' % (who, depth_t.dtype, tuple(depth_t.shape)))
    if not isinstance(image, Image.Image):
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in (3, 4)):
            raise _native.DepthStereoError('%s: image must be a PIL image or a uint8 array [h,w], [h,w,3] or [h,w,4], got %s %s'
                                           % (who, arr.dtype, arr.shape))
        image = Image.fromarray(np.ascontiguousarray(arr))
    rgb = np.array(image.convert('RGB'), dtype=np.uint8, order='C')
    h, w = depth_t.shape
    if rgb.shape[:2] != (h, w):
        raise _native.DepthStereoError('%s: image is %d x %d, depth map %d x %d (height x width)' % ((who,) + rgb.shape[:2] + (h, w)))
    H, W = _size(size, h, w, who)
    depth_t = depth_t.to(dev)
    out = _render_grid(torch, torch.from_numpy(rgb).to(dev), depth_t, traj, nframes, (x, y, z), dolly, ssaa, keep_edges, H, W, background)
    return [Image.fromarray(f) for f in np.ascontiguousarray(crop_border(out.cpu().numpy(), border))]


def _render_grid(torch, rgb_t, depth_t, traj, frames, shift, dolly, ssaa, keep_edges, H, W, background=(0, 0, 0)):
    """uint8 [F,H,W,3] on the device: the simple mesh of device tensors rgb_t [h,w,3] and depth_t [h,w] along a camera path."""
    h, w = depth_t.shape
    verts, faces, colors = mg.create_mesh_arrays(rgb_t, depth_t, keep_edges=keep_edges)
    D = float(depth_t[h // 2, w // 2]) if dolly else None
    cams = _grid_cameras(h, w, H, W, camera_path(traj, frames, *shift), D)
    return _native.mesh_render_u8(verts.to(torch.float64).contiguous(), colors.contiguous(), faces.to(torch.int32).contiguous(), cams, H, W,
                                  ssaa, 0.05, background)


def read_obj(path):
    """An OBJ that mesh_generation.write_obj wrote ("v x y z r g b" / "f a b c", 1-based): (verts float64 [N,3], colors uint8 [N,3],
    faces int32 [M,3])."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith('v '):
                v.append(line[2:])
            elif line.startswith('f '):
                f.append(line[2:])
    try:
        vc = np.array(' '.join(v).split(), np.float64).reshape(-1, 6)
        faces = (np.array(' '.join(f).split(), np.int64).reshape(-1, 3) - 1).astype(np.int32)
    except ValueError:
        raise ValueError("%s is not an OBJ with 'v x y z r g b' and 'f a b c' lines" % (path,)) from None
    return vc[:, :3].copy(), np.rint(vc[:, 3:] * 255.0).clip(0, 255).astype(np.uint8), faces


def obj_grid_width(n_verts, faces):
    """The width w of the pixel grid a simple mesh was made from: |faces[0][1] - faces[0][0]| (both triangle kinds of create_triangles,
    (tl, bl, tr) and (br, tr, bl), give w there).  ValueError without faces or when N % w != 0."""
    if len(faces) == 0:
        raise ValueError("the mesh has no faces: the grid width cannot be recovered")
    w = abs(int(faces[0][1]) - int(faces[0][0]))
    if w == 0 or n_verts % w != 0:
        raise ValueError("the mesh is no pixel grid: %d vertices, first face %r" % (n_verts, [int(i) for i in faces[0]]))
    return w


def run_makevideo(fn_mesh, vid_numframes, vid_fps, vid_traj, vid_shift, vid_border, dolly, vid_format, vid_ssaa, outpath=None, basename=None):
    """The reference's run_makevideo (src/core.py:614): its name, signature, string parsing and error texts, for an OBJ of the SIMPLE
    mesh as this package's funnel writes it.  vid_traj: 0, 1, 2 = 'straight-line', 'double-straight-line', 'circle'; vid_shift "x, y, z"
    in the mesh's units; vid_border "top, left, bottom, right" fractions; vid_format 'gif', 'webp', 'png' or 'apng' ('mp4' and 'mkv'
    raise NotImplementedError: no encoder is part of this build).  Returns the reference's triple (file, file, '')."""
    if len(fn_mesh) == 0 or not os.path.exists(fn_mesh):
        raise Exception("Could not open mesh.")
    vid_ssaa = int(vid_ssaa)
    if vid_traj in (0, 1, 2) and not isinstance(vid_traj, bool):
        vid_traj = TRAJS[vid_traj]
    num_fps = int(vid_fps)
    num_frames = int(vid_numframes)
    shifts = vid_shift.split(',')
    if len(shifts) != 3:
        raise Exception("Translate requires 3 elements.")
    shift = (float(shifts[0]), float(shifts[1]), float(shifts[2]))
    borders = vid_border.split(',')
    if len(borders) != 4:
        raise Exception("Crop Border requires 4 elements.")
    border = [float(borders[0]), float(borders[1]), float(borders[2]), float(borders[3])]
    if str(vid_format).lower() in ('mp4', 'mkv'):
        raise NotImplementedError("vid_format %r: no video encoder is part of this build; use 'gif', 'webp', 'png' or 'apng'" % (vid_format,))
    traj, num_frames, x, y, z, dolly, vid_ssaa, _ = _native.mesh_render_params((vid_traj, num_frames) + shift + (bool(dolly), vid_ssaa))
    if not outpath:
        outpath = os.path.dirname(os.path.abspath(fn_mesh))
    if not basename:
        stem = Path(fn_mesh).stem
        for i in range(500):
            basename = f"{stem}-{i:04}"
            if not os.path.exists(os.path.join(outpath, basename + '_' + traj + '.' + vid_format)):
                break
    print("Loading mesh ..")
    verts, colors, faces = read_obj(fn_mesh)
    w = obj_grid_width(len(verts), faces)
    h = len(verts) // w
    D = float(verts[(h // 2) * w + w // 2, 2]) if dolly else None                 # the reference's meanLoc: depth[h // 2, w // 2]
    cams = _grid_cameras(h, w, h, w, camera_path(traj, num_frames, x, y, z), D)
    print("Generating videos ..")
    frames = crop_border(render_mesh(verts, faces, colors, cams, (h, w), ssaa=vid_ssaa).cpu().numpy(), border)
    fn = os.path.join(outpath, basename + '_' + traj + '.' + vid_format)
    from .parallax_generation import save_animation
    save_animation([Image.fromarray(f) for f in np.ascontiguousarray(frames)], fn, fps=num_fps)
    return fn, fn, ''
