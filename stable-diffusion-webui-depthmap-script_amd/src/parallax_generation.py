"""Parallax frames from depth: short camera-motion clips of an image by its uint16 depth map, on two HIP kernels.

The reference renders such clips (GEN_INPAINTED_MESH_DEMOS: circle, swing, zoom-in, dolly-zoom-in) from a layered mesh, three
inpainting networks and an OpenGL renderer, none of which is built here.  This is the image-space renderer for SMALL camera motions:
every source pixel is pushed to where it lands in the new view, the nearest pixel wins each target pixel, and the disocclusion holes
are closed from the background side -- a smear that is good for a few pixels of disocclusion, not for walking around an object.  The
definition (landing point, footprint, depth test, hole filling -- all in integers) is in include/depthstereo.h, ds_parallax_u8;
tests/parallax_cases.py is its NumPy model, which the kernels reproduce bit for bit.

A camera position is (x, y, z): x and y the shift in PIXELS, z the change of scale as a fraction, that a depth difference of the full
uint16 range would get; a pixel at the focus depth does not move.  camera_path makes the positions of a clip:
    'circle'  (X cos a, Y sin a, Z cos a), a = 2 pi k / frames  (Y = 0: the reference's "swing")
    'line'    from (-X, -Y, -Z) to (X, Y, Z)                   (X = Y = 0: a zoom)
with shift = (X, Y) and zoom = Z; |shift| <= 64, |zoom| <= 0.25, 1 <= frames <= 256.  focus: a depth 0..65535 in the map's own units,
or ('point', fx, fy) with fx, fy in [0, 1]: the depth found at that position of the image.  fill: 1..64 pixels, how far a hole looks
for its background.  invert: black is near (the funnel's maps are white = near).  The defaults ('circle', 24, (12.0, 6.0), 0.04,
('point', 0.5, 0.5), 32) are starting points, not measured optima.  Only uint16 maps are accepted: the displacement is defined on
integer depth differences.

In the funnel: core_generation_funnel(..., ops={'parallax': (path, frames, shift_x, shift_y, zoom[, focus[, fill]])}).
"""
import os

import numpy as np
from PIL import Image

from . import _native


def _params(path, frames, shift, zoom, focus, fill, who):
    try:
        if isinstance(shift, (str, bytes)):
            raise ValueError("parallax: shift must be (shift_x, shift_y), got %r" % (shift,))
        try:
            shift_x, shift_y = shift
        except (TypeError, ValueError):
            raise ValueError("parallax: shift must be (shift_x, shift_y), got %r" % (shift,)) from None
        return _native.parallax_params((path, frames, shift_x, shift_y, zoom, focus, fill))
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None


def camera_path(kind, frames, shift=(12.0, 6.0), zoom=0.04):
    """The camera positions of a clip: float64 [frames,3] of (x, y, z) as above.  kind: 'circle' or 'line'.  A bad argument raises
    DepthStereoError."""
    if not isinstance(kind, str):
        raise _native.DepthStereoError("camera_path: kind must be one of %r, got %r" % (_native.PARALLAX_PATHS, kind))
    path, frames, shift_x, shift_y, zoom, _, _ = _params(kind, frames, shift, zoom, 0, 1, 'camera_path')
    return _native.parallax_path(path, frames, shift_x, shift_y, zoom)


def create_parallax_frames(image, depthmap, path='circle', frames=24, shift=(12.0, 6.0), zoom=0.04, focus=('point', 0.5, 0.5), fill=32,
                           invert=False):
    """image: PIL image or uint8 array (taken as its convert("RGB")); depthmap: uint16 array [h,w] or an 'I;16' image of the same size.
    path: 'circle' or 'line', or an explicit array [F,3] of camera positions (then `frames`, `shift` and `zoom` are not used).
    Returns the frames as a list of PIL RGB images.  Non-uint16 depth, a size mismatch or a bad parameter raises DepthStereoError
    before any launch."""
    if not isinstance(path, (str, bytes)) and path is not None:
        frames = None
    path, frames, shift_x, shift_y, zoom, focus, fill = _params(path, frames, shift, zoom, focus, fill, 'create_parallax_frames')
    if isinstance(depthmap, Image.Image):
        if depthmap.mode != 'I;16':
            raise _native.DepthStereoError("create_parallax_frames: a depth image must have mode 'I;16' (uint16), got %r" % (depthmap.mode,))
        depth = np.asarray(depthmap, dtype=np.uint16)
    else:
        depth = np.asarray(depthmap)
    if depth.ndim != 2 or depth.dtype != np.uint16 or depth.size == 0:
        raise _native.DepthStereoError('create_parallax_frames: depthmap must be a non-empty 2-D uint16 array (the displacement is defined '
                                       'on integer depth differences), got %s %s' % (depth.dtype, depth.shape))
    if not isinstance(image, Image.Image):
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in (3, 4)):
            raise _native.DepthStereoError('create_parallax_frames: image must be a PIL image or a uint8 array [h,w], [h,w,3] or [h,w,4], '
                                           'got %s %s' % (arr.dtype, arr.shape))
        image = Image.fromarray(np.ascontiguousarray(arr))
    rgb = np.asarray(image.convert('RGB'), dtype=np.uint8)
    if rgb.shape[:2] != depth.shape:
        raise _native.DepthStereoError('create_parallax_frames: image is %d x %d, depth map %d x %d (height x width)'
                                       % (rgb.shape[:2] + depth.shape))
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    out = _native.parallax_u8(torch.from_numpy(np.array(rgb, order='C')).to(dev).unsqueeze(0),
                              torch.from_numpy(np.array(depth, order='C')).to(dev).unsqueeze(0),
                              _native.parallax_poses(path, frames, shift_x, shift_y, zoom), focus, fill, invert=bool(invert))
    return [Image.fromarray(f) for f in out[0].cpu().numpy()]                # uint8 [h,w,3] each: mode 'RGB'


def create_parallax_batch(image_u8, depth_u16, poses, focus, fill=32, invert=False):
    """image_u8 [n,h,w,3] uint8 and depth_u16 [n,h,w] uint16, cuda tensors of one device -> uint8 [n,F,h,w,3] on that device.  poses:
    a host integer array [F,3] as _native.parallax_poses makes it (sixteenths of a pixel, 1/4096 of scale; within +-1024).  focus: as
    above for every image, or per image a list of n depths or a uint16 cuda tensor [n].  Images and views stay independent."""
    torch = _native.require_gpu()
    per_image = torch.is_tensor(focus) or (isinstance(focus, (list, tuple, np.ndarray)) and not (len(focus) and isinstance(focus[0], str)))
    _, _, _, _, _, one_focus, fill = _params('line', 1, (0.0, 0.0), 0.0, 0 if per_image else focus, fill, 'create_parallax_batch')
    return _native.parallax_u8(image_u8, depth_u16, poses, focus if per_image else one_focus, fill, invert=bool(invert))


_ANIMATION_FORMATS = {'.gif': 'GIF', '.webp': 'WEBP', '.png': 'PNG', '.apng': 'PNG'}


def save_animation(frames, filename, fps=25):
    """Write a list of PIL images as one looping animation through Pillow's save_all: GIF, WebP or APNG, chosen by the extension
    ('.gif', '.webp', '.png' / '.apng').  Returns filename."""
    frames = list(frames)
    fmt = _ANIMATION_FORMATS.get(os.path.splitext(str(filename))[1].lower())
    if fmt is None:
        raise _native.DepthStereoError("save_animation: the extension must be one of %s, got %r" % (sorted(_ANIMATION_FORMATS), filename))
    if not frames or not all(isinstance(f, Image.Image) for f in frames):
        raise _native.DepthStereoError("save_animation: frames must be a non-empty list of PIL images")
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not 0 < fps <= 1000:
        raise _native.DepthStereoError("save_animation: fps must be a number in (0, 1000], got %r" % (fps,))
    frames[0].save(filename, format=fmt, save_all=True, append_images=frames[1:], duration=int(round(1000.0 / fps)), loop=0)
    return filename
