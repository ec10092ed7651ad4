"""Lens blur from depth: a synthetic shallow depth of field of an image by its uint16 depth map, on a HIP kernel.

Not in the reference.  What a photo editor's "lens blur" filter does with a depth map: every pixel gets a circle of confusion that
grows with the distance of its depth from a focus depth, and the output gathers, per pixel, the pixels whose circle reaches it.  An
occlusion rule keeps an in-focus foreground hard against a blurred background: a farther pixel reaches a pixel only as far as that
pixel's own blur allows.  The definition (the circle of confusion, the disc weights, the rule, the rounding -- all in integers) is in
include/depthstereo.h, ds_lensblur_u8; tests/lensblur_cases.py is its NumPy model, which the kernel reproduces bit for bit.

radius: 1..32 pixels, the largest blur radius.  aperture: the blur radius in PIXELS that a depth difference of the full uint16 range
would get (quantised to quarter pixels).  focus: a depth 0..65535 in the map's own units, or ('point', fx, fy) with fx, fy in [0, 1]:
the depth found at that position of the image.  band: depth differences up to it stay sharp.  invert: black is near (the funnel's
maps are white = near).  The defaults (12, 48.0, ('point', 0.5, 0.5), 0) are starting points, not measured optima.  Only uint16 maps
are accepted: the circle of confusion is defined on integer depth differences.

In the funnel: core_generation_funnel(..., ops={'lensblur': (radius, aperture, focus[, band])}).
"""
import numpy as np
from PIL import Image

from . import _native


def _params(radius, aperture, focus, band, who):
    try:
        return _native.lensblur_params((radius, aperture, focus, band))
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None


def create_lensblur(image, depthmap, radius=12, aperture=48.0, focus=('point', 0.5, 0.5), band=0, invert=False):
    """image: PIL image or uint8 array (taken as its convert("RGB")); depthmap: uint16 array [h,w] or an 'I;16' image of the same size.
    Returns the blurred image as a PIL RGB image.  Non-uint16 depth, a size mismatch or a bad parameter raises DepthStereoError before
    any launch."""
    params = _params(radius, aperture, focus, band, 'create_lensblur')
    if isinstance(depthmap, Image.Image):
        if depthmap.mode != 'I;16':
            raise _native.DepthStereoError("create_lensblur: a depth image must have mode 'I;16' (uint16), got %r" % (depthmap.mode,))
        depth = np.asarray(depthmap, dtype=np.uint16)
    else:
        depth = np.asarray(depthmap)
    if depth.ndim != 2 or depth.dtype != np.uint16 or depth.size == 0:
        raise _native.DepthStereoError('create_lensblur: depthmap must be a non-empty 2-D uint16 array (the circle of confusion is defined '
                                       'on integer depth differences), got %s %s' % (depth.dtype, depth.shape))
    if not isinstance(image, Image.Image):
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in (3, 4)):
            raise _native.DepthStereoError('create_lensblur: image must be a PIL image or a uint8 array [h,w], [h,w,3] or [h,w,4], got '
                                           '%s %s' % (arr.dtype, arr.shape))
        image = Image.fromarray(np.ascontiguousarray(arr))
    rgb = np.asarray(image.convert('RGB'), dtype=np.uint8)
    if rgb.shape[:2] != depth.shape:
        raise _native.DepthStereoError('create_lensblur: image is %d x %d, depth map %d x %d (height x width)' % (rgb.shape[:2] + depth.shape))
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    out = create_lensblur_batch(torch.from_numpy(np.array(rgb, order='C')).to(dev).unsqueeze(0),
                                torch.from_numpy(np.array(depth, order='C')).to(dev).unsqueeze(0), *params, invert=invert)
    return Image.fromarray(out[0].cpu().numpy())                         # uint8 [h,w,3]: mode 'RGB'


def create_lensblur_batch(image_u8, depth_u16, radius=12, aperture=48.0, focus=('point', 0.5, 0.5), band=0, invert=False):
    """image_u8 [n,h,w,3] uint8 and depth_u16 [n,h,w] uint16, cuda tensors of one device -> uint8 [n,h,w,3] on that device: one
    ds_lensblur_u8 launch.  focus: as above for every image, or per image a list of n depths or a uint16 cuda tensor [n].  Images of
    a batch stay independent."""
    torch = _native.require_gpu()
    per_image = torch.is_tensor(focus) or (isinstance(focus, (list, tuple, np.ndarray)) and not (len(focus) and isinstance(focus[0], str)))
    radius, aperture, one_focus, band = _params(radius, aperture, 0 if per_image else focus, band, 'create_lensblur_batch')
    return _native.lensblur_u8(image_u8, depth_u16, radius, _native.lensblur_quarter_pixels(aperture), band,
                               focus if per_image else one_focus, invert=bool(invert))
