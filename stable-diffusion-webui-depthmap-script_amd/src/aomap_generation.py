"""Ambient-occlusion maps from uint16 depth maps, on a HIP kernel: the map that height-to-material tools ship next to the normal map.

Not in the reference.  A normal map says which way a surface faces; an ambient-occlusion (AO) map says how much of the sky a point
can see, and a renderer multiplies it into the diffuse term.  The depth map is taken as a height field (white = near = high) and, per
pixel, `directions` rays of `radius` pixels are scanned for their horizon: the value is 1 minus the mean sine of the horizon's
elevation, 255 = open.  This is the height-field form of horizon-based AO; it ignores the surface's own tilt, so a ramp darkens
uniformly, as in the height-to-AO bakers.  The definition (rays, the exact horizon compare, every rounding) is in
include/depthstereo.h, ds_aomap_u16; tests/aomap_cases.py is its NumPy model, which the kernel reproduces bit for bit.

radius: 1..32 pixels, how far a ray looks.  directions: 4, 8 or 16.  relief: the height in PIXELS that the full uint16 range stands
for (a larger relief means deeper crevices and a darker map).  intensity scales the occlusion before it is subtracted from 1.  invert:
black is high.  wrap: the map is one period of a tiling, rays continue on the other side.  The defaults (16, 8, 32.0, 1.0) are
starting points, not measured optima.  Only uint16 maps are accepted: the horizon compare is defined on integer differences.

In the funnel: core_generation_funnel(..., ops={'aomap': (radius, directions, relief[, intensity]), 'aomap_wrap': False | True | 'tiling'}).
"""
import numpy as np
from PIL import Image

from . import _native


def _params(radius, directions, relief, intensity, who):
    try:
        return _native.aomap_params((radius, directions, relief, intensity))
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None


def create_aomap(depthmap, radius=16, directions=8, relief=32.0, intensity=1.0, invert=False, wrap=False):
    """depthmap: uint16 array [h,w] or an 'I;16' image.  Returns the AO map as a PIL image of mode 'L' and the same size.  A
    non-uint16 map or a bad parameter raises DepthStereoError before any launch."""
    params = _params(radius, directions, relief, intensity, 'create_aomap')
    if isinstance(depthmap, Image.Image):
        if depthmap.mode != 'I;16':
            raise _native.DepthStereoError("create_aomap: a depth image must have mode 'I;16' (uint16), got %r" % (depthmap.mode,))
        depth = np.asarray(depthmap, dtype=np.uint16)
    else:
        depth = np.asarray(depthmap)
    if depth.ndim != 2 or depth.dtype != np.uint16 or depth.size == 0:
        raise _native.DepthStereoError('create_aomap: depthmap must be a non-empty 2-D uint16 array (the horizon compare is defined on '
                                       'integer height differences), got %s %s' % (depth.dtype, depth.shape))
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    out = create_aomap_batch(torch.from_numpy(np.array(depth, order='C')).to(dev).unsqueeze(0), *params, invert=invert, wrap=wrap)
    return Image.fromarray(out[0].cpu().numpy())                         # uint8 [h,w]: mode 'L'


def create_aomap_batch(depth_u16, radius=16, directions=8, relief=32.0, intensity=1.0, invert=False, wrap=False):
    """depth_u16 [n,h,w] uint16 cuda tensor -> uint8 [n,h,w] on that device: one ds_aomap_u16 launch.  Images of a batch stay
    independent."""
    radius, directions, relief, intensity = _params(radius, directions, relief, intensity, 'create_aomap_batch')
    return _native.aomap_u16(depth_u16, radius, directions, relief, intensity, invert=bool(invert), wrap=bool(wrap))
