"""Autostereograms from uint16 depth maps, on a HIP kernel: the single-image stereogram ("magic eye"; SIRDS, or its textured form).

Not in the reference.  It is the one classic stereo product of a depth map that needs neither glasses nor a viewer: ONE image in which
the depth map alone decides which pixels of a row must share a colour.  Looked at with the eyes converged behind the screen, pixels a
separation s apart fuse into one point; s is the period at the far plane and shrinks as the surface comes nearer.  Per row every
column links the two columns in which the two eyes see it, unless something nearer hides it from one eye, and a pixel takes its
colour -- a random dot, or a pixel of a repeating pattern -- from the connected component it ends up in.  The definition (separation,
hidden-surface test, components, the colour hash -- all in integers) is in include/depthstereo.h, ds_autostereogram_u8;
tests/autostereogram_cases.py is its NumPy model, which the kernel reproduces bit for bit.

period: 16..512 pixels, the separation of the far plane and the width of a strip (about half the distance between the eyes on the
screen it will be seen on; below ~ 50 the strips get hard to fuse, above ~ 150 most people cannot diverge that far).  depth_factor:
mu in (0, 0.5], quantised to m / 256: how far the near plane comes out of the far plane, as a share of the way to the eyes (1/3 is the
textbook value; the nearest separation is then 0.8 period).  pattern: 'dots' (coloured random dots), 'mono' (black / white dots) or an
image, a PIL image or a uint8 array, which is tiled: choose a tile about `period` wide.  seed: 0..2^32 - 1, another dot pattern.
invert: black is near (the funnel's maps are white = near).  The defaults (96, 1/3, 'dots', 0) are starting points, not measured
optima.  Only uint16 maps are accepted: the separation is defined on integer depths.

In the funnel: core_generation_funnel(..., ops={'autostereogram': (period, depth_factor[, pattern[, seed]])}).
"""
import numpy as np
from PIL import Image

from . import _native


def _params(period, depth_factor, pattern, seed, who):
    try:
        period, m, pattern, seed = _native.autostereogram_params((period, depth_factor, pattern, seed))
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None
    if isinstance(pattern, str):
        return period, m, _native.AUTOSTEREOGRAM_MODES[pattern], seed, None
    return period, m, 2, seed, pattern


def create_autostereogram(depthmap, period=96, depth_factor=1 / 3, pattern='dots', seed=0, invert=False):
    """depthmap: uint16 array [h,w] or an 'I;16' image.  Returns the stereogram as a PIL RGB image of the same size.  A non-uint16 map
    or a bad parameter raises DepthStereoError before any launch."""
    params = _params(period, depth_factor, pattern, seed, 'create_autostereogram')
    if isinstance(depthmap, Image.Image):
        if depthmap.mode != 'I;16':
            raise _native.DepthStereoError("create_autostereogram: a depth image must have mode 'I;16' (uint16), got %r" % (depthmap.mode,))
        depth = np.asarray(depthmap, dtype=np.uint16)
    else:
        depth = np.asarray(depthmap)
    if depth.ndim != 2 or depth.dtype != np.uint16 or depth.size == 0:
        raise _native.DepthStereoError('create_autostereogram: depthmap must be a non-empty 2-D uint16 array (the separation is defined on '
                                       'integer depths), got %s %s' % (depth.dtype, depth.shape))
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    out = _native.autostereogram_u8(torch.from_numpy(np.array(depth, order='C')).to(dev).unsqueeze(0), *params, invert=bool(invert))
    return Image.fromarray(out[0].cpu().numpy())                         # uint8 [h,w,3]: mode 'RGB'


def create_autostereogram_batch(depth_u16, period=96, depth_factor=1 / 3, pattern='dots', seed=0, invert=False):
    """depth_u16 [n,h,w] uint16 cuda tensor -> uint8 [n,h,w,3] on that device: one ds_autostereogram_u8 launch.  Images of a batch stay
    independent, and share the pattern and the seed."""
    return _native.autostereogram_u8(depth_u16, *_params(period, depth_factor, pattern, seed, 'create_autostereogram_batch'),
                                     invert=bool(invert))
