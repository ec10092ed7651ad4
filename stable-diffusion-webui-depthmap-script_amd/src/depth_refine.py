"""Depth refinement: a joint (cross) bilateral filter of the uint16 depth map guided by the RGB image, on a HIP kernel.

Not in the reference.  A network's depth map reaches the per-pixel path as an upsample of a few hundred pixels: at a silhouette the
depth changes over a ramp several output pixels wide that is rarely centred on the colour edge it belongs to, and the stereo warp
stretches exactly that ramp into a halo.  Here the spatial kernel is a Gaussian and the range weight is taken from the COLOUR
difference of the image, so depth averages only within a colour region and the transition collects at the colour edge.  The definition
(tables, tap order, every rounding) is in include/depthstereo.h, ds_joint_bilateral_u16; tests/depth_refine_cases.py is its float64
NumPy model, which the kernel reproduces bit for bit.

params = (d, sigma_color, sigma_space) or (d, sigma_color, sigma_space, iterations): d the odd window diameter 3..31; sigma_color in
units of SUMMED 8-bit channel difference |dR| + |dG| + |dB| (0..765); sigma_space in pixels; iterations 1..8, default 1 (pass i + 1
filters the uint16 result of pass i with the same guide).  (9, 25.0, 3.0) is a mild setting, (15, 25.0, 5.0, 4) a strong one.
wrap: taps read index modulo size instead of BORDER_REFLECT_101 (tileable maps; the same rule for the depth and the guide).

In the funnel: core_generation_funnel(..., ops={'depth_refine': params, 'depth_refine_wrap': False | True | 'tiling'}).
"""
import numpy as np
from PIL import Image

from . import _native


def _params(params, who):
    try:
        return _native.depth_refine_params(params)
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None


def refine_depthmap(image, depthmap, params, wrap=False):
    """image: PIL image or uint8 array (taken as its convert("RGB")); depthmap: uint16 array [h,w] or an 'I;16' image of the same size.
    Returns the refined map, a uint16 NumPy array [h,w].  Non-uint16 depth, a size mismatch or a bad tuple raises DepthStereoError
    before any launch."""
    d, sigma_color, sigma_space, iterations = _params(params, 'refine_depthmap')
    if isinstance(depthmap, Image.Image):
        if depthmap.mode != 'I;16':
            raise _native.DepthStereoError("refine_depthmap: a depth image must have mode 'I;16' (uint16), got %r" % (depthmap.mode,))
        depth = np.asarray(depthmap, dtype=np.uint16)
    else:
        depth = np.asarray(depthmap)
    if depth.ndim != 2 or depth.dtype != np.uint16:
        raise _native.DepthStereoError('refine_depthmap: depthmap must be a 2-D uint16 array (the filter is defined on, and returns, '
                                       'uint16 levels), got %s %s' % (depth.dtype, depth.shape))
    if not isinstance(image, Image.Image):
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in (3, 4)):
            raise _native.DepthStereoError('refine_depthmap: image must be a PIL image or a uint8 array [h,w], [h,w,3] or [h,w,4], got '
                                           '%s %s' % (arr.dtype, arr.shape))
        image = Image.fromarray(np.ascontiguousarray(arr))
    guide = np.asarray(image.convert('RGB'), dtype=np.uint8)
    if guide.shape[:2] != depth.shape:
        raise _native.DepthStereoError('refine_depthmap: image is %d x %d, depth map %d x %d (height x width)'
                                       % (guide.shape[:2] + depth.shape))
    if not wrap and d // 2 >= min(depth.shape):
        raise _native.DepthStereoError('refine_depthmap: d // 2 = %d must be below min(h, w) = %d without wrap' % (d // 2, min(depth.shape)))
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    out = refine_depthmap_batch(torch.from_numpy(np.array(depth, order='C')).to(dev).unsqueeze(0),
                                torch.from_numpy(np.array(guide, order='C')).to(dev).unsqueeze(0),
                                (d, sigma_color, sigma_space, iterations), wrap)
    return out[0].cpu().numpy()


def refine_depthmap_batch(depth_u16, guide_u8, params, wrap=False):
    """depth_u16 [n,h,w] uint16 and guide_u8 [n,h,w,3 or 4] uint8, cuda tensors of one device -> uint16 [n,h,w] on that device: one
    ds_joint_bilateral_u16 launch per iteration.  Images of a batch stay independent."""
    d, sigma_color, sigma_space, iterations = _params(params, 'refine_depthmap_batch')
    return _native.joint_bilateral_u16(depth_u16, guide_u8, d, sigma_color, sigma_space, iterations, wrap=bool(wrap))
