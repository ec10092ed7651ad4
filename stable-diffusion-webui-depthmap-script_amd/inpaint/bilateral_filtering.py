"""The depth preparation of the 3D-photo pipeline, with the reference's names and signatures (its inpaint/bilateral_filtering.py):

    from inpaint.bilateral_filtering import sparse_bilateral_filtering

Both callers of the reference's inpainting pipeline (run_3dphoto, src/core.py:468-475, and inpaint/main.py:76) run this stage first:
num_iter passes of a discontinuity-masked median over the float32 depth map.  There it is a Python loop over every pixel; here each
pass is one launch of an in-tree HIP kernel (csrc/ds_sparse_bilateral.hip; include/depthstereo.h, ds_sparse_bilateral_f32, holds the
definition) and the returned arrays equal the reference's bit for bit.  There is no host path for the filter: without the native
library or a GPU the call raises.

What the reference can be asked for and nothing in it ever asks -- a mask, label maps, the raw differences, the sigma-weighted branch
of bilateral_filter -- raises NotImplementedError naming the argument.  The mesh stages behind this one are not part of this package:
GEN_INPAINTED_MESH in the funnel still raises."""
import numpy as np

from src._native import DepthStereoError


def _refuse(function, argument, why):
    raise NotImplementedError("%s: %s is not supported (%s)" % (function, argument, why))


def _check_map(function, depth):
    if not (isinstance(depth, np.ndarray) and depth.ndim == 2 and depth.dtype == np.float32):
        raise DepthStereoError("%s: depth must be a 2-D float32 array, got %s %s"
                               % (function, getattr(depth, "dtype", type(depth)), getattr(depth, "shape", ())))
    if min(depth.shape) < 3:
        raise DepthStereoError("%s: depth must be at least 3 x 3, got %s" % (function, depth.shape))


def vis_depth_discontinuity(depth, config, vis_diff=False, label=False, mask=None):
    """The four float32 maps [u_over, b_over, l_over, r_over] of a depth map: 1.0 where the disparity 1 / depth of an interior pixel
    differs from that of its upper, lower, left or right neighbour by more than config['depth_threshold'], else 0.0; 0.0 on the
    outermost ring.  Computed on the host in the depth's own precision (interface parity only: sparse_bilateral_filtering gets its
    jump maps from the kernel)."""
    if mask is not None:
        _refuse("vis_depth_discontinuity", "mask", "nothing in the pipeline passes one")
    if label:
        _refuse("vis_depth_discontinuity", "label=True", "label maps belong to the mesh stages")
    if vis_diff:
        _refuse("vis_depth_discontinuity", "vis_diff=True", "the raw differences have no consumer")
    depth = np.asarray(depth)
    if depth.ndim != 2 or min(depth.shape) < 3:
        raise DepthStereoError("vis_depth_discontinuity: depth must be 2-D and at least 3 x 3, got %s" % (depth.shape,))
    with np.errstate(divide='ignore', invalid='ignore'):
        disp = 1. / depth
        mid = disp[1:-1, 1:-1]
        overs = []
        for neighbour in (disp[:-2, 1:-1], disp[2:, 1:-1], disp[1:-1, :-2], disp[1:-1, 2:]):
            over = (np.abs(mid - neighbour) > config['depth_threshold']).astype(np.float32)
            overs.append(np.pad(over, 1, mode='constant'))
    return overs


def bilateral_filter(depth, config, discontinuity_map=None, HR=False, mask=None, window_size=False):
    """Not a public stage of its own here: the reference reaches it only from sparse_bilateral_filtering, and the kernel of a pass
    derives the discontinuity map from the depth it filters.  Every call raises NotImplementedError."""
    if discontinuity_map is None:
        _refuse("bilateral_filter", "discontinuity_map=None",
                "the sigma_s / sigma_r weighted branch, which nothing in the pipeline reaches")
    if mask is not None:
        _refuse("bilateral_filter", "mask", "nothing in the pipeline passes one")
    _refuse("bilateral_filter", "a caller-made discontinuity_map",
            "a pass makes its own on the device; call sparse_bilateral_filtering")


def _windows(config, num_iter):
    from src import _native
    try:
        num_iter = int(num_iter)
    except (TypeError, ValueError):
        raise DepthStereoError("sparse_bilateral_filtering: num_iter must be an integer, got %r" % (num_iter,)) from None
    sizes = config['filter_size']
    if isinstance(sizes, list):
        if num_iter > len(sizes):
            raise DepthStereoError("sparse_bilateral_filtering: num_iter = %d but config['filter_size'] has %d entries" % (num_iter, len(sizes)))
        sizes = sizes[:max(num_iter, 0)]
    else:
        sizes = [sizes] * max(num_iter, 0)
    if not sizes:
        return []
    try:
        return _native.sparse_bilateral_windows(sizes)
    except ValueError as e:
        raise DepthStereoError("sparse_bilateral_filtering: config['filter_size']: %s" % e) from None


def sparse_bilateral_filtering(depth, image, config, HR=False, mask=None, gsHR=True, edge_id=None, num_iter=None, num_gs_iter=None,
                               spdb=False):
    """num_iter passes of the discontinuity-masked median.  depth: float32 [h, w], finite and >= 0 (0 marks a hole); image: uint8
    [h, w, 3]; config: 'filter_size' (an odd window in 1..15, or a list with one per pass), 'depth_threshold', and the 'sigma_s' /
    'sigma_r' the reference reads without using them.  Returns (save_images, save_depths), NumPy lists of num_iter arrays each, equal
    to the reference's: save_depths[i] is the INPUT of pass i (save_depths[0] a copy of depth) and save_images[i] the image with the
    pixels at that map's disparity jumps set to black.  The output of the last pass is returned by nobody, so that filter is not run:
    num_iter - 1 filter launches and one jump-map launch.  HR, gsHR, edge_id, num_gs_iter and spdb are accepted and, as in the
    reference, have no effect."""
    if mask is not None:
        _refuse("sparse_bilateral_filtering", "mask", "nothing in the pipeline passes one")
    _check_map("sparse_bilateral_filtering", depth)
    h, w = depth.shape
    if not (isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (h, w, 3)):
        raise DepthStereoError("sparse_bilateral_filtering: image must be a uint8 array %s, got %s %s"
                               % ((h, w, 3), getattr(image, "dtype", type(image)), getattr(image, "shape", ())))
    if not (np.isfinite(depth).all() and (depth >= 0).all()):
        raise DepthStereoError("sparse_bilateral_filtering: every depth must be finite and >= 0")
    try:
        threshold = float(config['depth_threshold'])
    except (TypeError, ValueError):
        raise DepthStereoError("sparse_bilateral_filtering: config['depth_threshold'] must be a number, got %r"
                               % (config['depth_threshold'],)) from None
    windows = _windows(config, num_iter)
    if not windows:
        return [], []
    from src import _native
    torch = _native.require_gpu()
    first = depth.copy()                                                    # save_depths[0]: the caller's array stays the caller's
    maps, jumps = _native.sparse_bilateral_f32(torch.from_numpy(first).cuda()[None], windows, threshold)
    jumps = torch.cat(jumps).cpu().numpy().astype(bool)
    later = torch.cat(maps[1:]).cpu().numpy() if len(maps) > 1 else []
    save_depths = [first] + [later[i].copy() for i in range(len(later))]
    save_images = []
    for jump in jumps:
        black = image.copy()
        black[jump] = 0
        save_images.append(black)
    return save_images, save_depths
