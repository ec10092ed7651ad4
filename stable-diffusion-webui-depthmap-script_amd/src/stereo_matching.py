"""Depth from stereo pairs, on HIP kernels: semi-global matching of a row-aligned left / right pair.

Not in the reference.  Every other product of this package runs image -> depth -> something for two eyes; this is the opposite
direction: side-by-side 3D photos, stereo camera shots and SBS video frames come in, and the depth map of the LEFT view comes out,
without a network, without weights and without guessing scale.  With that map everything the package makes from a depth map works on
stereo material: another divergence, anaglyphs, normal / AO maps, lens blur, parallax clips, autostereograms, the simple mesh.

The method is four-path semi-global matching (Hirschmueller 2008) on a 5x5 census: per pixel and candidate disparity a Hamming cost,
smoothed along the four axis directions by dynamic programming (P1 for a disparity step of one, P2 for a larger one), the cheapest
disparity per pixel, a uniqueness and a left-right consistency check, sub-pixel interpolation, a row fill of what the checks rejected
from the background side, a 3x3 median, and a per-image rescale to uint16 with white = near.  The definition, all-integer, is in
include/depthstereo.h, ds_stereo_match_u8; tests/stereo_match_cases.py is its NumPy model, which the kernels reproduce bit for bit.

max_disparity: 32, 64 or 128 candidates.  min_disparity: -128..127, the smallest one; negative for content in front of the screen
plane.  Disparity d means: left column x shows what the right image shows at column x - d.  p1 1..64, p2 p1..255.  uniqueness 0..50
percent, lr_check -1..3 pixels (-1: off).  The defaults (64, 0, 4, 48, 5, 1) are libSGM's 10 / 120 scaled from a 62-bit to a 24-bit
census: starting points, not measured optima.  Pairs are taken as rectified (row-aligned), as SBS material is.

paths=8 adds the four diagonal directions and speckle=(size, range) a speckle filter between the checks and the fill
(ds_stereo_match_ex_u8); paths=8, speckle=(64, 1) is a starting point for stereo photos, not a measured optimum.  filter_speckles is the
filter alone, for a disparity map of the caller's.

In the funnel: core_generation_funnel(..., ops={'stereo_input': (layout[, D[, d0[, P1, P2[, u[, lr]]]]])}), and beside it
'stereo_paths': 4 | 8 and 'stereo_speckle': (size, range).
"""
import numpy as np
from PIL import Image

from . import _native

LAYOUTS = ('left-right', 'right-left', 'top-bottom', 'bottom-top')           # the names create_stereoimages uses for its modes


def stereo_input_params(p):
    """ops['stereo_input']: (layout[, D[, d0[, P1, P2[, u[, lr]]]]]) as (layout, D, d0, P1, P2, u, lr), or ValueError.  Pure Python."""
    usage = "(layout[, D[, d0[, P1, P2[, u[, lr]]]]])"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) < 1:
            raise TypeError
    except TypeError:
        raise ValueError("stereo_input must be %s, got %r" % (usage, p)) from None
    if not isinstance(q[0], str) or q[0] not in LAYOUTS:
        raise ValueError("stereo_input: layout must be one of %r, got %r" % (LAYOUTS, q[0]))
    return (q[0],) + (_native.stereo_match_params(q[1:]) if len(q) > 1 else _native.STEREO_MATCH_DEFAULTS)


def split_stereo_pair(image, layout):
    """The two views of a stereo pair stored in one image: (left, right).  image: a PIL image or an array [h,w] / [h,w,c]; layout:
    'left-right', 'right-left', 'top-bottom' or 'bottom-top', naming what the first (left, or upper) half shows first.  The halves come
    back as what went in (PIL crops, or array views).  An odd split dimension, or another layout, is a ValueError."""
    if not isinstance(layout, str) or layout not in LAYOUTS:
        raise ValueError("split_stereo_pair: layout must be one of %r, got %r" % (LAYOUTS, layout))
    pil = isinstance(image, Image.Image)
    if pil:
        w, h = image.size
    else:
        image = np.asarray(image)
        if image.ndim not in (2, 3):
            raise ValueError("split_stereo_pair: an array must be [h,w] or [h,w,c], got %s" % (image.shape,))
        h, w = image.shape[:2]
    side = layout in ('left-right', 'right-left')
    size = w if side else h
    if size < 2 or size % 2:
        raise ValueError("split_stereo_pair: a %s pair needs an even %s, got %d" % (layout, "width" if side else "height", size))
    half = size // 2
    if pil:
        first, second = (image.crop((0, 0, half, h)), image.crop((half, 0, w, h))) if side else (image.crop((0, 0, w, half)), image.crop((0, half, w, h)))
    else:
        first, second = (image[:, :half], image[:, half:]) if side else (image[:half], image[half:])
    return (first, second) if layout in ('left-right', 'top-bottom') else (second, first)


def _pixels(view, who, name):
    """uint8 [h,w,c], c in {1, 3, 4}, C-contiguous: a PIL image ('L', 'RGBA', anything else through convert('RGB')) or a uint8 array."""
    if isinstance(view, Image.Image):
        view = np.asarray(view if view.mode in ('L', 'RGB', 'RGBA') else view.convert('RGB'), dtype=np.uint8)
    a = np.asarray(view)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3, 4) or a.size == 0:
        raise _native.DepthStereoError("%s: %s must be a PIL image or a non-empty uint8 array [h,w], [h,w,1], [h,w,3] or [h,w,4], got %s %s"
                                       % (who, name, a.dtype, a.shape))
    return np.array(a, order='C')


def _params(max_disparity, min_disparity, p1, p2, uniqueness, lr_check, who):
    try:
        return _native.stereo_match_params((max_disparity, min_disparity, p1, p2, uniqueness, lr_check))
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None


def _ex_params(paths, speckle, who):
    """(paths, speckle) as (paths, speckle_size, speckle_range), or ValueError.  speckle: None or (size, range); size 0 is off too."""
    if speckle is None:
        size, rng = 0, 0
    else:
        try:
            if isinstance(speckle, (str, bytes)):
                raise TypeError
            size, rng = tuple(speckle)
        except (TypeError, ValueError):
            raise ValueError("%s: speckle must be None or (size, range), got %r" % (who, speckle)) from None
    try:
        return _native.stereo_match_ex_params((paths, size, rng))
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e)) from None


def _ex_check(paths, speckle, who):
    try:
        return _ex_params(paths, speckle, who)
    except ValueError as e:
        raise _native.DepthStereoError(str(e)) from None


def _match(left, right, params, paths, speckle, who, **kwargs):
    """ds_stereo_match_u8 with the defaults of paths and speckle, ds_stereo_match_ex_u8 otherwise."""
    ex = _ex_check(paths, speckle, who)
    if ex[0] == 4 and ex[1] == 0:
        return _native.stereo_match_u8(left, right, *params, **kwargs)
    return _native.stereo_match_ex_u8(left, right, *params, *ex, **kwargs)


def depth_from_stereo(left, right, max_disparity=64, min_disparity=0, p1=4, p2=48, uniqueness=5, lr_check=1, return_disparity=False,
                      paths=4, speckle=None):
    """left, right: PIL images or uint8 arrays of one size and channel count.  Returns the depth map of the left view as a PIL 'I;16'
    image, white = near; with return_disparity also the disparity in pixels (float32 [h,w], exact sixteenths) and the bool mask of the
    pixels that passed the uniqueness and left-right checks (the others were filled from their row).  A bad input or parameter raises
    DepthStereoError before any launch.  paths: 4 or 8 aggregation directions (8 adds the diagonals: fewer streaks on slanted
    silhouettes and weak texture).  speckle: None or (size, range) -- connected regions of at most `size` pixels whose neighbouring
    disparities differ by at most `range` pixels are rejected before the fill.  With the defaults the call is ds_stereo_match_u8's;
    paths=8, speckle=(64, 1) is a starting point for stereo photos, not a measured optimum."""
    params = _params(max_disparity, min_disparity, p1, p2, uniqueness, lr_check, 'depth_from_stereo')
    _ex_check(paths, speckle, 'depth_from_stereo')
    a, b = _pixels(left, 'depth_from_stereo', 'left'), _pixels(right, 'depth_from_stereo', 'right')
    if a.shape != b.shape:
        raise _native.DepthStereoError('depth_from_stereo: left %s and right %s must have one shape' % (a.shape, b.shape))
    torch = _native.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())
    disparity, valid, depth = _match(torch.from_numpy(a).to(dev).unsqueeze(0), torch.from_numpy(b).to(dev).unsqueeze(0), params, paths,
                                     speckle, 'depth_from_stereo', want_valid=bool(return_disparity))
    image = Image.fromarray(depth[0].cpu().numpy())                          # uint16 [h,w]: mode 'I;16'
    if not return_disparity:
        return image
    return image, disparity[0].cpu().numpy().astype(np.float32) / np.float32(16.0), valid[0].cpu().numpy().astype(bool)


def depth_from_stereo_batch(left_u8, right_u8, max_disparity=64, min_disparity=0, p1=4, p2=48, uniqueness=5, lr_check=1, paths=4, speckle=None):
    """left_u8, right_u8 [n,h,w,c] uint8 cuda tensors -> uint16 [n,h,w] on that device: one ds_stereo_match_u8 call (with paths=8 or a
    speckle filter: one ds_stereo_match_ex_u8 call; see depth_from_stereo).  Images of a batch stay independent."""
    params = _params(max_disparity, min_disparity, p1, p2, uniqueness, lr_check, 'depth_from_stereo_batch')
    return _match(left_u8, right_u8, params, paths, speckle, 'depth_from_stereo_batch')[2]


def filter_speckles(disparity16, valid, size, t, return_sizes=False):
    """The speckle filter alone, for a disparity map of the caller's: disparity16 int16 [h,w] (any unit; depth_from_stereo's disparity
    times 16 is sixteenths of a pixel), valid a bool or uint8 mask [h,w], size 1..65535, t 0..65535 in the map's units.  Returns the bool
    mask of the valid pixels whose connected region (4-neighbours differing by at most t) has more than `size` pixels; with return_sizes
    also every pixel's region size (int32 [h,w], 0 for an invalid pixel).  Arrays in, arrays out; cuda tensors [n,h,w] (int16 / uint8)
    in, the tensors of _native.speckle_filter_i16 out."""
    torch = _native.require_gpu()
    if torch.is_tensor(disparity16) or torch.is_tensor(valid):
        out, sizes = _native.speckle_filter_i16(disparity16, valid, size, t, want_sizes=bool(return_sizes))
        return (out, sizes) if return_sizes else out
    d, v = np.asarray(disparity16), np.asarray(valid)
    if d.dtype != np.int16 or d.ndim != 2 or d.size == 0 or v.shape != d.shape or v.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise _native.DepthStereoError("filter_speckles: disparity16 must be a non-empty int16 array [h,w] and valid a bool or uint8 array of "
                                       "its shape, got %s %s and %s %s" % (d.dtype, d.shape, v.dtype, v.shape))
    dev = torch.device('cuda', torch.cuda.current_device())
    out, sizes = _native.speckle_filter_i16(torch.from_numpy(np.array(d, order='C')).to(dev).unsqueeze(0),
                                            torch.from_numpy(np.array(v != 0, order='C').astype(np.uint8)).to(dev).unsqueeze(0), size, t,
                                            want_sizes=bool(return_sizes))
    mask = out[0].cpu().numpy().astype(bool)
    return (mask, sizes[0].cpu().numpy()) if return_sizes else mask
