"""Drop-in for the reference's ``src/normalmap_generation.py`` (create_normalmap, :5-56) on HIP kernels."""
import numpy as np
from PIL import Image

from . import _native


def _ksize(v):
    return int(v) if v is not None and v > 0 else 0


def create_normalmap(depthmap, pre_blur=None, sobel_gradient=3, post_blur=None, invert=False, wrap=False, bilateral=None):
    """Generates normalmaps (reference: src/normalmap_generation.py:5-56).
    :param depthmap: HxW depthmap: uint16 from the funnel (core.py:262), or any other real array like the reference
    :param pre_blur: Gaussian blur before the gradient, None/<=0 to disable, otherwise kernel size
    :param sobel_gradient: Sobel kernel size, None/<=0 for np.gradient
    :param post_blur: Gaussian blur after the gradient, None/<=0 to disable, otherwise kernel size
    :param invert: depthmap will be inverted before calculating normalmap
    :param wrap: (not in the reference, whose :16 leaves it as a TODO) the depth map is one period of a tiling: Sobel / Gaussian taps
        read index modulo size instead of BORDER_REFLECT_101, np.gradient is the central difference at every pixel, so the normal
        map tiles like the depth map does -- normalmap(np.pad(d, R, mode='wrap'))[R:R+h, R:R+w] bit for bit (R: the summed radii
        of the passes).  Same dtype rules.  False: the reference's borders, byte for byte
    :param bilateral: (not in the reference, whose :17 leaves "bilateral filtering (16 bit deflickering)" as a TODO) None, or
        (d, sigma_color, sigma_space): an edge-preserving filter in front of everything else, which flattens the quantisation terraces
        of a 16-bit depth map without smearing silhouettes the way pre_blur does.  d: odd window diameter 3..31; sigma_color in uint16
        levels (256 = one 8-bit step); sigma_space in pixels.  The result is create_normalmap(F, ...) bit for bit, F the float64
        filtered map (definition: include/depthstereo.h, ds_bilateral_u16; borders follow `wrap`).  Defined for uint16 maps only,
        because the range table is indexed by an integer difference: any other dtype raises.  None: today's bytes
    """
    torch = _native.require_gpu()
    depth = np.asarray(depthmap)
    if depth.ndim != 2 or depth.dtype.kind not in 'buif':
        raise _native.DepthStereoError('create_normalmap: depthmap must be a 2-D real array, got %s %s' % (depth.dtype, depth.shape))
    if bilateral is not None:
        _check_bilateral(bilateral, depth.dtype == np.uint16, depth.dtype)
    if depth.dtype != np.uint16:
        # :20-21: `depthmap * (-1.0) / 256.0` promotes integers to float64 and keeps float32 / float16; cv2.Sobel is fed
        # np.float64(normalmap) (:28-29), but np.gradient (:31) and everything after it run in the array's own precision:
        # float32 and float16 have kernels of their own (every operation rounded like numpy's).  float16 cannot be blurred:
        # cv2.GaussianBlur rejects CV_16F arrays in the reference too.
        gradient = _ksize(sobel_gradient) == 0
        if depth.dtype == np.float16 and (_ksize(pre_blur) or (gradient and _ksize(post_blur))):
            raise _native.DepthStereoError('create_normalmap: float16 data cannot be blurred (cv2.GaussianBlur does not take CV_16F '
                                           'arrays, the reference raises cv2.error here); pass float32 / float64')
        if depth.dtype in (np.float16, np.float32) and not gradient:
            # :20-21 scale in the array's own precision BEFORE the promotion to float64 at :28 (the quotient rounds when it is
            # subnormal): hand the kernel 256 times that value, which its float64 `/ 256.0` undoes exactly
            depth = (depth / 256.0).astype(np.float64) * 256.0
        elif not (depth.dtype in (np.float16, np.float32) and gradient):
            depth = depth.astype(np.float64)
    dev = torch.device('cuda', torch.cuda.current_device())
    d = torch.from_numpy(np.array(depth, order='C')).to(dev).unsqueeze(0)
    out = create_normalmap_batch(d, pre_blur, sobel_gradient, post_blur, invert, wrap, bilateral)
    return Image.fromarray(out[0].cpu().numpy())


def _check_bilateral(bilateral, is_u16, dtype):
    """The (d, sigma_color, sigma_space) tuple and the dtype rule of the bilateral pre-filter, without touching the device."""
    try:
        params = _native.bilateral_params(bilateral)
    except ValueError as e:
        raise _native.DepthStereoError('create_normalmap: %s' % e) from None
    if not is_u16:
        raise _native.DepthStereoError('create_normalmap: the bilateral pre-filter is defined for uint16 depth maps only (its range '
                                       'table is indexed by an integer difference), got %s' % (dtype,))
    return params


def create_normalmap_batch(depth_u16, pre_blur=None, sobel_gradient=3, post_blur=None, invert=False, wrap=False, bilateral=None):
    """Device-resident batch: uint16 (or float64 / float32 / float16, see _native.normalmap) cuda tensor [N,H,W] -> uint8 cuda tensor [N,H,W,3].
    wrap: every image is one period of a tiling (see create_normalmap).
    bilateral: None, or (d, sigma_color, sigma_space): uint16 maps go ds_bilateral_u16 -> ds_normalmap_f64[_wrap] (see create_normalmap;
    uint16 only)."""
    if bilateral is not None:
        d, sigma_color, sigma_space = _check_bilateral(bilateral, str(depth_u16.dtype) == 'torch.uint16', depth_u16.dtype)
        depth_u16 = _native.bilateral_u16(depth_u16, d, sigma_color, sigma_space, wrap=bool(wrap))
    return _native.normalmap(depth_u16.contiguous(), _ksize(pre_blur), _ksize(sobel_gradient), _ksize(post_blur), bool(invert),
                             wrap=bool(wrap))
