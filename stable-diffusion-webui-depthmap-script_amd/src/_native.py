"""ctypes binding of libdepthstereo_hip.so (C ABI: include/depthstereo.h) for torch tensors in HBM.

PyTorch is plumbing here: it owns device memory and streams; every per-pixel operation is a
hand-written HIP kernel reached through the C ABI.  There is NO CPU fallback: if the shared library is
missing, or no MI355X is visible, the calls raise.
"""
import collections
import ctypes
import math
import os
import threading

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# DS_NATIVE_LIB: another build of the same library (the -DDS_EXPERIMENTS one of build_native.py, for A/B runs on hardware)
LIB_PATH = os.environ.get("DS_NATIVE_LIB") or os.path.join(_PKG_ROOT, "libdepthstereo_hip.so")

DS_DEPTH_U16, DS_DEPTH_F32, DS_DEPTH_F64 = 0, 1, 2
FILL_IDS = {"none": 0, "naive": 1, "naive_interpolating": 2, "polylines_soft": 3, "polylines_sharp": 4}

EXPORTS = [
    "ds_version", "ds_last_error", "ds_normalmap_f64", "ds_normalmap_gradient_f32", "ds_reassemble_readout", "ds_bias_act_nhwc", "ds_linear", "ds_linear_residual", "ds_linear_vt", "ds_linear_qkv", "ds_conv3x3_nhwc", "ds_ctx_create", "ds_ctx_destroy", "ds_stereo_warp", "ds_depth_minmax",
    "ds_stereo_last_exact_rows", "ds_copy_view", "ds_overlap_red_cyan", "ds_normalmap", "ds_depth_to_u16",
    "ds_convert_to_i16", "ds_profile_enable", "ds_profile_last_ms", "ds_stereo_last_stats", "ds_attention_fwd", "ds_attention_bias_pack", "ds_colorize_u16", "ds_residual_layernorm", "ds_boost_blend", "ds_upsample_bilinear_nhwc", "ds_dpt_head_tail", "ds_preprocess_bicubic", "ds_linear_reload_env", "ds_attention_reload_env", "ds_normalmap_selfcheck", "ds_normalmap_gradient_f16", "ds_normalmap_gradient_blur_f32",
    "ds_linear_shuffle", "ds_linear_readout", "ds_linear_rows4", "ds_conv3x3_nhwc_pair", "ds_kernel_timer_enable", "ds_kernel_timer_read", "ds_kernel_timer_read_each", "ds_group_norm_nchw",
    "ds_row_stats", "ds_linear_ln", "ds_linear_vt_ln", "ds_gconv3x3_nhwc_f32", "ds_add_relu_f32", "ds_bias_act_f32", "ds_relu_cat_f32",
    "ds_dwconv_nhwc", "ds_resize_lanczos", "ds_custom_depth_to_f64", "ds_conv3x3_nhwc_circular", "ds_dpt_head_tail_circular",
    "ds_normalmap_wrap", "ds_normalmap_f64_wrap", "ds_normalmap_gradient_f32_wrap", "ds_normalmap_gradient_f16_wrap", "ds_normalmap_gradient_blur_f32_wrap",
    "ds_bilateral_u16", "ds_joint_bilateral_u16", "ds_sparse_bilateral_f32", "ds_sparse_bilateral_jump_f32", "ds_aomap_u16", "ds_lensblur_u8", "ds_parallax_u8", "ds_mesh_render_workspace_bytes", "ds_mesh_render_u8", "ds_mesh_render_stages_u8", "ds_autostereogram_u8", "ds_autostereogram_rounds_u8", "ds_stereo_match_workspace_bytes", "ds_stereo_match_u8", "ds_stereo_match_stages_u8", "ds_stereo_match_ex_workspace_bytes", "ds_stereo_match_ex_u8", "ds_stereo_match_ex_stages_u8", "ds_speckle_filter_workspace_bytes", "ds_speckle_filter_i16", "ds_frame_luma_hist", "ds_temporal_smooth5_f32", "ds_temporal_joint_bilateral_u16",
    "ds_preprocess_bicubic_rows", "ds_tokens_fixup", "ds_upsample_bicubic_to_f32", "ds_im2col3x3_s2_nhwc", "ds_dpt_head_front",
]


class DepthStereoError(RuntimeError):
    pass


class ds_rows_problem(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("x_row_pitch", ctypes.c_int64), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("y", ctypes.c_void_p)]


class ds_eye(ctypes.Structure):
    _fields_ = [("divergence_px", ctypes.c_double), ("separation_px", ctypes.c_double),
                ("out", ctypes.c_void_p), ("out_row_stride", ctypes.c_int64), ("out_img_stride", ctypes.c_int64)]


_lib = None
_lib_lock = threading.Lock()

# How often each C-ABI entry point was reached through this binding (tests and bench.py's route_check assert that a forward
# really took the in-tree kernels it claims: a routing threshold that silently sends a shape to the library shows up here).
# ds_linear_qkv runs two of the counted GEMMs in one launch: it counts under its own name AND once under ds_linear and ds_linear_vt,
# so "how many Q/K and V^T GEMMs ran in-tree" reads the same on either route; ds_linear_qkv alone tells the routes apart.
# ds_linear_rows4 likewise: its own name once, and ds_linear once per GEMM it carries; ds_conv3x3_nhwc_pair: ds_conv3x3_nhwc twice;
# ds_dpt_head_front: ds_upsample_bilinear_nhwc and ds_conv3x3_nhwc once each.
CALLS = collections.Counter()


def lib():
    """Load the shared library (once).  Raises if it has not been built: there is no fallback."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise DepthStereoError(
                    f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
                    "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
            L = ctypes.CDLL(LIB_PATH)
            vp, ci, cd, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
            L.ds_version.restype = ci
            L.ds_last_error.restype = ctypes.c_char_p
            L.ds_ctx_create.argtypes = [ctypes.POINTER(vp), ci]
            L.ds_ctx_destroy.argtypes = [vp]
            L.ds_stereo_warp.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, cd, vp, ci, ctypes.POINTER(ds_eye), ci, vp]
            L.ds_depth_minmax.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
            L.ds_stereo_last_exact_rows.argtypes = [vp, ctypes.POINTER(i64), vp]
            L.ds_copy_view.argtypes = [vp, vp, i64, i64, vp, i64, i64, ci, ci, i64, vp]
            L.ds_overlap_red_cyan.argtypes = [vp, vp, i64, i64, vp, i64, i64, ci, ci, ci, ci, vp, vp]
            L.ds_normalmap.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]
            L.ds_normalmap_f64.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]
            L.ds_normalmap_gradient_f32.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
            L.ds_normalmap_gradient_f16.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
            L.ds_normalmap_gradient_blur_f32.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
            for name in ("ds_normalmap", "ds_normalmap_f64", "ds_normalmap_gradient_f32", "ds_normalmap_gradient_f16", "ds_normalmap_gradient_blur_f32"):
                getattr(L, name + "_wrap").argtypes = getattr(L, name).argtypes
            L.ds_bilateral_u16.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, vp, vp]
            L.ds_joint_bilateral_u16.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp]
            L.ds_sparse_bilateral_f32.argtypes = [vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, vp, vp, vp, vp]
            L.ds_sparse_bilateral_jump_f32.argtypes = [vp, vp, ci, ci, ci, ctypes.c_float, vp, vp]
            L.ds_aomap_u16.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, cd, cd, ci, ci, vp, vp, vp]
            L.ds_lensblur_u8.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]
            L.ds_parallax_u8.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, ci, ci, ci, vp, vp, vp, vp]
            L.ds_mesh_render_workspace_bytes.argtypes = [i64, i64, ci, ci, ci]
            L.ds_mesh_render_workspace_bytes.restype = ctypes.c_size_t
            L.ds_mesh_render_u8.argtypes = [vp, vp, vp, vp, i64, i64, vp, ci, ci, ci, ci, cd, ci, ci, ci, ci, vp, ci, vp, vp, vp]
            L.ds_mesh_render_stages_u8.argtypes = [vp, vp, vp, vp, i64, i64, vp, ci, ci, ci, ci, cd, ci, ci, ci, ci, vp, ci, vp, vp, ci, vp]
            L.ds_autostereogram_u8.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ctypes.c_uint32, vp, ci, ci, ci, vp, vp]
            L.ds_autostereogram_rounds_u8.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ctypes.c_uint32, vp, ci, ci, ci, vp, vp, vp]
            L.ds_stereo_match_workspace_bytes.argtypes = [ci, ci, ci]
            L.ds_stereo_match_workspace_bytes.restype = ctypes.c_size_t
            L.ds_stereo_match_u8.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp]
            L.ds_stereo_match_stages_u8.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, ci, vp]
            L.ds_stereo_match_ex_workspace_bytes.argtypes = [ci, ci, ci, ci, ci]
            L.ds_stereo_match_ex_workspace_bytes.restype = ctypes.c_size_t
            L.ds_stereo_match_ex_u8.argtypes = [vp, vp, vp] + [ci] * 13 + [vp, ci, vp, vp, vp, vp]
            L.ds_stereo_match_ex_stages_u8.argtypes = [vp, vp, vp] + [ci] * 13 + [vp, ci, vp, vp, vp, ci, vp]
            L.ds_speckle_filter_workspace_bytes.argtypes = [ci, ci]
            L.ds_speckle_filter_workspace_bytes.restype = ctypes.c_size_t
            L.ds_speckle_filter_i16.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp]
            L.ds_frame_luma_hist.argtypes =[vp, vp, ci, ci, ci, ci, vp, vp]
            L.ds_temporal_smooth5_f32.argtypes = [vp, vp, ci, i64, ci, ci, ci, ci, vp, vp]
            L.ds_temporal_joint_bilateral_u16.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, vp]
            L.ds_depth_to_u16.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
            L.ds_convert_to_i16.argtypes = [vp, vp, ci, i64, vp, vp]
            L.ds_stereo_last_stats.argtypes = [vp, ctypes.POINTER(i64), vp]
            L.ds_attention_fwd.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, ci, vp]
            L.ds_normalmap_selfcheck.argtypes = [vp, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ulonglong), vp]
            L.ds_attention_bias_pack.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
            L.ds_colorize_u16.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, vp, vp]
            L.ds_residual_layernorm.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, ci, ctypes.c_float, ci, vp]
            L.ds_boost_blend.argtypes = [vp, vp, i64, ci, ci, vp, ci, vp, ci, vp, ci, vp]
            L.ds_upsample_bilinear_nhwc.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
            L.ds_dpt_head_tail.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, ctypes.c_float, ci, vp, ci, vp]
            L.ds_dpt_head_tail_circular.argtypes = L.ds_dpt_head_tail.argtypes
            L.ds_dpt_head_front.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
            L.ds_preprocess_bicubic.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_float),
                                                ctypes.POINTER(ctypes.c_float), ci, vp]
            L.ds_preprocess_bicubic_rows.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_float),
                                                     ctypes.POINTER(ctypes.c_float), ci, ci, ci, ci, vp]
            L.ds_tokens_fixup.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]
            L.ds_upsample_bicubic_to_f32.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
            L.ds_im2col3x3_s2_nhwc.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
            L.ds_reassemble_readout.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
            L.ds_bias_act_nhwc.argtypes = [vp, vp, vp, vp, vp, vp, i64, ci, ci, ci, vp]
            L.ds_group_norm_nchw.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, ci, ci, vp]
            L.ds_linear.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, ci, ci, vp]
            L.ds_linear_residual.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, ci, vp]
            L.ds_linear_vt.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, ci, vp]
            L.ds_linear_qkv.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, ci, vp]
            L.ds_conv3x3_nhwc.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
            L.ds_conv3x3_nhwc_circular.argtypes = L.ds_conv3x3_nhwc.argtypes
            L.ds_conv3x3_nhwc_pair.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
            L.ds_linear_shuffle.argtypes = [vp, vp, vp, vp, vp, i64, i64, ci, ci, ci, ci, vp]
            L.ds_linear_readout.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, ci, vp]
            L.ds_linear_rows4.argtypes = [vp, ctypes.POINTER(ds_rows_problem), ci, i64, i64, i64, ci, vp]
            L.ds_row_stats.argtypes = [vp, vp, vp, i64, ci, ctypes.c_float, ci, vp]
            L.ds_linear_ln.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, ci, ci, vp]
            L.ds_linear_vt_ln.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, ci, vp]
            L.ds_gconv3x3_nhwc_f32.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
            L.ds_add_relu_f32.argtypes = [vp, vp, vp, vp, i64, vp]
            L.ds_bias_act_f32.argtypes = [vp, vp, vp, vp, vp, i64, ci, ci, vp]
            L.ds_relu_cat_f32.argtypes = [vp, vp, vp, vp, ci, i64, ci, ci, ci, vp]
            L.ds_dwconv_nhwc.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]
            L.ds_resize_lanczos.argtypes = [vp, vp, ci, ci, ci, ci, i64, i64, i64, vp, ci, ci, vp, vp, ci, vp, vp, ci, vp, vp]
            L.ds_custom_depth_to_f64.argtypes = [vp, vp, ci, ci, ci, ci, i64, i64, i64, ci, vp, vp, vp]
            L.ds_kernel_timer_enable.argtypes = [vp, ci]
            L.ds_kernel_timer_read.argtypes = [vp, ci, ctypes.POINTER(i64), ctypes.POINTER(cd)]
            L.ds_kernel_timer_read_each.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_float), i64, ctypes.POINTER(i64)]
            L.ds_profile_enable.argtypes = [vp, ci]
            L.ds_profile_last_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
            for name in EXPORTS:          # fail at load time, not at first use, if a symbol is missing
                getattr(L, name)
            _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise DepthStereoError(f"libdepthstereo_hip error {rc}: {lib().ds_last_error().decode(errors='replace')}")


_ctxs = {}


def ctx_for(device_index):
    """One ds_ctx per (thread, device)."""
    key = (threading.get_ident(), int(device_index))
    c = _ctxs.get(key)
    if c is None:
        h = ctypes.c_void_p()
        _check(lib().ds_ctx_create(ctypes.byref(h), int(device_index)))
        _ctxs[key] = c = h
    return c


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise DepthStereoError("no MI355X visible to torch (torch.cuda.is_available() is False); "
                               "this package has no CPU path")
    return torch


def _stream(t):
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dev_index(t):
    torch = _torch()
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _depth_dtype_id(t):
    torch = _torch()
    if t.dtype in (torch.uint16, torch.int16):
        return DS_DEPTH_U16
    if t.dtype == torch.float32:
        return DS_DEPTH_F32
    if t.dtype == torch.float64:
        return DS_DEPTH_F64
    raise DepthStereoError(f"unsupported device depth dtype {t.dtype}")


# ------------------------------------------------------------------------------------------------
def depth_minmax(depth):
    """Per-image {min,max} (float64, on device) of a [N,H,W] depth tensor."""
    torch = require_gpu()
    n, h, w = depth.shape
    out = torch.empty((n, 2), dtype=torch.float64, device=depth.device)
    CALLS["ds_depth_minmax"] += 1
    _check(lib().ds_depth_minmax(ctx_for(_dev_index(depth)), depth.data_ptr(), _depth_dtype_id(depth), n, h, w,
                                 out.data_ptr(), _stream(depth)))
    return out


def build_pow_lut(depth_u16, exponent):
    """norm**exponent for every uint16 code of every image, computed on the HOST with libm pow
    (what `normalized_depth[row][col] ** stereo_offset_exponent` does, stereoimage_generation.py:108,182)."""
    torch = require_gpu()
    mm = depth_minmax(depth_u16).cpu().numpy()
    n = mm.shape[0]
    lut = np.zeros((n, 65536), np.float64)
    codes = np.arange(65536, dtype=np.float64)
    for i in range(n):
        mn, mx = mm[i]
        if not mx > mn:
            lut[i, :] = np.nan
            continue
        norm = (codes - mn) / (mx - mn)
        lo, hi = int(mn), int(mx)
        vals = [math.pow(x, exponent) for x in norm[lo:hi + 1].tolist()]
        lut[i, lo:hi + 1] = vals
    return torch.from_numpy(lut).to(depth_u16.device)


def stereo_warp(image, depth, eyes, fill, exponent=1.0, pow_lut=None):
    """image [N,H,W,C] uint8, depth [N,H,W]; eyes = list of (divergence_px, separation_px, out_tensor_view_ptr,
    row_stride_bytes, img_stride_bytes)."""
    require_gpu()
    assert image.is_contiguous() and depth.is_contiguous()
    n, h, w, c = image.shape
    arr = (ds_eye * len(eyes))()
    for i, (dv, sp, ptr, rs, is_) in enumerate(eyes):
        arr[i].divergence_px = float(dv)
        arr[i].separation_px = float(sp)
        arr[i].out = ptr
        arr[i].out_row_stride = int(rs)
        arr[i].out_img_stride = int(is_)
    CALLS["ds_stereo_warp"] += 1
    _check(lib().ds_stereo_warp(ctx_for(_dev_index(image)), image.data_ptr(), depth.data_ptr(), _depth_dtype_id(depth),
                                n, h, w, c, float(exponent), pow_lut.data_ptr() if pow_lut is not None else None,
                                FILL_IDS[fill], arr, len(eyes), _stream(image)))


def last_exact_rows(image):
    v = ctypes.c_int64(0)
    _check(lib().ds_stereo_last_exact_rows(ctx_for(_dev_index(image)), ctypes.byref(v), _stream(image)))
    return int(v.value)


def last_stats(image):
    """(rows re-rendered by the exact sweep, queue chunks of general pixels) of the last polylines call."""
    v = (ctypes.c_int64 * 2)()
    _check(lib().ds_stereo_last_stats(ctx_for(_dev_index(image)), v, _stream(image)))
    return int(v[0]), int(v[1])


def profile_enable(device_index, enable=True):
    _check(lib().ds_profile_enable(ctx_for(device_index), 1 if enable else 0))


def profile_last_ms(device_index):
    """(render_kernel_ms, exact_fallback_ms) of the most recent ds_stereo_warp on this thread's ctx."""
    a, b = ctypes.c_float(0), ctypes.c_float(0)
    _check(lib().ds_profile_last_ms(ctx_for(device_index), ctypes.byref(a), ctypes.byref(b)))
    return float(a.value), float(b.value)


def copy_view(src_ptr, src_rs, src_is, dst_ptr, dst_rs, dst_is, n, h, row_bytes, like):
    CALLS["ds_copy_view"] += 1
    _check(lib().ds_copy_view(ctx_for(_dev_index(like)), src_ptr, src_rs, src_is, dst_ptr, dst_rs, dst_is, n, h, row_bytes,
                              _stream(like)))


def overlap_red_cyan(im1_ptr, r1, i1, im2_ptr, r2, i2, n, h, w, c, out):
    CALLS["ds_overlap_red_cyan"] += 1
    _check(lib().ds_overlap_red_cyan(ctx_for(_dev_index(out)), im1_ptr, r1, i1, im2_ptr, r2, i2, n, h, w, c, out.data_ptr(),
                                     _stream(out)))


def normalmap(depth, pre_blur, sobel_ksize, post_blur, invert, wrap=False):
    """depth [n,h,w]: uint16 (the funnel's depth maps; the fused kernel), float64 (any other dtype, cast by the caller), float32
    with np.gradient (the reference's float32 evaluation: ds_normalmap_gradient_f32 / ds_normalmap_gradient_blur_f32) or float16
    with np.gradient and no blur (numpy's float16 evaluation: ds_normalmap_gradient_f16).
    wrap: the depth map is one period of a tiling -- the `_wrap` entry point of the same name (include/depthstereo.h: every tap index
    modulo the image size, np.gradient's central difference at every pixel) instead of the reference's borders."""
    torch = require_gpu()
    n, h, w = depth.shape
    assert depth.dtype in (torch.uint16, torch.float64, torch.float32, torch.float16) and depth.is_contiguous()
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=depth.device)
    pre_blur, sobel_ksize, post_blur = int(pre_blur), int(sobel_ksize), int(post_blur)
    # (entry point, its kernel-size arguments) by dtype
    if depth.dtype == torch.float16:
        assert pre_blur == 0 and post_blur == 0 and sobel_ksize == 0, "float16 depth: np.gradient without blurs only"
        name, sizes = "ds_normalmap_gradient_f16", ()
    elif depth.dtype == torch.float32:
        assert sobel_ksize == 0, "float32 depth: np.gradient only (cv2.Sobel is fed float64)"
        if pre_blur == 0 and post_blur == 0:
            name, sizes = "ds_normalmap_gradient_f32", ()
        else:
            name, sizes = "ds_normalmap_gradient_blur_f32", (pre_blur, post_blur)
    else:
        name, sizes = ("ds_normalmap" if depth.dtype == torch.uint16 else "ds_normalmap_f64"), (pre_blur, sobel_ksize, post_blur)
    if wrap:
        name += "_wrap"
    CALLS[name] += 1
    _check(getattr(lib(), name)(ctx_for(_dev_index(depth)), depth.data_ptr(), n, h, w, *sizes, 1 if invert else 0,
                                out.data_ptr(), _stream(depth)))
    return out


# ---- the bilateral family: the normal map's pre-filter and depth refinement (csrc/ds_bilateral.hip: one tile routine, two kernels), video
# mode's temporal depth filter (csrc/ds_video.hip); csrc/ds_bilateral.h holds what the three kernels share.  Public interfaces:
# src/normalmap_generation.py, src/depth_refine.py, src/video_mode.py --------------------------------------------------------------------
_TABLES = collections.defaultdict(collections.OrderedDict)     # family -> {(device index, parameters ...): tensors on that device}, LRU
_TABLES_LOCK = threading.Lock()
DEPTH_REFINE_MAX_ITERATIONS = 8
STABILIZE_MAX_RADIUS = 4


def _tables_on(family, device, params, build, keep=4):
    """build(*params) -- NumPy arrays -- as tensors on the cuda `device`: uploaded once and kept for the family's last `keep`
    (device, params).  The family is part of the key: equal parameter tuples of two families name different tables, and a family
    evicts only its own."""
    torch = _torch()
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(),) + tuple(params)
    with _TABLES_LOCK:
        lru = _TABLES[family]
        tabs = lru.get(key)
        if tabs is None:
            tabs = lru[key] = tuple(torch.from_numpy(t).to(device) for t in build(*params))
            while len(lru) > keep:
                lru.popitem(last=False)
        else:
            lru.move_to_end(key)
    for t in tabs:                   # an evicted table may still be read by a launch on this stream: tell the allocator
        t.record_stream(torch.cuda.current_stream(device))
    return tabs


def cached_tables(family):
    """How many (device, params) the table cache holds for `family`: "bilateral", "depth_refine", "sparse_bilateral", "aomap", "lensblur",
    "stabilize" or "lanczos"."""
    with _TABLES_LOCK:
        return len(_TABLES[family])


def _as_int(v):
    """(int(v), whether v IS that integer and no bool, Python's or NumPy's).  Raises what int(v) raises."""
    return int(v), not isinstance(v, (bool, np.bool_)) and int(v) == v


def _filter_params(name, usage, p, size, lo, hi, odd, sigmas, max_iterations=None):
    """The validator behind bilateral_params, depth_refine_params and stabilize_params.  p: (size, sigma, sigma) or -- where
    max_iterations is given -- (size, sigma, sigma, iterations); returns it as (int, float, float[, int]) or raises ValueError:
    size an integer in lo..hi (odd where `odd`), both sigmas finite and > 0, iterations an integer in 1..max_iterations (default
    1); a bool is no integer.  `name`, `usage`, `size` and `sigmas` are the words of the messages."""
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in ((3, 4) if max_iterations else (3,)):
            raise TypeError
        (n, ok_n), s0, s1 = _as_int(q[0]), float(q[1]), float(q[2])
        it, ok_it = _as_int(q[3]) if len(q) == 4 else (1, True)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s must be %s, got %r" % (name, usage, p)) from None
    if not (ok_n and lo <= n <= hi and (n % 2 == 1 or not odd)):
        raise ValueError("%s: %s must be an %sinteger in %d..%d, got %r" % (name, size, "odd " if odd else "", lo, hi, q[0]))
    if not (0.0 < s0 < math.inf and 0.0 < s1 < math.inf):
        raise ValueError("%s: %s and %s must be finite and > 0, got %r, %r" % (name, sigmas[0], sigmas[1], s0, s1))
    if not max_iterations:
        return n, s0, s1
    if not (ok_it and 1 <= it <= max_iterations):
        raise ValueError("%s: iterations must be an integer in 1..%d, got %r" % (name, max_iterations, q[3] if len(q) == 4 else it))
    return n, s0, s1, it


def bilateral_params(bilateral):
    """(d, sigma_color, sigma_space) as (int, float, float), or ValueError: d odd in 3..31, both sigmas finite and > 0.  Pure
    Python (the funnel checks its option with it before any device work)."""
    return _filter_params("bilateral", "(d, sigma_color, sigma_space)", bilateral, "d", 3, 31, True, ("sigma_color", "sigma_space"))


def depth_refine_params(p):
    """(d, sigma_color, sigma_space) or (d, sigma_color, sigma_space, iterations) as (int, float, float, int), or ValueError: d odd in
    3..31, both sigmas finite and > 0, iterations an integer in 1..8 (default 1); a bool is no integer.  Pure Python (the funnel
    checks its option with it before any device work)."""
    return _filter_params("depth_refine", "(d, sigma_color, sigma_space) or (d, sigma_color, sigma_space, iterations)", p, "d", 3, 31, True,
                          ("sigma_color", "sigma_space"), DEPTH_REFINE_MAX_ITERATIONS)


def stabilize_params(params):
    """(radius, sigma_color, sigma_time) as (int, float, float), or ValueError: radius an integer in 1..4 (a bool is no integer), both
    sigmas finite and > 0.  Pure Python (gen_frames_sharded checks its option with it before any device work)."""
    return _filter_params("stabilize", "(radius, sigma_color, sigma_time)", params, "radius", 1, STABILIZE_MAX_RADIUS, False,
                          ("sigma_color", "sigma_time"))


def spatial_weight_table(d, sigma_space):
    """ws of ds_bilateral_u16 and ds_joint_bilateral_u16: d * d float64 in raster order, exp(-(dx^2 + dy^2) / (2 sigma_space^2)) inside
    the circle of radius d // 2, exactly 0 outside."""
    r = d // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    return np.where(dx * dx + dy * dy <= r * r, np.exp(-(dx * dx + dy * dy) / (2.0 * sigma_space**2)), 0.0).astype(np.float64).ravel()


def color_weight_table(sigma_color):
    """wc of ds_joint_bilateral_u16 and ds_temporal_joint_bilateral_u16: 766 float64, wc[k] = exp(-k^2 / (2 sigma_color^2)), indexed by
    the integer |dR| + |dG| + |dB| of two guide pixels."""
    return np.exp(-(np.arange(766, dtype=np.float64)**2) / (2.0 * sigma_color**2))


def bilateral_tables(d, sigma_color, sigma_space):
    """The two host-made tables of ds_bilateral_u16 (include/depthstereo.h), float64: ws (spatial_weight_table) and wr (65536,
    indexed by the integer |D(q) - D(p)|)."""
    return spatial_weight_table(d, sigma_space), np.exp(-(np.arange(65536, dtype=np.float64)**2) / (2.0 * sigma_color**2))


def depth_refine_tables(d, sigma_color, sigma_space):
    """The two host-made tables of ds_joint_bilateral_u16 (include/depthstereo.h), float64: ws (spatial_weight_table) and wc
    (color_weight_table)."""
    return spatial_weight_table(d, sigma_space), color_weight_table(sigma_color)


def temporal_joint_bilateral_tables(radius, sigma_color, sigma_time):
    """The two host-made tables of ds_temporal_joint_bilateral_u16 (include/depthstereo.h), float64: wt (radius + 1,
    wt[a] = exp(-a^2 / (2 sigma_time^2)), wt[0] == 1.0) and wc (color_weight_table: depth refinement's table)."""
    wt = np.exp(-(np.arange(radius + 1, dtype=np.float64)**2) / (2.0 * sigma_time**2))
    return wt, color_weight_table(sigma_color)


def stabilize_tables_on(device, radius, sigma_color, sigma_time):
    """(wt, wc) of temporal_joint_bilateral_tables as float64 tensors on `device`; on a GPU they are uploaded once and kept for the
    last 4 (device, radius, sigma_color, sigma_time)."""
    torch = _torch()
    if torch.device(device).type != "cuda":
        return tuple(torch.from_numpy(t) for t in temporal_joint_bilateral_tables(radius, sigma_color, sigma_time))
    return _tables_on("stabilize", device, (radius, sigma_color, sigma_time), temporal_joint_bilateral_tables)


def _check_depth_guide(name, depth_u16, guide_u8=None, contiguous=False):
    """DepthStereoError unless depth is a uint16 cuda tensor [n,h,w] and -- where given -- guide a uint8 cuda tensor [n,h,w,3 or 4] on
    the depth's device and of its size; contiguous: both must already be dense (a caller that may copy calls .contiguous() itself)."""
    torch = _torch()
    dense = "contiguous " if contiguous else ""
    if not (torch.is_tensor(depth_u16) and depth_u16.is_cuda and depth_u16.dtype == torch.uint16 and depth_u16.dim() == 3
            and (depth_u16.is_contiguous() or not contiguous)):
        raise DepthStereoError("%s: depth must be a %suint16 cuda tensor [n,h,w], got %s %s"
                               % (name, dense, getattr(depth_u16, "dtype", type(depth_u16)), tuple(getattr(depth_u16, "shape", ()))))
    if guide_u8 is None:
        return
    if not (torch.is_tensor(guide_u8) and guide_u8.is_cuda and guide_u8.dtype == torch.uint8 and guide_u8.dim() == 4
            and guide_u8.device == depth_u16.device and tuple(guide_u8.shape[:3]) == tuple(depth_u16.shape) and guide_u8.shape[3] in (3, 4)
            and (guide_u8.is_contiguous() or not contiguous)):
        raise DepthStereoError("%s: guide must be a %suint8 cuda tensor [n,h,w,3 or 4] on the depth's device and of its size %s, got %s %s"
                               % (name, dense, tuple(depth_u16.shape), getattr(guide_u8, "dtype", type(guide_u8)),
                                  tuple(getattr(guide_u8, "shape", ()))))


def bilateral_u16(depth_u16, d, sigma_color, sigma_space, wrap=False):
    """Bilateral filter of uint16 depth maps [n,h,w] (cuda) -> float64 [n,h,w] in the same units (ds_bilateral_u16: the definition is
    in include/depthstereo.h).  d: odd window diameter 3..31; sigma_color in uint16 levels (the range table is indexed by an integer
    difference); sigma_space in pixels; wrap: tap indices modulo the image size instead of BORDER_REFLECT_101 (which needs
    d // 2 < min(h, w)).  The tables are made on the host, uploaded once and kept for the last 4 (device, d, sigma_color,
    sigma_space)."""
    torch = require_gpu()
    try:
        d, sigma_color, sigma_space = bilateral_params((d, sigma_color, sigma_space))
    except ValueError as e:
        raise DepthStereoError("bilateral_u16: %s" % e) from None
    _check_depth_guide("bilateral_u16", depth_u16)
    depth_u16 = depth_u16.contiguous()
    n, h, w = depth_u16.shape
    if not wrap and d // 2 >= min(h, w):
        raise DepthStereoError("bilateral_u16: d // 2 = %d must be below min(h, w) = %d without wrap" % (d // 2, min(h, w)))
    ws, wr = _tables_on("bilateral", depth_u16.device, (d, sigma_color, sigma_space), bilateral_tables)
    out = torch.empty((n, h, w), dtype=torch.float64, device=depth_u16.device)
    CALLS["ds_bilateral_u16"] += 1
    _check(lib().ds_bilateral_u16(ctx_for(_dev_index(depth_u16)), depth_u16.data_ptr(), n, h, w, d // 2, ws.data_ptr(),
                                  wr.data_ptr(), 1 if wrap else 0, out.data_ptr(), _stream(depth_u16)))
    return out


def joint_bilateral_u16(depth_u16, guide_u8, d, sigma_color, sigma_space, iterations=1, wrap=False):
    """Joint bilateral filter of uint16 depth maps [n,h,w] (cuda) guided by uint8 images [n,h,w,c], c in {3, 4} (cuda, same device,
    any byte alignment; only the first three channels are read) -> uint16 [n,h,w] (ds_joint_bilateral_u16: the definition is in
    include/depthstereo.h).  d: odd window diameter 3..31; sigma_color in units of summed 8-bit channel difference; sigma_space in
    pixels; iterations 1..8: pass i + 1 filters the result of pass i with the same guide (one launch each, between two buffers);
    wrap: tap indices modulo the image size instead of BORDER_REFLECT_101 (which needs d // 2 < min(h, w)).  The tables are made on
    the host, uploaded once and kept for the last 4 (device, d, sigma_color, sigma_space)."""
    torch = require_gpu()
    try:
        d, sigma_color, sigma_space, iterations = depth_refine_params((d, sigma_color, sigma_space, iterations))
    except ValueError as e:
        raise DepthStereoError("joint_bilateral_u16: %s" % e) from None
    _check_depth_guide("joint_bilateral_u16", depth_u16, guide_u8)
    depth_u16, guide_u8 = depth_u16.contiguous(), guide_u8.contiguous()
    n, h, w = depth_u16.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("joint_bilateral_u16: empty depth %s" % (tuple(depth_u16.shape),))
    if not wrap and d // 2 >= min(h, w):
        raise DepthStereoError("joint_bilateral_u16: d // 2 = %d must be below min(h, w) = %d without wrap" % (d // 2, min(h, w)))
    ws, wc = _tables_on("depth_refine", depth_u16.device, (d, sigma_color, sigma_space), depth_refine_tables)
    src = depth_u16
    bufs = [torch.empty((n, h, w), dtype=torch.uint16, device=depth_u16.device) for _ in range(min(iterations, 2))]
    for i in range(iterations):
        out = bufs[i & 1]
        CALLS["ds_joint_bilateral_u16"] += 1
        _check(lib().ds_joint_bilateral_u16(ctx_for(_dev_index(depth_u16)), src.data_ptr(), guide_u8.data_ptr(), guide_u8.shape[3], n, h, w,
                                            d // 2, ws.data_ptr(), wc.data_ptr(), 1 if wrap else 0, out.data_ptr(),
                                            _stream(depth_u16)))
        src = out
    return src


# ---- the 3D-photo depth preparation (csrc/ds_sparse_bilateral.hip; public interface: inpaint/bilateral_filtering.py) ----------------
SPARSE_BILATERAL_MAX_WINDOW = 15


def sparse_bilateral_rank_table(nmax=225):
    """rank of ds_sparse_bilateral_f32 (include/depthstereo.h): nmax + 1 int32, rank[n] = which of n equally weighted taps, in ascending
    order, the reference's weighted median picks.  These are the reference's own NumPy calls on n float32 ones -- a float32 running sum
    of 1 / n cut at 0.5 -- and NOT n // 2; no closed form is used anywhere."""
    rank = np.zeros(nmax + 1, np.int32)
    for n in range(1, nmax + 1):
        c = np.ones(n, np.float32)
        rank[n] = np.digitize(0.5, np.cumsum(c / c.sum()))
    return rank


def _sparse_bilateral_tables(nmax):
    return (sparse_bilateral_rank_table(nmax),)


def sparse_bilateral_windows(window_sizes):
    """window_sizes as a list of ints, or ValueError: at least one, each an odd integer in 1..15 (a bool is no integer).  Pure Python."""
    try:
        if isinstance(window_sizes, (str, bytes)):
            raise TypeError
        got = [_as_int(s) for s in window_sizes]
    except (TypeError, ValueError, OverflowError):
        raise ValueError("window sizes must be a sequence of integers, got %r" % (window_sizes,)) from None
    if not got:
        raise ValueError("window sizes: at least one pass is needed")
    for (s, ok), given in zip(got, window_sizes):
        if not (ok and 1 <= s <= SPARSE_BILATERAL_MAX_WINDOW and s % 2 == 1):
            raise ValueError("window size must be an odd integer in 1..%d, got %r" % (SPARSE_BILATERAL_MAX_WINDOW, given))
    return [s for s, _ in got]


def _check_sparse_map(name, depth_f32):
    torch = _torch()
    if not (torch.is_tensor(depth_f32) and depth_f32.is_cuda and depth_f32.dtype == torch.float32 and depth_f32.dim() == 3
            and depth_f32.is_contiguous()):
        raise DepthStereoError("%s: depth must be a contiguous float32 cuda tensor [n,h,w], got %s %s"
                               % (name, getattr(depth_f32, "dtype", type(depth_f32)), tuple(getattr(depth_f32, "shape", ()))))
    n, h, w = depth_f32.shape
    if n < 1 or h < 3 or w < 3:
        raise DepthStereoError("%s: needs n >= 1 and h, w >= 3, got %s" % (name, tuple(depth_f32.shape)))
    return n, h, w


def sparse_bilateral_pass_f32(v, v0, window, threshold):
    """One pass (ds_sparse_bilateral_f32, include/depthstereo.h): v, v0 contiguous float32 cuda [n,h,w] (v0 the map of the first pass;
    v0 is v is legal) -> (the filtered map float32 [n,h,w], the jump map of v uint8 [n,h,w])."""
    torch = require_gpu()
    n, h, w = _check_sparse_map("sparse_bilateral_pass_f32", v)
    if v0 is not v:
        if _check_sparse_map("sparse_bilateral_pass_f32", v0) != (n, h, w) or v0.device != v.device:
            raise DepthStereoError("sparse_bilateral_pass_f32: v0 must have v's shape %s and device" % ((n, h, w),))
    try:
        window, = sparse_bilateral_windows([window])
    except ValueError as e:
        raise DepthStereoError("sparse_bilateral_pass_f32: %s" % e) from None
    rank, = _tables_on("sparse_bilateral", v.device, (SPARSE_BILATERAL_MAX_WINDOW**2,), _sparse_bilateral_tables, keep=1)
    out = torch.empty((n, h, w), dtype=torch.float32, device=v.device)
    jump = torch.empty((n, h, w), dtype=torch.uint8, device=v.device)
    CALLS["ds_sparse_bilateral_f32"] += 1
    _check(lib().ds_sparse_bilateral_f32(ctx_for(_dev_index(v)), v.data_ptr(), v0.data_ptr(), n, h, w, window, float(threshold),
                                         rank.data_ptr(), out.data_ptr(), jump.data_ptr(), _stream(v)))
    return out, jump


def sparse_bilateral_jump_f32(v, threshold):
    """The jump map alone (ds_sparse_bilateral_jump_f32): v contiguous float32 cuda [n,h,w] -> uint8 [n,h,w]."""
    torch = require_gpu()
    n, h, w = _check_sparse_map("sparse_bilateral_jump_f32", v)
    jump = torch.empty((n, h, w), dtype=torch.uint8, device=v.device)
    CALLS["ds_sparse_bilateral_jump_f32"] += 1
    _check(lib().ds_sparse_bilateral_jump_f32(ctx_for(_dev_index(v)), v.data_ptr(), n, h, w, float(threshold), jump.data_ptr(), _stream(v)))
    return jump


def sparse_bilateral_f32(depth_f32, window_sizes, threshold):
    """The passes of sparse_bilateral_filtering on float32 depth maps [n,h,w] (cuda, contiguous): pass i has the odd window
    window_sizes[i] in 1..15 and filters the result of pass i - 1 (the first one: depth_f32).  Returns (maps, jumps), two lists of
    len(window_sizes) device tensors: maps[i] float32, the INPUT of pass i (maps[0] is depth_f32 itself), and jumps[i] uint8, the jump
    map of maps[i] at `threshold` (float32).  One filter launch per pass except the last, whose output nothing asks for: that pass
    makes its jump map alone.  Precondition: every value finite and >= 0 (include/depthstereo.h; the caller checks -- a device-side
    test would cost a synchronisation)."""
    require_gpu()
    _check_sparse_map("sparse_bilateral_f32", depth_f32)
    try:
        windows = sparse_bilateral_windows(window_sizes)
        threshold = float(threshold)
    except (TypeError, ValueError) as e:
        raise DepthStereoError("sparse_bilateral_f32: %s" % e) from None
    maps, jumps = [depth_f32], []
    for window in windows[:-1]:
        out, jump = sparse_bilateral_pass_f32(maps[-1], depth_f32, window, threshold)
        maps.append(out)
        jumps.append(jump)
    jumps.append(sparse_bilateral_jump_f32(maps[-1], threshold))
    return maps, jumps


# ---- ambient-occlusion maps (csrc/ds_aomap.hip; public interface: src/aomap_generation.py) ------------------------------------------
AOMAP_MAX_RADIUS = 32
AOMAP_DIRECTIONS = (4, 8, 16)


def aomap_params(p):
    """(radius, directions, relief) or (radius, directions, relief, intensity) as (int, int, float, float), or ValueError: radius an
    integer in 1..32, directions one of 4, 8, 16 (a bool is no integer), relief and intensity finite and > 0 (intensity defaults to
    1.0).  Pure Python (the funnel checks its option with it before any device work)."""
    usage = "(radius, directions, relief) or (radius, directions, relief, intensity)"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in (3, 4):
            raise TypeError
        (radius, ok_r), (directions, ok_k), relief = _as_int(q[0]), _as_int(q[1]), float(q[2])
        intensity = float(q[3]) if len(q) == 4 else 1.0
    except (TypeError, ValueError, OverflowError):
        raise ValueError("aomap must be %s, got %r" % (usage, p)) from None
    if not (ok_r and 1 <= radius <= AOMAP_MAX_RADIUS):
        raise ValueError("aomap: radius must be an integer in 1..%d, got %r" % (AOMAP_MAX_RADIUS, q[0]))
    if not (ok_k and directions in AOMAP_DIRECTIONS):
        raise ValueError("aomap: directions must be 4, 8 or 16, got %r" % (q[1],))
    if not (0.0 < relief < math.inf and 0.0 < intensity < math.inf):
        raise ValueError("aomap: relief and intensity must be finite and > 0, got %r, %r" % (relief, intensity))
    return radius, directions, relief, intensity


def aomap_offsets(radius, directions):
    """The ray table of ds_aomap_u16 (include/depthstereo.h): (taps, dir_start), taps int32 [T, 2] of (dx, dy) ray after ray in
    increasing step, dir_start int32 [directions + 1].  Ray k is point k * 16 / directions of the 16-point rose; its steps s = 1..radius
    are (s, 0), (s, m), (s, s) or (m, s) with m = rint(s * (sqrt(2) - 1)), turned by quarter turns (x, y) -> (-y, x), and kept inside
    the circle dx^2 + dy^2 <= radius^2."""
    s = np.arange(1, radius + 1, dtype=np.int64)
    m = np.rint(s * (np.sqrt(2.0) - 1.0)).astype(np.int64)
    base = (np.stack([s, 0 * s], 1), np.stack([s, m], 1), np.stack([s, s], 1), np.stack([m, s], 1))
    quarter = np.array([[0, 1], [-1, 0]], dtype=np.int64)               # row vector (x, y) @ quarter = (-y, x)
    rays = []
    for k in range(directions):
        turns, pos = divmod(k * 16 // directions, 4)
        ray = base[pos] @ np.linalg.matrix_power(quarter, turns)
        rays.append(ray[(ray * ray).sum(1) <= radius * radius])
    dir_start = np.concatenate([[0], np.cumsum([len(r) for r in rays])]).astype(np.int32)
    return np.concatenate(rays).astype(np.int32).reshape(-1, 2), dir_start


def aomap_u16(depth_u16, radius, directions, relief, intensity=1.0, invert=False, wrap=False, want_f64=False, out=None):
    """Ambient-occlusion maps of uint16 depth maps [n,h,w] (cuda) taken as height fields -> uint8 [n,h,w], 255 = open sky
    (ds_aomap_u16: the definition is in include/depthstereo.h).  radius 1..32 pixels; directions 4, 8 or 16; relief: the height in
    pixels that the full uint16 range stands for; intensity scales the occlusion; invert: black is high; wrap: tap indices modulo
    the image size instead of skipping taps outside the image.  want_f64: return (uint8 map, the unclamped float64 value) instead.
    out: write the uint8 map into this contiguous uint8 cuda tensor [n,h,w].  The ray table is made on the host, uploaded once and
    kept for the last 4 (device, radius, directions)."""
    torch = require_gpu()
    try:
        radius, directions, relief, intensity = aomap_params((radius, directions, relief, intensity))
    except ValueError as e:
        raise DepthStereoError("aomap_u16: %s" % e) from None
    _check_depth_guide("aomap_u16", depth_u16)
    depth_u16 = depth_u16.contiguous()
    n, h, w = depth_u16.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("aomap_u16: empty depth %s" % (tuple(depth_u16.shape),))
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.uint8, device=depth_u16.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == depth_u16.device and tuple(out.shape) == (n, h, w)
              and out.is_contiguous()):
        raise DepthStereoError("aomap_u16: out must be a contiguous uint8 tensor %s on the depth's device" % ((n, h, w),))
    taps, dir_start = _tables_on("aomap", depth_u16.device, (radius, directions), aomap_offsets)
    out_f64 = torch.empty((n, h, w), dtype=torch.float64, device=depth_u16.device) if want_f64 else None
    CALLS["ds_aomap_u16"] += 1
    _check(lib().ds_aomap_u16(ctx_for(_dev_index(depth_u16)), depth_u16.data_ptr(), n, h, w, radius, directions, taps.data_ptr(),
                              dir_start.data_ptr(), relief / 65535.0, intensity / directions, 1 if invert else 0, 1 if wrap else 0,
                              out.data_ptr(), out_f64.data_ptr() if want_f64 else None, _stream(depth_u16)))
    return (out, out_f64) if want_f64 else out


# ---- lens blur from depth (csrc/ds_lensblur.hip; public interface: src/lensblur_generation.py) --------------------------------------
LENSBLUR_MAX_RADIUS = 32


def _lensblur_focus(focus):
    """focus as an int in 0..65535 or ('point', fx, fy) with fx, fy floats in [0, 1]; raises TypeError / ValueError otherwise."""
    if isinstance(focus, (tuple, list)):
        if len(focus) != 3 or focus[0] != 'point':
            raise TypeError
        fx, fy = float(focus[1]), float(focus[2])
        if not (0.0 <= fx <= 1.0 and 0.0 <= fy <= 1.0):
            raise ValueError
        return ('point', fx, fy)
    if isinstance(focus, (str, bytes)):
        raise TypeError
    value, ok = _as_int(focus)
    if not (ok and 0 <= value <= 65535):
        raise ValueError
    return value


def _focus_on_device(name, focus, depth_u16):
    """The focus depths of a dense uint16 cuda batch [n,h,w] as a uint16 tensor [n] on its device, without a host sync.  focus: one
    integer 0..65535 for every image, n of them, a uint16 cuda tensor [n], or ('point', fx, fy): each image's depth at
    [min(h - 1, floor(fy h)), min(w - 1, floor(fx w))].  Anything else is a DepthStereoError in `name`'s name.  Shared by lensblur_u8
    and parallax_u8."""
    torch = _torch()
    n, h, w = depth_u16.shape
    dev = depth_u16.device
    if torch.is_tensor(focus):
        if not (focus.dtype == torch.uint16 and focus.device == dev and tuple(focus.shape) == (n,)):
            raise DepthStereoError("%s: a focus tensor must be uint16 [%d] on the depth's device, got %s %s"
                                   % (name, n, focus.dtype, tuple(focus.shape)))
        return focus.contiguous()
    try:
        many = isinstance(focus, (tuple, list, np.ndarray)) and not (len(focus) and isinstance(focus[0], str))
        values = [_lensblur_focus(f) for f in focus] if many else _lensblur_focus(focus)
        if many and (len(values) != n or any(isinstance(v, tuple) for v in values)):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise DepthStereoError("%s: focus must be an integer in 0..65535, %d of them, a uint16 tensor or ('point', fx, fy) "
                               "with fx, fy in [0, 1], got %r" % (name, n, focus)) from None
    if many:
        return torch.from_numpy(np.asarray(values, dtype=np.uint16)).to(dev)
    if isinstance(values, tuple):
        return depth_u16[:, min(h - 1, int(values[2] * h)), min(w - 1, int(values[1] * w))].contiguous()
    # (an int16 fill of the same 16 bits)
    return torch.full((n,), values - 65536 if values >= 32768 else values, dtype=torch.int16, device=dev).view(torch.uint16)


def lensblur_params(p):
    """(radius, aperture, focus) or (radius, aperture, focus, band) as (int, float, focus, int), or ValueError: radius an integer in
    1..32 and band an integer in 0..65535 (default 0; a bool is no integer); aperture a positive float, the blur radius in pixels that
    a depth difference of the full uint16 range would get, with rint(4 aperture) in 1..65535; focus an integer in 0..65535 (a depth in
    the map's own units) or ('point', fx, fy) with fx, fy in [0, 1] (the depth found at that position of each image).  Pure Python
    (the funnel checks its option with it before any device work)."""
    usage = "(radius, aperture, focus) or (radius, aperture, focus, band)"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in (3, 4):
            raise TypeError
        (radius, ok_r), aperture = _as_int(q[0]), float(q[1])
        band, ok_b = _as_int(q[3]) if len(q) == 4 else (0, True)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("lensblur must be %s, got %r" % (usage, p)) from None
    if not (ok_r and 1 <= radius <= LENSBLUR_MAX_RADIUS):
        raise ValueError("lensblur: radius must be an integer in 1..%d, got %r" % (LENSBLUR_MAX_RADIUS, q[0]))
    if not (0.0 < aperture < math.inf and 1 <= lensblur_quarter_pixels(aperture) <= 65535):
        raise ValueError("lensblur: aperture must be a positive float with rint(4 * aperture) in 1..65535, got %r" % (q[1],))
    try:
        focus = _lensblur_focus(q[2])
    except (TypeError, ValueError, OverflowError):
        raise ValueError("lensblur: focus must be an integer in 0..65535 or ('point', fx, fy) with fx, fy in [0, 1], got %r"
                         % (q[2],)) from None
    if not (ok_b and 0 <= band <= 65535):
        raise ValueError("lensblur: band must be an integer in 0..65535, got %r" % (q[3],))
    return radius, aperture, focus, band


def lensblur_quarter_pixels(aperture):
    """A of ds_lensblur_u8 for an aperture in pixels per full uint16 range: rint(4 aperture), half to even."""
    return int(np.rint(4.0 * aperture))


def lensblur_table(radius):
    """The weight table of ds_lensblur_u8 (include/depthstereo.h): a 1-tuple of uint32 [4 radius + 1], W[rho] = 2^20 // n(rho) with
    n(rho) the number of integer (dx, dy) with 16 (dx^2 + dy^2) <= rho^2."""
    dy, dx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    d2 = np.sort((16 * (dx * dx + dy * dy)).ravel())
    rho = np.arange(4 * radius + 1, dtype=np.int64)
    return ((2**20 // np.searchsorted(d2, rho * rho, side='right')).astype(np.uint32),)


def lensblur_u8(image_u8, depth_u16, radius, A, band, focus, invert=False, want_coc=False, out=None):
    """Lens blur of uint8 images [n,h,w,3] (cuda) by their uint16 depth maps [n,h,w] (same device) -> uint8 [n,h,w,3]
    (ds_lensblur_u8: the definition is in include/depthstereo.h).  radius 1..32: the largest blur radius in pixels; A 1..65535: quarter
    pixels of blur radius per full uint16 range of depth difference; band 0..65535: depth differences up to it stay sharp.  focus: one
    integer 0..65535 for every image, n of them, a uint16 cuda tensor [n], or ('point', fx, fy): each image's depth at
    [min(h - 1, floor(fy h)), min(w - 1, floor(fx w))], read on the device without a host sync.  invert: black is near.  want_coc:
    return (blurred, uint8 [n,h,w] circle of confusion in quarter pixels) instead.  out: write the image into this contiguous uint8
    cuda tensor [n,h,w,3].  The weight table is made on the host, uploaded once and kept for the last 4 (device, radius)."""
    torch = require_gpu()
    (radius, ok_r), (A, ok_a), (band, ok_b) = _as_int(radius), _as_int(A), _as_int(band)
    if not (ok_r and 1 <= radius <= LENSBLUR_MAX_RADIUS and ok_a and 1 <= A <= 65535 and ok_b and 0 <= band <= 65535):
        raise DepthStereoError("lensblur_u8: radius must be an integer in 1..%d, A in 1..65535, band in 0..65535, got %r, %r, %r"
                               % (LENSBLUR_MAX_RADIUS, radius, A, band))
    _check_depth_guide("lensblur_u8", depth_u16, image_u8)
    if image_u8.shape[3] != 3:
        raise DepthStereoError("lensblur_u8: image must have 3 channels, got %s" % (tuple(image_u8.shape),))
    image_u8, depth_u16 = image_u8.contiguous(), depth_u16.contiguous()
    n, h, w = depth_u16.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("lensblur_u8: empty depth %s" % (tuple(depth_u16.shape),))
    dev = depth_u16.device
    focus_t = _focus_on_device("lensblur_u8", focus, depth_u16)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == dev and tuple(out.shape) == (n, h, w, 3)
              and out.is_contiguous()):
        raise DepthStereoError("lensblur_u8: out must be a contiguous uint8 tensor %s on the depth's device" % ((n, h, w, 3),))
    (table,) = _tables_on("lensblur", dev, (radius,), lensblur_table)
    coc = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_coc else None
    CALLS["ds_lensblur_u8"] += 1
    _check(lib().ds_lensblur_u8(ctx_for(_dev_index(depth_u16)), image_u8.data_ptr(), depth_u16.data_ptr(), focus_t.data_ptr(), n, h, w,
                                radius, A, band, 1 if invert else 0, table.data_ptr(), out.data_ptr(),
                                coc.data_ptr() if want_coc else None, _stream(depth_u16)))
    return (out, coc) if want_coc else out


# ---- parallax frames from depth (csrc/ds_parallax.hip; public interface: src/parallax_generation.py) ---------------------------------
PARALLAX_MAX_FRAMES = 256
PARALLAX_MAX_SHIFT = 64.0            # pixels per full uint16 range of depth difference: 1024 sixteenths
PARALLAX_MAX_ZOOM = 0.25             # scale fraction per full range: 1024 / 4096
PARALLAX_MAX_FILL = 64
PARALLAX_POSE_MAX = 1024
PARALLAX_PATHS = ('circle', 'line')
PARALLAX_WS_BYTES = 256 << 20        # the key workspace of one ds_parallax_u8 call; more views than fit are rendered in several calls


def _as_float(v, limit):
    """float(v) for a number with |v| <= limit; a bool, a string, a NaN or an out-of-range value raises TypeError / ValueError."""
    if isinstance(v, (bool, np.bool_, str, bytes)):
        raise TypeError
    f = float(v)
    if not abs(f) <= limit:              # (a NaN fails this too)
        raise ValueError
    return f


def _parallax_frames(frames):
    if isinstance(frames, (str, bytes)):
        raise TypeError
    value, ok = _as_int(frames)
    if not (ok and 1 <= value <= PARALLAX_MAX_FRAMES):
        raise ValueError
    return value


def parallax_path(path, frames, shift_x, shift_y, zoom):
    """The camera path as float64 [F,3] of (x in pixels, y in pixels, z as a scale fraction), each per full uint16 range of depth
    difference.  path 'circle': (X cos a_k, Y sin a_k, Z cos a_k) with a_k = 2 pi k / F (Y = 0 is the reference's "swing");
    'line': from (-X, -Y, -Z) to (X, Y, Z), linear in k / (F - 1), the origin for F = 1; X, Y, Z = shift_x, shift_y, zoom.  Or an
    explicit array [F,3] of such triples: frames must then be None or F, and shift and zoom are not used.  Limits: |x|, |y| <= 64,
    |z| <= 0.25, 1 <= F <= 256.  Raises ValueError."""
    if isinstance(path, str):
        if path not in PARALLAX_PATHS:
            raise ValueError("parallax: path must be one of %r or an array [F,3], got %r" % (PARALLAX_PATHS, path))
        try:
            F = _parallax_frames(frames)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("parallax: frames must be an integer in 1..%d, got %r" % (PARALLAX_MAX_FRAMES, frames)) from None
        try:
            X, Y = _as_float(shift_x, PARALLAX_MAX_SHIFT), _as_float(shift_y, PARALLAX_MAX_SHIFT)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("parallax: shift must be two numbers with |shift| <= %g pixels, got %r, %r"
                             % (PARALLAX_MAX_SHIFT, shift_x, shift_y)) from None
        try:
            Z = _as_float(zoom, PARALLAX_MAX_ZOOM)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("parallax: zoom must be a number with |zoom| <= %g, got %r" % (PARALLAX_MAX_ZOOM, zoom)) from None
        k = np.arange(F, dtype=np.float64)
        if path == 'circle':
            a = 2.0 * np.pi * k / F
            return np.stack([X * np.cos(a), Y * np.sin(a), Z * np.cos(a)], axis=1)
        t = 2.0 * k / (F - 1) - 1.0 if F > 1 else np.zeros(1)
        return np.stack([X * t, Y * t, Z * t], axis=1)
    try:
        if isinstance(path, bytes) or path is None:
            raise TypeError
        arr = np.asarray(path)
        if arr.dtype.kind not in 'iuf' or arr.ndim != 2 or arr.shape[1] != 3 or not 1 <= arr.shape[0] <= PARALLAX_MAX_FRAMES:
            raise TypeError
        arr = arr.astype(np.float64)
        if frames is not None and _parallax_frames(frames) != arr.shape[0]:
            raise ValueError
        if not (np.abs(arr[:, :2]) <= PARALLAX_MAX_SHIFT).all() or not (np.abs(arr[:, 2]) <= PARALLAX_MAX_ZOOM).all():
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("parallax: an explicit path must be a numeric array [F,3] with 1 <= F <= %d (frames None or F), |x|, |y| <= %g "
                         "and |z| <= %g, got %r" % (PARALLAX_MAX_FRAMES, PARALLAX_MAX_SHIFT, PARALLAX_MAX_ZOOM, path)) from None
    return arr


def parallax_poses(path, frames, shift_x, shift_y, zoom):
    """poses of ds_parallax_u8 (include/depthstereo.h) for a camera path (parallax_path): int32 [F,3] of tx = rint(16 x),
    ty = rint(16 y), tz = rint(4096 z), half to even; every component within +-1024.  Raises ValueError."""
    p = parallax_path(path, frames, shift_x, shift_y, zoom)
    return np.rint(p * np.array([16.0, 16.0, 4096.0])).astype(np.int32)


def parallax_params(p):
    """(path, frames, shift_x, shift_y, zoom), (..., focus) or (..., focus, fill) as (path, int, float, float, float, focus, int), or
    ValueError.  path, frames, shift_x, shift_y, zoom: what parallax_path takes (an explicit path comes back as a float64 array,
    frames as its length); focus: an integer in 0..65535 or ('point', fx, fy) with fx, fy in [0, 1] (default ('point', 0.5, 0.5));
    fill: an integer in 1..64, the reach in pixels of the hole filling (default 32; a bool is no integer).  Pure Python (the funnel
    checks its option with it before any device work)."""
    usage = "(path, frames, shift_x, shift_y, zoom[, focus[, fill]])"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in (5, 6, 7):
            raise TypeError
    except TypeError:
        raise ValueError("parallax must be %s, got %r" % (usage, p)) from None
    path, frames = q[0], q[1]
    track = parallax_path(path, frames, q[2], q[3], q[4])
    if not isinstance(path, str):
        path, shift_x, shift_y, zoom = track, 0.0, 0.0, 0.0
    else:
        shift_x, shift_y, zoom = float(q[2]), float(q[3]), float(q[4])
    try:
        focus = _lensblur_focus(q[5]) if len(q) > 5 else ('point', 0.5, 0.5)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("parallax: focus must be an integer in 0..65535 or ('point', fx, fy) with fx, fy in [0, 1], got %r"
                         % (q[5],)) from None
    try:
        fill, ok = _as_int(q[6]) if len(q) > 6 else (32, True)
        if not (ok and 1 <= fill <= PARALLAX_MAX_FILL):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("parallax: fill must be an integer in 1..%d, got %r" % (PARALLAX_MAX_FILL, q[6])) from None
    return path, len(track), shift_x, shift_y, zoom, focus, fill


def parallax_u8(image_u8, depth_u16, poses, focus, fill, invert=False, want_mask=False, out=None):
    """F novel views of uint8 images [n,h,w,3] (cuda) by their uint16 depth maps [n,h,w] (same device) -> uint8 [n,F,h,w,3]
    (ds_parallax_u8: the definition is in include/depthstereo.h).  poses: a host integer array [F,3] of (tx, ty, tz) within +-1024
    (parallax_poses makes one); anything else is refused here, before the kernel would clamp it.  focus: what lensblur_u8 takes: one
    integer 0..65535 for every image, n of them, a uint16 cuda tensor [n], or ('point', fx, fy).  fill 1..64: the reach of the hole
    filling.  invert: black is near.  want_mask: return (frames, uint8 [n,F,h,w]: 0 = a pixel landed, 1 = filled, 2 = nothing found)
    instead.  out: write the frames into this contiguous uint8 cuda tensor [n,F,h,w,3].  The key workspace (8 bytes per target pixel)
    comes from torch's allocator; when all F views need more than PARALLAX_WS_BYTES the views are rendered in several calls."""
    torch = require_gpu()
    try:
        fill, ok = _as_int(fill)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not (ok and 1 <= fill <= PARALLAX_MAX_FILL):
        raise DepthStereoError("parallax_u8: fill must be an integer in 1..%d, got %r" % (PARALLAX_MAX_FILL, fill))
    pose_arr = None if torch.is_tensor(poses) or isinstance(poses, (str, bytes)) or poses is None else np.asarray(poses)
    if (pose_arr is None or pose_arr.dtype.kind not in 'iu' or pose_arr.ndim != 2 or pose_arr.shape[1] != 3 or pose_arr.shape[0] == 0
            or int(np.abs(pose_arr.astype(np.int64)).max()) > PARALLAX_POSE_MAX):
        raise DepthStereoError("parallax_u8: poses must be a host integer array [F,3] with F >= 1 and every component within +-%d, got %r"
                               % (PARALLAX_POSE_MAX, poses))
    _check_depth_guide("parallax_u8", depth_u16, image_u8)
    if image_u8.shape[3] != 3:
        raise DepthStereoError("parallax_u8: image must have 3 channels, got %s" % (tuple(image_u8.shape),))
    image_u8, depth_u16 = image_u8.contiguous(), depth_u16.contiguous()
    n, h, w = depth_u16.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("parallax_u8: empty depth %s" % (tuple(depth_u16.shape),))
    F = pose_arr.shape[0]
    dev = depth_u16.device
    focus_t = _focus_on_device("parallax_u8", focus, depth_u16)
    if out is None:
        out = torch.empty((n, F, h, w, 3), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == dev and tuple(out.shape) == (n, F, h, w, 3)
              and out.is_contiguous()):
        raise DepthStereoError("parallax_u8: out must be a contiguous uint8 tensor %s on the depth's device" % ((n, F, h, w, 3),))
    mask = torch.empty((n, F, h, w), dtype=torch.uint8, device=dev) if want_mask else None
    poses_t = torch.from_numpy(np.ascontiguousarray(pose_arr, dtype=np.int32)).to(dev)
    per_call = max(1, min(F, PARALLAX_WS_BYTES // (8 * n * h * w), 65535 // n))      # views per call (the entry point's n * F <= 65535)
    keys = torch.empty((n * per_call * h * w,), dtype=torch.int64, device=dev)
    ctx, st = ctx_for(_dev_index(depth_u16)), _stream(depth_u16)
    for k0 in range(0, F, per_call):
        k1 = min(F, k0 + per_call)
        whole = n == 1 or (k0 == 0 and k1 == F)                          # out[:, k0:k1] is dense: the call writes it in place
        part = out[:, k0:k1] if whole else torch.empty((n, k1 - k0, h, w, 3), dtype=torch.uint8, device=dev)
        part_mask = None if mask is None else mask[:, k0:k1] if whole else torch.empty((n, k1 - k0, h, w), dtype=torch.uint8, device=dev)
        CALLS["ds_parallax_u8"] += 1
        _check(lib().ds_parallax_u8(ctx, image_u8.data_ptr(), depth_u16.data_ptr(), focus_t.data_ptr(), n, h, w,
                                    poses_t.data_ptr() + 12 * k0, k1 - k0, fill, 1 if invert else 0, keys.data_ptr(), part.data_ptr(),
                                    part_mask.data_ptr() if part_mask is not None else None, st))
        if not whole:
            out[:, k0:k1].copy_(part)
            if mask is not None:
                mask[:, k0:k1].copy_(part_mask)
    return (out, mask) if want_mask else out


# ---- mesh videos (csrc/ds_mesh_render.hip; public interface: src/mesh_render.py) ------------------------------------------------------
MESH_RENDER_TRAJS = ('straight-line', 'double-straight-line', 'circle')
MESH_RENDER_MAX_FRAMES = 1024
MESH_RENDER_MAX_SHIFT = 1.0e6        # mesh units; anything finite would do, this keeps the arithmetic of a path far from overflow
MESH_RENDER_MAX_SSAA = 4
MESH_RENDER_MAX_SIDE = 16384
MESH_RENDER_CAP_MAX = 64
MESH_RENDER_SMALL_CAP = 16           # boxes of up to this many samples are walked by their face's own thread
MESH_RENDER_WS_BYTES = 1 << 30       # the workspace mesh_render_u8 allocates when the caller names no group
MESH_RENDER_DEFAULTS = (False, 1, True)              # dolly, ssaa, keep_edges


def _as_flag(v):
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    raise TypeError


def mesh_render_params(p):
    """(traj, frames, shift_x, shift_y, shift_z[, dolly[, ssaa[, keep_edges]]]) as (str, int, float, float, float, bool, int, bool), or
    ValueError; what is left out takes (False, 1, True).  traj: 'straight-line', 'double-straight-line' or 'circle' (the reference's
    trajectory kinds).  frames: an integer in 1..1024.  shift: three finite numbers, the camera translation in the mesh's units.  dolly,
    keep_edges: bools.  ssaa: an integer in 1..4.  A bool is no integer, a string no number.  Pure Python (the funnel checks its option
    with it before any device work)."""
    usage = "(traj, frames, shift_x, shift_y, shift_z[, dolly[, ssaa[, keep_edges]]])"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in (5, 6, 7, 8):
            raise TypeError
    except TypeError:
        raise ValueError("mesh_video must be %s, got %r" % (usage, p)) from None
    if not isinstance(q[0], str) or q[0] not in MESH_RENDER_TRAJS:
        raise ValueError("mesh_video: traj must be one of %r, got %r" % (MESH_RENDER_TRAJS, q[0]))
    try:
        if isinstance(q[1], (str, bytes)):
            raise TypeError
        frames, ok = _as_int(q[1])
        if not (ok and 1 <= frames <= MESH_RENDER_MAX_FRAMES):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("mesh_video: frames must be an integer in 1..%d, got %r" % (MESH_RENDER_MAX_FRAMES, q[1])) from None
    try:
        shift = tuple(_as_float(v, MESH_RENDER_MAX_SHIFT) for v in q[2:5])
    except (TypeError, ValueError, OverflowError):
        raise ValueError("mesh_video: shift must be three numbers with |shift| <= %g, got %r" % (MESH_RENDER_MAX_SHIFT, q[2:5])) from None
    dolly, ssaa, keep_edges = MESH_RENDER_DEFAULTS
    try:
        if len(q) > 5:
            dolly = _as_flag(q[5])
        if len(q) > 7:
            keep_edges = _as_flag(q[7])
    except TypeError:
        raise ValueError("mesh_video: dolly and keep_edges must be bools, got %r" % (q[5:6] + q[7:8],)) from None
    if len(q) > 6:
        try:
            if isinstance(q[6], (str, bytes)):
                raise TypeError
            ssaa, ok = _as_int(q[6])
            if not (ok and 1 <= ssaa <= MESH_RENDER_MAX_SSAA):
                raise ValueError
        except (TypeError, ValueError, OverflowError):
            raise ValueError("mesh_video: ssaa must be an integer in 1..%d, got %r" % (MESH_RENDER_MAX_SSAA, q[6])) from None
    return (q[0], frames) + shift + (dolly, ssaa, keep_edges)


def mesh_render_workspace_bytes(N, M, H, W, s):
    """ds_mesh_render_workspace_bytes: one frame's share of the workspace, 0 for sizes the entry point refuses."""
    return int(lib().ds_mesh_render_workspace_bytes(int(N), int(M), int(H), int(W), int(s)))


def mesh_render_u8(verts, colors, faces, cameras, H, W, s=1, near=0.05, background=(0, 0, 0), small_cap=None, group=None, want_hits=False,
                   stages=None):
    """F views of a coloured triangle mesh (ds_mesh_render_u8: the definition is in include/depthstereo.h).  verts float64 [N,3], colors
    uint8 [N,3], faces int32 [M,3] (M = 0 is legal): cuda tensors of one device.  cameras: a HOST array [F,6] of finite numbers (tx, ty,
    tz, f, cx, cy); a NaN or an infinity is refused here, before the kernel would kill the frame.  H, W: the output size; s: 1..4
    samples per pixel side; near > 0; background: three integers 0..255.  small_cap 0..64 (None: MESH_RENDER_SMALL_CAP) and group 1..F
    (None: the largest whose workspace stays within MESH_RENDER_WS_BYTES) change launches, never a bit.  Returns uint8 [F,H,W,3], with
    want_hits (that, uint8 [F,H,W]).  The workspace comes from torch's allocator.  stages: ds_mesh_render_stages_u8 (timing only)."""
    torch = require_gpu()
    who = "mesh_render_u8"
    for name, t, dt, cols in (("verts", verts, torch.float64, 3), ("colors", colors, torch.uint8, 3), ("faces", faces, torch.int32, 3)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape[1] == cols):
            raise DepthStereoError("%s: %s must be a %s cuda tensor [*,%d], got %s %s"
                                   % (who, name, str(dt).replace("torch.", ""), cols, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    if not (verts.device == colors.device == faces.device) or verts.shape[0] != colors.shape[0] or verts.shape[0] == 0:
        raise DepthStereoError("%s: verts %s and colors %s must have one length >= 1, and all arrays one device"
                               % (who, tuple(verts.shape), tuple(colors.shape)))
    cams = None if torch.is_tensor(cameras) or isinstance(cameras, (str, bytes)) or cameras is None else np.asarray(cameras)
    if (cams is None or cams.dtype.kind not in 'iuf' or cams.ndim != 2 or cams.shape[1] != 6 or not 1 <= cams.shape[0] <= 65535
            or not np.isfinite(cams.astype(np.float64)).all()):
        raise DepthStereoError("%s: cameras must be a host array [F,6] of finite numbers with 1 <= F <= 65535, got %r" % (who, cameras))
    ints = []
    for name, v, lo, hi in (("H", H, 1, MESH_RENDER_MAX_SIDE), ("W", W, 1, MESH_RENDER_MAX_SIDE), ("s", s, 1, MESH_RENDER_MAX_SSAA),
                            ("small_cap", MESH_RENDER_SMALL_CAP if small_cap is None else small_cap, 0, MESH_RENDER_CAP_MAX)):
        try:
            if isinstance(v, (str, bytes)):
                raise TypeError
            iv, ok = _as_int(v)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not (ok and lo <= iv <= hi):
            raise DepthStereoError("%s: %s must be an integer in %d..%d, got %r" % (who, name, lo, hi, v))
        ints.append(iv)
    H, W, s, small_cap = ints
    try:
        near = _as_float(near, 1.0e300)
        if not near > 0.0:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise DepthStereoError("%s: near must be a finite number > 0, got %r" % (who, near)) from None
    try:
        bg = [_as_int(v) for v in background]
        if len(bg) != 3 or not all(ok and not isinstance(v, (bool, np.bool_)) and 0 <= iv <= 255 for (iv, ok), v in zip(bg, background)):
            raise ValueError
        bg = [iv for iv, _ in bg]
    except (TypeError, ValueError, OverflowError):
        raise DepthStereoError("%s: background must be three integers in 0..255, got %r" % (who, background)) from None
    N, M, F = verts.shape[0], faces.shape[0], cams.shape[0]
    share = mesh_render_workspace_bytes(N, M, H, W, s)
    if share == 0:
        raise DepthStereoError("%s: s H and s W must be <= %d and one frame's workspace <= 2 GiB, got N=%d M=%d H=%d W=%d s=%d"
                               % (who, MESH_RENDER_MAX_SIDE, N, M, H, W, s))
    if group is None:
        group = max(1, min(F, MESH_RENDER_WS_BYTES // share))
    else:
        try:
            group, ok = _as_int(group)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not (ok and 1 <= group <= F):
            raise DepthStereoError("%s: group must be an integer in 1..F = %d, got %r" % (who, F, group))
    verts, colors, faces = verts.contiguous(), colors.contiguous(), faces.contiguous()
    dev = verts.device
    cams_t = torch.from_numpy(np.array(cams, dtype=np.float64, order="C")).to(dev)
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    hits = torch.empty((F, H, W), dtype=torch.uint8, device=dev) if want_hits else None
    workspace = torch.empty((group * share,), dtype=torch.uint8, device=dev)              # (torch's blocks are 512-byte aligned)
    args = (ctx_for(_dev_index(verts)), verts.data_ptr(), colors.data_ptr(), faces.data_ptr() if M else None, N, M, cams_t.data_ptr(), F, H, W, s,
            near, bg[0], bg[1], bg[2], small_cap, workspace.data_ptr(), group, out.data_ptr(), hits.data_ptr() if hits is not None else None)
    if stages is None:
        CALLS["ds_mesh_render_u8"] += 1
        _check(lib().ds_mesh_render_u8(*args, _stream(verts)))
    else:
        CALLS["ds_mesh_render_stages_u8"] += 1
        _check(lib().ds_mesh_render_stages_u8(*args, int(stages), _stream(verts)))
    return (out, hits) if want_hits else out


# ---- autostereograms from depth (csrc/ds_autostereogram.hip; public interface: src/autostereogram_generation.py) ---------------------
AUTOSTEREOGRAM_PERIODS = (16, 512)
AUTOSTEREOGRAM_MAX_M = 128           # depth_factor = m / 256: at most 0.5
AUTOSTEREOGRAM_MAX_TILE = 4096
AUTOSTEREOGRAM_MODES = {'dots': 0, 'mono': 1}


def autostereogram_separation(z, period, m):
    """s(z) of ds_autostereogram_u8 (include/depthstereo.h): the on-screen separation in pixels of a point of nearness z (0..65535, an
    integer or an integer array) at period P and depth factor m / 256, rounded half up, as int64.  s(0) = P; s never increases with z."""
    z = np.asarray(z).astype(np.int64)
    a = 256 * 65535
    den = 2 * a - int(m) * z
    return (4 * int(period) * (a - int(m) * z) + den) // (2 * den)


def _autostereogram_pattern(pattern):
    """'dots', 'mono', or the tile of a pattern as a C-contiguous uint8 array [ph,pw,3]; raises TypeError / ValueError."""
    if isinstance(pattern, str):
        if pattern not in AUTOSTEREOGRAM_MODES:
            raise ValueError
        return pattern
    if isinstance(pattern, bytes) or pattern is None:
        raise TypeError
    if hasattr(pattern, 'convert') and hasattr(pattern, 'mode'):             # a PIL image: taken as its convert("RGB")
        pattern = np.asarray(pattern.convert('RGB'), dtype=np.uint8)
    tile = np.asarray(pattern)
    if tile.dtype != np.uint8 or tile.ndim not in (2, 3) or (tile.ndim == 3 and tile.shape[2] not in (3, 4)):
        raise TypeError
    tile = np.repeat(tile[:, :, None], 3, axis=2) if tile.ndim == 2 else tile[:, :, :3]
    if not (1 <= tile.shape[0] <= AUTOSTEREOGRAM_MAX_TILE and 1 <= tile.shape[1] <= AUTOSTEREOGRAM_MAX_TILE):
        raise ValueError
    return np.ascontiguousarray(tile)


def autostereogram_params(p):
    """(period, depth_factor), (..., pattern) or (..., pattern, seed) as (int period, int m, pattern, int seed), or ValueError.  period:
    an integer in 16..512, the separation in pixels of the far plane (a bool is no integer).  depth_factor: a number mu, quantised as
    m = rint(256 mu), which must land in 1..128 (a bool or a string is no number; a NaN is out of range).  pattern: 'dots' (coloured
    random dots, the default), 'mono' (black / white dots), or an image -- a PIL image, taken as its convert("RGB"), or a uint8 array
    [ph,pw], [ph,pw,3] or [ph,pw,4] with ph, pw in 1..4096 -- which comes back as a uint8 array [ph,pw,3].  seed: an integer in
    0..2^32 - 1 (default 0).  Pure Python (the funnel checks its option with it before any device work)."""
    usage = "(period, depth_factor[, pattern[, seed]])"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in (2, 3, 4):
            raise TypeError
    except TypeError:
        raise ValueError("autostereogram must be %s, got %r" % (usage, p)) from None
    try:
        if isinstance(q[0], (str, bytes)):
            raise TypeError
        period, ok = _as_int(q[0])
        if not (ok and AUTOSTEREOGRAM_PERIODS[0] <= period <= AUTOSTEREOGRAM_PERIODS[1]):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("autostereogram: period must be an integer in %d..%d, got %r" % (AUTOSTEREOGRAM_PERIODS + (q[0],))) from None
    try:
        m = int(np.rint(256.0 * _as_float(q[1], 1.0)))
        if not 1 <= m <= AUTOSTEREOGRAM_MAX_M:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("autostereogram: depth_factor must be a number with rint(256 * depth_factor) in 1..%d, got %r"
                         % (AUTOSTEREOGRAM_MAX_M, q[1])) from None
    try:
        pattern = _autostereogram_pattern(q[2]) if len(q) > 2 else 'dots'
    except (TypeError, ValueError, OverflowError):
        raise ValueError("autostereogram: pattern must be 'dots', 'mono', a PIL image or a uint8 array [ph,pw], [ph,pw,3] or [ph,pw,4] "
                         "with ph, pw in 1..%d, got %r" % (AUTOSTEREOGRAM_MAX_TILE, q[2])) from None
    try:
        if len(q) > 3 and isinstance(q[3], (str, bytes)):
            raise TypeError
        seed, ok = _as_int(q[3]) if len(q) > 3 else (0, True)
        if not (ok and 0 <= seed <= 0xFFFFFFFF):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError("autostereogram: seed must be an integer in 0..2^32 - 1, got %r" % (q[3],)) from None
    return period, m, pattern, seed


def autostereogram_u8(depth_u16, period, m, mode, seed, tile=None, invert=False, out=None):
    """Autostereograms of uint16 depth maps [n,h,w] (cuda) -> uint8 [n,h,w,3] (ds_autostereogram_u8: the definition is in
    include/depthstereo.h).  period 16..512; m 1..128 (the depth factor m / 256); mode 0 = coloured dots, 1 = black / white dots, 2 = the
    pattern `tile`, a uint8 [ph,pw,3] with ph, pw in 1..4096: a cuda tensor on the depth's device, or a host array, which is uploaded;
    seed 0..2^32 - 1; invert: black is near.  out: write into this contiguous uint8 cuda tensor [n,h,w,3].  One launch."""
    torch = require_gpu()
    try:
        ok = not any(isinstance(v, (str, bytes)) for v in (period, m, mode, seed))
        (period, ok_p), (m, ok_m), (mode, ok_k), (seed, ok_s) = _as_int(period), _as_int(m), _as_int(mode), _as_int(seed)
        ok = (ok and ok_p and ok_m and ok_k and ok_s and AUTOSTEREOGRAM_PERIODS[0] <= period <= AUTOSTEREOGRAM_PERIODS[1]
              and 1 <= m <= AUTOSTEREOGRAM_MAX_M and mode in (0, 1, 2) and 0 <= seed <= 0xFFFFFFFF)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise DepthStereoError("autostereogram_u8: period must be an integer in %d..%d, m in 1..%d, mode 0, 1 or 2 and seed in 0..2^32 - 1, "
                               "got %r, %r, %r, %r" % (AUTOSTEREOGRAM_PERIODS + (AUTOSTEREOGRAM_MAX_M, period, m, mode, seed)))
    _check_depth_guide("autostereogram_u8", depth_u16)
    depth_u16 = depth_u16.contiguous()
    n, h, w = depth_u16.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("autostereogram_u8: empty depth %s" % (tuple(depth_u16.shape),))
    dev = depth_u16.device
    ph = pw = 0
    tile_t = None
    if mode == 2:
        if isinstance(tile, np.ndarray) and tile.dtype == np.uint8:
            tile_t = torch.from_numpy(np.array(tile, order='C')).to(dev)      # (a copy: the caller's array may be read-only)
        elif torch.is_tensor(tile) and tile.dtype == torch.uint8 and tile.device == dev:
            tile_t = tile.contiguous()
        if (tile_t is None or tile_t.dim() != 3 or tile_t.shape[2] != 3 or not 1 <= tile_t.shape[0] <= AUTOSTEREOGRAM_MAX_TILE
                or not 1 <= tile_t.shape[1] <= AUTOSTEREOGRAM_MAX_TILE):
            raise DepthStereoError("autostereogram_u8: with mode 2 tile must be a uint8 array or cuda tensor (on the depth's device) [ph,pw,3] "
                                   "with ph, pw in 1..%d, got %s %s" % (AUTOSTEREOGRAM_MAX_TILE, getattr(tile, "dtype", type(tile)),
                                                                        tuple(getattr(tile, "shape", ()))))
        ph, pw = int(tile_t.shape[0]), int(tile_t.shape[1])
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == dev and tuple(out.shape) == (n, h, w, 3)
              and out.is_contiguous()):
        raise DepthStereoError("autostereogram_u8: out must be a contiguous uint8 tensor %s on the depth's device" % ((n, h, w, 3),))
    CALLS["ds_autostereogram_u8"] += 1
    _check(lib().ds_autostereogram_u8(ctx_for(_dev_index(depth_u16)), depth_u16.data_ptr(), n, h, w, period, m, mode, seed,
                                      tile_t.data_ptr() if tile_t is not None else None, ph, pw, 1 if invert else 0, out.data_ptr(),
                                      _stream(depth_u16)))
    return out


# ---- depth from stereo pairs (csrc/ds_stereo_match.hip; public interface: src/stereo_matching.py) -----------------------------------
STEREO_MATCH_DISPARITIES = (32, 64, 128)
STEREO_MATCH_DEFAULTS = (64, 0, 4, 48, 5, 1)         # D, d0, P1, P2, u, lr
STEREO_MATCH_WS_BYTES = 1 << 30                      # the workspace stereo_match_u8 allocates when the caller names no group
STEREO_MATCH_MAX_SIDE = 16384


def stereo_match_params(p):
    """(D,), (D, d0), (D, d0, P1, P2), (D, d0, P1, P2, u) or (D, d0, P1, P2, u, lr) as six ints, or ValueError; what is left out takes
    the defaults (64, 0, 4, 48, 5, 1).  D: 32, 64 or 128 disparities.  d0: the smallest disparity, an integer in -128..127.  P1 in 1..64
    and P2 in P1..255: the penalties of semi-global matching.  u: the uniqueness margin in percent, 0..50.  lr: the left-right tolerance,
    -1..3, -1 = no check.  All integers: a bool or a string is no number, and a NaN is out of range.  Pure Python (the funnel checks its
    option with it before any device work)."""
    usage = "(D[, d0[, P1, P2[, u[, lr]]]])"
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) not in (1, 2, 4, 5, 6):
            raise TypeError
    except TypeError:
        raise ValueError("stereo_match must be %s, got %r" % (usage, p)) from None
    names = ("D", "d0", "P1", "P2", "u", "lr")
    vals = list(STEREO_MATCH_DEFAULTS)
    for k, v in enumerate(q):
        try:
            if isinstance(v, (str, bytes)):
                raise TypeError
            vals[k], ok = _as_int(v)
            if not ok:
                raise ValueError
        except (TypeError, ValueError, OverflowError):
            raise ValueError("stereo_match: %s must be an integer, got %r" % (names[k], v)) from None
    D, d0, P1, P2, u, lr = vals
    if D not in STEREO_MATCH_DISPARITIES:
        raise ValueError("stereo_match: D must be one of %r, got %r" % (STEREO_MATCH_DISPARITIES, D))
    if not -128 <= d0 <= 127:
        raise ValueError("stereo_match: d0 must be in -128..127, got %r" % (d0,))
    if not (1 <= P1 <= 64 and P1 <= P2 <= 255):
        raise ValueError("stereo_match: P1 must be in 1..64 and P2 in P1..255, got %r, %r" % (P1, P2))
    if not 0 <= u <= 50:
        raise ValueError("stereo_match: u must be in 0..50, got %r" % (u,))
    if not -1 <= lr <= 3:
        raise ValueError("stereo_match: lr must be in -1..3, got %r" % (lr,))
    return D, d0, P1, P2, u, lr


def stereo_match_workspace_bytes(h, w, D):
    """ds_stereo_match_workspace_bytes: one image's share of the workspace, 0 for a size or a D the entry point refuses."""
    return int(lib().ds_stereo_match_workspace_bytes(int(h), int(w), int(D)))


def stereo_match_u8(left, right, D, d0, P1, P2, u, lr, want_valid=False, want_depth=True, group=None):
    """Disparity and depth of the left views of row-aligned stereo pairs: left, right uint8 cuda tensors [n,h,w,c], c in {1, 3, 4}, same
    shape and device (ds_stereo_match_u8: the definition is in include/depthstereo.h).  Returns (disparity int16 [n,h,w] in 1/16 pixel,
    valid uint8 [n,h,w] or None, depth uint16 [n,h,w] or None) on that device.  The workspace comes from torch's allocator and holds
    `group` images; group=None picks the largest group whose workspace stays within STEREO_MATCH_WS_BYTES (1 GiB), and at least 1.  The
    result does not depend on the group."""
    torch = require_gpu()
    try:
        D, d0, P1, P2, u, lr = stereo_match_params((D, d0, P1, P2, u, lr))
    except ValueError as e:
        raise DepthStereoError("stereo_match_u8: %s" % (e,)) from None
    for name, t in (("left", left), ("right", right)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] in (1, 3, 4)):
            raise DepthStereoError("stereo_match_u8: %s must be a uint8 cuda tensor [n,h,w,c] with c in {1, 3, 4}, got %s %s"
                                   % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    if tuple(left.shape) != tuple(right.shape) or left.device != right.device:
        raise DepthStereoError("stereo_match_u8: left %s and right %s must have one shape and one device"
                               % (tuple(left.shape), tuple(right.shape)))
    n, h, w, c = left.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("stereo_match_u8: empty images %s" % (tuple(left.shape),))
    per_image = stereo_match_workspace_bytes(h, w, D) if max(h, w) <= STEREO_MATCH_MAX_SIDE and n <= 65535 else 0
    if per_image == 0 or per_image > 1 << 31:
        raise DepthStereoError("stereo_match_u8: n must be <= 65535, h and w <= %d and one image's workspace <= 2 GiB, got %s at D = %d"
                               % (STEREO_MATCH_MAX_SIDE, tuple(left.shape), D))
    if group is None:
        group = max(1, min(n, STEREO_MATCH_WS_BYTES // per_image))
    else:
        try:
            group, ok = _as_int(group)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not (ok and 1 <= group <= n):
            raise DepthStereoError("stereo_match_u8: group must be an integer in 1..n = %d, got %r" % (n, group))
    left, right = left.contiguous(), right.contiguous()
    dev = left.device
    disparity = torch.empty((n, h, w), dtype=torch.int16, device=dev)
    valid = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_valid else None
    depth = torch.empty((n, h, w), dtype=torch.uint16, device=dev) if want_depth else None
    workspace = torch.empty((group * per_image,), dtype=torch.uint8, device=dev)          # (torch's blocks are 512-byte aligned)
    CALLS["ds_stereo_match_u8"] += 1
    _check(lib().ds_stereo_match_u8(ctx_for(_dev_index(left)), left.data_ptr(), right.data_ptr(), n, h, w, c, D, d0, P1, P2, u, lr,
                                    workspace.data_ptr(), group, disparity.data_ptr(), valid.data_ptr() if valid is not None else None,
                                    depth.data_ptr() if depth is not None else None, _stream(left)))
    return disparity, valid, depth


STEREO_MATCH_EX_DEFAULTS = (4, 0, 0)                 # paths, speckle_size, speckle_range: ds_stereo_match_u8
STEREO_MATCH_EX_PRESET = (8, 64, 1)                  # a starting point for stereo photos, not a measured optimum


def stereo_match_ex_params(p):
    """(paths, speckle_size, speckle_range) of ds_stereo_match_ex_u8 as three ints, or ValueError.  paths: 4 or 8.  speckle_size: 0..65535
    pixels, 0 = no speckle filter.  speckle_range: 0..16 pixels of disparity.  All integers: a bool or a string is no number, and a NaN is
    out of range.  Pure Python (the funnel checks its options with it before any device work)."""
    try:
        if isinstance(p, (str, bytes)):
            raise TypeError
        q = tuple(p)
        if len(q) != 3:
            raise TypeError
    except TypeError:
        raise ValueError("stereo_match_ex must be (paths, speckle_size, speckle_range), got %r" % (p,)) from None
    names = ("paths", "speckle_size", "speckle_range")
    vals = [0, 0, 0]
    for k, v in enumerate(q):
        try:
            if isinstance(v, (str, bytes)):
                raise TypeError
            vals[k], ok = _as_int(v)
            if not ok:
                raise ValueError
        except (TypeError, ValueError, OverflowError):
            raise ValueError("stereo_match_ex: %s must be an integer, got %r" % (names[k], v)) from None
    paths, size, rng = vals
    if paths not in (4, 8):
        raise ValueError("stereo_match_ex: paths must be 4 or 8, got %r" % (paths,))
    if not 0 <= size <= 65535:
        raise ValueError("stereo_match_ex: speckle_size must be in 0..65535, got %r" % (size,))
    if not 0 <= rng <= 16:
        raise ValueError("stereo_match_ex: speckle_range must be in 0..16, got %r" % (rng,))
    return paths, size, rng


def stereo_match_ex_workspace_bytes(h, w, D, paths, speckle_size):
    """ds_stereo_match_ex_workspace_bytes: one image's share of the workspace, 0 for what the entry point refuses."""
    return int(lib().ds_stereo_match_ex_workspace_bytes(int(h), int(w), int(D), int(paths), int(speckle_size)))


def speckle_filter_workspace_bytes(h, w):
    """ds_speckle_filter_workspace_bytes: one image's share of the workspace, 0 for a shape the entry point refuses."""
    return int(lib().ds_speckle_filter_workspace_bytes(int(h), int(w)))


def _stereo_group(who, group, n, per_image):
    if group is None:
        return max(1, min(n, STEREO_MATCH_WS_BYTES // per_image))
    try:
        group, ok = _as_int(group)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not (ok and 1 <= group <= n):
        raise DepthStereoError("%s: group must be an integer in 1..n = %d, got %r" % (who, n, group))
    return group


def stereo_match_ex_u8(left, right, D, d0, P1, P2, u, lr, paths, speckle_size, speckle_range, want_valid=False, want_depth=True, group=None):
    """stereo_match_u8 with eight paths and a speckle filter (ds_stereo_match_ex_u8: the definition is in include/depthstereo.h): paths 4
    or 8; speckle_size 0..65535, 0 = off; speckle_range 0..16 pixels.  The same inputs, outputs, workspace rule and group as
    stereo_match_u8; `valid` is the mask behind the speckle filter.  With (4, 0, r) the outputs are stereo_match_u8's bit for bit."""
    torch = require_gpu()
    try:
        D, d0, P1, P2, u, lr = stereo_match_params((D, d0, P1, P2, u, lr))
        paths, speckle_size, speckle_range = stereo_match_ex_params((paths, speckle_size, speckle_range))
    except ValueError as e:
        raise DepthStereoError("stereo_match_ex_u8: %s" % (e,)) from None
    for name, t in (("left", left), ("right", right)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] in (1, 3, 4)):
            raise DepthStereoError("stereo_match_ex_u8: %s must be a uint8 cuda tensor [n,h,w,c] with c in {1, 3, 4}, got %s %s"
                                   % (name, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    if tuple(left.shape) != tuple(right.shape) or left.device != right.device:
        raise DepthStereoError("stereo_match_ex_u8: left %s and right %s must have one shape and one device"
                               % (tuple(left.shape), tuple(right.shape)))
    n, h, w, c = left.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("stereo_match_ex_u8: empty images %s" % (tuple(left.shape),))
    per_image = stereo_match_ex_workspace_bytes(h, w, D, paths, speckle_size) if max(h, w) <= STEREO_MATCH_MAX_SIDE and n <= 65535 else 0
    if per_image == 0 or per_image > 1 << 31:
        raise DepthStereoError("stereo_match_ex_u8: n must be <= 65535, h and w <= %d and one image's workspace <= 2 GiB, got %s at D = %d"
                               % (STEREO_MATCH_MAX_SIDE, tuple(left.shape), D))
    group = _stereo_group("stereo_match_ex_u8", group, n, per_image)
    left, right = left.contiguous(), right.contiguous()
    dev = left.device
    disparity = torch.empty((n, h, w), dtype=torch.int16, device=dev)
    valid = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_valid else None
    depth = torch.empty((n, h, w), dtype=torch.uint16, device=dev) if want_depth else None
    workspace = torch.empty((group * per_image,), dtype=torch.uint8, device=dev)          # (torch's blocks are 512-byte aligned)
    CALLS["ds_stereo_match_ex_u8"] += 1
    _check(lib().ds_stereo_match_ex_u8(ctx_for(_dev_index(left)), left.data_ptr(), right.data_ptr(), n, h, w, c, D, d0, P1, P2, u, lr, paths,
                                       speckle_size, speckle_range, workspace.data_ptr(), group, disparity.data_ptr(),
                                       valid.data_ptr() if valid is not None else None, depth.data_ptr() if depth is not None else None,
                                       _stream(left)))
    return disparity, valid, depth


def speckle_filter_i16(disp, valid, size, t, want_sizes=False, group=None):
    """The speckle filter (ds_speckle_filter_i16: the definition is in include/depthstereo.h): disp int16 and valid uint8 cuda tensors
    [n,h,w] on one device; size 1..65535 pixels; t 0..65535 in disp's units.  Returns (valid_out uint8 [n,h,w], size_out int32 [n,h,w]
    or None): valid_out is 1 where a valid pixel's component -- 4-neighbours whose values differ by at most t -- has more than `size`
    pixels; size_out holds the component's pixel count (its bits are the uint32 counts, which stay below 2^28), 0 for an invalid
    pixel.  The workspace comes from torch's allocator, as stereo_match_u8's does."""
    torch = require_gpu()
    try:
        if isinstance(size, (str, bytes)) or isinstance(t, (str, bytes)):
            raise TypeError
        (size, ok_s), (t, ok_t) = _as_int(size), _as_int(t)
        if not (ok_s and ok_t and 1 <= size <= 65535 and 0 <= t <= 65535):
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise DepthStereoError("speckle_filter_i16: size must be an integer in 1..65535 and t one in 0..65535, got %r, %r" % (size, t)) from None
    for name, x, dt in (("disp", disp, torch.int16), ("valid", valid, torch.uint8)):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == dt and x.dim() == 3):
            raise DepthStereoError("speckle_filter_i16: %s must be a %s cuda tensor [n,h,w], got %s %s"
                                   % (name, dt, getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    if tuple(disp.shape) != tuple(valid.shape) or disp.device != valid.device:
        raise DepthStereoError("speckle_filter_i16: disp %s and valid %s must have one shape and one device"
                               % (tuple(disp.shape), tuple(valid.shape)))
    n, h, w = disp.shape
    if n == 0 or h == 0 or w == 0:
        raise DepthStereoError("speckle_filter_i16: empty maps %s" % (tuple(disp.shape),))
    per_image = speckle_filter_workspace_bytes(h, w) if max(h, w) <= STEREO_MATCH_MAX_SIDE and n <= 65535 else 0
    if per_image == 0 or per_image > 1 << 31:
        raise DepthStereoError("speckle_filter_i16: n must be <= 65535, h and w <= %d and h w <= 2^28, got %s"
                               % (STEREO_MATCH_MAX_SIDE, tuple(disp.shape)))
    group = _stereo_group("speckle_filter_i16", group, n, per_image)
    disp, valid = disp.contiguous(), valid.contiguous()
    dev = disp.device
    valid_out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    size_out = torch.empty((n, h, w), dtype=torch.int32, device=dev) if want_sizes else None
    workspace = torch.empty((group * per_image,), dtype=torch.uint8, device=dev)
    CALLS["ds_speckle_filter_i16"] += 1
    _check(lib().ds_speckle_filter_i16(ctx_for(_dev_index(disp)), disp.data_ptr(), valid.data_ptr(), n, h, w, size, t, workspace.data_ptr(),
                                       group, valid_out.data_ptr(), size_out.data_ptr() if size_out is not None else None, _stream(disp)))
    return valid_out, size_out


# ---- video mode (csrc/ds_video.hip; host half: src/video_mode.py) ------------------------------------------------------------------
def frame_luma_hist(frames_u8, out=None):
    """Per-frame histograms of the integer luma (ds_frame_luma_hist, include/depthstereo.h) of a dense uint8 cuda clip [n,h,w] or
    [n,h,w,c], c in {1, 3, 4}, at any byte alignment.  Returns [n,256] int32 whose BITS are the uint32 counts (torch has no
    arithmetic on uint32; a count of 2^31 or more reads negative until masked).  out: write into this [n,256] int32 cuda tensor; it is
    overwritten, not added to."""
    torch = require_gpu()
    if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() in (3, 4)
            and frames_u8.is_contiguous()):
        raise DepthStereoError("frame_luma_hist: frames must be a contiguous uint8 cuda tensor [n,h,w] or [n,h,w,c], got %s %s"
                               % (getattr(frames_u8, "dtype", type(frames_u8)), tuple(getattr(frames_u8, "shape", ()))))
    n, h, w = frames_u8.shape[:3]
    c = frames_u8.shape[3] if frames_u8.dim() == 4 else 1
    if out is None:
        out = torch.empty((n, 256), dtype=torch.int32, device=frames_u8.device)
    elif not (out.is_cuda and out.device == frames_u8.device and out.dtype == torch.int32 and tuple(out.shape) == (n, 256)
              and out.is_contiguous()):
        raise DepthStereoError("frame_luma_hist: out must be a contiguous int32 [%d,256] tensor on the frames' device" % n)
    CALLS["ds_frame_luma_hist"] += 1
    _check(lib().ds_frame_luma_hist(ctx_for(_dev_index(frames_u8)), frames_u8.data_ptr(), n, h, w, c, out.data_ptr(), _stream(frames_u8)))
    return out


def temporal_smooth5(src, first, count, lo, hi, out=None):
    """The clamped 5-tap temporal filter (ds_temporal_smooth5_f32, include/depthstereo.h): src float32 cuda [m, ...] contiguous ->
    float32 [count, ...], frames first .. first + count - 1 of src smoothed with taps clamped to frames lo..hi.  out: write into this
    contiguous float32 tensor of that shape (it must not overlap src)."""
    torch = require_gpu()
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.float32 and src.dim() >= 1 and src.is_contiguous()):
        raise DepthStereoError("temporal_smooth5: src must be a contiguous float32 cuda tensor [m, ...], got %s %s"
                               % (getattr(src, "dtype", type(src)), tuple(getattr(src, "shape", ()))))
    m = src.shape[0]
    plane = src[0].numel() if m else 0
    shape = (max(int(count), 0),) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif not (out.is_cuda and out.device == src.device and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
        raise DepthStereoError("temporal_smooth5: out must be a contiguous float32 %s tensor on src's device" % (shape,))
    CALLS["ds_temporal_smooth5_f32"] += 1
    _check(lib().ds_temporal_smooth5_f32(ctx_for(_dev_index(src)), src.data_ptr(), m, plane, int(first), int(count), int(lo), int(hi),
                                         out.data_ptr(), _stream(src)))
    return out


# the temporal depth filter (its tables and parameters: the bilateral family, above; public interface: video_mode.stabilize_depth)
def temporal_joint_bilateral_u16(depth_u16, guide_u8, radius, wt, wc, first, count, lo, hi, out=None):
    """The temporal joint bilateral filter (ds_temporal_joint_bilateral_u16, include/depthstereo.h): depth uint16 cuda [m,h,w] contiguous,
    guide uint8 cuda [m,h,w,3 or 4] contiguous (any byte alignment) -> uint16 [count,h,w], frames first .. first + count - 1 filtered over
    the frames within `radius` of each that lie in lo..hi.  wt, wc: float64 cuda tensors of radius + 1 and 766 values
    (stabilize_tables_on).  out: write into this contiguous uint16 tensor of that shape (it must not overlap depth)."""
    torch = require_gpu()
    _check_depth_guide("temporal_joint_bilateral_u16", depth_u16, guide_u8, contiguous=True)
    radius = int(radius)
    for name, t, n in (("wt", wt, radius + 1), ("wc", wc, 766)):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == depth_u16.device and t.dtype == torch.float64 and t.dim() == 1
                and t.numel() == n and t.is_contiguous()):
            raise DepthStereoError("temporal_joint_bilateral_u16: %s must be a contiguous float64 tensor of %d values on the depth's device"
                                   % (name, n))
    m, h, w = depth_u16.shape
    shape = (max(int(count), 0), h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint16, device=depth_u16.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == depth_u16.device and out.dtype == torch.uint16
              and tuple(out.shape) == shape and out.is_contiguous()):
        raise DepthStereoError("temporal_joint_bilateral_u16: out must be a contiguous uint16 %s tensor on the depth's device" % (shape,))
    CALLS["ds_temporal_joint_bilateral_u16"] += 1
    _check(lib().ds_temporal_joint_bilateral_u16(ctx_for(_dev_index(depth_u16)), depth_u16.data_ptr(), guide_u8.data_ptr(), guide_u8.shape[3],
                                                 m, h, w, radius, wt.data_ptr(), wc.data_ptr(), int(first), int(count), int(lo), int(hi),
                                                 out.data_ptr(), _stream(depth_u16)))
    return out


def depth_to_u16(pred_f32, invert=False, want_norm=False):
    torch = require_gpu()
    n, h, w = pred_f32.shape
    out = torch.empty((n, h, w), dtype=torch.uint16, device=pred_f32.device)
    norm = torch.empty((n, h, w), dtype=torch.float32, device=pred_f32.device) if want_norm else None
    CALLS["ds_depth_to_u16"] += 1
    _check(lib().ds_depth_to_u16(ctx_for(_dev_index(pred_f32)), pred_f32.data_ptr(), n, h, w, 1 if invert else 0,
                                 out.data_ptr(), norm.data_ptr() if want_norm else None, _stream(pred_f32)))
    return (out, norm) if want_norm else out


def convert_to_i16(arr):
    torch = require_gpu()
    assert arr.dtype in (torch.float32, torch.float64) and arr.is_contiguous()
    out = torch.empty(arr.shape, dtype=torch.uint16, device=arr.device)
    CALLS["ds_convert_to_i16"] += 1
    _check(lib().ds_convert_to_i16(ctx_for(_dev_index(arr)), arr.data_ptr(), 1 if arr.dtype == torch.float64 else 0,
                                   arr.numel(), out.data_ptr(), _stream(arr)))
    return out


# ---- custom-depth ingest (csrc/ds_resample.hip; host half: src/resample_model.py) -------------------------------------------------
CD_WIDEN, CD_SINGLE_BAND, CD_MULTI_BAND = 0, 1, 2
_CD_WORKSPACE_BLOCKS = 256                       # DS_CD_WORKSPACE_BLOCKS


def _pixel_plane(src):
    """(DS_PIX_* id, n, h, w, pixel / row / image stride in elements) of a dense CUDA tensor [n,h,w] of uint8 / uint16 / int32 /
    float32, or [n,h,w,c] uint8 (interleaved bands: band 0 is read in place)."""
    torch = _torch()
    from . import resample_model as rm
    pix = {torch.uint8: rm.PIX_U8, torch.uint16: rm.PIX_U16, torch.int32: rm.PIX_I32, torch.float32: rm.PIX_F32}.get(src.dtype)
    if pix is None or not src.is_cuda or not src.is_contiguous() or src.dim() not in (3, 4) or (src.dim() == 4 and pix != rm.PIX_U8):
        raise DepthStereoError(f"unsupported pixel tensor: dtype {src.dtype}, shape {tuple(src.shape)}")
    n, h, w = src.shape[:3]
    c = src.shape[3] if src.dim() == 4 else 1
    return pix, n, h, w, c, w * c, h * w * c


def _lanczos_tables(fixed_point, in_size, out_size):
    from . import resample_model as rm
    _, bounds, kk = rm.lanczos_coeffs(in_size, out_size)
    if fixed_point:
        kk = rm.fixed_point_coeffs(kk)
    return np.array(bounds), np.array(kk.T, order='C')


def _lanczos_coeffs_on(device, fixed_point, in_size, out_size):
    """(bounds, tap-major weights, taps) of one axis on the device, kept for the last 32 (device, fixed point?, in, out)."""
    bounds, weights = _tables_on("lanczos", device, (bool(fixed_point), int(in_size), int(out_size)), _lanczos_tables, keep=32)
    return bounds, weights, weights.shape[0]


def resize_lanczos(src, out_hw):
    """Image.resize((out_w, out_h), Image.Resampling.LANCZOS) of a batch of planes, byte for byte as the installed Pillow computes it
    (include/depthstereo.h: ds_resize_lanczos).  src: see _pixel_plane.  Returns [n, out_h, out_w] of src's dtype."""
    torch = require_gpu()
    from . import resample_model as rm
    pix, n, in_h, in_w, px, row, img = _pixel_plane(src)
    out_h, out_w = int(out_hw[0]), int(out_hw[1])
    horiz, vert = out_w != in_w, out_h != in_h
    dst = torch.empty((n, out_h, out_w), dtype=src.dtype, device=src.device)
    hb = hk = vb = vk = tmp = None
    ht = vt = 0
    if horiz:
        hb, hk, ht = _lanczos_coeffs_on(src.device, pix == rm.PIX_U8, in_w, out_w)
    if vert:
        vb, vk, vt = _lanczos_coeffs_on(src.device, pix == rm.PIX_U8, in_h, out_h)
    if horiz and vert:
        tmp = torch.empty((n, in_h, out_w), dtype=src.dtype, device=src.device)
    CALLS["ds_resize_lanczos"] += 1
    _check(lib().ds_resize_lanczos(ctx_for(_dev_index(src)), src.data_ptr(), pix, n, in_h, in_w, px, row, img, dst.data_ptr(), out_h, out_w,
                                   hb.data_ptr() if horiz else None, hk.data_ptr() if horiz else None, ht,
                                   vb.data_ptr() if vert else None, vk.data_ptr() if vert else None, vt,
                                   tmp.data_ptr() if tmp is not None else None, _stream(src)))
    return dst


def custom_depth_to_f64(src, rule, out=None):
    """np.asarray(depth, dtype="float") and the divide of the custom-depth ingest (include/depthstereo.h: ds_custom_depth_to_f64).
    src: see _pixel_plane; rule: CD_WIDEN / CD_SINGLE_BAND (value / 2^bits by the image's maximum) / CD_MULTI_BAND (band 0 / 256).
    Returns (float64 [n,h,w] -- `out` when given --, [n,2] float64 {maximum, divisor} per image for CD_SINGLE_BAND else None)."""
    torch = require_gpu()
    pix, n, h, w, px, row, img = _pixel_plane(src)
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.float64, device=src.device)
    assert out.dtype == torch.float64 and tuple(out.shape) == (n, h, w) and out.is_contiguous() and out.device == src.device
    ws = torch.empty((n * (2 + _CD_WORKSPACE_BLOCKS),), dtype=torch.float64, device=src.device) if rule == CD_SINGLE_BAND else None
    CALLS["ds_custom_depth_to_f64"] += 1
    _check(lib().ds_custom_depth_to_f64(ctx_for(_dev_index(src)), src.data_ptr(), pix, n, h, w, px, row, img, int(rule), out.data_ptr(),
                                        ws.data_ptr() if ws is not None else None, _stream(src)))
    return out, (ws[:2 * n].view(n, 2) if ws is not None else None)


def colorize_u16(depth, vmin_vmax, lut_rgba):
    """Heat map (include/depthstereo.h: ds_colorize_u16).  depth [n,h,w] uint16, vmin_vmax [n,2] float64, lut_rgba
    [N<=256, 4] uint8, all CUDA tensors.  Returns [n,h,w,4] uint8."""
    torch = require_gpu()
    assert depth.is_cuda and depth.dtype == torch.uint16 and depth.dim() == 3 and depth.is_contiguous()
    n, h, w = depth.shape
    vmm = vmin_vmax.to(device=depth.device, dtype=torch.float64).contiguous()
    lut = lut_rgba.to(device=depth.device, dtype=torch.uint8).contiguous()
    assert tuple(vmm.shape) == (n, 2) and lut.dim() == 2 and lut.shape[1] == 4
    out = torch.empty((n, h, w, 4), dtype=torch.uint8, device=depth.device)
    CALLS["ds_colorize_u16"] += 1
    _check(lib().ds_colorize_u16(ctx_for(_dev_index(depth)), depth.data_ptr(), n, h, w, vmm.data_ptr(), lut.data_ptr(),
                                 int(lut.shape[0]), out.data_ptr(), _stream(depth)))
    return out


class PackedAttentionBias:
    """The bias operand of attention_fwd: made by attention_bias_pack, opaque to the host code."""

    def __init__(self, data, heads, n, npad):
        self.data, self.heads, self.n, self.npad = data, heads, n, npad

    @property
    def dtype(self):
        return self.data.dtype


def attention_bias_pack(bias, npad, dtype):
    """bias [H, n, n] (CUDA tensor, any float dtype, natural units) -> PackedAttentionBias for sequences whose token stride is
    npad (include/depthstereo.h: ds_attention_bias_pack; the operand itself is laid out on npad rounded up to 64)."""
    torch = require_gpu()
    npad = (int(npad) + 63) // 64 * 64
    assert bias.is_cuda and bias.dim() == 3 and bias.shape[1] == bias.shape[2] and dtype in (torch.float16, torch.bfloat16)
    h, n = int(bias.shape[0]), int(bias.shape[1])
    src = bias.detach().float().contiguous()
    out = torch.empty((h * npad * npad,), dtype=dtype, device=bias.device)
    CALLS["ds_attention_bias_pack"] += 1
    _check(lib().ds_attention_bias_pack(ctx_for(_dev_index(src)), src.data_ptr(), h, n, int(npad),
                                        1 if dtype == torch.float16 else 2, out.data_ptr(), _stream(src)))
    return PackedAttentionBias(out, h, n, int(npad))


def attention_fwd(qk, vt, n_valid, scale, bias=None):
    """Fused MFMA attention (include/depthstereo.h: ds_attention_fwd).  qk [B,Np,2,H,64], vt [B,H*64,Np], float16 or
    bfloat16 CUDA tensors; bias: None or a PackedAttentionBias (attention_bias_pack) for the same H, Np and dtype.
    Returns [B,Np,H*64]."""
    torch = require_gpu()
    assert qk.is_cuda and vt.is_cuda and qk.dtype == vt.dtype and qk.dtype in (torch.float16, torch.bfloat16)
    b, npad, two, h, d = qk.shape
    assert two == 2 and d == 64 and npad % 8 == 0 and tuple(vt.shape) == (b, h * 64, npad), (qk.shape, vt.shape)
    qk = qk.contiguous()
    vt = vt.contiguous()
    if bias is not None:
        assert isinstance(bias, PackedAttentionBias), "bias must come from attention_bias_pack"
        assert (bias.heads, bias.npad, bias.dtype) == (h, (npad + 63) // 64 * 64, qk.dtype) and bias.data.device == qk.device
    out = torch.empty((b, npad, h * 64), dtype=qk.dtype, device=qk.device)
    dt = 1 if qk.dtype == torch.float16 else 2
    CALLS["ds_attention_fwd"] += 1
    _check(lib().ds_attention_fwd(ctx_for(_dev_index(qk)), qk.data_ptr(), vt.data_ptr(),
                                  bias.data.data_ptr() if bias is not None else None, out.data_ptr(),
                                  b, npad, h, int(n_valid), float(scale), dt, _stream(qk)))
    return out


def residual_layernorm(x, branch, gamma, ln_weight, ln_bias, eps=1e-6):
    """x_out = x + gamma * branch; h = LayerNorm(x_out) (include/depthstereo.h: ds_residual_layernorm), one pass.
    x, branch [..., C] float16/bfloat16 CUDA tensors (branch may be None: plain LayerNorm).  Returns (x_out, h)."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16)
    x = x.contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    h = torch.empty_like(x)
    dt = 1 if x.dtype == torch.float16 else 2
    if branch is None:
        x_out, bp = x, None
    else:
        branch = branch.contiguous()
        assert branch.shape == x.shape and branch.dtype == x.dtype
        x_out = torch.empty_like(x)
        bp = branch.data_ptr()
    g = None if gamma is None else gamma.to(x.dtype).contiguous()
    w, b = ln_weight.to(x.dtype).contiguous(), ln_bias.to(x.dtype).contiguous()
    CALLS["ds_residual_layernorm"] += 1
    _check(lib().ds_residual_layernorm(ctx_for(_dev_index(x)), x.data_ptr(), bp, None if g is None else g.data_ptr(),
                                       w.data_ptr(), b.data_ptr(), None if branch is None else x_out.data_ptr(), h.data_ptr(),
                                       rows, c, float(eps), dt, _stream(x)))
    return x_out, h


def reassemble_readout(proj, clsvec):
    """gelu(proj[:, 1:] + clsvec[:, None]) -> [B, N-1, C] (include/depthstereo.h: ds_reassemble_readout).
    proj [B, N, C], clsvec [B, C]: float16 / bfloat16 CUDA tensors."""
    torch = require_gpu()
    assert proj.is_cuda and proj.dtype in (torch.float16, torch.bfloat16) and proj.dim() == 3 and clsvec.dtype == proj.dtype
    b, n, c = proj.shape
    proj, clsvec = proj.contiguous(), clsvec.contiguous()
    assert tuple(clsvec.shape) == (b, c)
    out = torch.empty((b, n - 1, c), dtype=proj.dtype, device=proj.device)
    CALLS["ds_reassemble_readout"] += 1
    _check(lib().ds_reassemble_readout(ctx_for(_dev_index(proj)), proj.data_ptr(), clsvec.data_ptr(), out.data_ptr(), b, n, c,
                                       1 if proj.dtype == torch.float16 else 2, _stream(proj)))
    return out


def linear_env(**switches):
    """Set (a value) or remove (None) DS_LIN_* switches of the GEMM path in os.environ and make the library re-read them
    (include/depthstereo.h: ds_linear_reload_env -- the library reads them once, not per launch).  Tests and A/B runs only."""
    for k, v in switches.items():
        assert k.startswith("DS_LIN_")
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    _check(lib().ds_linear_reload_env())


def normalmap_selfcheck(k0, stride, count):
    """Number of operands n^2 = (k0 + stride * i) / 2^18, i < count, on which the fused normal-map kernels' square root / reciprocal
    differ from the generic float64 operations (include/depthstereo.h: ds_normalmap_selfcheck): must be 0."""
    torch = require_gpu()
    bad = ctypes.c_ulonglong(0)
    _check(lib().ds_normalmap_selfcheck(ctx_for(torch.cuda.current_device()), ctypes.c_ulonglong(k0), ctypes.c_ulonglong(stride),
                                        ctypes.c_ulonglong(count), ctypes.byref(bad), None))
    return int(bad.value)


def attention_env(**switches):
    """Set (a value) or remove (None) DS_ATT_* switches of ds_attention_fwd in os.environ and make the library re-read them
    (include/depthstereo.h: ds_attention_reload_env).  DS_ATT_GEN=2 / 4 selects the kernel generation.  Tests and A/B runs only."""
    for k, v in switches.items():
        assert k.startswith("DS_ATT_")
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    _check(lib().ds_attention_reload_env())


def linear_supported(x, weight):
    """Shapes ds_linear takes: out_features % 256 == 0, in_features % 128 == 0 (every ViT of the path qualifies)."""
    return weight.shape[0] % 256 == 0 and weight.shape[1] % 128 == 0 and 128 <= weight.shape[1] <= 16384 and x.numel() > 0


def linear(x, weight, bias=None, gelu=False):
    """[gelu](x @ weight.T + bias) by the in-tree MFMA GEMM (include/depthstereo.h: ds_linear).
    x [..., K] float16 / bfloat16 CUDA, weight [N, K], bias [N] or None -> [..., N]."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and linear_supported(x, weight)
    k = x.shape[-1]
    n = weight.shape[0]
    assert weight.shape[1] == k
    x2 = x.reshape(-1, k)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    rows = x2.shape[0]
    if rows < 256:                       # the kernel's unit is a 256-row tile: tiny inputs are padded, not special-cased
        x2 = torch.cat([x2, x2.new_zeros((256 - rows, k))])
    w = weight.detach()
    w = w if (w.dtype == x.dtype and w.is_contiguous()) else w.to(x.dtype).contiguous()
    b = None
    if bias is not None:
        b = bias.detach()
        b = b if (b.dtype == x.dtype and b.is_contiguous()) else b.to(x.dtype).contiguous()
    out = torch.empty((x2.shape[0], n), dtype=x.dtype, device=x.device)
    CALLS["ds_linear"] += 1
    _check(lib().ds_linear(ctx_for(_dev_index(x)), x2.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                           out.data_ptr(), x2.shape[0], n, k, n, 1 if gelu else 0,
                           1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out[:rows].view(x.shape[:-1] + (n,))


def linear_residual(x, weight, bias, gamma, residual):
    """residual + [gamma *] (x @ weight.T + bias) (include/depthstereo.h: ds_linear_residual).  x [..., K], residual [..., N]
    float16 / bfloat16 CUDA, at least 256 rows; gamma [N] or None."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and linear_supported(x, weight)
    k, n = x.shape[-1], weight.shape[0]
    x2 = x.reshape(-1, k).contiguous()
    r2 = residual.reshape(-1, n).contiguous()
    assert x2.shape[0] == r2.shape[0] >= 256 and r2.dtype == x.dtype

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == x.dtype and t.is_contiguous()) else t.to(x.dtype).contiguous()
    w, b, g = prep(weight), prep(bias), prep(gamma)
    out = torch.empty_like(r2)
    CALLS["ds_linear_residual"] += 1
    _check(lib().ds_linear_residual(ctx_for(_dev_index(x)), x2.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
                                    None if g is None else g.data_ptr(), r2.data_ptr(), out.data_ptr(), x2.shape[0], n, k,
                                    1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out.view(residual.shape)


def linear_readout_supported(x_padded, w_tok):
    """Shapes ds_linear_readout takes: x [B, Np, K] contiguous with B * Np >= 256, w_tok [N % 256 == 0, K % 128 == 0]."""
    return (x_padded.dim() == 3 and x_padded.is_contiguous() and x_padded.shape[0] * x_padded.shape[1] >= 256
            and w_tok.shape[0] % 256 == 0 and w_tok.shape[1] == x_padded.shape[2] and x_padded.shape[2] % 128 == 0
            and 128 <= x_padded.shape[2] <= 16384 and x_padded.shape[0] * x_padded.shape[1] * x_padded.shape[1] < (1 << 32))


def linear_readout(x_padded, n_tokens, w_tok, cls_vec):
    """GELU(x[b, t] @ w_tok.T + cls_vec[b]) for the tokens t = 1 .. n_tokens - 1 of every image, token-major = the NHWC patch grid
    (include/depthstereo.h: ds_linear_readout).  x_padded [B, Np, K] float16 / bfloat16 CUDA (the encoder's padded block output),
    w_tok [N, K], cls_vec [B, N] -> [B, n_tokens - 1, N] (a view of a buffer with one dummy row behind it)."""
    torch = require_gpu()
    assert x_padded.is_cuda and x_padded.dtype in (torch.float16, torch.bfloat16) and linear_readout_supported(x_padded, w_tok)
    b, npad, k = x_padded.shape
    n = w_tok.shape[0]
    assert 2 <= n_tokens <= npad and tuple(cls_vec.shape) == (b, n)
    w = w_tok.detach()
    w = w if (w.dtype == x_padded.dtype and w.is_contiguous()) else w.to(x_padded.dtype).contiguous()
    cv = cls_vec if (cls_vec.dtype == x_padded.dtype and cls_vec.is_contiguous()) else cls_vec.to(x_padded.dtype).contiguous()
    out = torch.empty((b * (n_tokens - 1) + 1, n), dtype=x_padded.dtype, device=x_padded.device)
    CALLS["ds_linear_readout"] += 1
    _check(lib().ds_linear_readout(ctx_for(_dev_index(x_padded)), x_padded.data_ptr(), w.data_ptr(), cv.data_ptr(), out.data_ptr(),
                                   b, npad, n_tokens, n, k, 1 if x_padded.dtype == torch.float16 else 2, _stream(x_padded)))
    return out[:b * (n_tokens - 1)].view(b, n_tokens - 1, n)


def linear_rows4_supported(taps, weights):
    """Shapes ds_linear_rows4 takes: 1 .. 4 contiguous padded taps [B, Np, K] of one shape and dtype, weights [N % 64 == 0, K % 128 == 0]."""
    t0, w0 = taps[0], weights[0]
    return (1 <= len(taps) == len(weights) <= 4 and t0.dim() == 3 and 1 <= t0.shape[0] <= 65536
            and all(t.shape == t0.shape and t.dtype == t0.dtype and t.device == t0.device and t.is_contiguous() for t in taps)
            and all(w.shape == w0.shape for w in weights) and w0.shape[1] == t0.shape[2] and w0.shape[0] % 64 == 0
            and w0.shape[1] % 128 == 0 and 128 <= w0.shape[1] <= 16384 and t0.shape[1] * t0.shape[2] < (1 << 25))


def linear_rows4(taps, weights, biases, out=None):
    """[tap[:, 0] @ w.T + b for tap, w, b in zip(taps, weights, biases)] in ONE launch that reads row 0 of every image where it lies in
    the padded tap (include/depthstereo.h: ds_linear_rows4).  taps: 1 .. 4 contiguous [B, Np, K] float16 / bfloat16 CUDA tensors,
    weights [N, K], biases [N] or None -> a list of [B, N] (views of `out` [len(taps), B, N] when given: contiguous, the taps' dtype).
    Bit-identical to linear(tap[:, 0].contiguous(), w, b) per tap."""
    torch = require_gpu()
    t0 = taps[0]
    assert t0.is_cuda and t0.dtype in (torch.float16, torch.bfloat16) and linear_rows4_supported(taps, weights) and len(biases) == len(taps)
    b, npad, k = t0.shape
    n = weights[0].shape[0]

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == t0.dtype and t.is_contiguous()) else t.to(t0.dtype).contiguous()
    ws, bs = [prep(w) for w in weights], [prep(v) for v in biases]
    if out is None:
        out = torch.empty((len(taps), b, n), dtype=t0.dtype, device=t0.device)
    assert tuple(out.shape) == (len(taps), b, n) and out.dtype == t0.dtype and out.device == t0.device and out.is_contiguous()
    probs = (ds_rows_problem * len(taps))()
    for i, (t, w, v) in enumerate(zip(taps, ws, bs)):
        probs[i] = ds_rows_problem(t.data_ptr(), npad * k, w.data_ptr(), None if v is None else v.data_ptr(), out[i].data_ptr())
    CALLS["ds_linear_rows4"] += 1
    CALLS["ds_linear"] += len(taps)
    _check(lib().ds_linear_rows4(ctx_for(_dev_index(t0)), probs, len(taps), b, n, k, 1 if t0.dtype == torch.float16 else 2, _stream(t0)))
    return list(out.unbind(0))


def conv_transpose_shuffle_supported(layer, x):
    """ConvTranspose2d layers ds_linear_shuffle takes: kernel == stride (square), no padding / output padding / groups / dilation,
    in_channels % 128 == 0, out_channels % 8 == 0, stride^2 * out_channels % 256 == 0, at least 256 input pixels."""
    ks, st = tuple(layer.kernel_size), tuple(layer.stride)
    return (ks == st and ks[0] == ks[1] and 1 <= ks[0] <= 8 and tuple(layer.padding) == (0, 0) and tuple(layer.output_padding) == (0, 0)
            and tuple(layer.dilation) == (1, 1) and layer.groups == 1 and layer.in_channels % 128 == 0 and 128 <= layer.in_channels <= 16384
            and layer.out_channels % 8 == 0 and (ks[0] * ks[0] * layer.out_channels) % 256 == 0 and x.dim() == 4
            and x.shape[1] == layer.in_channels and x.shape[0] * x.shape[2] * x.shape[3] >= 256)


def conv_transpose_shuffle(layer, x):
    """layer(x) for an nn.ConvTranspose2d with kernel == stride on a float16 / bfloat16 CUDA activation, channels_last in and out
    (include/depthstereo.h: ds_linear_shuffle).  The [(kH, kW, out), in] weight image and the per-tap bias are cached on the module."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and conv_transpose_shuffle_supported(layer, x)
    x = x.contiguous(memory_format=torch.channels_last)
    b, c, h, w = x.shape
    s, co = layer.stride[0], layer.out_channels
    key = (layer.weight.data_ptr(), layer.weight._version, x.dtype, None if layer.bias is None else layer.bias._version)
    hit = getattr(layer, "_ds_shuffle", None)
    if hit is None or hit[0] != key:
        if hit is not None:
            from . import vit_mi355x as _vm
            _vm.cache_evicted()                 # a live hipGraph may still read the old weight image
        wg = layer.weight.detach().permute(2, 3, 1, 0).reshape(s * s * co, c).to(x.dtype).contiguous()      # [in, out, kH, kW] -> [(kH, kW, out), in]
        bg = None if layer.bias is None else layer.bias.detach().to(x.dtype).repeat(s * s).contiguous()
        hit = (key, wg, bg)
        if not torch.is_grad_enabled():
            layer._ds_shuffle = hit
    _, wg, bg = hit
    out = torch.empty((b, h * s, w * s, co), dtype=x.dtype, device=x.device)
    xr = x.permute(0, 2, 3, 1)                   # the NHWC memory as [b, h, w, c]: contiguous
    CALLS["ds_linear_shuffle"] += 1
    _check(lib().ds_linear_shuffle(ctx_for(_dev_index(x)), xr.data_ptr(), wg.data_ptr(), None if bg is None else bg.data_ptr(), out.data_ptr(),
                                   b * h * w, c, w, s, co, 1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out.permute(0, 3, 1, 2)               # logical NCHW, channels_last memory


def gconv3x3_supported(x, weight, stride, padding, dilation, groups):
    """What ds_gconv3x3_nhwc_f32 takes: a float32 channels_last activation, 3x3, stride 1, padding 1, no dilation, channels == out
    channels, 8 / 16 / 32 channels per group, channels % 32 == 0."""
    torch = _torch()
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and groups > 1 and tuple(weight.shape[2:]) == (3, 3)):
        return False
    c = x.shape[1]
    cpg = c // groups
    return (weight.shape[0] == c and weight.shape[1] == cpg and cpg in (8, 16, 32) and c % 32 == 0 and tuple(stride) == (1, 1)
            and tuple(padding) == (1, 1) and tuple(dilation) == (1, 1) and x.is_contiguous(memory_format=torch.channels_last))


def gconv_weight_image(weight, groups):
    """torch's grouped weight [out, in / groups, 3, 3] -> [groups][9 taps][in / groups][out / groups] float32 (what the kernel's scalar
    loads walk: the outputs of one (group, tap, input channel) are consecutive)."""
    c, cpg = weight.shape[0], weight.shape[1]
    w = weight.detach().float().reshape(groups, c // groups, cpg, 9)          # [g][co][ci][tap]
    return w.permute(0, 3, 2, 1).contiguous()                                   # [g][tap][ci][co]


def gconv3x3(x, w_gtio, bias, relu, cpg):
    """[relu](grouped 3x3 convolution + bias) on a float32 channels_last activation (include/depthstereo.h: ds_gconv3x3_nhwc_f32)."""
    torch = require_gpu()
    b, c, h, w = x.shape
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    assert w_gtio.dtype == torch.float32 and w_gtio.is_contiguous() and w_gtio.numel() == (c // cpg) * 9 * cpg * cpg
    bb = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty_like(x, memory_format=torch.channels_last)
    CALLS["ds_gconv3x3_nhwc_f32"] += 1
    _check(lib().ds_gconv3x3_nhwc_f32(ctx_for(_dev_index(x)), x.data_ptr(), w_gtio.data_ptr(), None if bb is None else bb.data_ptr(), out.data_ptr(),
                                      b, h, w, c, cpg, 1 if relu else 0, _stream(x)))
    return out


def add_relu(a, b):
    """relu(a + b) for two float32 CUDA tensors of one shape and one memory layout (include/depthstereo.h: ds_add_relu_f32)."""
    torch = require_gpu()
    assert a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and a.stride() == b.stride()
    assert a.numel() % 4 == 0 and (a.is_contiguous() or a.is_contiguous(memory_format=torch.channels_last))
    out = torch.empty_like(a)                       # preserves the (dense) strides
    assert out.stride() == a.stride()
    CALLS["ds_add_relu_f32"] += 1
    _check(lib().ds_add_relu_f32(ctx_for(_dev_index(a)), a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream(a)))
    return out


def bias_act_f32_ok(x, bias, res=None):
    """What ds_bias_act_f32 takes: a float32 CUDA activation in channels_last memory (or a dense [rows, C] matrix), C % 4 == 0, a
    float32 bias of C values, res laid out like x."""
    torch = require_gpu()
    if not (x.is_cuda and x.dtype == torch.float32 and bias is not None and bias.dtype == torch.float32 and bias.is_cuda and bias.numel() == x.shape[1]):
        return False
    if not (x.dim() == 4 and x.shape[1] % 4 == 0 and x.is_contiguous(memory_format=torch.channels_last) and x.numel() > 0):
        return False
    return res is None or (res.dtype == torch.float32 and res.shape == x.shape and res.is_cuda and res.is_contiguous(memory_format=torch.channels_last))


def bias_act_f32(x, bias, relu=False, res=None):
    """[relu]((x + bias[c]) [+ res]) IN PLACE on a float32 channels_last activation (include/depthstereo.h: ds_bias_act_f32)."""
    assert bias_act_f32_ok(x, bias, res)
    b, c, h, w = x.shape
    bias = bias.contiguous()
    CALLS["ds_bias_act_f32"] += 1
    _check(lib().ds_bias_act_f32(ctx_for(_dev_index(x)), x.data_ptr(), bias.data_ptr(), None if res is None else res.data_ptr(), x.data_ptr(),
                                 b * h * w, c, 1 if relu else 0, _stream(x)))
    return x


def _relu_cat_layout(a, b):
    """0: both channels_last; 1: a channels_last, b NCHW-contiguous; 2: both NCHW-contiguous; None: not taken."""
    torch = require_gpu()
    if not (a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 4 and b.dim() == 4
            and a.shape[0] == b.shape[0] and a.shape[2:] == b.shape[2:] and a.numel() > 0 and b.numel() > 0):
        return None
    cl = torch.channels_last
    # (a tensor with one channel or a 1 x 1 plane is contiguous in both senses: NCHW is tested first for b, channels_last first for a)
    if b.is_contiguous():
        lay = 2 if (a.is_contiguous() and not a.is_contiguous(memory_format=cl)) else (1 if a.is_contiguous(memory_format=cl) else None)
        if lay is not None and a.shape[1] % 32 == 0 and b.shape[1] % 32 == 0:
            return lay
    if a.is_contiguous(memory_format=cl) and b.is_contiguous(memory_format=cl) and a.shape[1] % 4 == 0 and b.shape[1] % 4 == 0:
        return 0
    return None


def relu_cat_f32_ok(a, b):
    return _relu_cat_layout(a, b) is not None


def relu_cat_f32(a, b):
    """relu(torch.cat([a, b], 1)) for float32 activations, one pass (include/depthstereo.h: ds_relu_cat_f32): channels_last out of two
    channels_last inputs; NCHW when b is NCHW (a channels_last or NCHW) -- the memory format torch.cat itself would produce."""
    torch = require_gpu()
    lay = _relu_cat_layout(a, b)
    assert lay is not None
    n, ca, h, w = a.shape
    cb = b.shape[1]
    out = torch.empty((n, ca + cb, h, w), dtype=a.dtype, device=a.device, memory_format=torch.channels_last if lay == 0 else torch.contiguous_format)
    CALLS["ds_relu_cat_f32"] += 1
    _check(lib().ds_relu_cat_f32(ctx_for(_dev_index(a)), a.data_ptr(), b.data_ptr(), out.data_ptr(), n, h * w, ca, cb, lay, _stream(a)))
    return out


def dwconv(x, w_taps, bias_in, bias, kernel, stride, pad_top, pad_left, out_hw):
    """relu6(bias + depthwise_conv(relu6(x + bias_in), w)) for a float16 / float32 CUDA activation, channels_last in and out
    (include/depthstereo.h: ds_dwconv_nhwc): the padding (pad_top / pad_left before, what out_hw implies after) is applied to the
    ACTIVATED x.  w_taps [kernel * kernel, C] float32 (tap-major), bias_in / bias [C] float32.  Returns [B, C, out_h, out_w]."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.float32) and x.dim() == 4
    x = x.contiguous(memory_format=torch.channels_last)
    b, c, h, w = x.shape
    for t, n in ((w_taps, kernel * kernel * c), (bias_in, c), (bias, c)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    out = torch.empty((b, c, int(out_hw[0]), int(out_hw[1])), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    CALLS["ds_dwconv_nhwc"] += 1
    _check(lib().ds_dwconv_nhwc(ctx_for(_dev_index(x)), x.data_ptr(), w_taps.data_ptr(), bias_in.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                b, h, w, c, out.shape[2], out.shape[3], int(kernel), int(stride), int(pad_top), int(pad_left),
                                1 if x.dtype == torch.float16 else 3, _stream(x)))
    return out


KT_KINDS = {"linear_gelu": 0, "attention": 1, "linear_residual": 2, "linear": 3, "linear_vt": 4, "conv3x3": 5, "linear_readout": 6,
            "linear_shuffle": 7, "normalmap": 8, "depth_refine": 9, "sparse_bilateral": 10, "aomap": 11}
KT_RAGGED = 12


def kernel_timer_enable(device_index, enable=True):
    """In-step kernel timers of the C ABI (include/depthstereo.h: ds_kernel_timer_enable): event pairs around the launches."""
    _check(lib().ds_kernel_timer_enable(ctx_for(device_index), 1 if enable else 0))


def kernel_timer_read(device_index, kind):
    """(launches timed, sum of their durations in ms) of one kind: a name of KT_KINDS, or "<name>+ragged" for its ragged round."""
    base, _, rag = kind.partition("+")
    k = KT_KINDS[base] + (KT_RAGGED if rag == "ragged" else 0)
    n, ms = ctypes.c_int64(), ctypes.c_double()
    _check(lib().ds_kernel_timer_read(ctx_for(device_index), k, ctypes.byref(n), ctypes.byref(ms)))
    return int(n.value), float(ms.value)


def kernel_timer_read_each(device_index, kind):
    """Durations (ms) of the timed launches of one kind in launch order (include/depthstereo.h: ds_kernel_timer_read_each)."""
    base, _, rag = kind.partition("+")
    k = KT_KINDS[base] + (KT_RAGGED if rag == "ragged" else 0)
    buf = (ctypes.c_float * 1024)()
    n = ctypes.c_int64()
    _check(lib().ds_kernel_timer_read_each(ctx_for(device_index), k, buf, 1024, ctypes.byref(n)))
    return [float(buf[i]) for i in range(min(int(n.value), 1024))]


def row_stats(x, eps):
    """Per row {rstd, -mean * rstd} (float32 [rows, 2]) of x [..., C]: the statistics half of a LayerNorm, for the GEMMs that fold
    the LayerNorm into their epilogue (include/depthstereo.h: ds_row_stats).  C in 384 / 768 / 1024 / 1536."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.is_contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    out = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    CALLS["ds_row_stats"] += 1
    _check(lib().ds_row_stats(ctx_for(_dev_index(x)), x.data_ptr(), out.data_ptr(), rows, c, float(eps),
                              1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def linear_ln(x, w_scaled, colsum, bias, stats, gelu=False):
    """[gelu](LN(x) @ W.T + b) with the LayerNorm folded into the GEMM (include/depthstereo.h: ds_linear_ln): x [..., K] is the
    UN-normalised input, w_scaled = W * ln_weight [N, K], colsum = w_scaled.sum(1) float32 [N], bias = b + W @ ln_bias [N] or None,
    stats = row_stats(x)."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and linear_supported(x, w_scaled) and x.is_contiguous()
    k, n = x.shape[-1], w_scaled.shape[0]
    rows = x.numel() // k
    assert rows >= 256 and w_scaled.dtype == x.dtype and w_scaled.is_contiguous() and colsum.dtype == torch.float32 and colsum.numel() == n
    assert stats.dtype == torch.float32 and stats.numel() == 2 * rows and (bias is None or (bias.dtype == x.dtype and bias.is_contiguous()))
    out = torch.empty((rows, n), dtype=x.dtype, device=x.device)
    CALLS["ds_linear_ln"] += 1
    _check(lib().ds_linear_ln(ctx_for(_dev_index(x)), x.data_ptr(), w_scaled.data_ptr(), colsum.data_ptr(), None if bias is None else bias.data_ptr(),
                              stats.data_ptr(), out.data_ptr(), rows, n, k, n, 1 if gelu else 0, 1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out.view(x.shape[:-1] + (n,))


def linear_vt_ln(w_v_scaled, colsum, x, stats):
    """V^T with the LayerNorm folded in (include/depthstereo.h: ds_linear_vt_ln): x [B, Np, K] un-normalised -> [B, C, Np]."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and linear_vt_supported(w_v_scaled, x) and x.is_contiguous()
    b, npad, k = x.shape
    c = w_v_scaled.shape[0]
    assert w_v_scaled.dtype == x.dtype and w_v_scaled.is_contiguous() and colsum.dtype == torch.float32 and colsum.numel() == c
    assert stats.dtype == torch.float32 and stats.numel() == 2 * b * npad
    out = torch.empty((b, c, npad), dtype=x.dtype, device=x.device)
    CALLS["ds_linear_vt_ln"] += 1
    _check(lib().ds_linear_vt_ln(ctx_for(_dev_index(x)), w_v_scaled.data_ptr(), colsum.data_ptr(), x.data_ptr(), stats.data_ptr(), out.data_ptr(),
                                 c, b, npad, k, 1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def linear_vt_supported(w_v, h):
    """Shapes ds_linear_vt takes: h [B, Np, K] with Np % 8 == 0 and (B * Np) % 256 == 0, w_v [C >= 256, K], K % 128 == 0."""
    return (h.dim() == 3 and h.shape[1] % 8 == 0 and (h.shape[0] * h.shape[1]) % 256 == 0 and w_v.shape[0] >= 256
            and w_v.shape[1] == h.shape[2] and h.shape[2] % 128 == 0 and 128 <= h.shape[2] <= 16384
            and h.shape[0] * h.shape[1] * h.shape[1] < (1 << 32))


def linear_vt(w_v, h):
    """V^T = W_v . h^T per batch element, written transposed by the GEMM's epilogue (include/depthstereo.h: ds_linear_vt).
    w_v [C, K], h [B, Np, K] float16 / bfloat16 CUDA -> [B, C, Np]."""
    torch = require_gpu()
    assert h.is_cuda and h.dtype in (torch.float16, torch.bfloat16) and linear_vt_supported(w_v, h)
    b, npad, k = h.shape
    c = w_v.shape[0]
    h2 = h if h.is_contiguous() else h.contiguous()
    w = w_v.detach()
    w = w if (w.dtype == h.dtype and w.is_contiguous()) else w.to(h.dtype).contiguous()
    out = torch.empty((b, c, npad), dtype=h.dtype, device=h.device)
    CALLS["ds_linear_vt"] += 1
    _check(lib().ds_linear_vt(ctx_for(_dev_index(h)), w.data_ptr(), h2.data_ptr(), out.data_ptr(), c, b, npad, k,
                              1 if h.dtype == torch.float16 else 2, _stream(h)))
    return out


def linear_qkv_supported(h, w_qk, w_v):
    """Shapes ds_linear_qkv takes: those of linear (h, w_qk) and of linear_vt (w_v, h) at once."""
    return linear_vt_supported(w_v, h) and linear_supported(h, w_qk) and w_qk.shape[1] == h.shape[2]


def linear_qkv(h, w_qk, b_qk, w_v, out=None):
    """(h @ w_qk.T + b_qk, V^T = W_v . h^T per batch element) in ONE persistent GEMM launch (include/depthstereo.h: ds_linear_qkv),
    bit-identical to (linear(h, w_qk, b_qk), linear_vt(w_v, h)).  h [B, Np, K] float16 / bfloat16 CUDA, w_qk [N, K], b_qk [N] or
    None, w_v [C, K] -> (qk [B, Np, N], vt [B, C, Np]).  out: an optional (qk, vt) pair of contiguous tensors to write into.
    CALLS counts the entry point, and the two GEMMs it carries as the kinds they are (ds_linear, ds_linear_vt)."""
    torch = require_gpu()
    assert h.is_cuda and h.dtype in (torch.float16, torch.bfloat16) and linear_qkv_supported(h, w_qk, w_v)
    b, npad, k = h.shape
    n, c = w_qk.shape[0], w_v.shape[0]
    h2 = h if h.is_contiguous() else h.contiguous()

    def prep(t):
        if t is None:
            return None
        t = t.detach()
        return t if (t.dtype == h.dtype and t.is_contiguous()) else t.to(h.dtype).contiguous()
    wq, bq, wv = prep(w_qk), prep(b_qk), prep(w_v)
    if out is None:
        qk = torch.empty((b, npad, n), dtype=h.dtype, device=h.device)
        vt = torch.empty((b, c, npad), dtype=h.dtype, device=h.device)
    else:
        qk, vt = out
        assert tuple(qk.shape) == (b, npad, n) and tuple(vt.shape) == (b, c, npad) and qk.is_contiguous() and vt.is_contiguous()
        assert qk.dtype == vt.dtype == h.dtype and qk.device == vt.device == h.device
    CALLS["ds_linear_qkv"] += 1
    CALLS["ds_linear"] += 1
    CALLS["ds_linear_vt"] += 1
    _check(lib().ds_linear_qkv(ctx_for(_dev_index(h)), h2.data_ptr(), wq.data_ptr(), None if bq is None else bq.data_ptr(), wv.data_ptr(),
                               qk.data_ptr(), vt.data_ptr(), b, npad, n, c, k, 1 if h.dtype == torch.float16 else 2, _stream(h)))
    return qk, vt


def conv3x3_supported(conv, x):
    """What ds_conv3x3_nhwc takes: 3x3, stride 1, zero padding 1, no groups / dilation, in % 128 == 0, out % 128 == 0 (residual
    operands only with out % 256 == 0)."""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros'
            and conv.in_channels % 128 == 0 and conv.out_channels % 128 == 0 and x.dim() == 4 and x.shape[1] == conv.in_channels
            and x.shape[0] * x.shape[2] * x.shape[3] >= 256)


def conv3x3_circular_supported(conv, x):
    """What ds_conv3x3_nhwc_circular takes: conv3x3_supported's conditions with padding_mode == 'circular' (TILING_MODE,
    src/depthmap_generation.py: apply_tiling_mode)."""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'circular'
            and conv.in_channels % 128 == 0 and conv.out_channels % 128 == 0 and x.dim() == 4 and x.shape[1] == conv.in_channels
            and x.shape[0] * x.shape[2] * x.shape[3] >= 256)


def conv3x3(conv, x, relu=False, res1=None, res2=None, relu_in=False):
    """[relu](conv(x) + bias [+ res1] [+ res2]) for a 3x3 nn.Conv2d on a float16 / bfloat16 CUDA activation, channels_last
    in and out (include/depthstereo.h: ds_conv3x3_nhwc; padding_mode == 'circular': ds_conv3x3_nhwc_circular).  The [out, 3, 3, in]
    weight image is cached on the module (one image for both entry points).
    relu_in: conv(relu(x)) with the maximum taken inside the kernel (needs relu, no residual operands, out % 256 == 0)."""
    torch = require_gpu()
    circular = conv.padding_mode == 'circular'
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16)
    assert conv3x3_circular_supported(conv, x) if circular else conv3x3_supported(conv, x)
    x = x.contiguous(memory_format=torch.channels_last)
    b, c, h, w = x.shape
    wk, bk = _conv_weight_image(conv, x.dtype)
    out = torch.empty((b, conv.out_channels, h, w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    for r in (res1, res2):
        assert r is None or (r.shape == out.shape and r.dtype == x.dtype and r.is_contiguous(memory_format=torch.channels_last))
    name = "ds_conv3x3_nhwc_circular" if circular else "ds_conv3x3_nhwc"
    CALLS[name] += 1
    _check(getattr(lib(), name)(ctx_for(_dev_index(x)), x.data_ptr(), wk.data_ptr(), None if bk is None else bk.data_ptr(),
                                None if res1 is None else res1.data_ptr(), None if res2 is None else res2.data_ptr(),
                                out.data_ptr(), b, h, w, c, conv.out_channels, (2 if relu else 0) | (4 if relu_in else 0),
                                1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def _conv_weight_image(conv, dtype):
    """The cached [out, 3, 3, in] weight image (and bias) of conv3x3, built on first use."""
    key = (conv.weight.data_ptr(), conv.weight._version, dtype, None if conv.bias is None else conv.bias._version)
    hit = getattr(conv, "_ds_ohwi", None)
    if hit is None or hit[0] != key:
        if hit is not None:
            from . import vit_mi355x as _vm
            _vm.cache_evicted()                 # a live hipGraph may still read the old weight image
        wk = conv.weight.detach().to(dtype).permute(0, 2, 3, 1).contiguous()
        bk = None if conv.bias is None else conv.bias.detach().to(dtype).contiguous()
        hit = conv._ds_ohwi = (key, wk, bk)
    return hit[1], hit[2]


def conv3x3_pair_supported(conv0, x0, conv1, x1):
    """What ds_conv3x3_nhwc_pair takes: two zero-padded 3x3 convolutions without bias, equal in_channels (% 128 == 0) and equal
    out_channels (% 256 == 0), on two activations of one dtype and device; either may have fewer than 256 pixels."""
    def one(conv, x):
        return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1)
                and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros' and conv.bias is None
                and x.dim() == 4 and x.shape[1] == conv.in_channels and x.numel() > 0)
    return (one(conv0, x0) and one(conv1, x1) and conv0.in_channels == conv1.in_channels and conv0.in_channels % 128 == 0
            and conv0.in_channels <= 4096 and conv0.out_channels == conv1.out_channels and conv0.out_channels % 256 == 0
            and x0.dtype == x1.dtype and x0.device == x1.device)


def conv3x3_pair(conv0, x0, conv1, x1):
    """(conv0(x0), conv1(x1)) for two bias-free 3x3 convolutions with common in / out channels in ONE persistent launch over both
    tile lists (include/depthstereo.h: ds_conv3x3_nhwc_pair); channels_last in and out.  Bit-identical to two conv3x3 calls.  Each
    output is a view of a buffer with one dummy row behind it (the rows of a partial tile beyond the image go there)."""
    torch = require_gpu()
    assert x0.is_cuda and x0.dtype in (torch.float16, torch.bfloat16) and conv3x3_pair_supported(conv0, x0, conv1, x1)
    outs, args, xs = [], [], []
    for conv, x in ((conv0, x0), (conv1, x1)):
        x = x.contiguous(memory_format=torch.channels_last)
        b, c, h, w = x.shape
        wk, _ = _conv_weight_image(conv, x.dtype)
        n = conv.out_channels
        buf = torch.empty((b * h * w + 1, n), dtype=x.dtype, device=x.device)
        outs.append(buf[:b * h * w].view(b, h, w, n).permute(0, 3, 1, 2))
        args += [x.data_ptr(), wk.data_ptr(), buf.data_ptr(), b, h, w]
        xs.append(x)                            # (a channels_last copy lives until the launch is enqueued)
    CALLS["ds_conv3x3_nhwc_pair"] += 1
    CALLS["ds_conv3x3_nhwc"] += 2
    _check(lib().ds_conv3x3_nhwc_pair(ctx_for(_dev_index(x0)), *args, conv0.in_channels, conv0.out_channels,
                                      1 if x0.dtype == torch.float16 else 2, _stream(x0)))
    return outs[0], outs[1]


def bias_act(x, bias, relu=False, res1=None, res2=None, inplace=True):
    """[relu](x + bias[c] [+ res1] [+ res2]) for an NCHW-shaped float16/bfloat16 CUDA tensor in channels_last memory format
    (include/depthstereo.h: ds_bias_act_nhwc); res1 / res2 must have x's shape and memory format.  In place by default."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.dim() == 4 and x.shape[1] % 8 == 0
    assert x.is_contiguous(memory_format=torch.channels_last)
    for r in (res1, res2):
        assert r is None or (r.shape == x.shape and r.dtype == x.dtype and r.is_contiguous(memory_format=torch.channels_last))
    out = x if inplace else torch.empty_like(x)
    b = bias.detach().to(x.dtype).contiguous()
    CALLS["ds_bias_act_nhwc"] += 1
    _check(lib().ds_bias_act_nhwc(ctx_for(_dev_index(x)), x.data_ptr(), b.data_ptr(), None if res1 is None else res1.data_ptr(),
                                  None if res2 is None else res2.data_ptr(), out.data_ptr(), x.numel(), x.shape[1], 1 if relu else 0,
                                  1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def group_norm_supported(x, groups):
    """What ds_group_norm_nchw takes: a contiguous NCHW float16 / bfloat16 CUDA activation whose planes hold a multiple of 8 pixels."""
    torch = _torch()
    return (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.dim() == 4 and x.is_contiguous() and x.shape[1] % groups == 0
            and (x.shape[2] * x.shape[3]) % 8 == 0 and x.shape[0] * groups <= 4096 and x.data_ptr() % 16 == 0)


def group_norm(x, groups, weight, bias, eps, relu=False, res=None):
    """[relu](group_norm(x) [+ res]) (include/depthstereo.h: ds_group_norm_nchw); weight / bias in any float type (cast to x's)."""
    torch = require_gpu()
    assert group_norm_supported(x, groups)
    assert res is None or (res.shape == x.shape and res.dtype == x.dtype and res.is_contiguous() and res.data_ptr() % 16 == 0)
    out = torch.empty_like(x)
    g, b = weight.detach().to(x.dtype).contiguous(), bias.detach().to(x.dtype).contiguous()
    CALLS["ds_group_norm_nchw"] += 1
    _check(lib().ds_group_norm_nchw(ctx_for(_dev_index(x)), x.data_ptr(), g.data_ptr(), b.data_ptr(), None if res is None else res.data_ptr(),
                                    out.data_ptr(), x.shape[0], x.shape[1], x.shape[2] * x.shape[3], int(groups), float(eps), 1 if relu else 0,
                                    1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def boost_blend(dst, rects, coefs, preds, mask_template):
    """Blend all Boost patches into dst (float32 [H, W] CUDA, in place), in list order (include/depthstereo.h:
    ds_boost_blend).  rects: list of (x0, y0, w, h); coefs: list of (p0, p1); preds float32 [P, S, S]; mask_template
    float32 [M, M]."""
    torch = require_gpu()
    assert dst.is_cuda and dst.dtype == torch.float32 and dst.dim() == 2 and dst.stride(1) == 1
    n = len(rects)
    if n == 0:
        return dst
    preds = preds.contiguous()
    mask_template = mask_template.contiguous()
    assert preds.dtype == torch.float32 and preds.shape[0] == n and preds.shape[1] == preds.shape[2]
    assert mask_template.dtype == torch.float32 and mask_template.shape[0] == mask_template.shape[1]
    rec = np.zeros(n, dtype=[('x0', '<i4'), ('y0', '<i4'), ('w', '<i4'), ('h', '<i4'), ('p0', '<f8'), ('p1', '<f8')])
    for i, (r, c) in enumerate(zip(rects, coefs)):
        rec[i] = (int(r[0]), int(r[1]), int(r[2]), int(r[3]), float(c[0]), float(c[1]))
    buf = torch.from_numpy(rec.view(np.uint8).copy()).to(dst.device)
    CALLS["ds_boost_blend"] += 1
    _check(lib().ds_boost_blend(ctx_for(_dev_index(dst)), dst.data_ptr(), dst.stride(0), dst.shape[0], dst.shape[1],
                                buf.data_ptr(), n, preds.data_ptr(), preds.shape[1], mask_template.data_ptr(),
                                mask_template.shape[0], _stream(dst)))
    return dst


def preprocess_bicubic(images_u8, size_hw, mean, std, flip=True, dtype=None):
    """uint8 [B,H,W,3] CUDA -> normalised network input [B,3,h,w] (channels_last memory) in one pass
    (include/depthstereo.h: ds_preprocess_bicubic): channel flip, / 255, bicubic resize, (x - mean) / std, cast."""
    torch = require_gpu()
    assert images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[3] == 3
    dtype = torch.float32 if dtype is None else dtype
    code = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}[dtype]
    x = images_u8.contiguous()
    b, h, w, _ = x.shape
    oh, ow = int(size_hw[0]), int(size_hw[1])
    out = torch.empty((b, 3, oh, ow), dtype=dtype, device=x.device, memory_format=torch.channels_last)
    m = (ctypes.c_float * 3)(*[float(v) for v in (mean if hasattr(mean, "__len__") else (mean,) * 3)])
    s = (ctypes.c_float * 3)(*[float(v) for v in (std if hasattr(std, "__len__") else (std,) * 3)])
    CALLS["ds_preprocess_bicubic"] += 1
    _check(lib().ds_preprocess_bicubic(ctx_for(_dev_index(x)), x.data_ptr(), out.data_ptr(), b, h, w, oh, ow, 1 if flip else 0, m, s, code,
                                       _stream(x)))
    return out


def preprocess_bicubic_rows(images_u8, size_hw, mean, std, patch, n_pad, kpad, flip=True, dtype=None, out=None):
    """uint8 [B,H,W,3] CUDA -> [B, n_pad, kpad] float16 / bfloat16: the zero padded patch rows of the normalised network input, the
    operand of the patch-embedding GEMM, in one pass (include/depthstereo.h: ds_preprocess_bicubic_rows).  out: a contiguous buffer
    of that shape to write into (every element of it is written)."""
    torch = require_gpu()
    assert images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[3] == 3
    code = {torch.float16: 1, torch.bfloat16: 2}[dtype]
    x = images_u8.contiguous()
    b, h, w, _ = x.shape
    oh, ow = int(size_hw[0]), int(size_hw[1])
    if out is None:
        out = torch.empty((b, int(n_pad), int(kpad)), dtype=dtype, device=x.device)
    assert out.is_contiguous() and out.dtype == dtype and tuple(out.shape) == (b, int(n_pad), int(kpad)) and out.device == x.device
    m = (ctypes.c_float * 3)(*[float(v) for v in (mean if hasattr(mean, "__len__") else (mean,) * 3)])
    s = (ctypes.c_float * 3)(*[float(v) for v in (std if hasattr(std, "__len__") else (std,) * 3)])
    CALLS["ds_preprocess_bicubic_rows"] += 1
    _check(lib().ds_preprocess_bicubic_rows(ctx_for(_dev_index(x)), x.data_ptr(), out.data_ptr(), b, h, w, oh, ow, 1 if flip else 0, m, s,
                                            int(patch), int(n_pad), int(kpad), code, _stream(x)))
    return out


def tokens_fixup(tokens, cls, n_valid):
    """tokens [B, n_pad, C] in place: row 0 of every image <- cls [C], rows n_valid.. <- 0 (include/depthstereo.h: ds_tokens_fixup)."""
    torch = require_gpu()
    b, n_pad, c = tokens.shape
    assert tokens.is_cuda and tokens.is_contiguous() and tokens.dtype in (torch.float16, torch.bfloat16) and c % 8 == 0
    assert cls.is_cuda and cls.dtype == tokens.dtype and cls.is_contiguous() and cls.numel() == c and 1 <= n_valid <= n_pad
    CALLS["ds_tokens_fixup"] += 1
    _check(lib().ds_tokens_fixup(ctx_for(_dev_index(tokens)), tokens.data_ptr(), cls.data_ptr(), b, n_pad, int(n_valid), c,
                                 1 if tokens.dtype == torch.float16 else 2, _stream(tokens)))
    return tokens


def upsample_bicubic_to_f32(pred, size_hw):
    """[B, h, w] float16 / bfloat16 CUDA -> float32 [B, H, W]: F.interpolate(pred[:, None], size, mode="bicubic",
    align_corners=False)[:, 0].float(), bit for bit, in one pass (include/depthstereo.h: ds_upsample_bicubic_to_f32)."""
    torch = require_gpu()
    assert pred.is_cuda and pred.dim() == 3 and pred.dtype in (torch.float16, torch.bfloat16)
    x = pred.contiguous()
    b, h, w = x.shape
    oh, ow = int(size_hw[0]), int(size_hw[1])
    out = torch.empty((b, oh, ow), dtype=torch.float32, device=x.device)
    CALLS["ds_upsample_bicubic_to_f32"] += 1
    _check(lib().ds_upsample_bicubic_to_f32(ctx_for(_dev_index(x)), x.data_ptr(), out.data_ptr(), b, h, w, oh, ow,
                                            1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def im2col3x3_s2(x, circular=False):
    """NCHW-shaped float16 / bfloat16 CUDA tensor in channels_last memory -> [B * ho * wo, 9 * C]: the 3x3 / stride 2 / padding 1
    windows in [ky, kx, c] order, zero or circular padding (include/depthstereo.h: ds_im2col3x3_s2_nhwc)."""
    torch = require_gpu()
    b, c, h, w = x.shape
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and c % 8 == 0
    xin = x.contiguous(memory_format=torch.channels_last)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    rows = torch.empty((b * ho * wo, 9 * c), dtype=x.dtype, device=x.device)
    CALLS["ds_im2col3x3_s2_nhwc"] += 1
    _check(lib().ds_im2col3x3_s2_nhwc(ctx_for(_dev_index(x)), xin.data_ptr(), rows.data_ptr(), b, h, w, c, 1 if circular else 0,
                                      1 if x.dtype == torch.float16 else 2, _stream(x)))
    return rows


def upsample_bilinear(x, size=None, scale_factor=None, align_corners=True):
    """F.interpolate(x, mode="bilinear") for an NCHW-shaped float16/bfloat16 CUDA tensor in channels_last memory format
    (include/depthstereo.h: ds_upsample_bilinear_nhwc).  Returns a channels_last tensor."""
    torch = require_gpu()
    b, c, ih, iw = x.shape
    if size is None:
        size = (int(ih * scale_factor), int(iw * scale_factor))
    oh, ow = int(size[0]), int(size[1])
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and c % 8 == 0
    xin = x.contiguous(memory_format=torch.channels_last)
    out = torch.empty((b, c, oh, ow), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    CALLS["ds_upsample_bilinear_nhwc"] += 1
    _check(lib().ds_upsample_bilinear_nhwc(ctx_for(_dev_index(x)), xin.data_ptr(), out.data_ptr(), b, c, ih, iw, oh, ow,
                                           1 if align_corners else 0, 1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def dpt_head_front_supported(x, conv):
    """What ds_dpt_head_front takes: a zero-padded 3x3, stride-1 nn.Conv2d with 128 output channels and in % 64 == 0 on an NCHW-shaped
    activation with that many channels.  (The x2, align_corners upsample it fuses always fits the kernel's staging tile.)"""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros'
            and conv.out_channels == 128 and conv.in_channels % 64 == 0 and conv.in_channels <= 4096
            and x.dim() == 4 and x.shape[1] == conv.in_channels and x.numel() > 0)


def dpt_head_front(x, conv, out=None):
    """conv(upsample_bilinear(x, scale_factor=2, align_corners=True)) for the head's first convolution (3x3, 256 -> 128) in one kernel
    (include/depthstereo.h: ds_dpt_head_front): the upsampled map is never written.  Bit-identical to conv3x3(conv,
    upsample_bilinear(x, scale_factor=2)).  x: NCHW-shaped float16 / bfloat16 CUDA tensor (channels_last is zero-copy); returns a
    channels_last [B, 128, 2h, 2w] tensor (out: a caller-owned NHWC buffer of that many elements, for tests)."""
    torch = require_gpu()
    assert x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and dpt_head_front_supported(x, conv)
    x = x.contiguous(memory_format=torch.channels_last)
    b, c, ih, iw = x.shape
    oh, ow = 2 * ih, 2 * iw
    wk, bk = _conv_weight_image(conv, x.dtype)
    if out is None:
        out = torch.empty((b, conv.out_channels, oh, ow), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    else:
        assert out.is_cuda and out.dtype == x.dtype and out.is_contiguous() and out.numel() == b * oh * ow * conv.out_channels
    CALLS["ds_dpt_head_front"] += 1
    CALLS["ds_upsample_bilinear_nhwc"] += 1
    CALLS["ds_conv3x3_nhwc"] += 1
    _check(lib().ds_dpt_head_front(ctx_for(_dev_index(x)), x.data_ptr(), wk.data_ptr(), None if bk is None else bk.data_ptr(),
                                   out.data_ptr(), b, ih, iw, oh, ow, c, conv.out_channels,
                                   1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out


def dpt_head_tail(x, size, conv3, conv1, relu_out=True):
    """upsample(x, size, bilinear, align_corners=True) -> conv3 (3x3, 128->32) -> ReLU -> conv1 (1x1, 32->1) -> ReLU, fused
    (include/depthstereo.h: ds_dpt_head_tail; conv3.padding_mode == 'circular': ds_dpt_head_tail_circular, the 3x3 convolution
    reading the upsampled map circularly).  x: NCHW-shaped [B,128,h,w] float16/bfloat16 CUDA tensor (any memory format;
    channels_last is zero-copy).  conv3 / conv1: the nn.Conv2d modules.  Returns [B, 1, H, W]."""
    torch = require_gpu()
    b, c, ih, iw = x.shape
    assert c == 128 and tuple(conv3.weight.shape) == (32, 128, 3, 3) and tuple(conv1.weight.shape) == (1, 32, 1, 1)
    xin = x.contiguous(memory_format=torch.channels_last)
    # the repacked weights live ON the module (they die with it; a recycled id() of another model's head can never hit),
    # keyed by the storage and version of every parameter that went into them
    key = tuple((p.data_ptr(), p._version) for p in (conv3.weight, conv3.bias, conv1.weight, conv1.bias)) + (x.dtype, x.device)
    hit = getattr(conv3, "_ds_head_cache", None)
    if hit is None or hit[0] != key:
        if hit is not None:
            from . import vit_mi355x as _vm
            _vm.cache_evicted()
        w = conv3.weight.detach().to(x.dtype)                                   # [co, ci, ky, kx]
        # fragment order: [tap = ky*3+kx][slice s][half][co][j] with ci = 16 s + 8 half + j
        wf = w.permute(2, 3, 1, 0).reshape(9, 8, 2, 8, 32).permute(0, 1, 2, 4, 3).contiguous()
        hit = (key, wf, conv3.bias.detach().float().contiguous(), conv1.weight.detach().float().reshape(32).contiguous(),
               float(conv1.bias.detach().float().item()))
        conv3._ds_head_cache = hit
    _, wf, b2, w3, b3 = hit
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty((b, 1, oh, ow), dtype=x.dtype, device=x.device)
    assert conv3.padding_mode in ('zeros', 'circular') and tuple(conv3.padding) == (1, 1)
    name = "ds_dpt_head_tail_circular" if conv3.padding_mode == 'circular' else "ds_dpt_head_tail"
    CALLS[name] += 1
    _check(getattr(lib(), name)(ctx_for(_dev_index(x)), xin.data_ptr(), b, ih, iw, oh, ow, wf.data_ptr(), b2.data_ptr(),
                                w3.data_ptr(), b3, 1 if relu_out else 0, out.data_ptr(),
                                1 if x.dtype == torch.float16 else 2, _stream(x)))
    return out
