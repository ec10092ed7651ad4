"""Host side of the custom-depth ingest (reference: src/core.py:145-174): the LANCZOS coefficients of Pillow's resampler, a numpy
model of the arithmetic csrc/ds_resample.hip runs with them, the bit-depth rule, and the once-per-process comparison of that
model with the installed Pillow.  Nothing here touches the GPU.

Pillow's ``Image.resize(size, LANCZOS)`` is separable: a horizontal pass (when the width changes), then a vertical pass (when the
height changes), each rounded into the image's own pixel type.  Per axis and output index the taps and their weights are
``precompute_coeffs`` of Pillow's Resample.c, restated in `lanczos_coeffs`; they are built HERE with math.sin (the libm sin Pillow
calls -- the device's sin is not) and uploaded, like _native.build_pow_lut's table.
"""
import functools
import math

import numpy as np

# pixel types of ds_resize_lanczos / ds_custom_depth_to_f64 (include/depthstereo.h: DS_PIX_*)
PIX_U8, PIX_U16, PIX_I32, PIX_F32 = 0, 1, 2, 3
PIX_OF_MODE = {"L": PIX_U8, "RGB": PIX_U8, "I;16": PIX_U16, "I": PIX_I32, "F": PIX_F32}
PIX_DTYPE = {PIX_U8: np.uint8, PIX_U16: np.uint16, PIX_I32: np.int32, PIX_F32: np.float32}
MAX_TAPS = 1024                     # DS_RESAMPLE_MAX_TAPS: more taps per output pixel (a ~170-fold reduction) take the host route
_PRECISION_BITS = 32 - 8 - 2        # Pillow's fixed point for 8-bit pixels


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


@functools.lru_cache(maxsize=64)
def lanczos_coeffs(in_size, out_size):
    """(ksize, bounds int32 [out, 2] = (first tap, tap count), weights float64 [out, ksize] zero-filled past the count) of one
    axis: precompute_coeffs of Pillow's Resample.c for the LANCZOS filter (support 3) and the box (0, in_size)."""
    scale = float(np.float32(in_size) - np.float32(0)) / out_size          # the box is held as C floats
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * inv) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = w
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return ksize, bounds, kk


def fixed_point_coeffs(kk):
    """normalize_coeffs_8bpc: (int)(+-0.5 + w * 2^22), C truncation, the sign of the half follows w."""
    v = kk * float(1 << _PRECISION_BITS)
    return np.trunc(np.where(kk < 0, -0.5 + v, 0.5 + v)).astype(np.int32)


def _round_up(ss):
    """Pillow's ROUND_UP: (int)(ss >= 0 ? ss + 0.5 : ss - 0.5) -- add the half in float64, then truncate."""
    return np.trunc(np.where(ss >= 0.0, ss + 0.5, ss - 0.5))


def _model_pass(a, pix, in_size, out_size):
    """One pass along the LAST axis of a [..., in_size] array of pixel type `pix`; taps added in ascending order."""
    ksize, bounds, kk = lanczos_coeffs(in_size, out_size)
    xmin, xmax = bounds[:, 0].astype(np.int64), bounds[:, 1]
    if pix == PIX_U8:
        ki = fixed_point_coeffs(kk)
        acc = np.full(a.shape[:-1] + (out_size,), 1 << (_PRECISION_BITS - 1), np.int32)
        for t in range(ksize):
            idx = np.minimum(xmin + t, in_size - 1)
            acc += a[..., idx].astype(np.int32) * np.where(t < xmax, ki[:, t], 0).astype(np.int32)
        return np.clip(acc >> _PRECISION_BITS, 0, 255).astype(np.uint8)
    ss = np.zeros(a.shape[:-1] + (out_size,), np.float64)
    for t in range(ksize):
        idx = np.minimum(xmin + t, in_size - 1)
        live = t < xmax
        # (adding +0.0 for the taps past the count leaves the sum as it is: a sum that starts at +0.0 is never -0.0)
        ss = ss + np.where(live, a[..., idx].astype(np.float64) * np.where(live, kk[:, t], 0.0), 0.0)
    if pix == PIX_F32:
        return ss.astype(np.float32)
    r = _round_up(ss)
    if pix == PIX_I32:
        return r.astype(np.int64).astype(np.int32)
    r = r.astype(np.int64)
    # I;16: Pillow stores CLIP8(r % 256) and CLIP8(r >> 8) -- below 0 both bytes clip to 0, above 65535 only the HIGH byte clips
    return np.where(r < 0, 0, np.where(r > 65535, 0xFF00 | (r & 255), r)).astype(np.uint16)


def resize_model(planes, pix, out_hw):
    """numpy model of ds_resize_lanczos: [n, in_h, in_w] of PIX_DTYPE[pix] -> [n, out_h, out_w], horizontal pass first."""
    a = np.ascontiguousarray(planes, dtype=PIX_DTYPE[pix])
    out_h, out_w = out_hw
    n, in_h, in_w = a.shape
    if out_w != in_w:
        a = _model_pass(a, pix, in_w, out_w)
    if out_h != in_h:
        a = np.ascontiguousarray(_model_pass(np.ascontiguousarray(a.transpose(0, 2, 1)), pix, in_h, out_h).transpose(0, 2, 1))
    return a


def bit_depth(out_max):
    """reference: src/core.py:158-164.  A NaN maximum fails both tests: 32."""
    if out_max < 256:
        return 8
    if out_max < 65536:
        return 16
    return 32


_PROBE = {}


def pillow_matches_model():
    """Once per process: the model above (= the kernel's arithmetic) against the installed Pillow, one small enlargement and one
    small reduction per mode, band 0 of RGB included.  The arithmetic is Pillow's as installed, not a documented contract: on any
    difference (or any error) the custom-depth ingest stays on the host for the rest of the process."""
    if "ok" not in _PROBE:
        try:
            _PROBE["ok"] = _probe()
        except Exception:           # noqa: BLE001 -- a Pillow that cannot resize one of the modes with LANCZOS
            _PROBE["ok"] = False
    return _PROBE["ok"]


def _probe():
    from PIL import Image
    rng = np.random.default_rng(20240607)
    planes = {"L": rng.integers(0, 256, (7, 9)).astype(np.uint8), "I;16": rng.integers(0, 65536, (7, 9)).astype(np.uint16),
              "I": rng.integers(-(1 << 20), 1 << 20, (7, 9)).astype(np.int32), "F": rng.uniform(-1, 1, (7, 9)).astype(np.float32),
              "RGB": rng.integers(0, 256, (7, 9, 3)).astype(np.uint8)}
    for mode, a in planes.items():
        im = Image.fromarray(a)
        if im.mode != mode:
            return False
        for out_h, out_w in ((11, 16), (3, 4)):
            got = np.asarray(im.resize((out_w, out_h), Image.Resampling.LANCZOS))
            band0 = a[..., 0] if mode == "RGB" else a
            want = resize_model(band0[None], PIX_OF_MODE[mode], (out_h, out_w))[0]
            if mode == "RGB":
                got = got[..., 0]
            if got.shape != want.shape or got.dtype != want.dtype or got.tobytes() != want.tobytes():
                return False
    return True
