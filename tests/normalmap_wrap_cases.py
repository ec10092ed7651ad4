"""Shared by tests/test_normalmap_wrap_cpu.py and tests/test_gpu_normalmap_wrap.py: the DEFINITION of the wrap-around normal map and
the inputs both files use.

    normalmap_wrap(d) = normalmap(np.pad(d, R, mode='wrap'))[R:R+h, R:R+w]
    R = pre_blur // 2 + (max(sobel, 3) // 2 if Sobel else 1) + post_blur // 2          (a blur that is off contributes 0)

`normalmap` is whatever reference-exact function the caller hands in (the CPU oracle, or the project's own non-wrap entry point)."""
import numpy as np

# (pre_blur, sobel, post_blur); 0 = off (sobel 0 = np.gradient)
OPTIONS = [(0, 3, 0), (0, 0, 0), (5, 3, 0), (0, 5, 3), (3, 0, 3), (0, 1, 0), (7, 7, 7)]
OPTIONS_F32 = [(0, 0, 0), (3, 0, 3)]              # float32 stays float32 with np.gradient only (Sobel promotes it to float64)
SEPARABLE = [(5, 3, 0), (0, 5, 3), (3, 0, 3), (0, 1, 0), (7, 7, 7)]


def radius(pre_blur, sobel, post_blur):
    return (pre_blur // 2 if pre_blur > 0 else 0) + (max(sobel, 3) // 2 if sobel > 0 else 1) + (post_blur // 2 if post_blur > 0 else 0)


def _none(k):
    return k if k > 0 else None


def wrap_by_definition(normalmap, d, pre_blur, sobel, post_blur, invert=False):
    """normalmap(depth, pre_blur, sobel_gradient, post_blur, invert) -> h x w x 3 uint8 array-like, the reflect-border function."""
    r = radius(pre_blur, sobel, post_blur)
    h, w = d.shape
    out = np.asarray(normalmap(np.pad(d, r, mode='wrap'), _none(pre_blur), _none(sobel), _none(post_blur), invert))
    return out[r:r + h, r:r + w]


def plain(normalmap, d, pre_blur, sobel, post_blur, invert=False):
    return np.asarray(normalmap(d, _none(pre_blur), _none(sobel), _none(post_blur), invert))


def depth(h, w, dtype, seed):
    """Rough (white-noise) depth: every neighbour matters, every index mistake shows."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint16:
        return rng.integers(0, 65536, (h, w), dtype=np.uint16)
    return (rng.random((h, w)) * 60000.0).astype(dtype)              # finite in float16 too


def smooth_periodic(h=48, w=64):
    """A smooth map that is exactly periodic in both directions, with a slope across all four borders."""
    y, x = np.mgrid[0:h, 0:w]
    u, v = 2 * np.pi * x / w, 2 * np.pi * y / h
    f = 0.5 + 0.2 * np.sin(u + 0.7) + 0.2 * np.sin(v + 1.1) + 0.08 * np.sin(u + v + 0.3)
    return np.round(f * 65535.0).astype(np.uint16)


def ring_mask(h, w, r=1):
    m = np.ones((h, w), bool)
    if h > 2 * r and w > 2 * r:
        m[r:h - r, r:w - r] = False
    return m
