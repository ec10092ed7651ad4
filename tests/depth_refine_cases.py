"""Shared by tests/test_depth_refine_cpu.py and tests/test_gpu_depth_refine.py: the float64 NumPy MODEL of depth refinement (the joint
bilateral filter of a uint16 depth map guided by an RGB image; the definition is in include/depthstereo.h, ds_joint_bilateral_u16) and
the seeded inputs both files use.  The model is a loop over the taps in raster order, vectorised over the image: per pixel it performs
the operations of the definition in the definition's order (one rounded multiply for the weight, the product rounded and then the sum
rounded, one IEEE division, np.rint), so the kernel must reproduce it bit for bit.  It is written from the definition alone and shares
no code with the product's table builder -- nor with the unguided sibling's model in normalmap_bilateral_cases.py, although the two
kernels are one routine now: a model that shared the product's structure could share its mistakes.  Only the depth inputs are shared."""
import numpy as np

# the depth inputs are those of the unguided sibling's tests, under the names the tests of depth refinement use
from normalmap_bilateral_cases import CLIFF, STEP, cases as depth_cases, ramp_noise, random_depth, staircase  # noqa: F401


def tables(d, sigma_color, sigma_space):
    r = d // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    ws = np.exp(-(dx * dx + dy * dy) / (2.0 * sigma_space**2))               # the definition's expression, on the whole window
    ws[dx * dx + dy * dy > r * r] = 0.0
    wc = np.exp(-(np.arange(766, dtype=np.float64)**2) / (2.0 * sigma_color**2))
    return ws, wc


def model(depth, guide, params, wrap=False):
    """depth: uint16 [h, w] or [n, h, w]; guide: uint8 [h, w, c] or [n, h, w, c], c >= 3 (channels 0..2 are read);
    params = (d, sigma_color, sigma_space) or (d, sigma_color, sigma_space, iterations) -> uint16, the depth's shape."""
    depth, guide = np.asarray(depth), np.asarray(guide)
    assert depth.dtype == np.uint16 and guide.dtype == np.uint8
    if depth.ndim == 3:
        return np.stack([model(x, g, params, wrap) for x, g in zip(depth, guide)])
    if len(params) == 4:
        for _ in range(params[3]):
            depth = model(depth, guide, params[:3], wrap)
        return depth
    d, sigma_color, sigma_space = params
    r = d // 2
    h, w = depth.shape
    assert guide.shape[:2] == (h, w) and guide.shape[2] >= 3
    assert d % 2 == 1 and 3 <= d <= 31 and (wrap or r < min(h, w))
    ws, wc = tables(d, sigma_color, sigma_space)
    mode = 'wrap' if wrap else 'reflect'                                                  # 'reflect' = BORDER_REFLECT_101
    pad = np.pad(depth, r, mode=mode).astype(np.float64)
    rgb = guide[:, :, :3].astype(np.int64)
    gpad = np.pad(rgb, ((r, r), (r, r), (0, 0)), mode=mode)
    num = np.zeros((h, w), np.float64)
    den = np.zeros((h, w), np.float64)
    for dy in range(d):
        for dx in range(d):
            s = ws[dy, dx]
            if s == 0.0:
                continue
            k = np.abs(gpad[dy:dy + h, dx:dx + w] - rgb).sum(axis=2)
            wgt = s * wc[k]
            num = num + wgt * pad[dy:dy + h, dx:dx + w]
            den = den + wgt
    return np.rint(num / den).astype(np.uint16)


# ---- guide inputs ---------------------------------------------------------------------------------------------------------------------
def noise_guide(h, w, seed, n=None):
    """uint8 white noise: the colour differences of a window are all over 0..765."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, ((h, w, 3) if n is None else (n, h, w, 3)), dtype=np.uint8)


def regions_guide(h, w, seed, n=None, edge_at=None, noise=4):
    """Two colour regions that meet at column edge_at (default: the middle), each with +-noise levels of noise per channel."""
    rng = np.random.default_rng(seed)
    edge_at = w // 2 if edge_at is None else edge_at
    left, right = np.array([60, 110, 70]), np.array([190, 150, 90])
    base = np.where((np.arange(w) >= edge_at)[None, :, None], right, left)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    return (np.broadcast_to(base, shape) + rng.integers(-noise, noise + 1, shape)).astype(np.uint8)


def constant_guide(h, w, n=None):
    return np.full((h, w, 3) if n is None else (n, h, w, 3), 97, np.uint8)


def with_fourth_byte(guide, seed):
    """A c == 4 copy of a c == 3 guide whose fourth byte is random: it must not matter."""
    rng = np.random.default_rng(seed)
    return np.concatenate([guide, rng.integers(0, 256, guide.shape[:-1] + (1,), dtype=np.uint8)], axis=-1)


def guide_cases(h, w, seed, n=None):
    return [("noise", noise_guide(h, w, seed, n)), ("regions", regions_guide(h, w, seed + 1, n)), ("constant", constant_guide(h, w, n))]


# ---- the silhouette scene ------------------------------------------------------------------------------------------------------------
def silhouette_scene(seed=2024, h=24, w=64, edge=32, ramp=12, offset=2, lo=10000, hi=50000):
    """Two noisy colour regions that meet at column `edge`, and a lo -> hi depth ramp `ramp` columns wide centred `offset` columns off
    that colour edge.  Returns (depth uint16 [h,w], guide uint8 [h,w,3])."""
    x = np.arange(w, dtype=np.float64)
    start = edge + offset - ramp / 2.0                                       # the ramp covers [start, start + ramp)
    row = lo + (hi - lo) * np.clip((x - start + 0.5) / ramp, 0.0, 1.0)
    depth = np.broadcast_to(np.rint(row), (h, w)).astype(np.uint16).copy()
    return depth, regions_guide(h, w, seed, edge_at=edge)


def row_steps(depth):
    """|D[x+1] - D[x]| along the middle row, as int64 [w - 1]; step i lies between columns i and i + 1."""
    mid = np.asarray(depth)[depth.shape[0] // 2].astype(np.int64)
    return np.abs(np.diff(mid))
