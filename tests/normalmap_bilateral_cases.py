"""Shared by tests/test_normalmap_bilateral_cpu.py and tests/test_gpu_normalmap_bilateral.py: the float64 NumPy MODEL of the
bilateral pre-filter of the normal map (the definition is in include/depthstereo.h, ds_bilateral_u16) and the seeded inputs both
files use.  The model is a loop over the taps in raster order, vectorised over the image: per pixel it performs the operations of the
definition in the definition's order (one rounded multiply for the weight, the product rounded and then the sum rounded, one IEEE
division), so the kernel must reproduce it bit for bit.  It is written from the definition alone and shares no code with the
product's table builder."""
import numpy as np


def tables(d, sigma_color, sigma_space):
    r = d // 2
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    ws = np.exp(-(dx * dx + dy * dy) / (2.0 * sigma_space**2))               # the definition's expression, on the whole window
    ws[dx * dx + dy * dy > r * r] = 0.0
    wr = np.exp(-(np.arange(65536, dtype=np.float64)**2) / (2.0 * sigma_color**2))
    return ws, wr


def model(depth, params, wrap=False):
    """depth: uint16 [h, w] or [n, h, w]; params = (d, sigma_color, sigma_space) -> float64, same shape."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16
    if depth.ndim == 3:
        return np.stack([model(x, params, wrap) for x in depth])
    d, sigma_color, sigma_space = params
    r = d // 2
    h, w = depth.shape
    assert d % 2 == 1 and 3 <= d <= 31 and (wrap or r < min(h, w))
    ws, wr = tables(d, sigma_color, sigma_space)
    pad = np.pad(depth, r, mode='wrap' if wrap else 'reflect').astype(np.int64)          # 'reflect' = BORDER_REFLECT_101
    centre = depth.astype(np.int64)
    num = np.zeros((h, w), np.float64)
    den = np.zeros((h, w), np.float64)
    for dy in range(d):
        for dx in range(d):
            s = ws[dy, dx]
            if s == 0.0:
                continue
            q = pad[dy:dy + h, dx:dx + w]
            wgt = s * wr[np.abs(q - centre)]
            v = q.astype(np.float64)
            num = num + wgt * v
            den = den + wgt
    return num / den


def random_depth(h, w, seed, n=None):
    """Full-range white noise: every neighbour matters, every index mistake shows."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, ((h, w) if n is None else (n, h, w)), dtype=np.uint16)


def ramp_noise(h, w, seed, n=None):
    """A smooth ramp plus +-3 levels of noise: many range weights are non-zero and distinct."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if n is None else (n, h, w)
    y, x = np.mgrid[0:h, 0:w]
    base = 20000 + 11 * x + 7 * y
    return (base + rng.integers(-3, 4, shape)).astype(np.uint16)


STEP = 6            # staircase: one-level steps, 6 pixels wide
CLIFF = 4096


def staircase(h, w, n=None, cliff_at=None):
    """One-level steps STEP pixels wide along x, with one CLIFF-level cliff at column cliff_at (default: the middle)."""
    cliff_at = w // 2 if cliff_at is None else cliff_at
    x = np.arange(w)
    row = 30000 + x // STEP + np.where(x >= cliff_at, CLIFF, 0)
    img = np.broadcast_to(row, (h, w)).astype(np.uint16)
    return img.copy() if n is None else np.stack([img] * n)


def cases(h, w, seed, n=None):
    return [("random", random_depth(h, w, seed, n)), ("ramp", ramp_noise(h, w, seed + 1, n)), ("staircase", staircase(h, w, n))]
