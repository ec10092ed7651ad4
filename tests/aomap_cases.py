"""Shared by tests/test_aomap_cpu.py and tests/test_gpu_aomap.py: the NumPy MODEL of the ambient-occlusion map (include/depthstereo.h:
the comment of ds_aomap_u16 is the definition) and the seeded inputs.

The model is written from the definition alone: a Python loop over rays and taps, vectorised over the image, with int64 cross
products.  It shares no code with the product (its ray table is built here a second time, tap by tap) and no structure with the
kernel (which compares exact float64 products of squares kept per ray, inside tiles)."""
import functools

import numpy as np

RADII = range(1, 33)
DIRECTIONS = (4, 8, 16)


@functools.lru_cache(maxsize=None)
def rays(radius, directions):
    """The ray table: a tuple of `directions` tuples of (dx, dy, d2), taps in increasing step."""
    out = []
    for k in range(directions):
        o = k * 16 // directions
        q, r = o // 4, o % 4
        ray = []
        for s in range(1, radius + 1):
            m = int(np.rint(s * (np.sqrt(2.0) - 1.0)))
            dx, dy = {0: (s, 0), 1: (s, m), 2: (s, s), 3: (m, s)}[r]
            for _ in range(q):
                dx, dy = -dy, dx
            if dx * dx + dy * dy <= radius * radius:
                ray.append((dx, dy, dx * dx + dy * dy))
        out.append(tuple(ray))
    return tuple(out)


def table(radius, directions):
    """The table in the C ABI's layout: (taps int32 [T, 2], dir_start int32 [directions + 1])."""
    rs = rays(radius, directions)
    taps = np.array([(dx, dy) for ray in rs for dx, dy, _ in ray], np.int32).reshape(-1, 2)
    return taps, np.cumsum([0] + [len(ray) for ray in rs]).astype(np.int32)


def model(depth, radius, directions, relief, intensity=1.0, invert=False, wrap=False, tie_ge=False):
    """(uint8 map, float64 unclamped value) of one uint16 map [h, w], or of a batch [n, h, w] image by image.
    tie_ge: the OPPOSITE tie rule (a later tap of equal slope wins), for the census of tests/test_aomap_cpu.py only."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim in (2, 3)
    if depth.ndim == 3:
        both = [model(d, radius, directions, relief, intensity, invert, wrap, tie_ge) for d in depth]
        return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    H = depth.astype(np.int64)
    if invert:
        H = 65535 - H
    h, w = H.shape
    z = relief / 65535.0
    c = intensity / directions
    yy, xx = np.mgrid[0:h, 0:w]
    S = np.zeros((h, w), np.float64)
    for ray in rays(radius, directions):
        bn = np.zeros((h, w), np.int64)
        bd = np.ones((h, w), np.int64)
        for dx, dy, d2 in ray:
            y, x = yy + dy, xx + dx
            if wrap:
                inside = np.ones((h, w), bool)
                y, x = y % h, x % w
            else:
                inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
                y, x = np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)
            delta = H[y, x] - H
            lhs, rhs = delta * delta * bd, bn * bn * d2
            better = inside & (delta > 0) & ((lhs >= rhs) if tie_ge else (lhs > rhs))
            bn = np.where(better, delta, bn)
            bd = np.where(better, d2, bd)
        a = bn.astype(np.float64) * z
        S = S + a / np.sqrt(bd.astype(np.float64) + a * a)
    v = 1.0 - S * c
    return np.rint(255.0 * np.minimum(np.maximum(v, 0.0), 1.0)).astype(np.uint8), v


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def random_depth(h, w, seed, n=None):
    return np.random.default_rng(seed).integers(0, 65536, ((h, w) if n is None else (n, h, w)), dtype=np.uint16)


def ramp_noise(h, w, seed, n=None):
    y, x = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed).integers(-3, 4, ((h, w) if n is None else (n, h, w)))
    return (20000 + 11 * x + 7 * y + noise).astype(np.uint16)


def exact_ramp(h, w, ax, ay, n=None):
    """20000 + ax * x + ay * y: collinear taps of a ray have EQUAL slope, so the tie rule decides which (bn, bd) is kept."""
    y, x = np.mgrid[0:h, 0:w]
    d = (20000 + ax * x + ay * y).astype(np.uint16)
    return d if n is None else np.stack([d] * n)


def staircase(h, w, n=None):
    y, x = np.mgrid[0:h, 0:w]
    d = (30000 + x // 6 + np.where(x >= w // 2, 4096, 0) + 0 * y).astype(np.uint16)
    return d if n is None else np.stack([np.roll(d, 3 * i, axis=-1) for i in range(n)])


def flat(h, w, n=None):
    return np.full((h, w) if n is None else (n, h, w), 777, np.uint16)


def spike(h, w, n=None):
    d = np.full((h, w) if n is None else (n, h, w), 1000, np.uint16)
    d[..., h // 2, w // 3] = 60000
    return d


def depth_cases(h, w, seed, n=None):
    """[(name, uint16 [h, w] or [n, h, w])]: the inputs every kernel case runs on."""
    return [("random", random_depth(h, w, seed, n)), ("ramp", ramp_noise(h, w, seed + 1, n)), ("ramp12_12", exact_ramp(h, w, 12, 12, n)),
            ("ramp11_7", exact_ramp(h, w, 11, 7, n)), ("staircase", staircase(h, w, n)), ("flat", flat(h, w, n)), ("spike", spike(h, w, n))]


# (n, h, w), (radius, directions, relief, intensity): smaller than a tile, ragged in both directions, several 64 x 32 tiles at the
# largest radius and ray count, the largest table against a map narrower than the halo, a radius whose diagonals are empty.
# relief = 2000 with intensity 1.5 drives v below 0 on the random input (the clamp runs).
KERNEL_CASES = [((1, 5, 7), (3, 4, 65535.0, 1.0)), ((2, 9, 33), (8, 8, 64.0, 1.0)), ((1, 40, 70), (32, 16, 2000.0, 1.5)),
                ((3, 17, 16), (16, 16, 32.0, 1.0)), ((2, 9, 33), (1, 8, 300.0, 1.0))]
KERNEL_IDS = ["%dx%dx%d-R%d-K%d" % (s + p[:2]) for s, p in KERNEL_CASES]
INVERTED = ("ramp", "spike")                # the inputs that also run with invert


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """{name: depth [n, h, w]} of one shape (seeded: the same arrays for every test that asks; read-only)."""
    n, h, w = shape
    cases = dict(depth_cases(h, w, seed=100 * h + w, n=n))
    for d in cases.values():
        d.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def want(shape, params, name, invert, wrap):
    """The model's (uint8, float64) answer, computed once per (inputs, parameters, invert, border rule); read-only."""
    u8, f64 = model(inputs(shape)[name], *params, invert=invert, wrap=wrap)
    u8.setflags(write=False)
    f64.setflags(write=False)
    return u8, f64
