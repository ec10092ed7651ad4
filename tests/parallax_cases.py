"""Shared by tests/test_parallax_cpu.py and tests/test_gpu_parallax.py: the NumPy MODEL of the parallax renderer (include/depthstereo.h:
the comment of ds_parallax_u8 is the definition) and the seeded inputs.

The model is written from the definition alone, in int64: the splat is one np.maximum.at per corner of the footprint, the resolve one
pass per scan step over the whole view.  It shares no code with the product and no structure with the kernels (one thread per source
pixel, atomics, a skipped atomic, one thread per target)."""
import functools
import math

import numpy as np

POSE_MAX = 1024
# for every case: the identity, an extreme of every component, mixed signs
POSES = ((0, 0, 0), (1024, 0, 0), (0, 0, 1024), (-1024, -1024, -1024), (-333, 257, 0), (100, -1024, -700))
DIRECTIONS = ('left', 'right', 'up', 'down')


def resolve_focus(depth, focus):
    """The focus depth of one map [h, w]: an integer as it is, ('point', fx, fy) the depth at that position."""
    if isinstance(focus, tuple):
        h, w = depth.shape
        return int(depth[min(h - 1, int(math.floor(focus[2] * h))), min(w - 1, int(math.floor(focus[1] * w)))])
    return int(focus)


def landing(depth, focus, pose, invert=False):
    """(ux, uy, z) int64 [h, w] of one map under one pose: the landing point in sixteenths of a pixel, and the nearness."""
    h, w = depth.shape
    tx, ty, tz = (max(-POSE_MAX, min(POSE_MAX, int(t))) for t in pose)
    z = depth.astype(np.int64)
    z0 = int(focus)
    if invert:
        z, z0 = 65535 - z, 65535 - z0
    e = z - z0
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    sx, sy, m = (e * tx + 32768) >> 16, (e * ty + 32768) >> 16, (e * tz + 32768) >> 16
    cx, cy = 16 * x + 8 - 8 * w, 16 * y + 8 - 8 * h
    assert int(np.abs(cx * m).max()) < 2**28 and int(np.abs(cy * m).max()) < 2**28
    return 16 * x + 8 + sx + ((cx * m + 2048) >> 12), 16 * y + 8 + sy + ((cy * m + 2048) >> 12), z


def splat(depth, focus, pose, invert=False, census=None):
    """keys int64 [h, w] of one view."""
    h, w = depth.shape
    ux, uy, z = landing(depth, focus, pose, invert)
    X0, X1 = (ux - 5) >> 4, ((ux + 19) >> 4) - 1
    Y0, Y1 = (uy - 5) >> 4, ((uy + 19) >> 4) - 1
    assert ((X1 - X0 == 0) | (X1 - X0 == 1)).all() and ((X1 - X0 == 1) == ((((ux - 8) % 16) >= 5) & (((ux - 8) % 16) <= 12))).all()
    assert ((Y1 - Y0 == 0) | (Y1 - Y0 == 1)).all()
    key = ((z + 1) << 32) | np.arange(h * w, dtype=np.int64).reshape(h, w)
    keys = np.zeros(h * w, np.int64)
    offers = np.zeros(h * w, np.int64)
    dropped = 0
    for b in (0, 1):
        for a in (0, 1):
            X, Y = X0 + a, Y0 + b
            covered = (X <= X1) & (Y <= Y1)
            inside = covered & (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
            np.maximum.at(keys, (Y * w + X)[inside], key[inside])
            np.add.at(offers, (Y * w + X)[inside], 1)
            dropped += int((covered & ~inside).sum())
    if census is not None:
        census['collided'] = census.get('collided', 0) + int((offers > 1).sum())
        census['two_wide'] = census.get('two_wide', 0) + int(((X1 > X0) | (Y1 > Y0)).sum())
        census['dropped'] = census.get('dropped', 0) + dropped
    return keys.reshape(h, w)


def resolve(image, keys, G, census=None):
    """(out uint8 [h, w, 3], mask uint8 [h, w]) of one view from its keys."""
    h, w = keys.shape
    best = np.zeros((h, w), np.int64)
    winner = np.full((h, w), -1)
    for d, (dy, dx) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):           # left, right, up, down
        cand = np.zeros((h, w), np.int64)
        for s in range(1, G + 1):
            shifted = np.zeros((h, w), np.int64)                                # keys at (Y + s dy, X + s dx), 0 beyond the border
            ys, xs = s * dy, s * dx
            if abs(ys) >= h or abs(xs) >= w:
                break
            dst = (slice(max(0, -ys), h - max(0, ys)), slice(max(0, -xs), w - max(0, xs)))
            src = (slice(max(0, ys), h - max(0, -ys)), slice(max(0, xs), w - max(0, -xs)))
            shifted[dst] = keys[src]
            cand = np.where(cand == 0, shifted, cand)                           # the first key met
        take = (cand != 0) & ((best == 0) | ((cand >> 32) < (best >> 32)))      # the smallest z + 1; the earlier direction on a tie
        best = np.where(take, cand, best)
        winner = np.where(take, d, winner)
    hole = keys == 0
    own = np.arange(h * w, dtype=np.int64).reshape(h, w)
    src = np.where(~hole, keys & 0xFFFFFFFF, np.where(best != 0, best & 0xFFFFFFFF, own))
    mask = np.where(~hole, 0, np.where(best != 0, 1, 2)).astype(np.uint8)
    if census is not None:
        for d, name in enumerate(DIRECTIONS):
            census[name] = census.get(name, 0) + int((hole & (winner == d)).sum())
        census['fallback'] = census.get('fallback', 0) + int((mask == 2).sum())
    return image.reshape(h * w, 3)[src], mask


def model(image, depth, focus, poses, G, invert=False, census=None):
    """(out uint8 [F, h, w, 3], mask uint8 [F, h, w]) of one image [h, w, 3] and map [h, w]; a batch [n, ...] image by image -> [n, F,
    ...], with focus a sequence of n.  focus: what resolve_focus takes.  census: a dict that collects what tests/test_parallax_cpu.py
    asks about."""
    image, depth = np.asarray(image), np.asarray(depth)
    assert image.dtype == np.uint8 and depth.dtype == np.uint16 and 1 <= G <= 64
    if depth.ndim == 3:
        both = [model(i, d, f, poses, G, invert, census) for i, d, f in zip(image, depth, focus)]
        return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    f = resolve_focus(depth, focus)
    views = [resolve(image, splat(depth, f, pose, invert, census), G, census) for pose in poses]
    return np.stack([v[0] for v in views]), np.stack([v[1] for v in views])


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def random_image(h, w, seed, n=None):
    return np.random.default_rng(seed).integers(0, 256, ((h, w, 3) if n is None else (n, h, w, 3)), dtype=np.uint8)


def noise(h, w, seed, n=None):
    """Uniform uint16."""
    return np.random.default_rng(seed).integers(0, 65536, ((h, w) if n is None else (n, h, w)), dtype=np.uint16)


def ramp(h, w, seed, n=None):
    """A gradient from corner to corner over most of the range, +-3 levels of noise."""
    y, x = np.mgrid[0:h, 0:w]
    jitter = np.random.default_rng(seed).integers(-3, 4, ((h, w) if n is None else (n, h, w)))
    return (2000 + (60000 * (2 * x * max(1, h - 1) + y * max(1, w - 1))) // max(1, 3 * max(1, h - 1) * max(1, w - 1)) + jitter).astype(np.uint16)


def cliff(h, w, seed, n=None):
    """A near (white) rectangle around the middle on a far ground, 60000 levels apart, +-3 levels of noise."""
    y, x = np.mgrid[0:h, 0:w]
    jitter = np.random.default_rng(seed).integers(-3, 4, ((h, w) if n is None else (n, h, w)))
    rect = (y >= h // 3) & (y < h // 3 + max(1, h // 4)) & (x >= w // 3) & (x < w // 3 + max(1, w // 3))
    return (2000 + np.where(rect, 60000, 0) + jitter).astype(np.uint16)


# (n, h, w), fill, focus per image: smaller than any block of threads; ragged both ways with a focus per image; scans longer than a
# block, several blocks; narrower than a wave.  ('point', 0.5, 0.4) lies on the cliff's near rectangle.
KERNEL_CASES = [((1, 5, 7), 2, [('point', 0.5, 0.4)]), ((2, 19, 37), 4, [('point', 0.5, 0.4), 30000]),
                ((1, 40, 70), 64, [('point', 0.5, 0.4)]), ((1, 33, 16), 8, [('point', 0.5, 0.4)])]
KERNEL_IDS = ["%dx%dx%d-G%d" % (s + (g,)) for s, g, _ in KERNEL_CASES]
DEPTHS = ("ramp", "cliff", "noise")


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(image [n, h, w, 3], {name: depth [n, h, w]}) of one shape (seeded: the same arrays for every test that asks; read-only)."""
    n, h, w = shape
    seed = 100 * h + w
    image = random_image(h, w, seed, n)
    depths = {"ramp": ramp(h, w, seed + 1, n), "cliff": cliff(h, w, seed + 2, n), "noise": noise(h, w, seed + 3, n)}
    for a in (image,) + tuple(depths.values()):
        a.setflags(write=False)
    return image, depths


def focus_list(depth, focus):
    """The focus depths of a batch [n, h, w] as a list of n integers (what the binding is given)."""
    assert len(focus) == len(depth)
    return [resolve_focus(d, f) for d, f in zip(depth, focus)]


@functools.lru_cache(maxsize=None)
def want(case, name, invert):
    """The model's (out, mask) of KERNEL_CASES[case] on the depth input `name` under POSES, computed once; read-only."""
    shape, G, focus = KERNEL_CASES[case]
    image, depths = inputs(shape)
    got = model(image, depths[name], focus_list(depths[name], focus), POSES, G, invert)
    for a in got:
        a.setflags(write=False)
    return got
