"""Shared by tests/test_lensblur_cpu.py and tests/test_gpu_lensblur.py: the NumPy MODEL of the lens blur (include/depthstereo.h: the
comment of ds_lensblur_u8 is the definition), a second, per-pixel model for tiny shapes, and the seeded inputs.

Both models are written from the definition alone.  `model` loops over the offsets of the disc and is vectorised over the image, in
int64; `model_loops` is a double loop over p and q in Python integers with its own disc count.  Neither shares code with the product
(the weight table is built here a second and a third time) or structure with the kernel (tiles, a threshold table, skipped taps)."""
import functools
import math

import numpy as np


def quarter_pixels(aperture):
    """A of the definition for an aperture in pixels per full uint16 range."""
    return int(np.rint(4.0 * aperture))


@functools.lru_cache(maxsize=None)
def disc_counts(R):
    """n(rho) for rho = 0..4 R, by counting."""
    return tuple(sum(1 for dy in range(-R, R + 1) for dx in range(-R, R + 1) if 16 * (dx * dx + dy * dy) <= rho * rho)
                 for rho in range(4 * R + 1))


def weights(R):
    return np.array([2**20 // c for c in disc_counts(R)], np.int64)


def coc(depth, focus, R, A, band):
    """rho [h, w] int64 of one map."""
    e = np.maximum(np.abs(depth.astype(np.int64) - int(focus)) - band, 0)
    assert int(e.max()) * A + 32768 < 2**32
    return np.minimum(4 * R, (e * A + 32768) >> 16)


def resolve_focus(depth, focus):
    """The focus depth of one map [h, w]: an integer as it is, ('point', fx, fy) the depth at that position; 'near' / 'far' (the test
    inputs' own words) the largest / smallest depth of the map."""
    if isinstance(focus, tuple):
        h, w = depth.shape
        return int(depth[min(h - 1, int(math.floor(focus[2] * h))), min(w - 1, int(math.floor(focus[1] * w)))])
    if isinstance(focus, str):
        return int(depth.max() if focus == 'near' else depth.min())
    return int(focus)


def model(image, depth, focus, R, A, band, invert=False, census=None):
    """(out_rgb uint8 [h, w, 3], rho uint8 [h, w]) of one image [h, w, 3] and map [h, w]; a batch [n, ...] image by image with focus a
    sequence of n.  focus: what resolve_focus takes.  census: a dict that collects what tests/test_lensblur_cpu.py asks about."""
    image, depth = np.asarray(image), np.asarray(depth)
    assert image.dtype == np.uint8 and depth.dtype == np.uint16
    if depth.ndim == 3:
        both = [model(i, d, f, R, A, band, invert, census) for i, d, f in zip(image, depth, focus)]
        return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    h, w = depth.shape
    f = resolve_focus(depth, focus)
    z = depth.astype(np.int64)
    if invert:
        z = 65535 - z
    rho = coc(depth, f, R, A, band)
    W = weights(R)
    pad = lambda a: np.pad(a, [(R, R), (R, R)] + [(0, 0)] * (a.ndim - 2))      # noqa: E731
    zq_all, rq_all, cq_all, in_all = pad(z), pad(rho), pad(image.astype(np.int64)), pad(np.ones((h, w), bool))
    den = np.zeros((h, w), np.int64)
    num = np.zeros((h, w, 3), np.int64)
    stats = dict(occluded=0, took_own=0, skipped=0)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 > R * R:
                continue
            win = (slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
            inside, zq, rq = in_all[win], zq_all[win], rq_all[win]
            far = zq < z
            rho_e = np.where(far, np.minimum(rq, rho), rq)
            counts = inside & (16 * d2 <= rho_e * rho_e)
            wgt = np.where(counts, W[rho_e], 0)
            den += wgt
            num += wgt[..., None] * cq_all[win]
            stats['occluded'] += int((inside & ~counts & (16 * d2 <= rq * rq)).sum())
            stats['took_own'] += int((counts & far & (rho < rq)).sum())
            stats['skipped'] += int((~inside).sum())
    assert (den > 0).all()
    if census is not None:
        e_unbanded = np.abs(depth.astype(np.int64) - f)
        census['occluded'] = census.get('occluded', 0) + stats['occluded']
        census['took_own'] = census.get('took_own', 0) + stats['took_own']
        census['skipped'] = census.get('skipped', 0) + stats['skipped']
        census['clamped'] = census.get('clamped', 0) + int(((np.maximum(e_unbanded - band, 0) * A + 32768) >> 16 > 4 * R).sum())
        census['banded'] = census.get('banded', 0) + int(((rho == 0) & ((e_unbanded * A + 32768) >> 16 > 0)).sum())
        census['max_num'] = max(census.get('max_num', 0), int(num.max()))
        census['max_den'] = max(census.get('max_den', 0), int(den.max()))
    return ((2 * num + den[..., None]) // (2 * den[..., None])).astype(np.uint8), rho.astype(np.uint8)


def model_loops(image, depth, focus, R, A, band, invert=False):
    """The same outputs of one image, pixel by pixel in Python integers: for tiny shapes."""
    h, w = depth.shape
    f = resolve_focus(depth, focus)
    D = [[int(v) for v in row] for row in depth]
    Z = [[65535 - v if invert else v for v in row] for row in D]
    rho = [[min(4 * R, (max(abs(v - f) - band, 0) * A + 32768) >> 16) for v in row] for row in D]

    @functools.lru_cache(maxsize=None)
    def weight(r):
        reach = r // 4
        return 2**20 // sum(1 for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1) if 16 * (dx * dx + dy * dy) <= r * r)
    out = np.zeros((h, w, 3), np.uint8)
    for py in range(h):
        for px in range(w):
            den, num = 0, [0, 0, 0]
            for qy in range(max(0, py - R), min(h, py + R + 1)):
                for qx in range(max(0, px - R), min(w, px + R + 1)):
                    d2 = (qy - py)**2 + (qx - px)**2
                    if d2 > R * R:
                        continue
                    r = min(rho[qy][qx], rho[py][px]) if Z[qy][qx] < Z[py][px] else rho[qy][qx]
                    if 16 * d2 <= r * r:
                        den += weight(r)
                        for c in range(3):
                            num[c] += weight(r) * int(image[qy, qx, c])
            for c in range(3):
                out[py, px, c] = (2 * num[c] + den) // (2 * den)
    return out, np.array(rho, np.uint8)


def accumulator_bound(R=32):
    """(largest den, largest num) any pixel can reach: a tap at (dx, dy) adds at most W[ceil(4 sqrt(d2))], the largest weight of a disc
    that contains it."""
    W = weights(R)
    total = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 <= R * R:
                t = math.isqrt(16 * d2 - 1) + 1 if d2 else 0             # the least t with t^2 >= 16 d2
                total += int(W[t])
    return total, 255 * total


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def random_image(h, w, seed, n=None):
    return np.random.default_rng(seed).integers(0, 256, ((h, w, 3) if n is None else (n, h, w, 3)), dtype=np.uint8)


def random_depth(h, w, seed, n=None):
    return np.random.default_rng(seed).integers(0, 65536, ((h, w) if n is None else (n, h, w)), dtype=np.uint16)


def ramp_noise(h, w, seed, span, n=None):
    """A ramp over `span` levels from corner to corner, +-3 levels of noise."""
    y, x = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed).integers(-3, 4, ((h, w) if n is None else (n, h, w)))
    return (9000 + (span * (2 * x * (h - 1) + y * (w - 1))) // max(1, 3 * (h - 1) * (w - 1)) + noise).astype(np.uint16)


def cliff(h, w, seed, gap, n=None):
    """Two planes `gap` levels apart, the near one (white) right of the middle, +-3 levels of noise: at the same column in every image."""
    y, x = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed).integers(-3, 4, ((h, w) if n is None else (n, h, w)))
    return (8000 + np.where(x >= w // 2, gap, 0) + 0 * y + noise).astype(np.uint16)


def flat(h, w, n=None):
    return np.full((h, w) if n is None else (n, h, w), 777, np.uint16)


def span_of(R, A):
    """The depth range over which rho runs from 0 to 1.5 times its clamp 4 R."""
    return min(50000, (6 * R * 65536) // A)


# (n, h, w), (radius, aperture, focus, band): smaller than any tile; ragged both ways with a different focus per image; several tiles at
# the largest halo; narrower than the halo; the largest halo on a map of 24 pixels with A = 65535.  band is twice the depth difference
# at which rho leaves 0, so that it is what makes some rho 0.  focus: an entry per image where it is a list.
KERNEL_CASES = [((1, 5, 7), (2, 6.0, 'near', 2734)), ((2, 9, 33), (8, 24.0, [('point', 0.25, 0.5), 'far'], 686)),
                ((1, 40, 70), (32, 128.0, ('point', 0.3, 0.6), 130)), ((3, 17, 16), (16, 40.0, 'near', 412)),
                ((1, 4, 6), (32, 16383.75, ('point', 0.5, 0.5), 4))]
KERNEL_IDS = ["%dx%dx%d-R%d" % (s + p[:1]) for s, p in KERNEL_CASES]
DEPTHS = ("random", "ramp", "cliff", "flat")


@functools.lru_cache(maxsize=None)
def inputs(shape, R, A):
    """(image [n, h, w, 3], {name: depth [n, h, w]}) of one case (seeded: the same arrays for every test that asks; read-only)."""
    n, h, w = shape
    seed = 100 * h + w
    span = span_of(R, A)
    image = random_image(h, w, seed, n)
    depths = {"random": random_depth(h, w, seed + 1, n), "ramp": ramp_noise(h, w, seed + 2, span, n),
              "cliff": cliff(h, w, seed + 3, span // 2, n), "flat": flat(h, w, n)}
    for a in (image,) + tuple(depths.values()):
        a.setflags(write=False)
    return image, depths


def focus_list(depth, focus):
    """The focus depths of a batch [n, h, w] as a list of n integers (what the binding is given)."""
    specs = focus if isinstance(focus, list) else [focus] * len(depth)
    assert len(specs) == len(depth)
    return [resolve_focus(d, f) for d, f in zip(depth, specs)]


@functools.lru_cache(maxsize=None)
def want(case, name, invert):
    """The model's (out_rgb, rho) of KERNEL_CASES[case] on the depth input `name`, computed once; read-only."""
    shape, (R, aperture, focus, band) = KERNEL_CASES[case]
    image, depths = inputs(shape, R, quarter_pixels(aperture))
    got = model(image, depths[name], focus_list(depths[name], focus), R, quarter_pixels(aperture), band, invert)
    for a in got:
        a.setflags(write=False)
    return got
