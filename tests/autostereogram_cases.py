"""Shared by tests/test_autostereogram_cpu.py and tests/test_gpu_autostereogram.py: the NumPy MODEL of the single-image stereogram
(include/depthstereo.h: the comment of ds_autostereogram_u8 is the definition) and the seeded inputs.

The model is written from the definition alone: separation and visibility in int64 over a whole row at once, then the links of the row
one after the other through a sequential union-find that always hangs the smaller root under the larger, so that a component's root
IS its largest column.  It shares no code with the product and no structure with the kernel (label propagation in rounds, atomic
maxima, pointer jumping)."""
import functools

import numpy as np

A = 256 * 65535
MODES = (0, 1, 2)


def separation(z, P, m):
    """s(z) of the definition for an integer or an int64 array."""
    z = np.asarray(z, dtype=np.int64)
    den = 2 * A - m * z
    num = 2 * P * (A - m * z)
    return (2 * num + den) // (2 * den)


def nearness(depth_row, invert=False):
    z = np.asarray(depth_row).astype(np.int64)
    return 65535 - z if invert else z


def hidden(z, P, m):
    """bool [w]: the columns of a row of nearness z (int64) that the visibility test hides."""
    w = len(z)
    k = 2 * A - m * z
    hid = np.zeros(w, bool)
    alive = np.ones(w, bool)
    t = 0
    while True:
        t += 1
        zt = z + (2 * t * k) // (m * 2 * P)
        alive &= zt < 65535                                                   # stop at the first t with zt >= 65535
        if not alive.any():
            break
        assert t <= m * P // 512 + 1
        if t < w:                                                             # columns outside the row occlude nothing
            left = np.zeros(w, bool)
            right = np.zeros(w, bool)
            left[t:] = z[:-t] >= zt[t:]
            right[:-t] = z[t:] >= zt[:-t]
            hid |= alive & (left | right)
    return hid


def links(z, P, m):
    """(l, r, offered) of a row: column x offers {l[x], r[x]} where offered[x]."""
    w = len(z)
    x = np.arange(w, dtype=np.int64)
    s = separation(z, P, m)
    l = x - (s >> 1)
    r = l + s
    return l, r, (l >= 0) & (r < w) & ~hidden(z, P, m)


def representatives(z, P, m):
    """rep int64 [w]: the largest column of each column's component."""
    w = len(z)
    l, r, offered = links(z, P, m)
    parent = list(range(w))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for x in np.flatnonzero(offered).tolist():
        a, b = find(int(l[x])), find(int(r[x]))
        if a != b:
            parent[min(a, b)] = max(a, b)
    return np.array([find(x) for x in range(w)], dtype=np.int64)


def lowbias32(v):
    v = np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF
    v ^= v >> 16
    v = (v * 0x7FEB352D) & 0xFFFFFFFF
    v ^= v >> 15
    v = (v * 0x846CA68B) & 0xFFFFFFFF
    v ^= v >> 16
    return v


def colours(rep, mode, seed, tile=None):
    """uint8 [h, w, 3] from rep int64 [h, w]."""
    h, w = rep.shape
    y = np.arange(h, dtype=np.int64)[:, None]
    if mode == 2:
        ph, pw = tile.shape[:2]
        return tile[y % ph, rep % pw]
    hsh = lowbias32((int(seed) & 0xFFFFFFFF) ^ ((y * 0x9E3779B1) & 0xFFFFFFFF) ^ ((rep * 0x85EBCA77) & 0xFFFFFFFF))
    if mode == 0:
        return np.stack([hsh & 255, (hsh >> 8) & 255, (hsh >> 16) & 255], axis=-1).astype(np.uint8)
    return np.repeat((255 * (hsh >> 31)).astype(np.uint8)[..., None], 3, axis=-1)


def rep_map(depth, P, m, invert=False):
    """rep int64 [..., w] of a map [h, w] or a batch [n, h, w]."""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and 16 <= P <= 512 and 1 <= m <= 128
    rows = depth.reshape(-1, depth.shape[-1])
    return np.stack([representatives(nearness(row, invert), P, m) for row in rows]).reshape(depth.shape)


def model(depth, P, m, mode, seed, tile=None, invert=False):
    """uint8 [h, w, 3] of one map [h, w], [n, h, w, 3] of a batch [n, h, w]: the image index does not enter."""
    depth = np.asarray(depth)
    rep = rep_map(depth, P, m, invert)
    if depth.ndim == 3:
        return np.stack([colours(r, mode, seed, tile) for r in rep])
    return colours(rep, mode, seed, tile)


def census(depth, P, m, invert=False):
    """What the tests ask about one map [h, w]: hidden columns, offered links, the size of the largest component."""
    depth = np.asarray(depth)
    hid = links_n = 0
    largest = 1
    for row in depth.reshape(-1, depth.shape[-1]):
        z = nearness(row, invert)
        hid += int(hidden(z, P, m).sum())
        links_n += int(links(z, P, m)[2].sum())
        largest = max(largest, int(np.bincount(representatives(z, P, m)).max()))
    return {'hidden': hid, 'links': links_n, 'largest': largest}


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
def zeros(n, h, w, seed=0):
    return np.zeros((n, h, w), np.uint16)


def full(n, h, w, seed=0):
    return np.full((n, h, w), 65535, np.uint16)


def ramp(n, h, w, seed=0):
    """Far on the left, near on the right, over the whole range; each image and row shifted a little."""
    i, y, x = np.mgrid[0:n, 0:h, 0:w]
    return np.clip((65535 * x) // max(1, w - 1) + 997 * y - 1999 * i, 0, 65535).astype(np.uint16)


def rect(n, h, w, seed=0):
    """A near (white) rectangle on a far ground, 57000 levels apart, +-3 levels of noise; its left edge moves with the image."""
    i, y, x = np.mgrid[0:n, 0:h, 0:w]
    jitter = np.random.default_rng(seed).integers(-3, 4, (n, h, w))
    inside = (y >= h // 4) & (y < max(h // 4 + 1, (3 * h) // 4)) & (x >= w // 3 + i) & (x < (2 * w) // 3 + 1)
    return (3000 + np.where(inside, 57000, 0) + jitter).astype(np.uint16)


def noise(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 65536, (n, h, w), dtype=np.uint16)


DEPTHS = {"zeros": zeros, "full": full, "ramp": ramp, "rect": rect, "noise": noise}


def random_tile(ph, pw, seed):
    return np.random.default_rng(seed).integers(0, 256, (ph, pw, 3), dtype=np.uint8)


# tiles of mode 2: one row (ph = 1), a width that is no period of any case, more rows than any small case has (ph > h)
TILES = ((1, 7), (9, 50), (4, 96))
SEEDS = (0, 0xDEADBEEF)
PERIODS = (16, 96, 512)
FACTORS = (1, 85, 128)
# (n, h, w): the widths 1, 20 (no link from period 32 on), 67, 130, 257 at heights 1 and 5
SMALL_SHAPES = [(3, h, w) for w in (1, 20, 67, 130, 257) for h in (1, 5)]
# every (P, m) on the small shapes; on the larger ones the pairs that link there
SMALL_PARAMS = [(P, m) for P in PERIODS for m in FACTORS] + [(32, 85)]          # (P = 32 links nothing at width 20)
# one 96 x 300; 2 x 700: the only width here at which P = 512 links (s >= 341); 2 x 2100: above the width at which the entry point
# changes the size of its workgroups; 1 x 16384: the widest row, whose 96 KiB of LDS the entry point has to ask for, and with "full" at
# P = 16 chains of 1490 members
LARGE_CASES = [((1, 96, 300), [(96, 85), (16, 128), (96, 1)], ("rect", "noise")),
               ((1, 2, 700), [(512, 128), (512, 1), (96, 85)], ("rect", "noise", "ramp")),
               ((1, 2, 2100), [(96, 85), (16, 128), (512, 85)], ("rect", "noise", "full")),
               ((1, 1, 16384), [(96, 85), (16, 128)], ("rect", "full"))]
CHAIN = ((1, 1, 1500), 16, 128)                  # flat near: components of 137 members


@functools.lru_cache(maxsize=None)
def depth_input(name, shape):
    """The seeded depth [n, h, w] of one shape (the same array for every test that asks; read-only)."""
    n, h, w = shape
    a = DEPTHS[name](n, h, w, seed=100 * h + w)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_rep(name, shape, P, m, invert):
    """The model's rep of depth_input(name, shape), computed once; read-only."""
    r = rep_map(depth_input(name, shape), P, m, invert)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def tile_input(k):
    t = random_tile(TILES[k][0], TILES[k][1], 7 + k)
    t.setflags(write=False)
    return t


def want(name, shape, P, m, invert, mode, seed, tile=None):
    rep = want_rep(name, shape, P, m, invert)
    return np.stack([colours(r, mode, seed, tile) for r in rep])
