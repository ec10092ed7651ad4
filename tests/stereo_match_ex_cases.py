"""Shared by tests/test_stereo_match_ex_cpu.py, tests/test_gpu_stereo_match_ex.py and tests/test_gpu_speckle_filter.py: the NumPy MODEL of
ds_stereo_match_ex_u8 and ds_speckle_filter_i16 (include/depthstereo.h: their comment is the definition), on top of
tests/stereo_match_cases.py, whose steps it reuses unchanged.

Written from the definition alone.  A diagonal direction is one recurrence over the rows of whole planes: the previous row shifted by
one column, restarted where the predecessor lies outside the image.  The speckle filter is a plain flood fill over an explicit stack,
pixel by pixel -- no labels, no links, no merging: it shares nothing with the kernels' union-find."""
import functools

import numpy as np

import stereo_match_cases as sc

DIAGONALS = ((1, 1), (-1, -1), (1, -1), (-1, 1))                             # (dy, dx)
EX_OFF = (4, 0, 0)                                                            # paths, speckle_size, speckle_range: ds_stereo_match_u8
PRESET = (8, 64, 1)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def diagonal_path(C, P1, P2, dy, dx):
    """Step 4, one diagonal direction r = (dy, dx): L_r [h,w,D]."""
    V = C if dy > 0 else C[::-1]                                              # now the predecessor of row i is row i - 1
    h, w, D = V.shape
    L = np.empty_like(V)
    L[0] = V[0]
    absent = np.full((w, 1), 1 << 30, np.int64)
    x = np.arange(w)
    inside = (x - dx >= 0) & (x - dx < w)                                     # the predecessor's column x - dx lies in the row
    src = np.clip(x - dx, 0, w - 1)
    for i in range(1, h):
        q = L[i - 1][src]                                                     # [w, D]: L_r of the predecessor (garbage where outside)
        m = q.min(axis=1, keepdims=True)
        below = np.concatenate([absent, q[:, :-1]], axis=1) + P1
        above = np.concatenate([q[:, 1:], absent], axis=1) + P1
        step = V[i] + np.minimum(np.minimum(q, m + P2), np.minimum(below, above)) - m
        L[i] = np.where(inside[:, None], step, V[i])
    return L if dy > 0 else L[::-1]


def aggregate(C, P1, P2, paths):
    S = sc.aggregate(C, P1, P2)
    if paths == 8:
        for dy, dx in DIAGONALS:
            L = diagonal_path(C, P1, P2, dy, dx)
            assert L.min() >= 0 and L.max() <= sc.OUTSIDE + 255
            S = S + L
        assert S.max() <= 2232
    else:
        assert paths == 4
    return S


def speckle_sizes(disp, valid, t):
    """The pixel count of every pixel's component, 0 for a non-node: int64 [h,w].  One image; a flood fill from every unvisited node."""
    disp = np.asarray(disp).astype(np.int64)
    node = np.asarray(valid) != 0
    h, w = disp.shape
    sizes = np.zeros((h, w), np.int64)
    seen = np.zeros((h, w), bool)
    for y0 in range(h):
        for x0 in range(w):
            if not node[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack, members = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                members.append((y, x))
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < h and 0 <= xx < w and node[yy, xx] and not seen[yy, xx] and abs(disp[y, x] - disp[yy, xx]) <= t:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
            for y, x in members:
                sizes[y, x] = len(members)
    return sizes


def speckle_filter(disp, valid, size, t):
    """[n,h,w] x 2 -> (valid_out uint8 [n,h,w], size_out uint32 [n,h,w]): image by image."""
    sizes = np.stack([speckle_sizes(d, v, t) for d, v in zip(disp, valid)])
    return (sizes > size).astype(np.uint8), sizes.astype(np.uint32)


def component_sizes(sizes):
    """The sorted list of the component sizes of one image, from its size map: a component of k pixels shows k times the value k."""
    vals, counts = np.unique(sizes[sizes > 0], return_counts=True)
    assert (counts % vals == 0).all()
    return sorted(int(v) for v, c in zip(vals, counts) for _ in range(int(c // v)))


def match_front(left, right, D, d0, P1, P2, u, lr, paths):
    """Steps 1-7 with the extended step 4, for one pair [h,w,c] uint8: a dict of int64 / bool planes, 'disp16' and 'valid7' (the mask of
    step 7) among them."""
    cl, cr = sc.census_words(sc.luma(left)), sc.census_words(sc.luma(right))
    h, w = cl.shape
    S = aggregate(sc.cost_volume(cl, cr, D, d0), P1, P2, paths)
    ds = S.argmin(axis=2)                                                     # step 5
    S1 = S.min(axis=2)
    e = np.arange(D)[None, None, :]
    far = np.abs(e - ds[:, :, None]) > 1
    uniq_fail = (far & (S * (100 - u) < S1[:, :, None] * 100)).any(axis=2)
    lr_fail = np.zeros((h, w), bool)
    if lr >= 0:                                                               # step 6
        dR = sc.right_view(S, d0)
        yy, xx = np.mgrid[0:h, 0:w]
        xr = xx - (d0 + ds)
        inside = (xr >= 0) & (xr < w)
        r = dR[yy, np.clip(xr, 0, w - 1)]
        lr_fail = ~inside | (r < 0) | (np.abs(r - ds) > lr)
    frac = np.zeros((h, w), np.int64)                                         # step 7
    yy, xx = np.nonzero((ds > 0) & (ds < D - 1))
    a, b, c = S[yy, xx, ds[yy, xx] - 1], S[yy, xx, ds[yy, xx]], S[yy, xx, ds[yy, xx] + 1]
    assert (a > b).all()
    den = a + c - 2 * b
    assert den.size == 0 or (den.min() > 0 and den.max() <= 2 * 2232)
    f = (16 * (a - c) + den) // (2 * den)
    assert f.size == 0 or (f.min() >= -8 and f.max() <= 8)
    frac[yy, xx] = f
    return dict(dstar=ds, frac=frac, disp16=16 * (d0 + ds) + frac, uniq_fail=uniq_fail, lr_fail=lr_fail, valid7=~uniq_fail & ~lr_fail, d0=d0)


def match_back(front, speckle_size, speckle_range, sizes=None):
    """Steps 7b-10 behind match_front: its dict, and 'sizes' (the component sizes at t = 16 speckle_range over valid7), 'valid', 'filled',
    'disparity', 'depth'.  sizes: the size map, if the caller has it already."""
    disp16, valid7, d0 = front["disp16"], front["valid7"], front["d0"]
    h, w = disp16.shape
    if sizes is None:
        sizes = speckle_sizes(disp16, valid7, 16 * speckle_range)             # step 7b
    valid = valid7 & (sizes > speckle_size) if speckle_size > 0 else valid7
    x = np.arange(w)[None, :]                                                 # step 8
    li = np.maximum.accumulate(np.where(valid, x, -1), axis=1)
    ri = np.minimum.accumulate(np.where(valid, x, w)[:, ::-1], axis=1)[:, ::-1]
    rows = np.arange(h)[:, None]
    lv = np.where(li >= 0, disp16[rows, np.clip(li, 0, w - 1)], 1 << 30)
    rv = np.where(ri < w, disp16[rows, np.clip(ri, 0, w - 1)], 1 << 30)
    near = np.minimum(lv, rv)
    filled = np.where(valid, disp16, np.where(near == 1 << 30, 16 * d0, near))
    P = np.pad(filled, 1, mode="edge")                                        # step 9
    nine = np.stack([P[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
    disparity = np.sort(nine, axis=0)[4]
    depth = sc.depth_rule(disparity)                                          # step 10
    assert disparity.min() >= -32768 and disparity.max() <= 32767
    return dict(front, filled=filled, sizes=sizes, disparity=disparity.astype(np.int16), valid=valid.astype(np.uint8), depth=depth)


def match_one_ex(left, right, D, d0, P1, P2, u, lr, paths, speckle_size, speckle_range):
    """Steps 1-10 with the extended step 4 and step 7b, for one pair [h,w,c] uint8."""
    return match_back(match_front(left, right, D, d0, P1, P2, u, lr, paths), speckle_size, speckle_range)


def model_ex(left, right, D=64, d0=0, P1=4, P2=48, u=5, lr=1, paths=4, speckle_size=0, speckle_range=0):
    """[n,h,w,c] uint8 x 2 -> (disparity int16 [n,h,w], valid uint8 [n,h,w], depth uint16 [n,h,w]): image by image."""
    outs = [match_one_ex(l, r, D, d0, P1, P2, u, lr, paths, speckle_size, speckle_range) for l, r in zip(left, right)]
    return tuple(np.stack([o[k] for o in outs]) for k in ("disparity", "valid", "depth"))


@functools.lru_cache(maxsize=None)
def _fronts(name, shape, c, params, paths):
    l, r = sc.pair(name, shape, c)
    return tuple(match_front(a, b, *params, paths) for a, b in zip(l, r))


@functools.lru_cache(maxsize=None)
def _sizes(name, shape, c, params, paths, speckle_range):
    return tuple(speckle_sizes(f["disp16"], f["valid7"], 16 * speckle_range) for f in _fronts(name, shape, c, params, paths))


@functools.lru_cache(maxsize=None)
def _parts(name, shape, c, params, ex):
    fronts = _fronts(name, shape, c, params, ex[0])
    sizes = _sizes(name, shape, c, params, ex[0], ex[2]) if ex[1] > 0 else [np.zeros_like(f["disp16"]) for f in fronts]
    return tuple(match_back(f, ex[1], ex[2], sizes=z) for f, z in zip(fronts, sizes))


@functools.lru_cache(maxsize=None)
def _want(name, shape, c, params, ex):
    outs = tuple(np.stack([o[k] for o in _parts(name, shape, c, params, ex)]) for k in ("disparity", "valid", "depth"))
    for o in outs:
        o.setflags(write=False)
    return outs


def want(name, shape, c=3, params=None, ex=PRESET):
    """The model's (disparity, valid, depth) of a named pair.  Computed once, read-only."""
    return _want(name, tuple(shape), c, tuple(params if params is not None else sc.DEFAULTS.values()), tuple(ex))


# ---- shapes and parameters of the matcher's GPU tests -----------------------------------------------------------------------------------
# sc.SMALL_SHAPES and one h > w shape: (1,1,1), (3,1,67), (1,5,1): every diagonal has length 1; (1,7,20): w < D; (1,33,257), (2,9,130):
# h < w; (1,67,5): h > w, lines from length 1 to 5 on both sides of the four or eight a workgroup owns
EX_SHAPES = sc.SMALL_SHAPES + [(1, 67, 5)]
# (D, d0, P1, P2, u, lr, c) x (paths, speckle_size, speckle_range): every D sees 8 paths with the filter off and on, 4 paths with the
# filter on, and the extremes of P1 / P2 under eight paths (the bound S <= 2232)
EX_PARAMS = [
    ((128, 0, 4, 48, 5, 1, 3), (8, 0, 0)),
    ((128, -7, 64, 255, 0, -1, 1), (8, 6, 1)),
    ((128, 5, 1, 1, 25, 0, 4), (4, 3, 0)),
    ((64, 0, 4, 48, 5, 1, 3), (8, 64, 1)),
    ((64, -7, 64, 255, 0, -1, 4), (8, 0, 16)),
    ((64, 5, 1, 1, 25, 0, 1), (4, 65535, 16)),
    ((32, 0, 4, 48, 5, 1, 1), (8, 0, 0)),
    ((32, -7, 1, 1, 50, 3, 3), (8, 2, 2)),
    ((32, 5, 64, 255, 25, 0, 4), (4, 9, 1)),
]
# the two cases whose components the issue counted, with t = 16
PLANES_EX = ("planes", sc.PLANES_CASE[0], sc.PLANES_CASE[1])
STRIPES_EX = ("stripes", (1, 33, 257), tuple(sc.DEFAULTS.values()))
LARGE_EX = ("planes",) + sc.LARGE_CASES[0][:2]                                # (1, 96, 300) at D = 64
# The guarded cases (tests/test_stereo_match_ex_cpu.py holds the guards): (name, shape, params, paths, speckle_range, sizes).  Their
# components at t = 16, counted on this model: planes at 4 paths 10 x 1, 2, 764, 3808; at 8 paths 8 x 1, 3 x 2, 4, 719, 3845; stripes at
# 4 paths 1285 components from 1 to 1314 pixels, 74, 110, 150 and 171 among them; at 8 paths 1680, 28, 43, 44, 105 and 1385 among them.
# Every size but the last of a row removes a component and keeps one; the sizes sit on both sides of the components present, on a
# component's count (it goes) and on that count minus 1 (it stays).  The last size of the rows that have a 65535 removes everything.
SPECKLE_CASES = [
    PLANES_EX + (4, 1, (1, 2, 763, 764)),
    PLANES_EX + (8, 1, (1, 2, 3, 4, 718, 719, 65535)),
    STRIPES_EX + (4, 1, (73, 74, 170, 171)),
    STRIPES_EX + (8, 1, (8, 27, 28, 104, 105, 1384)),
    LARGE_EX + (8, 1, (64,)),
]
EIGHT_PATH_CASES = [PLANES_EX, STRIPES_EX, LARGE_EX]


def sizes_of(name, shape, params, paths, speckle_range, c=3):
    """The flood fill's size maps (one per image) of a named pair's (disp16, valid) of step 7; computed once."""
    return _sizes(name, tuple(shape), c, tuple(params), paths, speckle_range)


# ---- patterns of the speckle filter's own tests -------------------------------------------------------------------------------------------
SPECKLE_SHAPES = [(1, 1, 1), (1, 1, 67), (1, 5, 1), (3, 5, 67), (2, 9, 130), (1, 33, 257), (1, 40, 300)]
# (1, 40, 300): 12000 pixels, 47 workgroups of 256 pixels, each of which covers less than a row: components span many of them both ways
PATTERNS = ("constant", "checkerboard", "serpentine", "spiral", "comb", "ramp_t", "ramp_t1", "extremes", "random", "borders")
PATTERN_T = 5


def _spiral(h, w):
    """A one-pixel-wide corridor winding inwards from the corner, a one-pixel wall between its turns: one long thin component."""
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    m[0, 0] = 1
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax]):
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1                                # a right turn
    return m


@functools.lru_cache(maxsize=None)
def _pattern(name, shape):
    n, h, w = shape
    rng = np.random.default_rng([PATTERNS.index(name)] + list(shape))
    y, x = np.mgrid[0:h, 0:w]
    t = PATTERN_T
    disp = np.full((n, h, w), 100, np.int64)
    valid = np.ones((n, h, w), np.uint8)
    if name == "constant":
        pass
    elif name == "checkerboard":                                              # diagonal contact is no link
        valid[:] = ((y + x) % 2 == 0)
    elif name == "serpentine":                                                # even rows whole, odd rows one pixel at alternating ends
        valid[:] = (y % 2 == 0) | ((y % 4 == 1) & (x == w - 1)) | ((y % 4 == 3) & (x == 0))
    elif name == "spiral":
        valid[:] = _spiral(h, w)
    elif name == "comb":                                                      # a spine along the last row, teeth on every other column
        valid[:] = (y == h - 1) | (x % 2 == 0)
    elif name == "ramp_t":                                                    # steps of t along both axes: one component
        disp[:] = -3000 + t * (x + y)
    elif name == "ramp_t1":                                                   # steps of t + 1: all singletons
        disp[:] = -3000 + (t + 1) * (x + 2 * y) if w > 1 else -3000 + (t + 1) * y
    elif name == "extremes":                                                  # -32768 beside 32767: the difference needs more than 16 bits
        disp[:] = np.where((x // 2 + y) % 2 == 0, -32768, 32767)
    elif name == "random":
        disp[:] = rng.integers(0, 4 * t, (n, h, w))
        valid[:] = rng.random((n, h, w)) < 0.8
    elif name == "borders":                                                   # the last row of an image and the first of the next would
        valid[:] = (y == 0) | (y == h - 1) | (x == w - 1)                     # link if rows ran on; so would a row's end and the next's start
        disp[:] = 100
    else:
        raise KeyError(name)
    disp, valid = np.ascontiguousarray(disp.astype(np.int16)), np.ascontiguousarray(valid.astype(np.uint8))
    disp.setflags(write=False)
    valid.setflags(write=False)
    return disp, valid


def pattern(name, shape):
    """(disp int16 [n,h,w], valid uint8 [n,h,w]), read-only, seeded by name and shape; to be filtered with t = PATTERN_T."""
    return _pattern(name, tuple(shape))


@functools.lru_cache(maxsize=None)
def _pattern_sizes(name, shape):
    disp, valid = _pattern(name, shape)
    sizes = np.stack([speckle_sizes(d, v, PATTERN_T) for d, v in zip(disp, valid)]).astype(np.uint32)
    sizes.setflags(write=False)
    return sizes


def pattern_sizes(name, shape):
    """The flood fill's size map of a pattern at t = PATTERN_T, uint32 [n,h,w]; computed once, read-only."""
    return _pattern_sizes(name, tuple(shape))
