"""Shared by tests/test_stereo_match_cpu.py and tests/test_gpu_stereo_match.py: the NumPy MODEL of depth from stereo pairs
(include/depthstereo.h: the comment of ds_stereo_match_u8 is the definition) and the seeded inputs.

The model is written from the definition alone, step by step and in int64: the census as 24 compared planes, the cost as a full volume
[h,w,D] (the kernels never store one), each path direction as one recurrence over whole planes -- all lines of a direction at once --,
the winner, the checks and the fill by argmin / cumulative maxima over rows, the median by a sort of nine planes.  It shares no code
with the product and no structure with the kernels (lanes = disparities, two directions in one packed value, costs on the fly)."""
import functools

import numpy as np

DEFAULTS = dict(D=64, d0=0, P1=4, P2=48, u=5, lr=1)
OUTSIDE = 24
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def luma(img):
    """Step 1: [h,w,c] uint8 -> int64 [h,w]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (1, 3, 4)
    v = img.astype(np.int64)
    if img.shape[2] == 1:
        return v[:, :, 0]
    return (77 * v[:, :, 0] + 150 * v[:, :, 1] + 29 * v[:, :, 2] + 128) >> 8


def census_words(Y):
    """Step 2: int64 [h,w], 24 bits each (the order is this model's own)."""
    h, w = Y.shape
    P = np.pad(Y, 2, mode="edge")
    word = np.zeros((h, w), np.int64)
    for dy in range(5):
        for dx in range(5):
            if dy == 2 and dx == 2:
                continue
            word = (word << 1) | (P[dy:dy + h, dx:dx + w] < Y)
    return word


def popcount(v):
    return _POP8[v & 255] + _POP8[(v >> 8) & 255] + _POP8[(v >> 16) & 255]


def cost_volume(cl, cr, D, d0):
    """Step 3: int64 [h,w,D]."""
    h, w = cl.shape
    C = np.full((h, w, D), OUTSIDE, np.int64)
    x = np.arange(w)
    for d in range(D):
        xr = x - (d0 + d)
        ok = (xr >= 0) & (xr < w)
        if ok.any():
            C[:, ok, d] = popcount(cl[:, ok] ^ cr[:, xr[ok]])
    return C


def path(C, P1, P2, axis, reverse):
    """Step 4, one direction: L_r [h,w,D].  All lines of the direction advance together."""
    V = np.moveaxis(C, axis, 0)                                               # [len, lines, D]
    if reverse:
        V = V[::-1]
    L = np.empty_like(V)
    L[0] = V[0]
    absent = np.full(V[0][:, :1].shape, 1 << 30, np.int64)
    for i in range(1, V.shape[0]):
        q = L[i - 1]
        m = q.min(axis=1, keepdims=True)
        below = np.concatenate([absent, q[:, :-1]], axis=1) + P1              # L_r(q, d - 1) + P1
        above = np.concatenate([q[:, 1:], absent], axis=1) + P1               # L_r(q, d + 1) + P1
        L[i] = V[i] + np.minimum(np.minimum(q, m + P2), np.minimum(below, above)) - m
    if reverse:
        L = L[::-1]
    return np.moveaxis(L, 0, axis)


def aggregate(C, P1, P2):
    S = np.zeros_like(C)
    for axis in (1, 0):
        for reverse in (False, True):
            L = path(C, P1, P2, axis, reverse)
            assert L.max() <= OUTSIDE + 255
            S += L
    assert S.max() <= 1116
    return S


def right_view(S, d0):
    """Step 6: dR [h,w] int64, -1 where undefined."""
    h, w, D = S.shape
    big = 1 << 30
    R = np.full((h, w, D), big, np.int64)
    xr = np.arange(w)
    for d in range(D):
        x = xr + d0 + d
        ok = (x >= 0) & (x < w)
        if ok.any():
            R[:, ok, d] = S[:, x[ok], d]
    dR = R.argmin(axis=2)                                                     # the first, so the smallest, minimiser
    dR[R.min(axis=2) == big] = -1
    return dR


def match_one(left, right, D, d0, P1, P2, u, lr):
    """Steps 1-10 for one pair [h,w,c] uint8.  Returns a dict of int64 / bool planes; 'disparity' int16, 'valid' uint8, 'depth' uint16
    are the three outputs of ds_stereo_match_u8."""
    cl, cr = census_words(luma(left)), census_words(luma(right))
    h, w = cl.shape
    S = aggregate(cost_volume(cl, cr, D, d0), P1, P2)
    ds = S.argmin(axis=2)                                                     # step 5
    S1 = S.min(axis=2)
    e = np.arange(D)[None, None, :]
    far = np.abs(e - ds[:, :, None]) > 1
    uniq_fail = (far & (S * (100 - u) < S1[:, :, None] * 100)).any(axis=2)
    lr_fail = np.zeros((h, w), bool)
    if lr >= 0:
        dR = right_view(S, d0)
        yy, xx = np.mgrid[0:h, 0:w]
        xr = xx - (d0 + ds)
        inside = (xr >= 0) & (xr < w)
        r = dR[yy, np.clip(xr, 0, w - 1)]
        lr_fail = ~inside | (r < 0) | (np.abs(r - ds) > lr)
    frac = np.zeros((h, w), np.int64)                                         # step 7
    inner = (ds > 0) & (ds < D - 1)
    yy, xx = np.nonzero(inner)
    a, b, c = S[yy, xx, ds[yy, xx] - 1], S[yy, xx, ds[yy, xx]], S[yy, xx, ds[yy, xx] + 1]
    assert (a > b).all()
    den = a + c - 2 * b
    f = np.where(den > 0, (16 * (a - c) + den) // np.maximum(2 * den, 1), 0)  # // floors
    assert f.size == 0 or (f.min() >= -8 and f.max() <= 8)
    frac[yy, xx] = f
    disp16 = 16 * (d0 + ds) + frac
    valid = ~uniq_fail & ~lr_fail
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
    lo, hi = int(disparity.min()), int(disparity.max())                      # step 10
    depth = (((disparity - lo) * 131070 + (hi - lo)) // (2 * (hi - lo))) if hi > lo else np.zeros_like(disparity)
    assert disparity.min() >= -32768 and disparity.max() <= 32767 and depth.min() >= 0 and depth.max() <= 65535
    return dict(dstar=ds, frac=frac, disp16=disp16, uniq_fail=uniq_fail, lr_fail=lr_fail, filled=filled,
                disparity=disparity.astype(np.int16), valid=valid.astype(np.uint8), depth=depth.astype(np.uint16))


def model(left, right, D=64, d0=0, P1=4, P2=48, u=5, lr=1):
    """[n,h,w,c] uint8 x 2 -> (disparity int16 [n,h,w], valid uint8 [n,h,w], depth uint16 [n,h,w]): image by image."""
    outs = [match_one(l, r, D, d0, P1, P2, u, lr) for l, r in zip(left, right)]
    return tuple(np.stack([o[k] for o in outs]) for k in ("disparity", "valid", "depth"))


def depth_rule(disparity):
    """Step 10 alone, for one image."""
    v = np.asarray(disparity).astype(np.int64)
    lo, hi = int(v.min()), int(v.max())
    return ((((v - lo) * 131070 + (hi - lo)) // (2 * (hi - lo))) if hi > lo else np.zeros_like(v)).astype(np.uint16)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
INPUTS = ("planes", "ramp", "noise", "flat", "stripes")
PLANES_BG, PLANES_FG = 2, 9                                                   # the disparities of the two planes
STRIPES_PERIOD = 8


def planes_rect(h, w):
    """(y0, y1, x0, x1) of the near rectangle of `planes` in the LEFT image: 20 x 40 in the 40 x 120 case."""
    return h // 4, h // 4 + (h + 1) // 2, w // 3, w // 3 + (w + 2) // 3


def _seed(name, shape, c):
    return [INPUTS.index(name)] + list(shape) + [c]


@functools.lru_cache(maxsize=None)
def _pair(name, shape, c):
    n, h, w = shape
    rng = np.random.default_rng(_seed(name, shape, c))
    if name == "planes":
        # a background plane at disparity 2 and a rectangle at 9, each with its own noise texture: left column x shows the background
        # point the right image shows at x - 2, and the rectangle stands 9 columns further left in the right image
        pad = 16
        bg = rng.integers(0, 256, (n, h, w + 2 * pad, c), dtype=np.uint8)
        y0, y1, x0, x1 = planes_rect(h, w)
        fg = rng.integers(0, 256, (n, y1 - y0, x1 - x0, c), dtype=np.uint8)
        left = bg[:, :, pad:pad + w].copy()
        right = bg[:, :, pad + PLANES_BG:pad + PLANES_BG + w].copy()
        left[:, y0:y1, x0:x1] = fg
        a, b = max(x0 - PLANES_FG, 0), max(x1 - PLANES_FG, 0)
        right[:, y0:y1, a:b] = fg[:, :, a - (x0 - PLANES_FG):b - (x0 - PLANES_FG)]
    elif name == "ramp":
        # a slanted plane: the right image is the left one resampled at a disparity that grows along the row from 1 to about 7
        left = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
        xr = np.arange(w)
        src = np.clip(xr + 1 + (6 * xr) // max(w - 1, 1), 0, w - 1)
        right = left[:, :, src]
    elif name == "noise":
        left = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
        right = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    elif name == "flat":
        left = np.full((n, h, w, c), 100, np.uint8)
        right = np.full((n, h, w, c), 100, np.uint8)
    elif name == "stripes":
        # one random row of STRIPES_PERIOD columns repeated along the row and down the image, under a little noise of each view's own:
        # every disparity that is a multiple of the period matches about as well as 0, and no cost is exactly 0
        tile = rng.integers(0, 256, (n, 1, STRIPES_PERIOD, c), dtype=np.int64)
        base = np.tile(tile, (1, h, -(-w // STRIPES_PERIOD), 1))[:, :, :w]
        left = np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8)
        right = np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8)
    else:
        raise KeyError(name)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


def pair(name, shape, c=3):
    """(left, right) uint8 [n,h,w,c], read-only, seeded by name, shape and c."""
    return _pair(name, tuple(shape), c)


@functools.lru_cache(maxsize=None)
def _want(name, shape, c, params):
    outs = model(*pair(name, shape, c), *params)
    for o in outs:
        o.setflags(write=False)
    return outs


def want(name, shape, c=3, params=None):
    """The model's (disparity, valid, depth) of a named pair; params = (D, d0, P1, P2, u, lr).  Computed once, read-only."""
    return _want(name, tuple(shape), c, tuple(params if params is not None else DEFAULTS.values()))


def census(left, right, D=64, d0=0, P1=4, P2=48, u=5, lr=1):
    """What a case (one pair [h,w,c]) contains, counted on the model: invalid pixels by cause, filled pixels, pixels the median changed,
    pixels with a sub-pixel part."""
    o = match_one(left, right, D, d0, P1, P2, u, lr)
    return dict(uniqueness=int(o["uniq_fail"].sum()), left_right=int(o["lr_fail"].sum()), filled=int((o["valid"] == 0).sum()),
                median=int((o["disparity"] != o["filled"]).sum()), frac=int((o["frac"] != 0).sum()))


# ---- shapes and parameters ------------------------------------------------------------------------------------------------------------
# n x h x w: one pixel; w < D; heights 1 and 5 in a batch of 3; widths and heights below, across and above what a workgroup of the path
# kernels owns (4 rows or columns, 8 at D = 32) and a 256-thread row of the winner kernel; one column, where only vertical paths move
SMALL_SHAPES = [(1, 1, 1), (1, 7, 20), (3, 1, 67), (3, 5, 67), (2, 9, 130), (1, 33, 257), (1, 5, 1)]
# (D, d0, P1, P2, u, lr, c), pruned from the product: every value of every parameter occurs at D = 128 (the first five rows), and the
# other two D see the defaults and the extremes
SMALL_PARAMS = [
    (128, 0, 4, 48, 5, 1, 3),
    (128, -7, 1, 1, 0, -1, 1),
    (128, 5, 64, 255, 25, 0, 4),
    (128, -7, 4, 48, 50, 3, 3),
    (128, 5, 1, 1, 5, 1, 1),
    (64, 0, 4, 48, 5, 1, 3),
    (64, -7, 64, 255, 0, -1, 4),
    (64, 5, 1, 1, 25, 0, 1),
    (32, 0, 4, 48, 5, 1, 1),
    (32, -7, 1, 1, 50, 3, 3),
    (32, 5, 64, 255, 25, 0, 4),
]
LARGE_CASES = [((1, 96, 300), (64, 0, 4, 48, 5, 1), 3), ((2, 40, 700), (128, -16, 4, 48, 5, 1), 3)]
PLANES_CASE = ((1, 40, 120), (32, -4, 4, 48, 5, 1))                          # the case the definition was tried on
