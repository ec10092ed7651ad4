"""Shared by tests/test_sparse_bilateral_cpu.py, tests/test_gpu_sparse_bilateral.py and tests/golden/make_golden_sparse_bilateral.py:
the NumPy MODEL of the 3D-photo depth preparation (include/depthstereo.h: ds_sparse_bilateral_f32 holds the definition) and the seeded
inputs of the golden cases.  The golden file holds only what the reference's sparse_bilateral_filtering returned for these inputs.

The model is written from the definition alone: the jump map by slicing, the clamp rule as an index table, the selection as a sort of
the window's valid taps.  It shares no code with the product (its rank table is built here a second time) and no structure with the
kernel (which never sorts)."""
import functools

import numpy as np

THRESHOLD = 0.04
SIGMAS = {'sigma_s': 4.0, 'sigma_r': 0.5}                 # read by the reference, never used on the branch it takes
ODD_RANKS_TO_49 = (20, 22, 28, 36, 40, 44, 48)            # where rank[n] != n // 2 for n <= 49


@functools.lru_cache(maxsize=None)
def rank_table(nmax=225):
    """rank[n] for n equally weighted taps: the reference's normalise / cumsum / digitize on float32 ones."""
    rank = np.zeros(nmax + 1, np.int64)
    for n in range(1, nmax + 1):
        c = np.ones(n, np.float32)
        rank[n] = np.digitize(0.5, np.cumsum(c / c.sum()))
    rank.setflags(write=False)
    return rank


def jump_map(v, t=THRESHOLD):
    """J of a float32 map [h, w] as bool [h, w]."""
    v = np.asarray(v)
    assert v.dtype == np.float32 and v.ndim == 2
    t = np.float32(t)
    with np.errstate(divide='ignore', invalid='ignore'):
        disp = np.float32(1) / v
        mid = disp[1:-1, 1:-1]
        over = np.zeros(mid.shape, bool)
        for nb in (disp[:-2, 1:-1], disp[2:, 1:-1], disp[1:-1, :-2], disp[1:-1, 2:]):
            over |= np.abs(mid - nb) > t
    j = np.zeros(v.shape, bool)
    j[1:-1, 1:-1] = over
    return j


def filter_pass(v, v0, window, t=THRESHOLD, census=None):
    """One pass: (out float32 [h, w], J bool [h, w]).  census: a set that receives every n met by a window with a discontinuity."""
    v, v0 = np.asarray(v), np.asarray(v0)
    assert v.dtype == np.float32 and v0.dtype == np.float32 and v.shape == v0.shape and v.ndim == 2
    h, w = v.shape
    assert h >= 3 and w >= 3 and window % 2 == 1 and 1 <= window <= 15
    m = window // 2
    rank = rank_table()
    j = jump_map(v, t)
    d = j | (v0 == 0)
    ys = np.clip(np.arange(-m, h + m), 1, h - 2)                             # row of the tap at padded index i
    xs = np.clip(np.arange(-m, w + m), 1, w - 2)
    vp, dp = v[np.ix_(ys, xs)], d[np.ix_(ys, xs)]
    out = vp[m:m + h, m:m + w].copy()                                        # the centre taps
    for y in range(h):
        for x in range(w):
            dwin = dp[y:y + window, x:x + window]
            if not dwin.any():
                continue
            valid = np.sort(vp[y:y + window, x:x + window][~dwin])
            if census is not None:
                census.add(valid.size)
            if valid.size:
                out[y, x] = valid[rank[valid.size]]
    return out, j


def model(depth, image, windows, t=THRESHOLD, census=None):
    """The driver: (save_images, save_depths) as the reference returns them, for the window list `windows` (one entry per pass)."""
    depth, image = np.asarray(depth), np.asarray(image)
    images, depths = [], []
    v = depth.copy()
    for i, window in enumerate(windows):
        depths.append(v)
        if i + 1 < len(windows):
            v, j = filter_pass(v, depth, window, t, census)
        else:
            j = jump_map(v, t)                                               # the last pass's output is never returned
        img = image.copy()
        img[j] = 0
        images.append(img)
    return images, depths


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _image(rng, h, w):
    return rng.integers(1, 256, (h, w, 3), dtype=np.uint8)                   # no zero: a blackened pixel is told from an untouched one


def steps_noise(h, w, seed, amplitude=0.03):
    """A full-height disparity step at w // 2, a raised rectangle in the middle third, uniform noise of +-amplitude; as depth."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    disp = 0.30 + 0.25 * (x >= w // 2) + 0.20 * ((y >= h // 3) & (y < 2 * h // 3) & (x >= w // 3) & (x < 2 * w // 3))
    disp = disp + rng.uniform(-amplitude, amplitude, (h, w))
    return (1.0 / disp).astype(np.float32)


def white_noise(h, w, seed):
    return np.random.default_rng(seed).uniform(0.5, 8.0, (h, w)).astype(np.float32)


def tied_zeros(h, w, seed):
    """Four depth levels only (every window holds ties) and three zero depths, one of them on the ring."""
    rng = np.random.default_rng(seed)
    d = rng.choice(np.array([1.0, 1.25, 2.0, 4.0], np.float32), (h, w))
    d[4, 5] = d[5, 5] = d[0, 9] = 0.0
    return d


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (depth float32 [h, w], image uint8 [h, w, 3], config, num_iter)}; the arrays are read-only."""
    rng = np.random.default_rng(77)
    out = {}

    def add(name, depth, filter_size, num_iter=None):
        h, w = depth.shape
        config = dict(SIGMAS, depth_threshold=THRESHOLD, filter_size=filter_size)
        image = _image(rng, h, w)
        depth.setflags(write=False)
        image.setflags(write=False)
        out[name] = (depth, image, config, len(filter_size) if num_iter is None else num_iter)
    add('3x3', white_noise(3, 3, 1), [7, 5, 3])
    add('4x5', white_noise(4, 5, 2), [7, 5, 3])
    add('9x11_noise', white_noise(9, 11, 3), [5, 3, 7])
    add('12x17_ties_zeros', tied_zeros(12, 17, 4), [7, 5])
    add('33x70_steps', steps_noise(33, 70, 5), [7, 7, 5, 5, 5])
    add('40x70_wide', steps_noise(40, 70, 6, amplitude=0.022), [15, 11, 9, 3])
    add('10x13_scalar', steps_noise(10, 13, 7), 5, num_iter=3)
    add('8x9_fewer_passes', steps_noise(8, 9, 8), [3, 7, 5, 5], num_iter=2)
    return out


def windows_of(config, num_iter):
    fs = config['filter_size']
    return [fs[i] if isinstance(fs, list) else fs for i in range(num_iter)]


def census_of_all_cases():
    """Every n met by a window with a discontinuity, over all cases and passes."""
    seen = set()
    for depth, image, config, num_iter in cases().values():
        model(depth, image, windows_of(config, num_iter), config['depth_threshold'], seen)
    return seen


def census_is_complete(seen):
    rank = rank_table()
    return (set(ODD_RANKS_TO_49) | {0}) <= seen and any(n > 49 and rank[n] != n // 2 for n in seen)
