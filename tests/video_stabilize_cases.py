"""Shared by tests/test_video_stabilize_cpu.py, tests/test_video_stabilize_gloo.py and tests/test_gpu_video_stabilize.py: the float64
NumPy MODEL of video mode's temporal depth filter (the joint bilateral filter along time of uint16 depth frames guided by the uint8
frames; the definition is in include/depthstereo.h, ds_temporal_joint_bilateral_u16) and the seeded inputs the three files use.  The
model is a plain loop over the output frames and their taps, vectorised over the pixels of a frame: per pixel it performs the
operations of the definition in the definition's order (one rounded multiply for the weight, the product rounded and then the sum
rounded, one IEEE division, np.rint), so the kernel and the host route must reproduce it bit for bit.  It is written from the
definition alone and shares no code with the product's table builder."""
import numpy as np


def tables(radius, sigma_color, sigma_time):
    wt = np.exp(-(np.arange(radius + 1, dtype=np.float64)**2) / (2.0 * sigma_time**2))
    wc = np.exp(-(np.arange(766, dtype=np.float64)**2) / (2.0 * sigma_color**2))
    return wt, wc


def model_range(depth, guide, params, first, count, lo, hi):
    """depth uint16 [m,h,w], guide uint8 [m,h,w,c] (channels 0..2 are read), params = (radius, sigma_color, sigma_time) ->
    uint16 [count,h,w]: frames first .. first + count - 1 filtered, taps outside lo..hi omitted."""
    depth, guide = np.asarray(depth), np.asarray(guide)
    assert depth.dtype == np.uint16 and guide.dtype == np.uint8 and guide.shape[:3] == depth.shape and guide.shape[3] >= 3
    radius, sigma_color, sigma_time = params
    m = depth.shape[0]
    assert 0 <= lo <= first and first + count - 1 <= hi < m and count > 0
    wt, wc = tables(radius, sigma_color, sigma_time)
    assert wt[0] == 1.0 and wc[0] == 1.0
    rgb = guide[..., :3].astype(np.int64)
    out = np.empty((count,) + depth.shape[1:], np.uint16)
    for j in range(count):
        i = first + j
        num = np.zeros(depth.shape[1:], np.float64)
        den = np.zeros(depth.shape[1:], np.float64)
        for u in range(-radius, radius + 1):
            s = i + u
            if s < lo or s > hi:
                continue
            k = np.abs(rgb[s] - rgb[i]).sum(axis=2)
            wgt = wt[abs(u)] * wc[k]
            num = num + wgt * depth[s].astype(np.float64)
            den = den + wgt
        assert (den >= 1.0).all()
        out[j] = np.rint(num / den).astype(np.uint16)
    return out


def model(depth, guide, params, cuts=None):
    """The whole clip, scene by scene: cuts are the first frames of new scenes."""
    bounds = [0] + [int(c) for c in (cuts or [])] + [depth.shape[0]]
    return np.concatenate([model_range(depth, guide, params, g0, g1 - g0, g0, g1 - 1) for g0, g1 in zip(bounds[:-1], bounds[1:])])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def noise_clip(m, h, w, c, seed):
    """Full-range white noise in both tensors: every tap matters, k is all over 0..765, every index mistake shows."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (m, h, w, c), dtype=np.uint8), rng.integers(0, 65536, (m, h, w), dtype=np.uint16)


def static_clip(m, h, w, c, seed, noise=3):
    """One image with +-noise levels of noise per channel and frame (small k: the weights that matter in use), depth a ramp plus
    +-200 levels per pixel and frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 236, (1, h, w, c))
    frames = (base + rng.integers(-noise, noise + 1, (m, h, w, c))).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    depth = (30000 + 90 * x + 40 * y + rng.integers(-200, 201, (m, h, w))).astype(np.uint16)
    return frames, depth


def extreme_clip(m=6, h=4, w=6, seed=5):
    """Depth values 0 and 65535 only, guide pixels (0,0,0) and (255,255,255) only: k is 0 or 765, the sums hold 65535 * den."""
    rng = np.random.default_rng(seed)
    frames = np.repeat((rng.integers(0, 2, (m, h, w, 1)) * 255).astype(np.uint8), 3, axis=3)
    depth = (rng.integers(0, 2, (m, h, w)) * 65535).astype(np.uint16)
    frames[:, 0, 0] = 255                                   # one pixel static and white, with both depth extremes along time
    depth[:, 0, 0] = [0, 65535] * (m // 2) + [0] * (m % 2)
    return frames, depth


FLICKER = dict(m=12, h=24, w=40, bar_rows=(8, 16), bar_width=3, bar_step=3)


def flicker_clip(seed=10):
    """12 frames of 24 x 40: a fixed random RGB background, a bar on rows 8..15, 3 columns wide, moving 3 columns per frame, of colour
    255 - bg // 2; depth is the ramp 20000 + 100 x + 50 y plus a per-frame offset drawn from +-300.  |255 - b // 2 - b| vanishes at
    b = 170, so the bar's summed colour difference from the background depends on the seed: on this one it is at least 54 (asserted
    below), which at sigma_color = 10 is a weight below 5e-7.  Returns (frames uint8 [12,24,40,3], depth uint16 [12,24,40], bar: bool
    [12,24,40], True where the bar is in that frame)."""
    rng = np.random.default_rng(seed)
    m, h, w = FLICKER['m'], FLICKER['h'], FLICKER['w']
    bg = rng.integers(0, 256, (h, w, 3))
    frames = np.broadcast_to(bg, (m, h, w, 3)).copy()
    bar = np.zeros((m, h, w), bool)
    r0, r1 = FLICKER['bar_rows']
    for f in range(m):
        x0 = FLICKER['bar_step'] * f
        bar[f, r0:r1, x0:x0 + FLICKER['bar_width']] = True
        frames[f, r0:r1, x0:x0 + FLICKER['bar_width']] = 255 - bg[r0:r1, x0:x0 + FLICKER['bar_width']] // 2
    frames = frames.astype(np.uint8)
    assert np.abs(frames[bar].astype(np.int64) - np.broadcast_to(bg, (m, h, w, 3))[bar]).sum(axis=1).min() >= 54
    y, x = np.mgrid[0:h, 0:w]
    offs = rng.integers(-300, 301, m)
    depth = (20000 + 100 * x + 50 * y + offs[:, None, None]).astype(np.uint16)
    return frames, depth, bar


def static_rows():
    r0, r1 = FLICKER['bar_rows']
    return np.r_[0:r0, r1:FLICKER['h']]


def temporal_std(depth, rows):
    """The mean over the pixels of `rows` of the standard deviation along time."""
    return float(np.asarray(depth)[:, rows].astype(np.float64).std(axis=0).mean())
