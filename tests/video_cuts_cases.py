"""NumPy models and seeded inputs of video mode's scene-cut path (include/depthstereo.h: ds_frame_luma_hist,
ds_temporal_smooth5_f32; src/video_mode.py: cut_scores, detect_cuts), written from the definitions, sharing no code with src/."""
import numpy as np


# ---- luma histogram, cut rule ---------------------------------------------------------------------------------------------------
def luma(frames):
    """Integer Y of uint8 frames [n,h,w] or [n,h,w,c]: c == 1 the sample, c == 3 / 4 (77 R + 150 G + 29 B + 128) >> 8."""
    f = np.asarray(frames)
    assert f.dtype == np.uint8
    if f.ndim == 3:
        return f.astype(np.int64)
    if f.shape[3] == 1:
        return f[..., 0].astype(np.int64)
    c = f.astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def hist_model(frames):
    y = luma(frames)
    return np.stack([np.bincount(y[i].reshape(-1), minlength=256) for i in range(y.shape[0])]).astype(np.int64).reshape(-1, 256)


def cut_scores_model(frames, bins=64):
    h = hist_model(frames)
    n = h.shape[0]
    npix = int(np.asarray(frames).shape[1]) * int(np.asarray(frames).shape[2])
    score = np.zeros(n, dtype=np.float64)
    for t in range(1, n):
        s = 0
        for b in range(bins):
            k = 256 // bins
            s += abs(int(h[t, b * k:(b + 1) * k].sum()) - int(h[t - 1, b * k:(b + 1) * k].sum()))
        score[t] = np.float64(s) / np.float64(2 * npix)
    return score


def detect_cuts_model(frames, threshold=0.4, min_len=1, bins=64):
    score = cut_scores_model(frames, bins)
    n, prev, cuts = len(score), 0, []
    for t in range(1, n):
        if score[t] > threshold and t - prev >= min_len and n - t >= min_len:
            cuts.append(t)
            prev = t
    return cuts


def scene(rng, n, h, w, c, mean, spread):
    """n frames of one synthetic scene: a fixed random picture around `mean` plus a little per-frame noise."""
    shape = (h, w) if c == 0 else (h, w, c)
    base = rng.normal(mean, spread, shape)
    frames = [np.clip(np.rint(base + rng.normal(0.0, 2.0, shape)), 0, 255).astype(np.uint8) for _ in range(n)]
    return np.stack(frames) if n else np.zeros((0,) + shape, dtype=np.uint8)


def clip_of(seed, lengths, means, h=16, w=24, c=3, spread=12.0):
    """Scenes of `lengths` frames around the grey levels `means`, concatenated.  c == 0: [F,h,w] without a channel axis."""
    rng = np.random.default_rng(seed)
    return np.concatenate([scene(rng, n, h, w, c, m, spread) for n, m in zip(lengths, means)])


# ---- temporal filter --------------------------------------------------------------------------------------------------------------
TAPS = [np.float32(0.10), np.float32(0.20), np.float32(0.40), np.float32(0.20), np.float32(0.10)]


def smooth5_model(src, first, count, lo, hi):
    """out[j] = ((((+0 + W0 src[k0]) + W1 src[k1]) + W2 src[k2]) + W3 src[k3]) + W4 src[k4], k_u = clamp(first + j + u - 2, lo, hi):
    every product and every sum a separate float32 operation (NumPy's float32 arrays do exactly that)."""
    src = np.asarray(src, dtype=np.float32)
    out = np.zeros((count,) + src.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(count):
            f = np.zeros(src.shape[1:], dtype=np.float32)
            for u in range(5):
                k = min(max(first + j + u - 2, lo), hi)
                f = f + TAPS[u] * src[k]
            out[j] = f
    return out


def smooth_input(m, plane, seed):
    """float32 [m, plane]: normal values, and -- where the plane has room -- columns of specials that never meet a special of the other
    sign (inf - inf would make a NaN, whose bits the definition leaves open): -0.0 in every frame of column 0; values near 1e-38
    (products with 0.1 / 0.2 / 0.4 are subnormal) in column 1; +inf in one frame of column 2, -inf in one frame of column 3."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (m, plane)).astype(np.float32)
    x[:, 0] = np.float32(-0.0)
    if plane > 1:
        x[:, 1] = (rng.uniform(1.0, 4.0, m) * 1e-38).astype(np.float32) * np.where(rng.integers(0, 2, m) == 0, -1, 1).astype(np.float32)
    if plane > 3:
        x[m // 2, 2] = np.float32(np.inf)
        x[m // 3, 3] = np.float32(-np.inf)
    return x


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
