"""Video mode of the funnel, frame parallel.

Reference: src/video_mode.py -- process_predicitons :103-128, gen_video :131-190 (first pass: raw predictions of all
frames; global normalisation; second pass: the funnel again with the normalised predictions as custom depth maps).

What is built: the COMPUTE of video mode on frame tensors --
  * ``process_predicitons`` (same name, same semantics, numpy in / numpy out) and
  * ``process_predictions_sharded``: the same normalisation when the frames are sharded over ranks (one process per
    GPU): 'none' needs the global min/max -> ONE all-reduce(MIN) of the pair (min, -max); 'experimental' needs
    +-2 frames of halo at the shard edges (an all-gather of every shard's first / last two frames) and the global
    0.5 / 99.5 percentiles, found
    EXACTLY by bisection on the float32 bit pattern with one all-reduce(SUM) of a counter per step (numpy's linear
    interpolation between the two neighbouring order statistics reproduced) -- no rank ever holds all frames;
  * ``gen_frames_sharded``: two passes over this rank's contiguous block of frames (network batched on the device,
    normalisation with the collectives above, depth -> uint16 -> stereo on the device) and a single gather of the
    collated output to rank 0 (src/multigpu.gather_units; RCCL over xGMI under the 'nccl' backend);
  * scene cuts, the reference's TODO at :114 ("Detect cuts and process segments separately"): ``cut_scores`` / ``detect_cuts``
    compare the luma histograms of neighbouring frames (csrc/ds_video.hip on the device, torch.bincount on the host, sharded: one
    all-gather of 1 KB per frame), and ``cuts=`` on the three functions above normalises every scene as the reference normalises a
    clip.  The 5-tap filter of float32 device frames is a kernel of the same file (DS_VIDEO_SMOOTH=0: torch passes);
  * ``stabilize_depth`` / ``stabilize_depth_sharded`` / ``gen_frames_sharded(stabilize=)``: a motion-adaptive temporal filter of the
    uint16 depth guided by the frames (not in the reference; a third kernel of that file), off by default.
Container I/O (moviepy / imageio-ffmpeg / av: open_path_as_images :13-64, frames_to_video :67-100) is outside the hot
path and not built; callers hand in decoded frames.
"""
import numpy as np


def process_predicitons(predictions, smoothening='none', cuts=None):
    """Drop-in for the reference's process_predicitons (:103-128; the spelling is the reference's): a list of [H,W]
    arrays in, a list of normalised arrays out ('none': float32, global min/max; 'experimental': float64, the 0.5 / 99.5
    percentiles of the 5-tap temporally smoothed clip; anything else: returned unchanged).  The work is the same tensor
    code that runs frame-parallel (process_predictions_sharded) on the whole clip as one local shard -- on the GPU when
    one is visible; nothing here is specific to a device.
    cuts (not in the reference, which leaves it as a TODO at :114): frame indices at which a new scene starts, strictly
    increasing, in 1..F-1 (ValueError otherwise; detect_cuts makes such a list).  The result is then the reference's function
    applied to every scene on its own, concatenated.  None or []: the whole clip is one scene."""
    if cuts:
        _check_cuts(cuts, len(predictions))
    if smoothening not in ('none', 'experimental') or len(predictions) == 0:
        return predictions
    import torch
    stack = torch.from_numpy(np.stack([np.asarray(p, dtype=np.float32) for p in predictions]))
    if torch.cuda.is_available():
        stack = stack.cuda()
    out = process_predictions_sharded(stack, smoothening, group=_LOCAL, cuts=cuts).cpu().numpy()
    return [out[i] for i in range(out.shape[0])]


_LOCAL = object()          # group sentinel: treat `local` as the whole clip even inside an initialised process group


def _is_multi(group):
    """True when `group` names more than one rank.  The _LOCAL sentinel is never collective: callers that work on data one
    rank holds completely (process_predicitons, the funnel's per-image 'Outliers' clipping, Boost's rank-0 post-processing)
    must not issue collectives other ranks do not take part in."""
    if group is _LOCAL:
        return False
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1


# ---- sharded over ranks -------------------------------------------------------------------------------------------------------
def _f32_key(t):
    """Order-preserving map float32 -> int64 (sign-magnitude bit pattern -> two's-complement order)."""
    import torch
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7fffffff) - 1, i)


def _key_to_f32(k):
    k = int(k)
    bits = k if k >= 0 else ((-(k + 1)) | 0x80000000)
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def _kth_smallest(keys, k, group):
    """Exact k-th smallest (0-based) of the union of every rank's `keys` (int64 tensor): bisection on the value with one
    all-reduce of a count per step (33 steps for the float32 key range)."""
    import torch
    import torch.distributed as dist
    multi = _is_multi(group)
    lo, hi = -(1 << 31) - 1, (1 << 31)
    while hi - lo > 1:                                      # invariant: count(keys <= lo) <= k < count(keys <= hi)
        mid = (lo + hi) // 2
        c = (keys <= mid).sum().to(torch.int64).reshape(1)
        if multi:
            dist.all_reduce(c, op=dist.ReduceOp.SUM, group=group)
        if int(c.item()) > k:
            hi = mid
        else:
            lo = mid
    return hi


def _global_percentiles(local, qs, group):
    """np.percentile(all values of all ranks, qs) with numpy's default linear interpolation, float32 data.
    group=_LOCAL: the values of THIS rank only, no collective (even inside an initialised multi-rank process)."""
    import torch
    import torch.distributed as dist
    n = torch.tensor([local.numel()], dtype=torch.int64, device=local.device)
    if _is_multi(group):
        dist.all_reduce(n, op=dist.ReduceOp.SUM, group=group)
    n = int(n.item())
    keys = _f32_key(local.reshape(-1).float())
    out = []
    for q in qs:
        pos = (n - 1) * (q / 100.0)
        i0 = int(np.floor(pos))
        frac = pos - i0
        v0 = _key_to_f32(_kth_smallest(keys, i0, group))
        v1 = _key_to_f32(_kth_smallest(keys, min(i0 + 1, n - 1), group)) if frac > 0 else v0
        # numpy (>= 1.22, method='linear'; lib/_function_base_impl._lerp): the difference of the two order statistics is
        # taken in the dtype of the data (float32), the product with the float64 weight and the sum in float64, and from the
        # right end when the weight is >= 0.5
        d = np.float64(np.float32(v1) - np.float32(v0))
        v0, v1 = np.float64(v0), np.float64(v1)
        out.append(float(v1 - d * (1 - frac)) if frac >= 0.5 else float(v0 + d * frac))
    return out


def _scale_f64(x, a, b):
    """global_scaling(objs, a, b) of the reference (:104-111) with float64 percentiles: (x - a) / (b - a) in float64.  The divisor
    is handed to torch as a TENSOR: on the device a division by a host scalar is computed as a product with its reciprocal, which
    is off by one unit in the last place in a share of the pixels; tensor by tensor is a true IEEE division on either device."""
    import torch
    return (x.double() - a) / torch.tensor(b - a, dtype=torch.float64, device=x.device)


def _check_cuts(cuts, n_frames):
    """cuts: global frame indices, strictly increasing, each in 1..n_frames-1 (the first frame of a new scene)."""
    prev = 0
    for c in cuts:
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError("cuts must be integers, got %r" % (c,))
        if not prev < c <= n_frames - 1:
            raise ValueError("cuts must be strictly increasing frame indices in 1..%d, got %r" % (n_frames - 1, list(cuts)))
        prev = int(c)


def _shard_counts(n_local, device, group):
    """Frames per rank of the group (one all-gather; [n_local] without a group)."""
    import torch
    import torch.distributed as dist
    if not _is_multi(group):
        return [n_local]
    counts = [torch.zeros(1, dtype=torch.int64, device=device) for _ in range(dist.get_world_size(group))]
    dist.all_gather(counts, torch.tensor([n_local], dtype=torch.int64, device=device), group=group)
    return [int(c.item()) for c in counts]


def _segments(cuts, start, n_local, n_frames):
    """The scenes of a clip of n_frames frames cut at `cuts`, seen from the rank that holds frames start .. start + n_local - 1:
    a list of (g0, g1, ls, le) -- the scene is global frames [g0, g1), of which this rank holds local[ls:le] (ls == le: none)."""
    bounds = [0] + [int(c) for c in cuts] + [n_frames]
    out = []
    for g0, g1 in zip(bounds[:-1], bounds[1:]):
        ls = min(max(g0 - start, 0), n_local)
        le = min(max(g1 - start, ls), n_local)
        out.append((g0, g1, ls, le))
    return out


def _kernel_smooth():
    """DS_VIDEO_SMOOTH=0 sends float32 device frames through the torch passes too (the route CPU tensors always take)."""
    import os
    return os.environ.get('DS_VIDEO_SMOOTH', '1') != '0'


def process_predictions_sharded(local, smoothening='none', group=None, cuts=None):
    """The normalisation of process_predicitons for frames sharded in CONTIGUOUS blocks over the ranks.
    local: float32 tensor [n_local, H, W] (this rank's frames, any device).  Returns the normalised tensor (float64 for
    'experimental', like numpy's promotion with the float64 percentiles; float32 for 'none').
    cuts: GLOBAL frame indices at which a new scene starts (the same list on every rank; ValueError unless strictly increasing
    in 1..F-1); every scene is normalised on its own -- 'none': the per-scene pairs (min, -max) in ONE all-reduce(MIN) of an
    [S, 2] tensor; 'experimental': the taps of the temporal filter are clamped to the scene (its bounds in global indices,
    intersected with this rank's frames and halo), its percentiles are the scene's -- a scene may span several ranks, and ranks
    that hold no frame of it take part in its collectives with empty data.  None or []: the clip is one scene.
    The 5-tap filter of float32 device frames is ONE kernel launch per scene (_native.temporal_smooth5, csrc/ds_video.hip;
    DS_VIDEO_SMOOTH=0: the five torch passes that CPU tensors take); same bits either way."""
    import torch
    import torch.distributed as dist
    multi = _is_multi(group)               # the _LOCAL sentinel is handed on as it is: the percentile helpers honour it too
    cuts = list(cuts) if cuts is not None else []
    if smoothening not in ('none', 'experimental'):
        return local
    n_local = local.shape[0]
    counts = _shard_counts(n_local, local.device, group) if (cuts or smoothening == 'experimental') else None
    rank = dist.get_rank(group) if multi else 0
    world = dist.get_world_size(group) if multi else 1
    segs = None
    if cuts:
        _check_cuts(cuts, sum(counts))
        segs = _segments(cuts, sum(counts[:rank]), n_local, sum(counts))
    if smoothening == 'none' and not cuts:
        mm = torch.stack((local.min(), -local.max())) if local.numel() else torch.tensor([float('inf')] * 2, device=local.device)
        if multi:
            dist.all_reduce(mm, op=dist.ReduceOp.MIN, group=group)          # min and (negated) max in one collective
        mn, mx = mm[0], -mm[1]
        return (local - mn) / (mx - mn)
    if smoothening == 'none':
        mm = torch.full((len(segs), 2), float('inf'), dtype=local.dtype, device=local.device)
        for i, (_, _, ls, le) in enumerate(segs):
            if le > ls:
                mm[i, 0] = local[ls:le].min()
                mm[i, 1] = -local[ls:le].max()
        if multi:
            dist.all_reduce(mm, op=dist.ReduceOp.MIN, group=group)          # every scene's min and (negated) max in one collective
        out = torch.empty_like(local)
        for i, (_, _, ls, le) in enumerate(segs):
            if le > ls:
                mn, mx = mm[i, 0], -mm[i, 1]
                out[ls:le] = (local[ls:le] - mn) / (mx - mn)
        return out
    # halo: the two frames before and after this rank's block (the global first / last frame replicated: clip() of the
    # reference).  Every rank publishes its first and last (up to) two frames -- zero placeholders where it holds fewer,
    # so the collectives have one fixed shape even for empty shards -- and walks outwards over its neighbours until it
    # has two frames on each side (a neighbour may hold a single frame, or none).
    hw = tuple(local.shape[1:])
    if multi:
        k = min(n_local, 2)
        head = torch.zeros((2,) + hw, dtype=local.dtype, device=local.device)
        tail = torch.zeros((2,) + hw, dtype=local.dtype, device=local.device)
        if k:
            head[:k] = local[:k]                              # left aligned
            tail[2 - k:] = local[n_local - k:]                # right aligned
        heads = [torch.empty_like(head) for _ in range(world)]
        tails = [torch.empty_like(tail) for _ in range(world)]
        dist.all_gather(heads, head, group=group)
        dist.all_gather(tails, tail, group=group)
        before, after = [], []
        for r in range(rank - 1, -1, -1):
            c = min(counts[r], 2)
            before = [tails[r][2 - c + i] for i in range(c)] + before
            if len(before) >= 2:
                break
        for r in range(rank + 1, world):
            c = min(counts[r], 2)
            after = after + [heads[r][i] for i in range(c)]
            if len(after) >= 2:
                break
    else:
        before, after = [], []
    if n_local == 0:                                          # nothing to smooth here; still part of every collective below
        left = right = local.new_zeros((2,) + hw)
    else:
        before, after = before[-2:], after[:2]
        first = before[0] if before else local[0]             # exhausted the ranks on that side: the global first frame
        last = after[-1] if after else local[-1]
        left = torch.stack([first] * (2 - len(before)) + before)
        right = torch.stack(after + [last] * (2 - len(after)))
    kernel = local.is_cuda and local.dtype == torch.float32 and _kernel_smooth()
    if not cuts and not kernel:
        ext = torch.cat((left, local, right), dim=0)
        processed = torch.zeros_like(local)
        for u, mul in enumerate([0.10, 0.20, 0.40, 0.20, 0.10]):            # same order of accumulation as the reference
            processed += mul * ext[u:u + n_local]
        a, b = _global_percentiles(processed, [0.5, 99.5], group)
        return _scale_f64(local, a, b)
    # Per scene, or on the kernel route.  Every tap index is clamped to the scene, so one rank alone needs no halo at all (the
    # clamp is the reference's clip()); sharded, ext[0] is global frame start - 2, and a scene that starts at the clip's first
    # frame never reaches the replicated placeholders in front of it (likewise at the end).
    start, total = sum(counts[:rank]), sum(counts)
    if segs is None:
        segs = [(0, total, 0, n_local)]
    local = local.contiguous()
    ext, off = (torch.cat((left, local, right), dim=0), 2) if multi else (local, 0)
    m = ext.shape[0]
    processed = torch.empty_like(local)
    for g0, g1, ls, le in segs:
        if le == ls:
            continue
        lo, hi = max(g0 - start + off, 0), min(g1 - 1 - start + off, m - 1)
        if kernel:
            from . import _native
            _native.temporal_smooth5(ext, ls + off, le - ls, lo, hi, out=processed[ls:le])
            continue
        idx = torch.arange(ls + off, le + off, device=local.device)
        acc = torch.zeros_like(local[ls:le])
        for u, mul in enumerate([0.10, 0.20, 0.40, 0.20, 0.10]):            # same order of accumulation as the reference
            acc += mul * ext.index_select(0, (idx + (u - 2)).clamp(lo, hi))
        processed[ls:le] = acc
    out = torch.empty(local.shape, dtype=torch.float64, device=local.device)
    for g0, g1, ls, le in segs:                                             # every rank, also one without a frame of the scene
        a, b = _global_percentiles(processed[ls:le], [0.5, 99.5], group)
        if le > ls:
            out[ls:le] = _scale_f64(local[ls:le], a, b)
    return out


# ---- scene cuts -----------------------------------------------------------------------------------------------------------------
# The reference has no cut detector (:114 is a TODO); the rule below and the comment of ds_frame_luma_hist in include/depthstereo.h
# are the definition.  Everything is integer arithmetic up to one float64 division per frame, so the device route, the host route
# and a sharded run agree bit for bit and every rank derives the same cut list.
def _as_frames(frames_u8):
    import torch
    f = torch.from_numpy(np.ascontiguousarray(frames_u8)) if isinstance(frames_u8, np.ndarray) else frames_u8
    if not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() in (3, 4) and (f.dim() == 3 or f.shape[3] in (1, 3, 4))):
        raise ValueError("frames must be uint8 [F,H,W] or [F,H,W,C] with C in {1, 3, 4}, got %s %s"
                         % (getattr(f, "dtype", type(f)), tuple(getattr(f, "shape", ()))))
    return f


def _luma_hist(frames):
    """int64 [n, 256] on the frames' device: the pixels of every frame per integer luma Y (grey: the sample; RGB / RGBA:
    (77 R + 150 G + 29 B + 128) >> 8).  Device frames: the kernel; host frames: torch.bincount on the same Y."""
    import torch
    n = frames.shape[0]
    if n == 0:
        return torch.zeros((0, 256), dtype=torch.int64, device=frames.device)
    if frames.is_cuda:
        from . import _native
        return _native.frame_luma_hist(frames.contiguous()).to(torch.int64) & 0xffffffff
    rows = []
    for f in frames:                                                        # frame by frame: int64 copies of one frame, not of the clip
        if f.dim() == 2 or f.shape[2] == 1:
            y = f.reshape(-1).to(torch.int64)
        else:
            c = f.reshape(-1, f.shape[2]).to(torch.int64)
            y = (77 * c[:, 0] + 150 * c[:, 1] + 29 * c[:, 2] + 128) >> 8
        rows.append(torch.bincount(y, minlength=256))
    return torch.stack(rows)


def _cut_scores_local(local_frames, n_frames, bins, group):
    """cut_scores from this rank's contiguous block of frames (multigpu.shard_bounds): the [n_local, 256] tables are all-gathered
    as uint32 bits, 1 KB per frame, padded to the largest shard (empty shards take part), and every rank computes all scores."""
    import torch
    import torch.distributed as dist
    from . import multigpu
    if bins not in (2, 4, 8, 16, 32, 64, 128, 256):
        raise ValueError("bins must be a power of two in 2..256, got %r" % (bins,))
    table = _luma_hist(local_frames)
    if _is_multi(group):
        bounds = multigpu.shard_bounds(n_frames, dist.get_world_size(group))
        assert bounds[dist.get_rank(group)][1] - bounds[dist.get_rank(group)][0] == local_frames.shape[0]
        per = max(e - s for s, e in bounds)
        pad = torch.zeros((per, 256), dtype=torch.int32, device=table.device)
        pad[:table.shape[0]] = table.to(torch.int32)                        # the low 32 bits: a count of 2^31 or more wraps, and is masked back
        parts = [torch.empty_like(pad) for _ in bounds]
        dist.all_gather(parts, pad, group=group)
        table = torch.cat([p[:e - s] for p, (s, e) in zip(parts, bounds)]).to(torch.int64) & 0xffffffff
    hist = table.cpu().numpy()
    assert hist.shape == (n_frames, 256)
    npix = int(np.prod(local_frames.shape[1:3]))
    folded = hist.reshape(n_frames, bins, 256 // bins).sum(axis=2)          # neighbours summed: exact
    score = np.zeros(n_frames, dtype=np.float64)
    if n_frames > 1:
        score[1:] = np.abs(np.diff(folded, axis=0)).sum(axis=1).astype(np.float64) / np.float64(2 * npix)
    return score


def cut_scores(frames_u8, bins=64, group=None):
    """How much the luma histogram changes from frame t - 1 to frame t: float64 [F] in [0, 1], score[0] = 0.
    frames_u8: the whole clip, uint8 [F,H,W] or [F,H,W,C] (C = 1, 3 or 4; torch tensor on any device, or numpy).  The 256-bin
    histograms are folded to `bins` (a power of two in 2..256) by summing neighbours, S_t = sum_b |H_t[b] - H_{t-1}[b]| in int64,
    score[t] = S_t / (2 H W) as one float64 division.  With a process group each rank histograms its own block of frames
    (multigpu.my_shard) and the tables are all-gathered; every rank returns the same vector."""
    import torch.distributed as dist
    from . import multigpu
    frames = _as_frames(frames_u8)
    s, e = 0, frames.shape[0]
    if _is_multi(group):
        s, e = multigpu.my_shard(frames.shape[0], dist.get_rank(group), dist.get_world_size(group))
    return _cut_scores_local(frames[s:e], frames.shape[0], bins, group)


def _cuts_from_scores(score, threshold, min_len):
    cuts, prev, n = [], 0, len(score)
    for t in range(1, n):
        if score[t] > threshold and t - prev >= min_len and n - t >= min_len:
            cuts.append(t)
            prev = t
    return cuts


def detect_cuts(frames_u8, threshold=0.4, min_len=1, bins=64, group=None):
    """Scene cuts of a clip: the sorted list of the frames t in 1..F-1 (each the FIRST frame of a new scene), scanned upwards,
    with cut_scores(...)[t] > threshold that lie at least min_len frames after the previous cut (or the start) and at least
    min_len frames before the end of the clip.  The default threshold is a starting point, not a measured optimum."""
    return _cuts_from_scores(cut_scores(frames_u8, bins, group), threshold, min_len)


# ---- temporal depth filter ------------------------------------------------------------------------------------------------------
# Not in the reference: every frame is predicted on its own, and neither smoothening mode changes a frame relative to its neighbours
# ('experimental' only finds its two percentiles on smoothed frames), so the depth of a static wall moves from frame to frame by the
# network's noise and the stereo warp turns that into horizontal jitter.  The filter is a joint bilateral filter ALONG TIME of the
# uint16 depth guided by the frames; the comment of ds_temporal_joint_bilateral_u16 in include/depthstereo.h is the definition, the
# kernel is in csrc/ds_video.hip, and tests/video_stabilize_cases.py is its float64 NumPy model.
# params = (radius, sigma_color, sigma_time): radius 1..4 frames on each side; sigma_color in units of SUMMED 8-bit channel difference
# |dR| + |dG| + |dB| (0..765) of the same pixel in two frames; sigma_time in frames.  (2, 12.0, 1.5) is a mild setting, (4, 12.0, 2.5) a
# strong one: starting points, not measured optima.
def _stabilize_params(params, who):
    from . import _native
    try:
        return _native.stabilize_params(params)
    except ValueError as e:
        raise _native.DepthStereoError('%s: %s' % (who, e)) from None


def _stabilize_check(frames, depth, who):
    import torch
    from . import _native
    if not (torch.is_tensor(depth) and depth.dtype == torch.uint16 and depth.dim() == 3):
        raise _native.DepthStereoError('%s: depth must be uint16 [F,H,W] (the filter is defined on, and returns, uint16 levels), got %s %s'
                                       % (who, getattr(depth, 'dtype', type(depth)), tuple(getattr(depth, 'shape', ()))))
    if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] in (3, 4)):
        raise _native.DepthStereoError('%s: frames must be uint8 [F,H,W,3] or [F,H,W,4], got %s %s'
                                       % (who, getattr(frames, 'dtype', type(frames)), tuple(getattr(frames, 'shape', ()))))
    if tuple(frames.shape[:3]) != tuple(depth.shape) or frames.device != depth.device:
        raise _native.DepthStereoError('%s: frames %s on %s and depth %s on %s must agree in [F,H,W] and device'
                                       % (who, tuple(frames.shape), frames.device, tuple(depth.shape), depth.device))
    if depth.shape[1] == 0 or depth.shape[2] == 0:
        raise _native.DepthStereoError('%s: empty frames %s' % (who, tuple(depth.shape)))


def _stabilize_torch(depth, guide, radius, wt, wc, first, count, lo, hi):
    """ds_temporal_joint_bilateral_u16 as float64 torch ops on the tensors' device, operation for operation (the route CPU tensors take,
    and the torch side of tools/video_stabilize_ab.py): for every tap u in increasing order, over the output frames whose tap lies in
    lo..hi, one rounded product wt * wc[k], the product with the depth rounded, then the two sums; one tensor-by-tensor division,
    torch.round (half to even).  Same bits as the kernel."""
    import torch
    h, w = depth.shape[1:]
    num = torch.zeros((count, h, w), dtype=torch.float64, device=depth.device)
    den = torch.zeros((count, h, w), dtype=torch.float64, device=depth.device)
    rgb = guide[..., :3].to(torch.int16)
    for u in range(-radius, radius + 1):
        a, b = max(first, lo - u), min(first + count - 1, hi - u)            # the outputs i whose tap i + u lies in lo..hi
        if a > b:
            continue
        k = (rgb[a + u:b + u + 1] - rgb[a:b + 1]).abs().sum(dim=3, dtype=torch.int64)
        wgt = wt[abs(u)] * wc[k]
        num[a - first:b - first + 1] += wgt * depth[a + u:b + u + 1].to(torch.float64)
        den[a - first:b - first + 1] += wgt
    return torch.round(num / den).to(torch.uint16)


def stabilize_depth_sharded(local_frames, local_depth, params, group=None, cuts=None):
    """stabilize_depth for frames sharded in CONTIGUOUS blocks over the ranks (multigpu.my_shard): local_frames uint8 [n_local,H,W,3|4]
    and local_depth uint16 [n_local,H,W], torch tensors of one device -> uint16 [n_local,H,W], bit for bit the rows stabilize_depth
    gives on the gathered clip, for every split.
    Halo: every rank publishes its first and last min(n_local, radius) frames of BOTH tensors as bytes (the collectives have no 16-bit
    integers) in one fixed-shape buffer, zero placeholders where it holds fewer, so an empty shard takes part too (one all-gather of
    the counts, one of the buffer), and walks outwards over its neighbours until it has `radius` frames on each side or runs out of
    ranks.  A side that runs out simply ends: those taps lie outside the clip and are omitted, nothing is replicated.  cuts: GLOBAL
    frame indices, the same list on every rank; per scene the filter's lo / hi are the scene's bounds intersected with what this rank
    holds.  One launch per scene of which the rank holds a frame (CPU tensors: the float64 torch route)."""
    import torch
    import torch.distributed as dist
    radius, sigma_color, sigma_time = _stabilize_params(params, 'stabilize_depth_sharded')
    _stabilize_check(local_frames, local_depth, 'stabilize_depth_sharded')
    multi = _is_multi(group)
    cuts = list(cuts) if cuts is not None else []
    n_local = local_depth.shape[0]
    counts = _shard_counts(n_local, local_depth.device, group)
    rank = dist.get_rank(group) if multi else 0
    world = dist.get_world_size(group) if multi else 1
    start, total = sum(counts[:rank]), sum(counts)
    if cuts:
        _check_cuts(cuts, total)
    local_frames, local_depth = local_frames.contiguous(), local_depth.contiguous()
    before_f, before_d, after_f, after_d = [], [], [], []
    if multi:
        h, w, c = local_frames.shape[1:]
        fb, db = h * w * c, h * w * 2                                       # bytes of one frame and of its depth
        k = min(n_local, radius)
        halo = torch.zeros((2, radius, fb + db), dtype=torch.uint8, device=local_depth.device)      # [0]: head, [1]: tail
        if k:
            halo[0, :k, :fb] = local_frames[:k].reshape(k, fb)                                        # left aligned
            halo[0, :k, fb:] = local_depth[:k].view(torch.uint8).reshape(k, db)
            halo[1, radius - k:, :fb] = local_frames[n_local - k:].reshape(k, fb)                     # right aligned
            halo[1, radius - k:, fb:] = local_depth[n_local - k:].view(torch.uint8).reshape(k, db)
        halos = [torch.empty_like(halo) for _ in range(world)]
        dist.all_gather(halos, halo, group=group)
        got = 0
        for r in range(rank - 1, -1, -1):
            take = min(counts[r], radius, radius - got)
            if take:
                rows = halos[r][1, radius - take:]
                before_f.insert(0, rows[:, :fb].reshape(take, h, w, c))
                before_d.insert(0, rows[:, fb:].contiguous().view(torch.uint16).reshape(take, h, w))
                got += take
            if got >= radius:
                break
        got = 0
        for r in range(rank + 1, world):
            take = min(counts[r], radius, radius - got)
            if take:
                rows = halos[r][0, :take]
                after_f.append(rows[:, :fb].reshape(take, h, w, c))
                after_d.append(rows[:, fb:].contiguous().view(torch.uint16).reshape(take, h, w))
                got += take
            if got >= radius:
                break
    out = torch.empty_like(local_depth)
    if n_local == 0:
        return out
    if before_f or after_f:                                                # ext[0] is global frame start - off
        ext_f = torch.cat(before_f + [local_frames] + after_f).contiguous()
        ext_d = torch.cat(before_d + [local_depth] + after_d).contiguous()
    else:
        ext_f, ext_d = local_frames, local_depth
    off = sum(t.shape[0] for t in before_d)
    m = ext_d.shape[0]
    from . import _native
    wt, wc = _native.stabilize_tables_on(local_depth.device, radius, sigma_color, sigma_time)
    for g0, g1, ls, le in _segments(cuts, start, n_local, total):
        if le == ls:
            continue
        lo, hi = max(g0 - start + off, 0), min(g1 - 1 - start + off, m - 1)
        if local_depth.is_cuda:
            _native.temporal_joint_bilateral_u16(ext_d, ext_f, radius, wt, wc, ls + off, le - ls, lo, hi, out=out[ls:le])
        else:
            out[ls:le] = _stabilize_torch(ext_d, ext_f, radius, wt, wc, ls + off, le - ls, lo, hi)
    return out


def stabilize_depth(frames_u8, depth_u16, params, cuts=None):
    """The temporal depth filter on a whole clip held by one device: frames_u8 uint8 [F,H,W,3|4] and depth_u16 uint16 [F,H,W], both
    torch tensors (of one device) or both NumPy arrays -> uint16 [F,H,W] of the same kind.  params = (radius, sigma_color, sigma_time),
    see above.  cuts: frame indices at which a new scene starts (detect_cuts makes such a list); nothing is averaged across one, and
    a scene of one frame comes back unchanged.  Device tensors: ONE ds_temporal_joint_bilateral_u16 launch per scene; CPU tensors and
    arrays: the same loop in float64 torch ops, the same bits.  A bad tuple, dtype or shape raises DepthStereoError and bad cuts
    ValueError, before any launch."""
    import torch
    from . import _native
    _stabilize_params(params, 'stabilize_depth')
    as_numpy = isinstance(depth_u16, np.ndarray)
    if as_numpy != isinstance(frames_u8, np.ndarray):
        raise _native.DepthStereoError('stabilize_depth: frames and depth must both be torch tensors or both NumPy arrays, got %s and %s'
                                       % (type(frames_u8).__name__, type(depth_u16).__name__))
    if as_numpy:
        if depth_u16.dtype != np.uint16 or frames_u8.dtype != np.uint8:
            raise _native.DepthStereoError('stabilize_depth: frames must be uint8 and depth uint16, got %s and %s'
                                           % (frames_u8.dtype, depth_u16.dtype))
        frames_u8, depth_u16 = torch.from_numpy(np.ascontiguousarray(frames_u8)), torch.from_numpy(np.ascontiguousarray(depth_u16))
    _stabilize_check(frames_u8, depth_u16, 'stabilize_depth')
    if cuts:
        _check_cuts(cuts, depth_u16.shape[0])
    out = stabilize_depth_sharded(frames_u8, depth_u16, params, group=_LOCAL, cuts=cuts)
    return out.numpy() if as_numpy else out


def gen_frames_sharded(frames_u8, predict_batch, inp, smoothening='none', group=None, batch=8, dst=0, invert=False,
                       cuts=None, cut_threshold=0.4, cut_min_len=1, stabilize=None):
    """Two-pass video pipeline on decoded frames, frame parallel.
    stabilize: None -- nothing is added (no launch, no collective, no copy); (radius, sigma_color, sigma_time) -- the temporal depth
    filter (stabilize_depth_sharded) runs on the uint16 depth between the quantisation and the stereo warp, with the cuts of this call,
    and 'depth' in the result is the filtered map.  A bad tuple raises DepthStereoError before the first pass.
    cuts: None -- the clip is one scene; 'auto' -- detect_cuts(threshold=cut_threshold, min_len=cut_min_len) on the decoded frames,
    each rank on its own block; a list -- used as given.  With cuts the result on rank `dst` also has the key 'cuts' (the list).
    frames_u8: uint8 tensor [F, H, W, 3] (every rank may hold the full clip or just index its block); predict_batch:
    callable uint8 [b,H,W,3] -> float32 [b,H,W] raw prediction (e.g. DepthAnythingV2.infer_batch) on the rank's device.
    invert: True for the models whose raw output is near-is-dark (ids 0, 7-9, 10: depthmap_generation.py:402) -- the
    first pass of the reference yields 'depth_prediction' AFTER ``out *= -1`` (core.py:192-195), so the normalisation sees
    the negated predictions.  Returns on rank `dst` a dict {mode: uint8 [F, ...]} for the requested stereo modes plus
    'depth' (uint16 [F,H,W]); None elsewhere."""
    import torch
    import torch.distributed as dist
    from . import _native, multigpu
    from .stereoimage_generation import create_stereoimages_batch
    if stabilize is not None:
        stabilize = _stabilize_params(stabilize, 'gen_frames_sharded')
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank = dist.get_rank(group) if multi else 0
    world = dist.get_world_size(group) if multi else 1
    n = frames_u8.shape[0]
    s, e = multigpu.my_shard(n, rank, world)
    dev = torch.device('cuda', torch.cuda.current_device())
    mine = frames_u8[s:e].to(dev)
    preds = [predict_batch(mine[i:i + batch]) for i in range(0, e - s, batch)]                    # pass 1 (:139-150)
    preds = torch.cat(preds) if preds else torch.empty((0,) + tuple(frames_u8.shape[1:3]), device=dev)
    if invert:
        preds = preds * -1                                                                        # core.py:192-195
    if isinstance(cuts, str):
        if cuts != 'auto':
            raise ValueError("cuts must be None, 'auto' or a list of frame indices, got %r" % (cuts,))
        cuts = _cuts_from_scores(_cut_scores_local(mine, n, 64, group), cut_threshold, cut_min_len)
    elif cuts is not None:
        cuts = list(cuts)
    norm = process_predictions_sharded(preds, smoothening, group, cuts=cuts)                      # :151
    # second pass: the normalised frames re-enter the funnel as custom depth maps, np.asarray(dp, dtype='float') = float64
    # (core.py:170-174), and are quantised in float64 (:211) -- also in 'none' mode, whose frames are float32
    if e > s:
        d16 = _native.convert_to_i16(norm.double().contiguous())
    else:
        d16 = torch.empty((0,) + tuple(frames_u8.shape[1:3]), dtype=torch.uint16, device=dev)
    if stabilize is not None:                                                                     # every rank, also one without frames
        d16 = stabilize_depth_sharded(mine, d16, stabilize, group=group, cuts=cuts)
    modes = list(inp.get('stereo_modes', ['left-right']))
    outs = {'depth': d16}
    if inp.get('gen_stereo', True) and e > s:                                                     # pass 2 (:160)
        res = create_stereoimages_batch(mine, d16, inp.get('stereo_divergence', 2.5), inp.get('stereo_separation', 0.0), modes,
                                        inp.get('stereo_balance', 0.0), inp.get('stereo_offset_exponent', 1.0),
                                        inp.get('stereo_fill_algo', 'polylines_sharp'))
        outs.update(dict(zip(modes, res)))
    gathered = {}
    for k, v in outs.items():                                                                     # ONE gather per output
        if v.dtype == torch.uint16:                          # collectives have no uint16: same bits as int16
            g = multigpu.gather_units(v.view(torch.int16), n, group=group, dst=dst)
            gathered[k] = None if g is None else g.view(torch.uint16)
        else:
            gathered[k] = multigpu.gather_units(v, n, group=group, dst=dst)
    if cuts is not None:
        gathered['cuts'] = cuts
    return gathered if rank == dst else None
