"""Video mode's two kernels (include/depthstereo.h: ds_frame_luma_hist, ds_temporal_smooth5_f32; csrc/ds_video.hip) and the scene-cut
path on the device.  The histogram is compared with np.bincount on the integer luma by integer equality, the temporal filter with its
float32 NumPy model on the BIT PATTERNS (tests/video_cuts_cases.py), the normalisation with the reference's own function run scene by
scene (tests/golden/video_cuts_cases.npz): nothing here has a tolerance, the definitions fix every rounding."""
import os

import numpy as np
import pytest

import conftest
import make_golden_video_cuts as mgc
import video_cuts_cases as vc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(conftest.ROOT, "tests", "golden")
# (n, h, w, c); c == 0: [n,h,w] without a channel axis.  (2, 300, 301, 3) has more than one workgroup per frame.
HIST_SHAPES = [(1, 1, 1, 3), (3, 7, 13, 3), (2, 5, 9, 4), (2, 4, 6, 1), (2, 4, 6, 0), (2, 33, 65, 3), (2, 300, 301, 3)]


def _counts(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _hist_inputs(n, h, w, c, seed):
    shape = (n, h, w) if c == 0 else (n, h, w, c)
    rng = np.random.default_rng(seed)
    one = np.empty(shape, dtype=np.uint8)
    one[...] = 93 if c in (0, 1) else np.array([10, 200, 30, 7][:c], dtype=np.uint8)
    smooth = np.clip(rng.normal(120, 3, shape), 0, 255).astype(np.uint8)          # a few neighbouring bins: contended, not uniform
    return [("random", rng.integers(0, 256, shape, dtype=np.uint8)), ("zeros", np.zeros(shape, dtype=np.uint8)),
            ("all255", np.full(shape, 255, dtype=np.uint8)), ("one-colour", one), ("smooth", smooth)]


@pytest.mark.parametrize("shape", HIST_SHAPES, ids=["x".join(map(str, s)) for s in HIST_SHAPES])
def test_histogram_kernel_equals_bincount(gpu, shape):
    torch = gpu
    from src import _native
    n, h, w, c = shape
    for name, f in _hist_inputs(n, h, w, c, seed=h * 1000 + w):
        want = vc.hist_model(f)
        assert want.sum() == n * h * w
        dev = torch.from_numpy(f).cuda()
        before = _native.CALLS["ds_frame_luma_hist"]
        got = _native.frame_luma_hist(dev)
        assert _native.CALLS["ds_frame_luma_hist"] == before + 1
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (n, 256)
        assert np.array_equal(_counts(got), want), (name, np.argwhere(_counts(got) != want)[:6].tolist())
        # the table is overwritten, not added to: garbage first, then twice into the same tensor
        out = torch.full((n, 256), 12345, dtype=torch.int32, device="cuda")
        assert _native.frame_luma_hist(dev, out=out) is out and np.array_equal(_counts(out), want), name
        _native.frame_luma_hist(dev, out=out)
        assert np.array_equal(_counts(out), want), name
        # a base pointer one byte off 16-byte alignment
        buf = torch.zeros(f.size + 32, dtype=torch.uint8, device="cuda")
        off = 1 + (-buf.data_ptr()) % 16
        view = buf[off:off + f.size]
        view.copy_(dev.reshape(-1))
        view = view.view(f.shape)
        assert view.data_ptr() % 16 == 1 and view.is_contiguous()
        assert np.array_equal(_counts(_native.frame_luma_hist(view)), want), name
        if n > 1:                     # frame 1 of the batch is that frame run alone
            assert np.array_equal(_counts(_native.frame_luma_hist(dev[1:2].contiguous()))[0], want[1]), name


def test_histogram_entry_point_rejects_bad_arguments(gpu):
    torch = gpu
    from src import _native
    L, ctx = _native.lib(), _native.ctx_for(torch.cuda.current_device())
    f = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    hist = torch.full((2 * 256 + 1,), 7, dtype=torch.int32, device="cuda")
    st = _native._stream(f)
    ok = (ctx, f.data_ptr(), 2, 4, 4, 3, hist.data_ptr(), st)
    bad = [(None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:6] + (None, st), ok[:2] + (0,) + ok[3:], ok[:3] + (0,) + ok[4:],
           ok[:4] + (-1,) + ok[5:], ok[:5] + (2,) + ok[6:], ok[:5] + (5,) + ok[6:], ok[:6] + (hist.data_ptr() + 2, st)]
    for args in bad:
        assert L.ds_frame_luma_hist(*args) == -1, args           # DS_EINVAL
    assert L.ds_frame_luma_hist(ctx, f.data_ptr(), 1, 65536, 65536, 1, hist.data_ptr(), st) == -2        # DS_EUNSUPPORTED: h * w = 2^32
    torch.cuda.synchronize()
    assert bool((hist == 7).all()), "a rejected call wrote to hist"
    with pytest.raises(_native.DepthStereoError):
        _native.frame_luma_hist(f.float())
    with pytest.raises(_native.DepthStereoError):
        _native.frame_luma_hist(f, out=torch.zeros((2, 256), dtype=torch.int64, device="cuda"))


# ---- temporal filter --------------------------------------------------------------------------------------------------------------
def _smooth_forms(count):
    """(m, first, lo, hi): the whole-clip form, and the halo form (first = 2, m = count + 4) with the clamp bounds at the halo's
    ends, one frame inside it, and exactly around the frames that are smoothed."""
    m = count + 4
    return [(count, 0, 0, count - 1), (m, 2, 0, m - 1), (m, 2, 1, m - 2), (m, 2, 2, m - 3), (m, 2, 0, m - 3), (m, 2, 2, m - 1)]


@pytest.mark.parametrize("plane", [1, 7, 126, 4099])
def test_filter_kernel_equals_the_float32_model_bit_for_bit(gpu, plane):
    torch = gpu
    from src import _native
    for count in range(1, 13):
        x = vc.smooth_input(count + 4, plane, seed=100 * plane + count)
        dev = torch.from_numpy(x).cuda()
        for m, first, lo, hi in _smooth_forms(count):
            before = _native.CALLS["ds_temporal_smooth5_f32"]
            got = _native.temporal_smooth5(dev[:m], first, count, lo, hi)
            assert _native.CALLS["ds_temporal_smooth5_f32"] == before + 1
            assert got.dtype == torch.float32 and tuple(got.shape) == (count, plane)
            want = vc.smooth5_model(x[:m], first, count, lo, hi)
            assert not np.isnan(want).any()
            g = vc.bits(got.cpu().numpy())
            assert np.array_equal(g, vc.bits(want)), (count, m, first, lo, hi, np.argwhere(g != vc.bits(want))[:6].tolist())
    # the inputs do what they are there for: +0 out of -0, infinities, subnormal products
    assert vc.bits(want[:, 0]).max() == 0
    if plane > 3:
        assert np.isposinf(want[:, 2]).any() and np.isneginf(want[:, 3]).any()
        tiny = np.abs(x[:, 1].astype(np.float64)) * 0.1
        assert (tiny < np.finfo(np.float32).tiny).any()


def test_filter_single_frame_scene_and_shapes_with_more_axes(gpu):
    """lo == hi: every tap reads the one frame.  A [m, h, w] tensor is [m, h * w]."""
    torch = gpu
    from src import _native
    x = vc.smooth_input(5, 35, seed=3)
    dev = torch.from_numpy(x).cuda()
    for k in range(5):
        got = _native.temporal_smooth5(dev, k, 1, k, k).cpu().numpy()
        assert np.array_equal(vc.bits(got), vc.bits(vc.smooth5_model(x, k, 1, k, k))), k
    got = _native.temporal_smooth5(dev.view(5, 5, 7), 1, 3, 0, 4)
    assert tuple(got.shape) == (3, 5, 7)
    assert np.array_equal(vc.bits(got.cpu().numpy().reshape(3, 35)), vc.bits(vc.smooth5_model(x, 1, 3, 0, 4)))


def test_filter_misaligned_base_and_out_slice(gpu):
    """src 4 bytes off 16-byte alignment with an odd plane (every frame at another alignment), out a slice of a larger tensor."""
    torch = gpu
    from src import _native
    m, plane = 9, 126 + 1
    x = vc.smooth_input(m, plane, seed=8)
    buf = torch.zeros(m * plane + 8, dtype=torch.float32, device="cuda")
    off = 1 + ((-buf.data_ptr()) % 16) // 4
    view = buf[off:off + m * plane]
    view.copy_(torch.from_numpy(x).cuda().reshape(-1))
    view = view.view(m, plane)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    big = torch.full((m + 2, plane), -7.0, dtype=torch.float32, device="cuda")
    ret = _native.temporal_smooth5(view, 2, 5, 1, 7, out=big[1:6])
    assert ret.data_ptr() == big[1:6].data_ptr()
    assert np.array_equal(vc.bits(big[1:6].cpu().numpy()), vc.bits(vc.smooth5_model(x, 2, 5, 1, 7)))
    assert bool((big[0] == -7.0).all()) and bool((big[6:] == -7.0).all()), "the kernel wrote outside out"


def test_filter_entry_point_rejects_bad_arguments(gpu):
    torch = gpu
    from src import _native
    L, ctx = _native.lib(), _native.ctx_for(torch.cuda.current_device())
    m, plane = 6, 10
    src = torch.zeros((m, plane), dtype=torch.float32, device="cuda")
    out = torch.full((m, plane), 3.0, dtype=torch.float32, device="cuda")
    st = _native._stream(src)

    def call(src_p=src.data_ptr(), m_=m, plane_=plane, first=1, count=3, lo=0, hi=5, out_p=out.data_ptr(), ctx_=ctx):
        return L.ds_temporal_smooth5_f32(ctx_, src_p, m_, plane_, first, count, lo, hi, out_p, st)
    bad = [dict(ctx_=None), dict(src_p=None), dict(out_p=None), dict(m_=0), dict(plane_=0), dict(plane_=-4), dict(count=0), dict(count=-1),
           dict(lo=-1), dict(lo=2), dict(hi=2), dict(hi=6), dict(first=4, count=3), dict(first=-1, lo=-1), dict(src_p=src.data_ptr() + 2),
           dict(out_p=out.data_ptr() + 1), dict(out_p=src.data_ptr() + 4 * plane), dict(out_p=src.data_ptr())]
    for kw in bad:
        assert call(**kw) == -1, kw                              # DS_EINVAL, before any launch
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), "a rejected call wrote to out"
    assert call() == 0
    with pytest.raises(_native.DepthStereoError):
        _native.temporal_smooth5(src.double(), 1, 3, 0, 5)
    with pytest.raises(_native.DepthStereoError):
        _native.temporal_smooth5(src, 1, 3, 0, 6)
    with pytest.raises(_native.DepthStereoError):
        _native.temporal_smooth5(src, 1, 3, 0, 5, out=out)        # the wrong shape


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "experimental"])
def test_scenes_on_the_device_equal_the_reference_scene_by_scene(gpu, mode):
    from src import _native, video_mode
    gold = np.load(os.path.join(GOLD, "video_cuts_cases.npz"))
    for case, cuts in sorted(mgc.CUTS.items()):
        preds = mgc.predictions(case)
        before = _native.CALLS["ds_temporal_smooth5_f32"]
        got = np.stack(video_mode.process_predicitons([x for x in preds], mode, cuts=cuts))
        launches = _native.CALLS["ds_temporal_smooth5_f32"] - before
        assert launches == (len(cuts) + 1 if mode == "experimental" else 0), (case, launches)       # one launch per scene
        want = gold[f"{case}/{mode}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), (case, np.argwhere(got != want)[:4].tolist())


def test_cutless_experimental_takes_the_kernel_and_the_switch_changes_no_bit(gpu, monkeypatch):
    torch = gpu
    import make_golden_video as mgv
    from src import _native, video_mode
    gold = np.load(os.path.join(GOLD, "video_cases.npz"))
    for spec in mgv.CASES:
        preds = mgv.make_predictions(*spec[1:])
        want = gold[f"{spec[0]}/experimental"]
        dev = torch.from_numpy(preds).cuda()
        monkeypatch.delenv("DS_VIDEO_SMOOTH", raising=False)
        before = _native.CALLS["ds_temporal_smooth5_f32"]
        on = video_mode.process_predictions_sharded(dev, "experimental", group=video_mode._LOCAL)
        assert _native.CALLS["ds_temporal_smooth5_f32"] == before + 1, spec[0]
        monkeypatch.setenv("DS_VIDEO_SMOOTH", "0")
        off = video_mode.process_predictions_sharded(dev, "experimental", group=video_mode._LOCAL)
        assert _native.CALLS["ds_temporal_smooth5_f32"] == before + 1, "DS_VIDEO_SMOOTH=0 still launched the kernel"
        assert on.dtype == torch.float64 and torch.equal(on, off), spec[0]
        assert np.array_equal(on.cpu().numpy(), want), spec[0]
        if spec[0] in mgc.CUTS:                                                       # the switch with cuts: the torch gather route
            off_c = video_mode.process_predictions_sharded(dev, "experimental", group=video_mode._LOCAL, cuts=mgc.CUTS[spec[0]])
            assert _native.CALLS["ds_temporal_smooth5_f32"] == before + 1
            assert np.array_equal(off_c.cpu().numpy(), np.load(os.path.join(GOLD, "video_cuts_cases.npz"))[f"{spec[0]}/experimental"])


def test_device_cut_detector_equals_the_model(gpu):
    torch = gpu
    from src import _native, video_mode
    for c in (0, 1, 3, 4):
        frames = vc.clip_of(50 + c, [3, 1, 4], [50, 220, 120], h=33, w=65, c=c)
        before = _native.CALLS["ds_frame_luma_hist"]
        score = video_mode.cut_scores(torch.from_numpy(frames).cuda())
        assert _native.CALLS["ds_frame_luma_hist"] == before + 1
        assert score.dtype == np.float64 and np.array_equal(score, vc.cut_scores_model(frames)), c
        assert np.array_equal(score, video_mode.cut_scores(frames)), "device and host routes disagree"
        assert video_mode.detect_cuts(torch.from_numpy(frames).cuda(), min_len=2) == vc.detect_cuts_model(frames, min_len=2) == [3]


@pytest.mark.parametrize("mode", ["none", "experimental"])
def test_gen_frames_sharded_detects_the_cut_and_normalises_each_scene(gpu, mode):
    """A 6-frame 16 x 24 clip of a dark and a bright scene through the two-pass pipeline with a stub network (exact in float32 on
    either device): cuts='auto' finds [3]; 'depth' is convert_to_i16 of the per-scene normalisation done on the host."""
    torch = gpu
    from src import _native, video_mode
    frames = torch.from_numpy(vc.clip_of(61, [3, 3], [40, 210], h=16, w=24, c=3))

    def predict(b):
        assert b.is_cuda and b.dtype == torch.uint8
        return b[..., 0].float() * 0.5 + b[..., 1].float() * 0.25 + b[..., 2].float()

    res = video_mode.gen_frames_sharded(frames, predict, {'gen_stereo': False}, mode, batch=4, cuts='auto')
    assert res['cuts'] == [3] and set(res.keys()) == {'depth', 'cuts'}
    host = video_mode.process_predictions_sharded(predict_host(frames), mode, group=video_mode._LOCAL, cuts=[3])
    assert not host.is_cuda
    want = _native.convert_to_i16(host.double().contiguous().cuda())
    assert res['depth'].dtype == torch.uint16 and torch.equal(res['depth'].view(torch.int16), want.view(torch.int16))
    given = video_mode.gen_frames_sharded(frames, predict, {'gen_stereo': False}, mode, batch=4, cuts=[3])
    assert given['cuts'] == [3] and torch.equal(given['depth'].view(torch.int16), want.view(torch.int16))
    plain = video_mode.gen_frames_sharded(frames, predict, {'gen_stereo': False}, mode, batch=4)
    assert set(plain.keys()) == {'depth'} and not torch.equal(plain['depth'].view(torch.int16), want.view(torch.int16))


def predict_host(frames):
    return frames[..., 0].float() * 0.5 + frames[..., 1].float() * 0.25 + frames[..., 2].float()
