"""Video mode's temporal depth filter on the host (src/video_mode.py: stabilize_depth; no GPU): its float64 torch route against the
NumPy model of the definition (tests/video_stabilize_cases.py) BIT FOR BIT, what the filter is for (a static region loses its
flicker, a moving bar keeps its depth), scene cuts, and the checks that refuse bad input before any work."""
import numpy as np
import pytest
import torch

import video_stabilize_cases as sc


def _vm():
    from src import _native, video_mode
    return _native, video_mode


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_host_route_equals_the_model_on_the_flicker_clip(radius):
    _, vm = _vm()
    frames, depth, _ = sc.flicker_clip()
    for params in ((radius, 10.0, 1.5), (radius, 40.0, 0.8)):
        want = sc.model(depth, frames, params)
        got = vm.stabilize_depth(frames, depth, params)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and got.shape == depth.shape
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
        t = vm.stabilize_depth(torch.from_numpy(frames), torch.from_numpy(depth), params)       # tensors in, a tensor out
        assert torch.is_tensor(t) and t.dtype == torch.uint16 and not t.is_cuda and np.array_equal(t.numpy(), want)
        assert not np.array_equal(want, depth)


def test_host_route_equals_the_model_on_extreme_values_noise_and_rgba():
    _, vm = _vm()
    frames, depth = sc.extreme_clip()
    assert set(np.unique(depth)) == {0, 65535} and set(np.unique(frames)) == {0, 255}
    for params in ((1, 300.0, 1.0), (3, 300.0, 2.0), (4, 1000.0, 50.0)):
        want = sc.model(depth, frames, params)
        assert np.array_equal(vm.stabilize_depth(frames, depth, params), want), params
        assert 0 < want[:, 0, 0].min() and want[:, 0, 0].max() < 65535            # the static pixel really mixes 0 and 65535
    frames, depth = sc.noise_clip(7, 5, 9, 4, seed=3)                             # k all over 0..765; the fourth byte is random
    for params in ((2, 200.0, 1.5), (4, 12.0, 2.5)):
        want = sc.model(depth, frames, params)
        assert np.array_equal(vm.stabilize_depth(frames, depth, params), want), params
        assert np.array_equal(vm.stabilize_depth(np.ascontiguousarray(frames[..., :3]), depth, params), want), "channel 3 was read"


def test_table_makers_share_the_colour_table_with_depth_refinement():
    nat, _ = _vm()
    wt, wc = nat.temporal_joint_bilateral_tables(3, 12.0, 1.5)
    mt, mc = sc.tables(3, 12.0, 1.5)
    assert wt.dtype == wc.dtype == np.float64 and wt.shape == (4,) and wc.shape == (766,)
    assert np.array_equal(wt, mt) and np.array_equal(wc, mc) and wt[0] == 1.0 and wc[0] == 1.0
    assert np.array_equal(wc, nat.depth_refine_tables(5, 12.0, 2.0)[1])
    assert nat.stabilize_params((2, 12, 1.5)) == (2, 12.0, 1.5) and nat.stabilize_params([np.int64(4), 1.0, 2]) == (4, 1.0, 2.0)


def test_static_rows_lose_their_flicker_and_the_moving_bar_keeps_its_depth():
    """(2, 10.0, 1.5) on flicker_clip(): the mean temporal standard deviation over the static rows (0..7, 16..23) of the output is
    below 0.7 of the input's -- the model gives 0.393 on this clip (0.549 at (1, 10, 1), 0.266 at (4, 10, 2)) -- and every bar pixel
    in its own frame keeps its input value exactly: its colour differs from what the other frames show there by k >= 54, a weight
    below 5e-7 at sigma_color = 10, against depth differences of at most 600 levels."""
    _, vm = _vm()
    frames, depth, bar = sc.flicker_clip()
    rows = sc.static_rows()
    assert rows.tolist() == list(range(0, 8)) + list(range(16, 24)) and not bar[:, rows].any()
    out = vm.stabilize_depth(frames, depth, (2, 10.0, 1.5))
    ratio = sc.temporal_std(out, rows) / sc.temporal_std(depth, rows)
    print("temporal std ratio over the static rows:", ratio)
    assert ratio < 0.7
    assert bar.sum() == 12 * 8 * 3 and np.array_equal(out[bar], depth[bar])
    for params, want in (((2, 10.0, 1.5), 0.393), ((1, 10.0, 1.0), 0.549), ((4, 10.0, 2.0), 0.266)):
        o = sc.model(depth, frames, params)
        assert abs(sc.temporal_std(o, rows) / sc.temporal_std(depth, rows) - want) < 5e-4, params


def test_cuts_are_never_crossed():
    _, vm = _vm()
    frames, depth, _ = sc.flicker_clip()
    params = (3, 10.0, 2.0)
    whole = vm.stabilize_depth(frames, depth, params)
    cut = vm.stabilize_depth(frames, depth, params, cuts=[5])
    assert np.array_equal(cut[:5], vm.stabilize_depth(frames[:5], depth[:5], params))
    assert np.array_equal(cut[5:], vm.stabilize_depth(frames[5:], depth[5:], params))
    assert np.array_equal(cut, sc.model(depth, frames, params, cuts=[5])) and not np.array_equal(cut, whole)
    assert np.array_equal(vm.stabilize_depth(frames, depth, params, cuts=[]), whole)
    # a scene of one frame comes back unchanged, as does a clip of one frame
    one = vm.stabilize_depth(frames, depth, params, cuts=[4, 5, 11])
    assert np.array_equal(one[4], depth[4]) and np.array_equal(one[11], depth[11]) and not np.array_equal(one[3], depth[3])
    assert np.array_equal(one, sc.model(depth, frames, params, cuts=[4, 5, 11]))
    assert np.array_equal(vm.stabilize_depth(frames[:1], depth[:1], params), depth[:1])


def test_colour_weights_that_underflow_to_zero_leave_the_centre_tap():
    """sigma_color = 0.5: wc[k] is exactly 0.0 from k = 20 on, so a pixel whose colour changed in every neighbouring frame has
    den == 1 exactly and keeps its value; nothing divides by zero."""
    nat, vm = _vm()
    wc = nat.temporal_joint_bilateral_tables(2, 0.5, 1.0)[1]
    assert wc[0] == 1.0 and wc[40] == 0.0 and wc[765] == 0.0
    frames, depth = sc.noise_clip(6, 4, 5, 3, seed=11)
    out = vm.stabilize_depth(frames, depth, (2, 0.5, 1.0))
    assert np.array_equal(out, sc.model(depth, frames, (2, 0.5, 1.0)))
    rgb = frames.astype(np.int64)
    moved = np.ones(depth.shape, bool)
    for i in range(6):
        for s in range(max(0, i - 2), min(5, i + 2) + 1):
            if s != i:
                moved[i] &= np.abs(rgb[s] - rgb[i]).sum(axis=2) >= 40
    assert moved.any() and np.array_equal(out[moved], depth[moved])


@pytest.mark.parametrize("params", [(0, 10.0, 1.5), (5, 10.0, 1.5), (2.5, 10.0, 1.5), (True, 10.0, 1.5), (2, 0.0, 1.5), (2, -1.0, 1.5),
                                    (2, float("nan"), 1.5), (2, float("inf"), 1.5), (2, 10.0, 0.0), (2, 10.0, -2.0), (2, 10.0, float("nan")),
                                    (2, 10.0, float("inf")), (2, 10.0), (2, 10.0, 1.5, 1), "2,10,1.5", None, (2, "x", 1.5)],
                         ids=repr)
def test_bad_parameters_are_refused(params):
    nat, vm = _vm()
    frames, depth = sc.noise_clip(4, 3, 5, 3, seed=1)
    with pytest.raises(ValueError):
        nat.stabilize_params(params)
    with pytest.raises((nat.DepthStereoError, ValueError)):
        vm.stabilize_depth(frames, depth, params)
    with pytest.raises((nat.DepthStereoError, ValueError)):
        vm.stabilize_depth_sharded(torch.from_numpy(frames), torch.from_numpy(depth), params)


def test_bad_dtypes_shapes_and_cuts_are_refused():
    nat, vm = _vm()
    frames, depth = sc.noise_clip(4, 3, 5, 3, seed=1)
    p = (2, 10.0, 1.5)
    refuse = (nat.DepthStereoError, ValueError)
    for bad_depth in (depth.astype(np.int16), depth.astype(np.float32), depth.astype(np.int32), depth[0], depth[:3], depth[:, :2],
                      depth[:, :, :4]):
        with pytest.raises(refuse):
            vm.stabilize_depth(frames, bad_depth, p)
    for bad_frames in (frames.astype(np.float32), frames[..., :2], frames[..., :1], frames[..., 0], frames[:3],
                       np.concatenate([frames, frames[..., :2]], axis=3)):
        with pytest.raises(refuse):
            vm.stabilize_depth(bad_frames, depth, p)
    with pytest.raises(refuse):
        vm.stabilize_depth(torch.from_numpy(frames), depth, p)                       # one tensor, one array
    with pytest.raises(refuse):
        vm.stabilize_depth(torch.from_numpy(frames), torch.from_numpy(depth.astype(np.int16)), p)
    for cuts in ([0], [4], [2, 2], [3, 1], [1.5], [True], [-1]):
        with pytest.raises(ValueError):
            vm.stabilize_depth(frames, depth, p, cuts=cuts)
    assert vm.stabilize_depth(frames, depth, p, cuts=[1, 3]).shape == depth.shape


def test_gen_frames_sharded_refuses_a_bad_tuple_before_the_first_pass():
    nat, vm = _vm()
    frames = torch.from_numpy(sc.noise_clip(4, 3, 5, 3, seed=1)[0])

    def predict(_):
        raise AssertionError("the first pass ran")
    for bad in ((0, 10.0, 1.5), (2, 0.0, 1.5), (2, 10.0), "mild", (2.5, 10.0, 1.0)):
        with pytest.raises((nat.DepthStereoError, ValueError)):
            vm.gen_frames_sharded(frames, predict, {}, stabilize=bad)
